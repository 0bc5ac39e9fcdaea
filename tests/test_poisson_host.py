"""The oracle of the shot-noise tests (tests/_poisson_oracle.py) checked on the host: the generator against the published
Philox4x32-10 known answers, the range of the uniform mapping, the exclusion caps of the bit-for-bit GPU comparisons (from the
restatement alone), that the statistics accept numpy's Poisson sampler and the unmodified restatement at every mean of the
GPU grid, and -- the power check -- that at the GPU tests' own sample sizes and thresholds every planted defect is rejected by
a statistic the GPU test asserts.  What rejected each, as figure / limit at alpha = 1e-9 / 158 (printed by the tests, `-s`):

    direct float32 log-pmf, mean 30000, N 2^24      per-count chi2 1.99, coarse chi2 1.55; the moments pass
    log(2 pi L) for log(2 pi k), mean 7500, N 2^24  z of the mean 3.5 (|z| = 24), coarse chi2 3.6, third moment 2.6, chi2 1.24
    squeeze without us >= 0.07, mean 12.5, N 2^22   every statistic, by factors of 36 to 3e5 (candidates far outside the range)
    mean scaled by 1 + 2e-4, mean 7500, N 2^24      z of the mean 10.4 (|z| = 71), coarse chi2 30, third moment 8.1, chi2 5.9
    PTRS below 10, mean 3, N 2^22                   per-count chi2 2.4 alone
    shared first candidate of a pixel pair          correlation z of pairs (2q, 2q+1) = 641 against 6.87
"""
import numpy as np
import pytest

from tests import _poisson_oracle as orc

LV = orc.Level()


def test_philox_known_answers():
    kat = {(0, 0, 0, 0): "6627e8d5 e169c58d bc57ac4c 9b00dbd8",
           (2 ** 64 - 1, 0xFFFFFFFF, 0xFFFFFFFF, 2 ** 64 - 1): "408f276d 41c83b0e a20bc7c6 6d5451fd",
           (0x85A308D3243F6A88, 0x13198A2E, 0x03707344, 0x299F31D0A4093822): "d16cfe09 94fdcceb 5001e420 24126ea1"}
    for (ctr, sub, tag, key), want in kat.items():
        assert " ".join("%08x" % w for w in orc.philox4x32_10(ctr, sub, tag, key)) == want
    # vectorised over counters and keys alike
    w = orc.philox4x32_10(np.array([0, 0x85A308D3243F6A88], dtype=np.uint64), np.array([0, 0x13198A2E]), np.array([0, 0x03707344]),
                          np.array([0, 0x299F31D0A4093822], dtype=np.uint64))
    assert "%08x" % w[0, 0] == "6627e8d5" and "%08x" % w[3, 1] == "24126ea1"


def test_uniform_mapping_range():
    """Not (0, 1): the + 0.5f is rounded away from 2^23 on (ties to even), the top mantissa gives exactly 1.0; never more,
    never 0."""
    top = np.arange(2 ** 24 - 4096, 2 ** 24, dtype=np.uint64) << np.uint64(8) | np.uint64(0xFF)
    u = orc.uniform_f32(top.astype(np.uint32))
    assert u.dtype == np.float32 and u[-1] == np.float32(1.0) and u.max() == np.float32(1.0)
    every = orc.uniform_f32((np.arange(2 ** 24, dtype=np.uint64) << np.uint64(8)).astype(np.uint32))     # every c >> 8
    assert every.min() == np.float32(2.0 ** -25) and every.max() == np.float32(1.0) and np.all(np.diff(every) >= 0)
    assert np.count_nonzero(every == np.float32(1.0)) == 1
    assert orc.uniform_f32(np.uint32(2 ** 23 << 8)) == np.float32(0.5)          # (2^23 + 0.5) is a tie: rounds to even


def test_first_candidate_word_assignment():
    p = np.arange(64, dtype=np.uint64)
    U, V = orc.first_candidate(p, 77)
    w = orc.uniform_f32(orc.philox4x32_10(p >> np.uint64(1), 0, orc.TAG_FIRST, 77))
    assert np.array_equal(U[0::2], w[0][0::2] - np.float32(0.5)) and np.array_equal(V[0::2], w[1][0::2])
    assert np.array_equal(U[1::2], w[2][1::2] - np.float32(0.5)) and np.array_equal(V[1::2], w[3][1::2])


def test_unit_uniform_pixels_exist():
    """The (seed, pixel) pairs the GPU edge test uses: first-candidate words 0xFFFFFFxx, so u = 1.0 (U = +0.5 or V = 1)."""
    assert orc.find_unit_uniform(0) == orc.UNIT_U and orc.find_unit_uniform(1) == orc.UNIT_V
    for which, (seed, p) in ((0, orc.UNIT_U), (1, orc.UNIT_V)):
        U, V = orc.first_candidate(np.array([p]), seed)
        assert (U[0] == np.float32(0.5)) if which == 0 else (V[0] == np.float32(1.0))


def test_exclusion_caps_from_the_restatement():
    """What the bit-for-bit GPU comparisons leave out, counted without any kernel: at most 2 % of the squeeze-accepted pixels
    (first candidate), at least 70 % of all pixels checked at a mean of 7500 (the kernel's comment: 78 % pass the squeeze),
    at most 0.1 % of the product-of-uniforms draws."""
    p = np.arange(orc.EXACT_N, dtype=np.uint64)
    for j, lam in enumerate(orc.FIRST_LAMS):
        _, squeeze, checked = orc.first_candidate_check(np.full(p.size, lam), p, orc.key("first", 0, j))
        assert 1 - checked.sum() / squeeze.sum() <= 0.02, (lam, checked.sum(), squeeze.sum())
        if lam == 7500.0:
            assert 0.70 <= checked.mean() <= 0.80, checked.mean()
    for j, lam in enumerate(orc.PRODUCT_LAMS):
        info = {}
        orc.sample(np.full(1 << 18, lam), orc.PhiloxSource(orc.key("product", 0, j)), info=info)
        assert np.mean(info["near"] <= orc.PRODUCT_NEAR) <= 1e-3, lam


def _fit(h, lam):
    """The statistics the GPU goodness-of-fit test asserts at one mean, as {name: rejected, figure}."""
    fine, coarse = orc.chi2_fine(h, lam), orc.chi2_coarse(h, lam)
    z = orc.moment_z(h, lam)
    res = {"chi2": (LV.rejects_chi2(fine), fine[0] / LV.chi2_limit(fine[1])),
           "coarse chi2": (LV.rejects_chi2(coarse), coarse[0] / LV.chi2_limit(coarse[1]))}
    for name, v in zip(("z mean", "z variance", "z third moment"), z):
        res[name] = (LV.rejects_z(v), abs(v) / LV.zmax)
    return res


@pytest.mark.parametrize("lam", orc.LAM_GRID)
def test_statistics_accept_correct_samplers(lam):
    N = orc.fit_size(lam)
    rng = np.random.default_rng([int(lam * 1000), 17])
    hists = {"numpy": np.bincount(rng.poisson(lam, N)), "restatement": orc.sample_hist(lam, N, orc.NumpySource(rng))}
    for name, h in hists.items():
        assert h.sum() == N
        if lam <= 1e-3:
            assert orc.binom_p(N - h[0], N, lam) >= LV.alpha, (name, lam)
        else:
            res = _fit(h, lam)
            assert not any(r for r, _ in res.values()), (name, lam, res)


POWER = [("direct_f32", 30000.0), ("stirling_logL", 7500.0), ("no_guard", 12.5), ("lam_scale", 7500.0), ("ptrs_small", 3.0)]


@pytest.mark.parametrize("defect,lam", POWER)
def test_power_goodness_of_fit(defect, lam):
    """A planted defect in the restatement, drawn at the GPU test's size for this mean: some asserted statistic rejects it."""
    assert lam in orc.LAM_GRID
    N = orc.fit_size(lam)
    rng = np.random.default_rng([POWER.index((defect, lam)), 23])
    res = _fit(orc.sample_hist(lam, N, orc.NumpySource(rng), defects=(defect,)), lam)
    print(defect, lam, N, {k: ("REJECTED" if r else "passed", round(v, 2)) for k, (r, v) in res.items()}, "(figure / limit)")
    assert any(r for r, _ in res.values()), (defect, res)


def test_power_independence():
    """Two neighbours given the same first candidate: the correlation of the pair (2q, 2q+1) rejects; the same statistic
    accepts the unmodified restatement."""
    lam = np.full(orc.EXACT_N, 7500.0)
    for defects, want in (((), False), (("shared_candidate",), True)):
        rng = np.random.default_rng(29)
        x = orc.sample(lam, orc.NumpySource(rng), defects=defects)
        g = orc.normal_scores(orc.pit(x, lam, rng))
        z = orc.corr_z(g[0::2], g[1::2])
        print("shared candidate" if want else "independent", "z = %.1f, limit %.2f" % (z, LV.zmax))
        assert LV.rejects_z(z) == want, z


def test_pit_is_uniform_for_numpy_draws_on_the_varying_fields():
    rng = np.random.default_rng(31)
    for lam in (orc.smooth_field(300007), orc.cycle_field(300007, 2), orc.lone_pending_field(300007)):
        lam = lam.astype(np.float64)
        u = orc.pit(rng.poisson(lam), lam, rng)
        assert not LV.rejects_chi2(orc.chi2_uniform(u))


def test_assertion_count_of_the_gpu_file():
    """alpha = 1e-9 / T: T as the GPU file's plan gives it (that file checks the count of each test as it runs)."""
    fit = sum(5 if lam >= 0.1 else 1 for lam in orc.LAM_GRID)
    varying = sum(len(orc.strata(f)) for _, f in orc.varying_fields() if f.size >= orc.PIT_MIN)
    assert orc.GPU_ASSERTIONS == {"fit": fit, "varying": varying, "independence": 2 * 18}
    assert orc.T_GPU == fit + varying + 36
