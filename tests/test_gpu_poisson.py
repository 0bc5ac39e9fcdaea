"""The shot-noise kernel k_poisson against the exact Poisson distribution (through ops.poisson / ops.poisson_multi).

Goodness of fit at constant means across both sampler branches and the log-pmf switch, the randomised probability-integral
transform on images whose mean varies inside a wave, the first PTRS candidate and the product-of-uniforms draw bit for bit
against the host restatement of the generator (tests/_poisson_oracle.py), independence of neighbouring pixels, of the images
of one launch and of neighbouring keys, and the edges of the mean's range.

Every statistical assertion is made at alpha = 1e-9 / T (T = 158 at PSX_FUZZ=1, counted per test below; alpha / k under
PSX_FUZZ=k, which repeats every test under k sets of keys): a correct sampler fails the file with probability <= 1e-9, and
the keys being fixed the outcome is deterministic.  tests/test_poisson_host.py shows that these sizes and thresholds reject
the planted defects.  A failing statistic is a finding about the kernel: keys, sizes and alpha stay.
"""
import os

import numpy as np
import pytest
import torch

from tests import _poisson_oracle as orc

pytestmark = pytest.mark.gpu

MULT = max(1, int(os.environ.get("PSX_FUZZ", "1")))
LV = orc.Level(mult=MULT)
IMG = 1 << 20                    # pixels per image of the goodness-of-fit launches
REPS = range(MULT)


@pytest.fixture(scope="module")
def ops():
    from paresis_amd import ops as _ops
    from paresis_amd._lib import lib
    assert lib().psx_device_ok() == 1, lib().psx_last_error()
    yield _ops
    print("\n" + summary())


def summary():
    """The tightest margins the kernel left (printed when the module ends; `pytest -s` shows it)."""
    out = []
    for kind in ("chi2", "z", "p"):
        rows = [r for r in LV.log if r[1] == kind]
        if rows:
            worst = max(rows, key=lambda r: (r[2] / r[3]) if kind != "p" else -r[2])
            out.append("%s: %d assertions, tightest %s = %.4g against %.4g" % (kind, len(rows), worst[0], worst[2], worst[3]))
    return "poisson margins (alpha %.2e): " % LV.alpha + "; ".join(out)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def draw(ops, lam, keys, misaligned=False):
    """One image per key from the mean image lam (a tensor), all in ONE poisson_multi launch; misaligned: every image starts one
    float past a 16-byte boundary, so the launch takes the scalar path."""
    n = lam.numel()
    if misaligned:
        bufs = [torch.empty(n + 4, dtype=torch.float32, device="cuda") for _ in keys]
        imgs = [b[1:1 + n] for b in bufs]
        assert all(im.data_ptr() % 16 == 4 for im in imgs)
    else:
        imgs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in keys]
        assert all(im.data_ptr() % 16 == 0 for im in imgs)
    for im in imgs:
        im.copy_(lam.reshape(-1))
    ops.poisson_multi(imgs, list(keys))
    return imgs


def counts_ok(x):
    return bool(torch.all((x == torch.floor(x)) & (x >= 0)))


def histogram(imgs):
    """Exact integer histogram of the launches' counts (index = count), on the host as int64."""
    h = None
    for x in imgs:
        assert counts_ok(x)
        c = torch.bincount(x.to(torch.int64))
        if h is None or c.numel() > h.numel():
            c, h = h, c
        if c is not None:
            h[:c.numel()] += c
    return h.cpu().numpy()


# ------------------------------------------------------------------------------------------------ goodness of fit
@pytest.mark.parametrize("rep", REPS)
def test_fit_at_constant_mean(ops, rep):
    """(a) per-count chi2, (b) coarse chi2, (c) z of mean, variance and third moment at every mean >= 0.1 of the grid; the
    nonzero count against the binomial below.  From 10 on, half of the images go through the scalar path."""
    made = LV.made
    for li, lam in enumerate(orc.LAM_GRID):
        nimg = orc.fit_size(lam) // IMG
        field = torch.full((IMG,), lam, dtype=torch.float32, device="cuda")
        keys = [orc.key("fit", rep, li * 64 + j) for j in range(nimg)]      # consecutive integers, as Detector numbers them
        imgs = []
        for g in range(0, nimg, 8):
            half = keys[g:g + 8]
            if lam >= 10:
                imgs += draw(ops, field, half[:len(half) // 2]) + draw(ops, field, half[len(half) // 2:], misaligned=True)
            else:
                imgs += draw(ops, field, half)
        h = histogram(imgs)
        N = int(h.sum())
        assert N == orc.fit_size(lam)
        tag = "mean %.9g" % lam
        if lam < 0.1:
            LV.p(orc.binom_p(N - int(h[0]), N, lam), tag + " nonzero count %d" % (N - int(h[0])))
            continue
        LV.chi2(orc.chi2_fine(h, lam), tag + " per-count chi2")
        LV.chi2(orc.chi2_coarse(h, lam), tag + " coarse chi2")
        for name, z in zip(("mean", "variance", "third moment"), orc.moment_z(h, lam)):
            LV.z(z, tag + " z " + name)
    LV.settle(made, orc.GPU_ASSERTIONS["fit"])


# ------------------------------------------------------------------------------------------------ varying mean
@pytest.mark.parametrize("rep", REPS)
def test_varying_mean_pit(ops, rep):
    """(d) on images whose mean varies inside a wave: all lanes of a wave no longer take one branch, the pending pixels of
    several branches meet in the redistribution through LDS, and the sizes leave the last round with inactive lanes.  Fields up
    to 300007 pixels are also compared draw by draw with the restatement where it is safe from float32 rounding."""
    made = LV.made
    for fi, (name, lam) in enumerate(orc.varying_fields()):
        k = orc.key("varying", rep, fi)
        x = ops.poisson(dev(lam), seed=k)
        assert counts_ok(x), name
        x = x.cpu().numpy().astype(np.float64)
        assert np.all(x[lam == 0] == 0), name
        if lam.size <= orc.COMPARE_MAX:
            info = {}
            want = orc.sample(lam, orc.PhiloxSource(k), info=info)
            safe = orc.safe_draws(info)
            assert safe.mean() >= 0.98, (name, safe.mean())
            bad = np.flatnonzero(safe & (x != want))
            assert bad.size == 0, (name, bad.size, bad[:8], x[bad[:8]], want[bad[:8]], lam[bad[:8]])
        if lam.size >= orc.PIT_MIN:
            u = orc.pit(x, lam, np.random.default_rng([k, 1]))
            for sname, m in orc.strata(lam):
                LV.chi2(orc.chi2_uniform(u[m]), "%s PIT chi2, stratum %s" % (name, sname))
    LV.settle(made, orc.GPU_ASSERTIONS["varying"])


@pytest.mark.parametrize("rep", REPS)
def test_zero_image_with_a_live_tail(ops, rep):
    """0 everywhere but the last one to three pixels (the scalar tail of an aligned image and the last quad's lanes): zeros
    stay zeros, the live pixels carry the restatement's draws."""
    for t in (1, 2, 3):
        for n in (orc.SIZES[0] + t, orc.SIZES[0], orc.SIZES[1] - 3 + t):
            lam = np.zeros(n, dtype=np.float32)
            lam[n - t:] = (7500.0, 12.0, 3.0)[:t]
            k = orc.key("varying", rep, 100 + 10 * t + (n > 1000))
            info = {}
            want = orc.sample(lam, orc.PhiloxSource(k), info=info)
            for mis in (False, True):
                x = draw(ops, dev(lam), [k], misaligned=mis)[0].cpu().numpy()
                assert np.all(x[:n - t] == 0) and np.all(x[n - t:] == np.floor(x[n - t:])) and np.all(x >= 0)
                safe = orc.safe_draws(info)
                assert np.array_equal(x[safe], want[safe]), (n, t, mis, x[n - t:], want[n - t:])


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("rep", REPS)
def test_first_candidate_bit_for_bit(ops, rep):
    """Where the restated first candidate passes the squeeze with margin and its value is not within DELTA of an integer
    (orc.first_candidate_check derives DELTA), the kernel's count IS floor of the float64 value: this pins the generator, the
    word assignment of the shared Philox block and the candidate's arithmetic without any statistics.  The caps keep the
    exclusions from hiding a failure (tests/test_poisson_host.py shows them from the restatement alone)."""
    p = np.arange(orc.EXACT_N, dtype=np.uint64)
    for j, lam in enumerate(orc.FIRST_LAMS):
        key = orc.key("first", rep, j)
        k, squeeze, checked = orc.first_candidate_check(np.full(p.size, lam), p, key)
        assert 1 - checked.sum() / squeeze.sum() <= 0.02
        if lam == 7500.0:
            assert checked.mean() >= 0.70
        field = torch.full((p.size,), lam, dtype=torch.float32, device="cuda")
        for mis in (False, True):
            x = draw(ops, field, [key], misaligned=mis)[0].cpu().numpy().astype(np.float64)
            bad = np.flatnonzero(checked & (x != k))
            assert bad.size == 0, (lam, mis, bad.size, bad[:8], x[bad[:8]], k[bad[:8]])


@pytest.mark.parametrize("rep", REPS)
def test_product_of_uniforms_bit_for_bit(ops, rep):
    """Below 10 the whole draw against the restated product of uniforms (counter p, sub 1, 2, ..., tag 0x5059), but for the
    pixels whose running product passes within a few float32 ulp of exp(-mean) (<= 0.1 % of them)."""
    n = 1 << 18
    for j, lam in enumerate(orc.PRODUCT_LAMS):
        key = orc.key("product", rep, j)
        info = {}
        want = orc.sample(np.full(n, lam), orc.PhiloxSource(key), info=info)
        safe = info["near"] > orc.PRODUCT_NEAR
        assert 1 - safe.mean() <= 1e-3
        field = torch.full((n,), lam, dtype=torch.float32, device="cuda")
        for mis in (False, True):
            x = draw(ops, field, [key], misaligned=mis)[0].cpu().numpy().astype(np.float64)
            bad = np.flatnonzero(safe & (x != want))
            assert bad.size == 0, (lam, mis, bad.size, bad[:8], x[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("rep", REPS)
def test_independence(ops, rep):
    """(e) z = r sqrt(n) of the normal scores of the PIT between pixel sets that share generator state if anything is wrong:
    the two pixels of one Philox block, pixels across blocks and quads, lags, an image row (1024), the images of one launch,
    neighbouring integer keys, poisson_key arguments one apart, and a draw against its own rejected first candidate."""
    made = LV.made
    n, row = orc.EXACT_N, 1024
    for fi, (name, lam) in enumerate((("smooth", orc.smooth_field(n)), ("constant 7500", np.full(n, 7500.0, dtype=np.float32)))):
        lam_d = dev(lam)
        base = orc.key("indep", rep, 16 * fi)

        def scores(x, salt):
            assert counts_ok(x)
            return orc.normal_scores(orc.pit(x.cpu().numpy(), lam, np.random.default_rng([base, salt])))

        x0 = ops.poisson(lam_d, seed=base)
        g = scores(x0, 0)
        LV.z(orc.corr_z(g[0::2], g[1::2]), name + ": pixels (2q, 2q+1)")
        LV.z(orc.corr_z(g[1:-1:2], g[2::2]), name + ": pixels (2q+1, 2q+2)")
        LV.z(orc.corr_z(g[3:-1:4], g[4::4]), name + ": pixels (4q+3, 4q+4)")
        for lag in (2, 3, 4, 64, 256, row):
            LV.z(orc.corr_z(g[:-lag], g[lag:]), name + ": lag %d" % lag)
        keys = [(rep << 20) + 1 + fi * 8 + j for j in range(4)]             # (seed << 20) + draws, the unkeyed Detector numbering
        gm = [scores(x, 1 + j) for j, x in enumerate(draw(ops, lam_d, keys))]
        for j in range(3):
            LV.z(orc.corr_z(gm[j], gm[j + 1]), name + ": images %d and %d of one launch" % (j, j + 1))
        LV.z(orc.corr_z(g, scores(ops.poisson(lam_d, seed=base + 1), 5)), name + ": keys s and s + 1")
        args = (5 + rep, 3, 1, 0)
        ga = scores(ops.poisson(lam_d, seed=ops.poisson_key(*args)), 6)
        for f in range(4):
            nb = tuple(v + (i == f) for i, v in enumerate(args))
            LV.z(orc.corr_z(ga, scores(ops.poisson(lam_d, seed=ops.poisson_key(*nb)), 7 + f)),
                 name + ": poisson_key field %d one apart" % f)
        # the pixel's own stream must not echo the first candidate it replaced
        info = {}
        orc.sample(lam, orc.PhiloxSource(base), info=info)
        later = (info["ncand"] >= 2) & orc.safe_draws(info)
        assert later.sum() >= n // 20, later.sum()
        U0, _ = orc.first_candidate(np.arange(n, dtype=np.uint64), base)
        LV.z(orc.corr_z(U0[later], g[later]), name + ": draw against its rejected first candidate")
    LV.settle(made, orc.GPU_ASSERTIONS["independence"])


# ------------------------------------------------------------------------------------------------ edges
def test_means_that_give_zero(ops):
    vals = np.array([0.0, -1.0, -0.0, np.nan, 1e-45, 1e-39, -np.inf, -1e-45], dtype=np.float32)
    lam = np.tile(vals, 64 * 5)
    for mis in (False, True):
        x = draw(ops, dev(lam), [11], misaligned=mis)[0]
        assert bool(torch.all(x == 0)), (mis, x[:8])


def test_means_beyond_the_supported_range(ops):
    """Above 2^23 and at +inf (include/paresis_hip.h: outside the supported range) both paths still give the same bits, and the
    status word stays clear."""
    vals = np.array([np.inf, 2.0 ** 24, 3e7, 1e12, 3e38, 2.0 ** 23], dtype=np.float32)
    lam = np.repeat(vals, 512)
    ops.check_status(torch.device("cuda", torch.cuda.current_device()), "before")
    a = draw(ops, dev(lam), [12])[0]
    b = draw(ops, dev(lam), [12], misaligned=True)[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ops.check_status(a.device, "poisson beyond 2^23")
    top = a[-512:]                                                       # 2^23 is the top of the supported range
    assert counts_ok(top) and abs(float(top.double().mean()) - 2.0 ** 23) < 6 * np.sqrt(2.0 ** 23 / 512)


@pytest.mark.parametrize("which", (0, 1))
def test_unit_uniform_first_candidate(ops, which):
    """u = 1.0 in the first candidate (U = +0.5: us = 0, rcp(0) = inf in the candidate; or V = 1): the candidate is dropped or
    judged like any other and the draw is the restatement's, at a PTRS mean and at a product-of-uniforms mean."""
    seed, p = (orc.UNIT_U, orc.UNIT_V)[which]
    U, V = orc.first_candidate(np.array([p]), seed)
    assert (U[0] == np.float32(0.5)) if which == 0 else (V[0] == np.float32(1.0))
    n = p + 5
    for lam in (7500.0, 3.0):
        field = np.full(n, lam, dtype=np.float32)
        info = {}
        want = orc.sample(field, orc.PhiloxSource(seed), info=info)
        assert orc.safe_draws(info)[p], (info["margin"][p], info["edge"][p], info["near"][p])
        for mis in (False, True):
            x = draw(ops, dev(field), [seed], misaligned=mis)[0].cpu().numpy()
            assert np.isfinite(x[p]) and x[p] >= 0 and x[p] == np.floor(x[p]) and x[p] == want[p], (lam, mis, x[p], want[p])
