"""Dark-field retrieval (LCS-DF) without a GPU: the float64 oracle of the contract (tests/_retrieval_df_oracle.py), the unit
conversion retrieval.scattering_angle against a forward model of the chain's re-splat, and the argument and flag checks that
come before any device."""
import numpy as np
import pytest
import torch

from oracle import paresis_oracle as orc
from tests import _retrieval_df_oracle as odf
from tests import _retrieval_oracle as orl


def test_oracle_recovers_exact_model():
    T, Dx, Dy, Df, S, R = odf.exact_model(64, 48, 8, seed=1)
    r = odf.lcs_df(S, R, dtype=np.float64, return_mask=True)
    fb = r['fallback']
    # the four corners are singular by construction: there L = g0 + g1 (one-sided differences, replicated neighbours)
    corners = np.zeros(fb.shape, bool)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    assert np.array_equal(fb, corners)
    ok = ~fb
    assert np.abs(r['transmission'] - T)[ok].max() < 1e-9
    assert np.abs(r['dx'] - Dx)[ok].max() < 1e-9
    assert np.abs(r['dy'] - Dy)[ok].max() < 1e-9
    assert np.abs(r['df'] - Df)[ok].max() < 1e-9
    assert Df.min() > 0.0 and np.abs(Dx).max() > 0.1


def test_laplacian_edge_replicated_by_hand():
    R = np.array([[1, 2, 4, 7, 11],
                  [3, 0, 5, 2, 8],
                  [6, 9, 1, 4, 0],
                  [2, 5, 3, 8, 6]], np.float32)
    # e.g. (0, 0): 3 + 1 + 2 + 1 - 4*1 = 3 (the missing up / left neighbours replicate R[0, 0]);
    # (3, 4): 0 + 6 + 8 + 6 - 4*6 = -4;  (1, 1): 2 + 9 + 3 + 5 - 0 = 19
    want = np.array([[3, -1, 2, -4, -7],
                     [-2, 19, -13, 16, -11],
                     [-4, -24, 17, -5, 18],
                     [7, -1, 5, -11, -4]], np.float64)
    L = odf.laplacian(R)
    assert L.dtype == np.float64
    assert np.array_equal(L, want)


def test_ldl_pivots_give_det_and_match_a_cholesky():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((50, 6, 4))
    M = np.einsum("bki,bkj->bij", A, A)
    d = odf.ldl_pivots(M)
    assert np.allclose(np.prod(d, -1), np.linalg.det(M), rtol=1e-10)
    assert np.allclose(d, np.diagonal(np.linalg.cholesky(M), axis1=-2, axis2=-1) ** 2, rtol=1e-10)


def test_oracle_fallbacks():
    T, Dx, Dy, Df, S, R = odf.exact_model(40, 40, 6, seed=3)
    S = [s.astype(np.float32) for s in S]
    for k in range(6):
        R[k][5:15, 5:15] = 5000.0                    # constant reference: g0 = g1 = L = 0, det M = 0
        S[k][5:15, 5:15] = 4000.0
        S[k][25:30, 25:30] = 0.0                     # S = 0: the first pivot is 0
    M, _ = odf.normal_equations(S, R)
    flat = (slice(6, 14), slice(6, 14))
    assert np.all(M[flat][..., 1:, :] == 0.0)                 # three zero rows
    r = odf.lcs_df(S, R, return_mask=True)
    for blk in (flat, (slice(25, 30), slice(25, 30))):
        assert r['fallback'][blk].all()
        for key, v in (('transmission', 1.0), ('dx', 0.0), ('dy', 0.0), ('df', 0.0)):
            assert np.all(r[key][blk] == v), key
    # x0 <= 0: a sample image that is the NEGATED model at one pixel solves to x0 = -1/T exactly, with non-zero pivots
    S2 = [s.copy() for s in S]
    for k in range(6):
        S2[k][33, 20] = -S2[k][33, 20]
    r2 = odf.lcs_df(S2, R, return_mask=True, dtype=np.float64)
    M2, v2 = odf.normal_equations(S2, R)
    assert not odf.singular(M2)[33, 20]
    assert np.linalg.solve(M2[33, 20], v2[33, 20])[0] < 0
    assert r2['fallback'][33, 20] and not r2['fallback'][32, 20]
    assert (r2['transmission'][33, 20], r2['dx'][33, 20], r2['dy'][33, 20], r2['df'][33, 20]) == (1.0, 0.0, 0.0, 0.0)


def test_oracle_clamp_leaves_df():
    T, Dx, Dy, Df, S, R = odf.exact_model(40, 40, 6, seed=4, dmax=2.0, dfmax=1.5)
    a = odf.lcs_df(S, R)
    c = odf.lcs_df(S, R, max_shift=0.5)
    assert np.abs(Dx).max() > 1.0 and np.abs(a['df']).max() > 0.5
    assert np.all(np.abs(c['dx']) <= np.float32(0.5)) and np.all(np.abs(c['dy']) <= np.float32(0.5))
    assert np.array_equal(c['df'], a['df']) and np.array_equal(c['transmission'], a['transmission'])


# ----------------------------------------------------------------------- the references the GPU parity tests are held to
def test_exact_reference_agrees_with_the_float64_oracles():
    S, R = orl.case_inputs(odf.exact_model, 6, 7, 6, 9)
    ref, o, f = odf.lcs_df_exact(S, R), odf.lcs_df(S, R, dtype=np.float64, return_mask=True), odf.lcs_df_f64(S, R)
    c = odf.corners(6, 7)
    assert np.array_equal(ref['fallback'], c) and np.array_equal(o['fallback'], c) and np.array_equal(f['fallback'], c)
    for k in odf.MAPS:
        assert np.abs(o[k] - ref[k]).max() < 1e-9 and np.abs(f[k] - ref[k]).max() < 1e-9, k
    # the exact Laplacian is the float64 one (exact for float32 data), and the exact pivots are ldl_pivots' up to rounding
    a, _ = orl.kernel_columns(S[0], R[0])
    assert np.array_equal(a[3], odf.laplacian(R[0]))
    M, _ = odf.normal_equations(S, R)
    d = odf.ldl_pivots(M)
    ratio = (d / np.stack([M[..., i, i] for i in range(4)], -1)).min(-1)
    assert np.allclose(ref['pivot_ratio'][~c], ratio[~c], rtol=1e-6)
    # the corners: L = g0 + g1 up to the float32 rounding of the two differences, so the last pivot is 0 or next to it
    assert np.all(ref['pivot_ratio'][c] < 1e-9) and np.all(ref['det_ratio'][c] < 1.0)


@pytest.mark.parametrize("n,m,K,seed,max_shift", odf.LCS_DF_CASES)
def test_lcs_df_parity_case_conditions(n, m, K, seed, max_shift):
    """tests/test_retrieval_host.test_lcs_parity_case_conditions for LCS-DF: 8 Y <= 2^-24; the four corners are structural
    fallbacks in the exact reference and in the restatement, and the only ones; no other pixel is within a relative 1e-6 of a
    fallback rule (a pivot against its diagonal entry, det against its threshold, x0 against the largest)."""
    S, R, ref, f64, Y = odf.lcs_df_parity(n, m, K, seed)
    c = odf.corners(n, m)
    print("lcs_df %dx%d K=%d seed %d: Y = %.2e, min det/threshold %.2e, min pivot/diagonal %.2e" %
          (n, m, K, seed, Y, ref['det_ratio'][~c].min(), ref['pivot_ratio'][~c].min()))
    assert 0.0 < 8.0 * Y <= orl.EPS32
    assert np.array_equal(ref['fallback'], c) and np.array_equal(f64['fallback'], c)
    assert ref['det_ratio'][~c].min() > 1.0 + 1e-6 and ref['pivot_ratio'][~c].min() > 1e-6
    assert ref['x0'].min() > 1e-6 * ref['x0'].max()
    if max_shift is not None:
        ms = float(np.float32(max_shift))
        over = (np.abs(ref['dx']) > ms) | (np.abs(ref['dy']) > ms)
        assert 0.1 * n * m < over.sum() < 0.9 * n * m


@pytest.mark.parametrize("n,m,K,seed", [c[:4] for c in odf.LCS_DF_CASES if c[4] is None])
def test_lcs_df_parity_bound_rejects_wrong_kernels(n, m, K, seed):
    """float32 accumulation, a border spacing of 0.5, a wrapped border neighbour, (odd K) a dropped last position and a
    zero-padded Laplacian each exceed the bound at least 10 times at some pixel; the right restatement stays within it."""
    S, R, ref, f64, Y = odf.lcs_df_parity(n, m, K, seed)
    bound = orl.parity_bound(ref, Y, odf.MAPS)
    f32 = lambda r: {k: r[k].astype(np.float32) for k in odf.MAPS}
    assert orl.worst_ratio(f32(f64), ref, bound, odf.MAPS) <= 1.0
    for variant in odf.VARIANTS:
        if variant == 'droplast' and K % 2 == 0:
            continue
        ratio = orl.worst_ratio(f32(odf.lcs_df_f64(S, R, variant)), ref, bound, odf.MAPS)
        print("lcs_df %dx%d K=%d %s: %.1e bounds" % (n, m, K, variant, ratio))
        assert ratio >= 10.0, variant


def test_lcs_df_steep_case_rejects_float64_differences():
    """tests/test_retrieval_host.test_lcs_steep_case_rejects_float64_differences for LCS-DF."""
    n, m, K, seed = orl.LCS_STEEP_CASE
    S, R, ref, f64, Y = odf.lcs_df_parity(n, m, K, seed, steep=True)
    c = odf.corners(n, m)
    assert orl.steep_fraction(R) > 0.1
    assert 0.0 < 8.0 * Y <= orl.EPS32 and np.array_equal(ref['fallback'], c) and np.array_equal(f64['fallback'], c)
    assert ref['det_ratio'][~c].min() > 1.0 + 1e-6 and ref['pivot_ratio'][~c].min() > 1e-6
    assert ref['x0'].min() > 1e-6 * ref['x0'].max()
    bound = orl.parity_bound(ref, Y, odf.MAPS)
    f32 = lambda r: {k: r[k].astype(np.float32) for k in odf.MAPS}
    assert orl.worst_ratio(f32(f64), ref, bound, odf.MAPS) <= 1.0
    for variant in ('diff64', 'acc32', 'spacing', 'wrap', 'zeropad'):
        ratio = orl.worst_ratio(f32(odf.lcs_df_f64(S, R, variant)), ref, bound, odf.MAPS)
        print("lcs_df steep %s: %.1e bounds" % (variant, ratio))
        assert ratio >= 10.0, variant


def test_lcs_df_nonfinite_rule_on_the_host():
    """The non-finite rule of include/paresis_hip.h in the three CPU references of LCS-DF (lcs_df_f64 follows the kernel's
    own tests: a pivot turns NaN, and `d > 0` refuses it)."""
    S, R = orl.case_inputs(odf.exact_model, 9, 66, 5, 2)
    Sb, Rb = orl.nonfinite_inputs(S, R)
    mask = orl.nonfinite_pixels(Sb, Rb) | odf.corners(9, 66)
    for fn in (odf.lcs_df_exact, lambda s, r: odf.lcs_df(s, r, dtype=np.float64, return_mask=True), odf.lcs_df_f64):
        clean, dirty = fn(S, R), fn(Sb, Rb)
        assert np.array_equal(clean['fallback'], odf.corners(9, 66)) and np.array_equal(dirty['fallback'], mask)
        for k, v in zip(odf.MAPS, (1.0, 0.0, 0.0, 0.0)):
            assert np.all(dirty[k][mask] == v), k
            assert np.array_equal(dirty[k][~mask], clean[k][~mask]), k


def _blur_periodic(x, patch):
    s = patch.shape[0] // 2
    out = np.zeros_like(x)
    for a in range(-s, s + 1):
        for b in range(-s, s + 1):
            out += patch[a + s, b + s] * np.roll(np.roll(x, a, 0), b, 1)
    return out


def test_scattering_angle_inverts_the_chain_resplat():
    """A known theta -> the chain's re-splat width sigma_study = theta*z/(2*h*M) study pixels (RF2:114, gaussian_shape(DF/2);
    h = p/(ov*M), EXP:188) -> the reference's own discrete patch on a seeded speckle at study resolution -> the detector's
    2 x 2 binning, over 10 shifted speckles -> oracle LCS-DF -> scattering_angle gives theta back."""
    from paresis_amd.retrieval import scattering_angle
    p_um, z, E, M, ov = 6.0, 3.6, 52.0, 145.2 / 141.6, 2
    h = p_um / ov / M * 1e-6
    theta = 1.6e-6                                                  # rad: sigma_det = theta*z/(2p) = 0.48 px
    sigma_study = theta * z / (h * M) / 2
    patch = orc.create_gaussian_shape(sigma_study)
    rng = np.random.default_rng(7)
    N = 128
    base = orl.speckle(ov * N, ov * N, rng, grain=8.0)
    bin2 = lambda a: a.reshape(N, ov, N, ov).mean(axis=(1, 3))
    S, R = [], []
    for _ in range(10):
        sh = rng.integers(0, ov * N, 2)
        r = np.roll(np.roll(base, sh[0], 0), sh[1], 1)
        R.append(bin2(r).astype(np.float32))
        S.append((0.8 * bin2(_blur_periodic(r, patch))).astype(np.float32))
    o = odf.lcs_df(S, R)
    inner = (slice(4, -4), slice(4, -4))
    got = float(np.median(scattering_angle(o['df'][inner].astype(np.float64), p_um, z)))
    # the patch actually applied is truncated at round(3 sigma): its per-axis variance, binned, is the df it should give
    q = np.arange(patch.shape[0]) - patch.shape[0] // 2
    df_patch = float((patch.sum(1) * q ** 2).sum()) / ov ** 2 / 2
    want = scattering_angle(df_patch, p_um, z)
    # calibration of this configuration: got/want = 1.002 (theta/want = 1.001: the truncation costs 0.1 %); a tolerance of
    # 10 % holds any wrong factor of ov, 2 or sqrt(2) (>= 41 % off) outside
    tol = 0.10
    assert abs(want / theta - 1) < 0.01
    print("scattering_angle forward model: got/want %.4f, theta/want %.4f" % (got / want, theta / want))
    assert abs(got / want - 1) < tol, (got, want)
    for f in (ov, 2.0, np.sqrt(2.0), 1 / ov, 0.5, 1 / np.sqrt(2.0)):
        assert abs(f * got / want - 1) > tol
    assert np.abs(np.median(o['transmission'][inner]) - 0.8) < 1e-3
    # the tensor form gives the same numbers, and negative df gives 0
    t = scattering_angle(torch.tensor([df_patch, -0.2, 0.0], dtype=torch.float64), p_um, z)
    assert abs(float(t[0]) - want) <= 1e-15 * want and float(t[1]) == 0.0 and float(t[2]) == 0.0


def test_argument_errors_before_any_device():
    from paresis_amd import ops
    from paresis_amd._lib import PsxError
    img = lambda K, n=8, m=8: torch.ones((K, n, m), dtype=torch.float32)
    with pytest.raises(PsxError, match="K=3"):
        ops.lcs_df(img(3), img(3))
    with pytest.raises(PsxError, match="K=2"):
        ops.lcs_df(img(2), img(2))
    with pytest.raises(PsxError, match="K=65"):
        ops.lcs_df(img(65), img(65))
    with pytest.raises(PsxError, match="shape"):
        ops.lcs_df([torch.ones(8, 8)] * 3 + [torch.ones(8, 9)], img(4))
    with pytest.raises(PsxError, match="shape"):
        ops.lcs_df(img(4), img(4, 8, 9))
    with pytest.raises(PsxError, match="positions"):
        ops.lcs_df(img(4), img(5))
    with pytest.raises(PsxError, match="HBM"):                            # CPU tensors: no CPU path
        ops.lcs_df(img(4), img(4))
    with pytest.raises(PsxError, match="HBM"):
        ops.lcs_df(img(4), img(4), out=[torch.empty(8, 8)] * 4)


def test_retrieve_needs_four_positions_for_dark_field():
    from paresis_amd import retrieval
    res = {p: (np.ones((1, 8, 8), np.float32), np.ones((1, 8, 8), np.float32)) for p in range(3)}
    with pytest.raises(ValueError, match="at least 4"):
        retrieval.retrieve(res, dark_field=True)


def test_dark_field_flag_rules(tmp_path):
    """main.py: --dark-field only with --retrieve and --points 4 or more; main.run(dark_field=...) the same; the retrieval CLI:
    --dark-field on a run directory of 3 positions stops before any device."""
    from paresis_amd import main, retrieval
    out = str(tmp_path / "out")
    for argv in (["--dark-field", "--points", "12"], ["--retrieve", "--dark-field", "--points", "3"]):
        with pytest.raises(SystemExit) as e:
            main.main(argv + ["--out", out])
        assert e.value.code == 2
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": out + "/", "overSampling": 2, "nbExpPoints": 3,
          "simulation_type": "RayT", "noise": False}
    with pytest.raises(ValueError, match="at least 4"):
        main.run(dict(ed), save=False, retrieve=True, dark_field=True)
    with pytest.raises(ValueError, match="option of retrieve"):
        main.run(dict(ed, nbExpPoints=12), save=False, dark_field=True)
    from tests.test_retrieval_host import _layout
    _layout(tmp_path / "run", "X", [0, 1, 2], ".npy")
    with pytest.raises(SystemExit) as e:
        retrieval.main([str(tmp_path / "run"), "--dark-field"])
    assert e.value.code == 2


def test_flag_messages(tmp_path, capsys):
    from paresis_amd import main
    with pytest.raises(SystemExit):
        main.main(["--retrieve", "--dark-field", "--points", "3", "--out", str(tmp_path)])
    assert "--dark-field needs --points 4 or more" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main.main(["--dark-field", "--points", "5", "--out", str(tmp_path)])
    assert "--dark-field is an option of --retrieve" in capsys.readouterr().err
