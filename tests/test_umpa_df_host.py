"""UMPA's dark-field term without a GPU: the float64 oracle of the contract (tests/_umpa_df_oracle.py) against the contract read
literally, what the model recovers, what the inputs of the GPU sweep hold, and the argument rules that come before any device."""
import numpy as np
import pytest
import torch

from tests import _retrieval_oracle as orl
from tests import _umpa_df_oracle as od
from tests import _umpa_oracle as ou


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in od.KEYS)


def test_oracle_is_exact_on_integer_images():
    """umpa_df() == umpa_df_brute() bit for bit on all five maps: the planted instance at w = 1, s = 2, K = 2 (25 x 43: zero
    block, flat block and negated block), a near-flat one, and a periodic one in which every interior pixel is an exact tie."""
    for w, s, K, kw in ((1, 2, 2, {}), (1, 1, 3, {'near_flat': True}), (2, 2, 1, {'period': (2, 3), 'shape': (15, 17)})):
        S, R, mu = od.integer_df_model(w, s, K, seed=5, **kw)
        o = od.umpa_df(S, R, mu, w, s)
        assert o['fallback'].any() == ('period' not in kw)
        assert (o['gap'][o['interior']] == 0).all() == ('period' in kw)
        for key, b in zip(od.KEYS, od.umpa_df_brute(S, R, mu, w, s)):
            assert np.array_equal(o[key], b.astype(np.float32)), key
        od.compare_exact_df(o, o, ties='period' in kw, label="oracle on itself")
        with pytest.raises(AssertionError):
            wrong = {k: o[k].copy() for k in od.KEYS}
            wrong['visibility'][w + s, w + s] = np.nextafter(wrong['visibility'][w + s, w + s], np.float32(9))
            od.compare_exact_df(wrong, o, ties=True)
    with pytest.raises(AssertionError, match="exact ties"):
        od.compare_exact_df(o, o)


def _known(T=0.8, V=0.4, shift=(2.0, -3.0), n=64, m=72, K=4, seed=10):
    """S_k = T (mu_k + V (R_k(q - shift) - mu_k)), the shift by a Fourier ramp (exact for whole pixels)."""
    rng = np.random.default_rng(seed)
    R = [orl.speckle(n, m, rng).astype(np.float32) for _ in range(K)]
    mu = [float(r.astype(np.float64).mean()) for r in R]
    kx, ky = np.fft.fftfreq(n)[:, None], np.fft.fftfreq(m)[None, :]
    ramp = np.exp(-2j * np.pi * (kx * shift[0] + ky * shift[1]))
    S = [np.float32(T * (u + V * (np.fft.ifft2(np.fft.fft2(r.astype(np.float64)) * ramp).real - u))) for r, u in zip(R, mu)]
    return S, R, mu


def test_known_answer_parabola_and_fallback():
    """T = 0.8, V = 0.4, shift (2, -3) at w = 2, s = 3: dy is on the search boundary and exactly -3, dx = 2 up to the parabola
    through asymmetric neighbours, T and V to the float32 rounding of the images (1e-5), the residual vanishes.  Then a block
    without reference: exactly (1, 0, 0, 1, 0) two pixels inside it."""
    S, R, mu = _known()
    o = od.umpa_df(S, R, mu, 2, 3)
    inner = o['interior']
    assert not o['fallback'].any()
    assert np.array_equal(o['dy'][inner], np.full(inner.sum(), -3.0, np.float32))
    assert np.array_equal(o['b'][inner], np.full(inner.sum(), -3)) and np.array_equal(o['a'][inner], np.full(inner.sum(), 2))
    et = np.abs(o['transmission'][inner].astype(np.float64) - 0.8).max()
    ev = np.abs(o['visibility'][inner].astype(np.float64) - 0.4).max()
    med = np.median(np.abs(o['dx'][inner].astype(np.float64) - 2.0))
    print("known answer: |T-0.8| %.2e, |V-0.4| %.2e, residual max %.2e, median |dx-2| %.4f"
          % (et, ev, o['residual'][inner].max(), med))
    assert et <= 1e-5 and ev <= 1e-5
    assert o['residual'][inner].max() <= 1e-10
    assert med <= 0.05
    assert (np.abs(o['dx'][inner] - 2.0) <= 0.5).all()
    for k in range(len(R)):
        R[k][20:36, 24:40] = 0.0
    o = od.umpa_df(S, R, mu, 2, 3)
    blk = (slice(27, 29), slice(31, 33))
    assert o['fallback'][blk].all()
    for key in od.KEYS:
        assert np.all(o[key][blk] == od.FILL[key]), key
    for key in od.KEYS:
        assert np.all(o[key][~o['interior']] == od.FILL[key]), key


def test_visibility_falls_with_blur_and_transmission_stays():
    """96 x 96, K = 8, w = 2, s = 3, T = 0.8, shift (2, -1), speckle of grain 3, the sample blurred by a Gaussian of sigma px:
    the median V falls monotonically (about 1.000, 0.998, 0.952, 0.868, 0.748), the median T stays within 1 % of 0.8, and the
    shift is found exactly at every sigma."""
    import scipy.ndimage as ndi
    meds = []
    for sig in (0.0, 0.3, 0.5, 0.8, 1.2):
        rng = np.random.default_rng(1)
        S, R = [], []
        for _ in range(8):
            r = orl.speckle(96, 96, rng, grain=3.0).astype(np.float64)
            sh = np.roll(r, (2, -1), (0, 1))
            S.append(np.float32(0.8 * (ndi.gaussian_filter(sh, sig, mode='wrap') if sig else sh)))
            R.append(np.float32(r))
        mu = [float(r.astype(np.float64).mean()) for r in R]
        o = od.umpa_df(S, R, mu, 2, 3)
        inner = o['interior']
        mt, mv = np.median(o['transmission'][inner]), np.median(o['visibility'][inner])
        print("sigma %.1f: median T %.4f, median V %.4f" % (sig, mt, mv))
        assert abs(mt - 0.8) <= 0.008
        assert (o['a'][inner] == 2).mean() > 0.99 and (o['b'][inner] == -1).mean() > 0.99
        meds.append(mv)
    assert abs(meds[0] - 1.0) <= 1e-4
    assert all(b < a for a, b in zip(meds, meds[1:]))
    assert meds[-1] < 0.85


# ------------------------------------------------------------------------------ the inputs of the exact GPU sweep
def _restated(S, R, mu, w, s, mutant=None, vol=None):
    """The oracle's five maps with one wrong kernel restated: 'skip_c0' skips a candidate only when C == 0 (what a division
    by det == 0 then gives is NaN, which never wins a strict comparison and is no parabola neighbour, exactly as in the
    kernel: it is treated as skipped); 'g_at_r' takes G at r instead of r - u; 'h_plain' leaves the (2w+1)^2 out of H;
    'v_beta' returns beta/T for V."""
    E, F, B, C, G, H = vol if vol is not None else od.cost_volume_df(S, R, mu, w, s)
    if mutant == 'g_at_r':
        G = np.broadcast_to(G[(2 * s + 1) * s + s], G.shape)
    if mutant == 'h_plain':
        H = H / float(2 * w + 1) ** 2
    if mutant == 'skip_c0':
        with np.errstate(invalid='ignore', divide='ignore'):
            p = C * H
            det = p - G * G
            al = (B * H - F[None] * G) / det
            be = (C * F[None] - G * B) / det
            L = E[None] - (al * B + be * F[None])
            ok = (C != 0) & np.isfinite(L)
        L, al, be = np.where(ok, L, np.inf), np.where(ok, al, 0.0), np.where(ok, be, 0.0)
        T = al + be
    else:
        ok, al, be, L, T = od.solve(E[None], F[None], B, C, G, H)
    return od.finish(L, T, be if mutant == 'v_beta' else al, E, np.asarray(S[0]).shape, w, s)


@pytest.mark.parametrize("w", range(1, 9))
def test_integer_sweep_holds_every_class_and_wrong_kernels_show(w):
    """For s = 1..8 at this w, on the very inputs of test_umpa_df_every_window_and_search_exact: 3 x 3 pixels with C == 0 at
    every candidate, 3 x 3 with every candidate skipped through det == 0 at C != 0, partly skipped pixels, T <= 0 pixels,
    ordinary pixels in two tile rows and two tile columns, no exact tie; the restatement equals the oracle bit for bit, and
    the wrong kernels 'g_at_r', 'h_plain' and 'v_beta' each change at least one output value.
    'skip_c0' cannot show here: where det == 0 exactly the unskipped division gives 0/0 = NaN, which the kernel's strict
    comparison never selects, and on integers up to 4095 with unrelated mu no window has 0 < det <= 1e-12 p.
    test_near_flat_windows_need_the_relative_test covers it."""
    for s in range(1, 9):
        S, R, mu = od.sweep_instance(w, s)
        n, m = S[0].shape
        assert max(n, m) <= 100 and n % ou.TILE_H and m % ou.tile_width(w)
        assert np.array_equal(mu, np.rint(mu)) and mu.min() >= 1 and mu.max() <= 4095
        vol = od.cost_volume_df(S, R, mu, w, s)
        o = od.umpa_df(S, R, mu, w, s, vol=vol)
        c = od.classes_df(S, R, mu, w, s, vol=vol)
        count = {k: int(c[k].sum()) for k in c if c[k].dtype == bool}
        print("w=%d s=%d K=%d %dx%d: %s" % (w, s, len(S), n, m, count))
        assert count['zero_skipped'] == 9 and count['flat_skipped'] == 9 and count['all_skipped'] == 18, (s, count)
        assert count['some_skipped'] >= 1 and count['nonpositive'] >= 1, (s, count)
        assert len(set(c['tile_row'][c['ordinary']])) >= 2 and len(set(c['tile_col'][c['ordinary']])) >= 2, s
        assert not (o['gap'][o['interior']] == 0).any(), s
        assert np.array_equal(o['fallback'], c['all_skipped'] | c['nonpositive'])
        live = o['interior'] & ~o['fallback']
        assert len(np.unique(o['visibility'][live & c['ordinary']])) > 5              # the planted (a, b) pairs and mixtures
        assert not _differs(_restated(S, R, mu, w, s, vol=vol), o), s
        assert not _differs(_restated(S, R, mu, w, s, 'skip_c0', vol=vol), o), s
        for mutant in ('g_at_r', 'h_plain', 'v_beta'):
            wrong = _restated(S, R, mu, w, s, mutant, vol=vol)
            assert _differs(wrong, o), (s, mutant)
            with pytest.raises(AssertionError):
                od.compare_exact_df(wrong, o)


def test_near_flat_windows_need_the_relative_test():
    """The near-flat instances of the GPU test: mu_k = 4095 - k and a block of R_k = mu_k - 1, whose windows have
    0 < det <= 1e-12 p.  The contract skips all their candidates (3 x 3 pixels more than the two other skipped blocks), a
    kernel whose skip test reads C == 0 only divides by a det of a few units in the last place and differs."""
    for w, s, K in od.NEAR_FLAT_CASES:
        S, R, mu = od.near_flat_instance(w, s, K)
        E, F, B, C, G, H = od.cost_volume_df(S, R, mu, w, s)
        p = C * H
        det = p - G * G
        tiny = (det > 0) & (det <= od.REL_DET * p)
        c = od.classes_df(S, R, mu, w, s)
        print("w=%d s=%d K=%d: %d pixels with every candidate skipped, %d candidates with 0 < det <= 1e-12 p"
              % (w, s, K, c['all_skipped'].sum(), tiny.sum()))
        assert c['all_skipped'].sum() == 27 and tiny.all(0).sum() == 9
        o = od.umpa_df(S, R, mu, w, s)
        assert not (o['gap'][o['interior']] == 0).any()
        assert not _differs(_restated(S, R, mu, w, s), o)
        wrong = _restated(S, R, mu, w, s, 'skip_c0')
        assert _differs(wrong, o), (w, s)
    assert {ou.tile_width(w) for w, s, K in od.NEAR_FLAT_CASES} == {16, 32}


def test_periodic_references_tie_everywhere():
    """The two tie cases of the GPU test (one per tile width): every interior pixel is an exact tie and none falls back."""
    from tests.test_gpu_umpa_df import TIES
    assert {ou.tile_width(w) for w, s, p in TIES} == {16, 32} and all(t in ou.TIE_CASES for t in TIES)
    for w, s, period in TIES:
        S, R, mu = od.tie_instance(w, s, period)
        o = od.umpa_df(S, R, mu, w, s)
        assert (o['gap'][o['interior']] == 0).all() and not o['fallback'].any(), (w, s)


def test_warped_sweep_excludes_no_pixel():
    """The oracle alone stays inside compare_df()'s cap at every (w, s) of test_umpa_df_every_window_and_search_warped: no
    interior pixel has its two best costs within GAP_MIN.  The planted visibility shows: the half with V = 0.6 has the lower
    median (neither median is the planted value: a displacement between two integer candidates lowers V as a blur does).
    At (1, 7), K = 1, the oracle falls back at 8 pixels through T(u*) <= 0, the nearest |T(u*)| to 0 being 5e-3."""
    ties = 0
    for w, s in ou.PAIRS:
        S, R, mu = od.warped_instance(w, s)
        o = od.umpa_df(S, R, mu, w, s)
        assert max(S[0].shape) <= 100 and o['fallback'].sum() <= 8, (w, s)
        ties += int((o['gap'][o['interior']] < ou.GAP_MIN).sum())
        inner = o['interior']
        h = S[0].shape[1] // 2
        left, right = inner[:, :h - w - s], inner[:, h + w + s:]
        if left.any() and right.any():
            assert np.median(o['visibility'][:, h + w + s:][right]) < 0.8 * np.median(o['visibility'][:, :h - w - s][left]), (w, s)
    assert ties == 0


# ------------------------------------------------------------------------------ argument rules, before any device
def test_argument_errors_before_any_device():
    from paresis_amd import ops
    from paresis_amd._lib import PsxError
    img = lambda K, n=16, m=16: torch.ones((K, n, m), dtype=torch.float32)
    for mean, text in (([1.0], "one value per position"), ([1.0, 2.0, 3.0], "one value per position"),
                       ([1.0, float('nan')], "finite"), ([float('inf'), 1.0], "finite"), (["a", 1.0], "sequence of 2 finite")):
        with pytest.raises(PsxError, match=text):
            ops.umpa_df(img(2), img(2), mean=mean)
    with pytest.raises(PsxError, match="K=0"):
        ops.umpa_df(img(0), img(0))
    for kw in ({'window': 0}, {'search': 9}, {'window': 1.5}):
        with pytest.raises(PsxError, match="integer in"):
            ops.umpa_df(img(1), img(1), **kw)
    with pytest.raises(PsxError, match="smaller than 11x11"):
        ops.umpa_df(img(1, 10, 16), img(1, 10, 16))
    with pytest.raises(PsxError, match="positions"):
        ops.umpa_df(img(2), img(3), mean=[1.0, 2.0])
    with pytest.raises(PsxError, match="out must hold five"):
        ops.umpa_df(img(2), img(2), mean=[1.0, 2.0], out=[torch.empty(16, 16)] * 4)
    with pytest.raises(PsxError, match="HBM"):                            # CPU tensors: no CPU path, with or without means
        ops.umpa_df(img(2), img(2), mean=[1.0, 2.0])
    with pytest.raises(PsxError, match="HBM"):
        ops.umpa_df(img(1), img(1))


def test_method_rules(tmp_path, capsys):
    """'umpa-df' is a method of retrieve(), main.run and both command lines, under the rules of 'umpa'."""
    from paresis_amd import main, retrieval
    assert retrieval.METHODS == ("lcs", "umpa", "umpa-df")
    res = {p: (np.ones((1, 16, 16), np.float32), np.ones((1, 16, 16), np.float32)) for p in range(4)}
    with pytest.raises(ValueError, match="dark_field is an option of method='lcs'"):
        retrieval.retrieve(res, method='umpa-df', dark_field=True)
    with pytest.raises(ValueError, match="max_shift"):
        retrieval.retrieve(res, method='umpa-df', max_shift=1.0)
    with pytest.raises(ValueError, match="at least 1"):
        retrieval.retrieve({}, method='umpa-df')
    with pytest.raises(ValueError, match="mean is an option of dark_field"):
        retrieval.umpa(res[0][0], res[0][1], mean=[1.0])
    out = str(tmp_path / "out")
    for argv, text in ((["--method", "umpa-df"], "--method is an option of --retrieve"),
                       (["--retrieve", "--method", "umpa-df", "--dark-field", "--points", "5"], "options of --method lcs"),
                       (["--retrieve", "--method", "umpa-df", "--max-shift", "2"], "options of --method lcs"),
                       (["--retrieve", "--method", "umpa-df", "--window", "9"], "must be in 1..8")):
        with pytest.raises(SystemExit) as e:
            main.main(argv + ["--out", out])
        assert e.value.code == 2
        assert text in capsys.readouterr().err
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": out + "/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": "RayT", "noise": False}
    with pytest.raises(ValueError, match="dark_field"):
        main.run(dict(ed, nbExpPoints=5), save=False, retrieve=True, method='umpa-df', dark_field=True)
    with pytest.raises(ValueError, match="max_shift"):
        main.run(dict(ed), save=False, retrieve=True, method='umpa-df', max_shift=2.0)
    from tests.test_retrieval_host import _layout
    _layout(tmp_path / "run", "X", [0], ".npy")
    for argv, text in ((["--method", "umpa-df", "--dark-field"], "options of --method lcs"),
                       (["--method", "umpa-df", "--max-shift", "1"], "options of --method lcs"),
                       (["--method", "umpa-df", "--search", "9"], "must be in 1..8")):
        with pytest.raises(SystemExit) as e:
            retrieval.main([str(tmp_path / "run")] + argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err
