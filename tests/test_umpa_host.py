"""UMPA without a GPU: the float64 oracle of the contract (tests/_umpa_oracle.py) against the contract read literally, and
the argument and flag checks that come before any device."""
import numpy as np
import pytest
import torch

from tests import _retrieval_oracle as orl
from tests import _umpa_oracle as ou


def test_oracle_matches_brute_force():
    """21 x 23, K = 2, w = 1, s = 1: the vectorised oracle against plain loops over pixels, candidates and window pixels.  The
    two sum in different orders: 1e-9 px on the displacement (the parabola divides cost differences)."""
    rng = np.random.default_rng(0)
    R = [orl.speckle(21, 23, rng, grain=2.0).astype(np.float32) for _ in range(2)]
    S = [(0.7 * np.roll(np.roll(r, 1, 0), -1, 1)).astype(np.float32) for r in R]
    S[0][8:11, 8:11] += 300.0                                         # not an exact shift everywhere
    o = ou.umpa(S, R, 1, 1)
    t, dx, dy, res = ou.umpa_brute(S, R, 1, 1)
    assert o['interior'].sum() == 17 * 19 and o['gap'][o['interior']].min() > 1e-6
    assert np.abs(o['transmission'] - t).max() <= 1e-6 * 0.7
    assert np.abs(o['dx'] - dx).max() <= 1e-6 and np.abs(o['dy'] - dy).max() <= 1e-6     # float32 rounding of the maps
    assert np.abs(o['residual'] - res).max() <= 1e-7
    inner = o['interior']
    far = inner.copy()
    far[5:14, 5:14] = False
    assert np.all(o['dx'][far] == 1.0) and np.all(o['dy'][far] == -1.0)                  # on the search boundary: exact
    assert np.all(o['transmission'][~inner] == 1.0) and np.all(o['dx'][~inner] == 0.0) and np.all(o['residual'][~inner] == 0.0)
    assert not o['fallback'].any()


def test_oracle_fallback_and_skipped_candidates():
    rng = np.random.default_rng(1)
    R = [orl.speckle(30, 30, rng).astype(np.float32) for _ in range(3)]
    S = [(0.9 * r).astype(np.float32) for r in R]
    for k in range(3):
        R[k][4:16, 4:16] = 0.0
        S[k][16:28, 16:28] = 0.0
    o = ou.umpa(S, R, 1, 1)
    for blk in ((slice(6, 14), slice(6, 14)), (slice(18, 26), slice(18, 26))):
        assert o['fallback'][blk].all()
        for key, v in (('transmission', 1.0), ('dx', 0.0), ('dy', 0.0), ('residual', 0.0)):
            assert np.all(o[key][blk] == v), key
    t, dx, dy, res = ou.umpa_brute(S, R, 1, 1)
    ok = o['gap'] >= ou.GAP_MIN
    assert np.abs(o['dx'] - dx)[ok].max() <= 1e-6 and np.abs(o['transmission'] - t)[ok].max() <= 1e-6


def test_warped_model_is_beyond_lcs():
    """The generator of the GPU tests gives displacements of several pixels that the oracle tracks and LCS does not."""
    T, Dx, Dy, S, R = ou.warped_model(64, 60, 4, seed=3, dmax=3.0)
    o = ou.umpa(S, R, 2, 3)
    big = o['interior'] & ((np.abs(Dx) > 1.5) | (np.abs(Dy) > 1.5))
    assert big.sum() > 100
    err = np.hypot(o['dx'] - Dx, o['dy'] - Dy)[big]
    lcs = orl.lcs(S, R)
    err_lcs = np.hypot(lcs['dx'] - Dx, lcs['dy'] - Dy)[big]
    print("warped 64x60: median error umpa %.3f px, lcs %.3f px" % (np.median(err), np.median(err_lcs)))
    assert np.median(err) <= 0.15 and np.median(err_lcs) >= 0.5


def test_argument_errors_before_any_device():
    from paresis_amd import ops
    from paresis_amd._lib import PsxError
    img = lambda K, n=16, m=16: torch.ones((K, n, m), dtype=torch.float32)
    with pytest.raises(PsxError, match="K=0"):
        ops.umpa(img(0), img(0))
    with pytest.raises(PsxError, match="K=65"):
        ops.umpa(img(65), img(65))
    for kw in ({'window': 0}, {'window': 9}, {'search': 0}, {'search': 9}, {'window': 1.5}):
        with pytest.raises(PsxError, match="integer in"):
            ops.umpa(img(1), img(1), **kw)
    with pytest.raises(PsxError, match="smaller than 11x11"):
        ops.umpa(img(1, 10, 16), img(1, 10, 16))
    with pytest.raises(PsxError, match="smaller than 7x7"):
        ops.umpa(img(1, 16, 6), img(1, 16, 6), window=1, search=2)
    with pytest.raises(PsxError, match="shape"):
        ops.umpa(img(2), img(2, 16, 17))
    with pytest.raises(PsxError, match="positions"):
        ops.umpa(img(2), img(3))
    with pytest.raises(PsxError, match="HBM"):                            # CPU tensors: no CPU path
        ops.umpa(img(1), img(1))


def test_retrieve_method_rules():
    from paresis_amd import retrieval
    res = {p: (np.ones((1, 16, 16), np.float32), np.ones((1, 16, 16), np.float32)) for p in range(4)}
    with pytest.raises(ValueError, match="dark-field"):
        retrieval.retrieve(res, method='umpa', dark_field=True)
    with pytest.raises(ValueError, match="max_shift"):
        retrieval.retrieve(res, method='umpa', max_shift=1.0)
    with pytest.raises(ValueError, match="method must be"):
        retrieval.retrieve(res, method='xst')
    with pytest.raises(ValueError, match="at least 3"):                   # the default method keeps its rule
        retrieval.retrieve({0: res[0]})
    with pytest.raises(ValueError, match="at least 1"):
        retrieval.retrieve({}, method='umpa')


def test_method_flag_rules(tmp_path, capsys):
    """main.py and the retrieval CLI: --method umpa needs --retrieve, excludes --dark-field and --max-shift, bounds --window and
    --search; main.run the same; all before any device."""
    from paresis_amd import main, retrieval
    out = str(tmp_path / "out")
    for argv, text in ((["--method", "umpa"], "--method is an option of --retrieve"),
                       (["--retrieve", "--method", "umpa", "--dark-field", "--points", "5"], "options of --method lcs"),
                       (["--retrieve", "--method", "umpa", "--max-shift", "2"], "options of --method lcs"),
                       (["--retrieve", "--method", "umpa", "--window", "9"], "must be in 1..8"),
                       (["--retrieve", "--method", "umpa", "--search", "0"], "must be in 1..8"),
                       (["--retrieve", "--method", "xst"], "invalid choice"),
                       (["--retrieve", "--method", "lcs", "--points", "2"], "--retrieve needs --points 3 or more")):
        with pytest.raises(SystemExit) as e:
            main.main(argv + ["--out", out])
        assert e.value.code == 2
        assert text in capsys.readouterr().err
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": out + "/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": "RayT", "noise": False}
    with pytest.raises(ValueError, match="dark-field"):
        main.run(dict(ed, nbExpPoints=5), save=False, retrieve=True, method='umpa', dark_field=True)
    with pytest.raises(ValueError, match="max_shift"):
        main.run(dict(ed), save=False, retrieve=True, method='umpa', max_shift=2.0)
    with pytest.raises(ValueError, match="at least 3"):
        main.run(dict(ed), save=False, retrieve=True)
    from tests.test_retrieval_host import _layout
    _layout(tmp_path / "run", "X", [0], ".npy")
    for argv, text in ((["--method", "umpa", "--dark-field"], "options of --method lcs"),
                       (["--method", "umpa", "--max-shift", "1"], "options of --method lcs"),
                       (["--method", "umpa", "--search", "9"], "must be in 1..8")):
        with pytest.raises(SystemExit) as e:
            retrieval.main([str(tmp_path / "run")] + argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err
    assert len(retrieval.discover(str(tmp_path / "run"), min_positions=1)[0][3]) == 1
    with pytest.raises(ValueError, match="at least 3"):
        retrieval.discover(str(tmp_path / "run"))


# ------------------------------------------------------------------------------ exact comparison on integer images
# On images of small integers E, B, C are exact in float64 whatever the order of summation, and the contract fixes every later
# operation, so the oracle, the literal loops and a correct kernel agree bit for bit (tests/test_gpu_umpa.py compares the
# kernel).  Below: that the two CPU readings do agree, that the GPU sweep's inputs hold every class of pixel, and that
# kernels wrong in five specific ways would each change an output value on them.
def _chunk(s):
    """Candidates per chunk of a row of 2s+1 candidates b (csrc/umpa.hip): as few chunks of at most 7 as hold them, all of
    one length; one surplus candidate b = s+1 where that overshoots."""
    nch = -(-(2 * s + 1) // 7)
    return -(-(2 * s + 1) // nch), nch


def test_chunk_lengths_as_described():
    assert [_chunk(s) for s in range(1, 9)] == [(3, 1), (5, 1), (7, 1), (5, 2), (6, 2), (7, 2), (5, 3), (6, 3)]
    assert [s for s in range(1, 9) if _chunk(s)[0] * _chunk(s)[1] > 2 * s + 1] == [4, 5, 6, 8]


def _scan(E, B, C, alist, blist, s, mutant=None):
    """The contract as a scan in the kernel's manner, vectorised over pixels: candidates a outer, b inner, a running strict
    minimum that carries its four parabola neighbours, NaN for a skipped or absent one.  B, C: [len(alist), len(blist), ni,
    mi].  `mutant` restates one wrong kernel: 'last' keeps the last of equal minima; 'c_at_r' takes C at r instead of r - u;
    'skip_as_E' gives a skipped candidate the cost E instead of skipping it; 'chunk' forgets the b-1 neighbour at the first
    candidate of every chunk.  -> the four float32 maps of the interior."""
    nan = np.full(E.shape, np.nan)
    bestL, bestT = np.full(E.shape, np.inf), np.zeros(E.shape)
    ba, bb = np.full(E.shape, -100), np.full(E.shape, -100)
    Lam, Lap, Lbm, Lbp = nan.copy(), nan.copy(), nan.copy(), nan.copy()
    prev = [nan.copy() for _ in blist]
    nb = _chunk(s)[0]
    for ia, a in enumerate(alist):
        last = nan.copy()
        for ib, b in enumerate(blist):
            Cv = C[list(alist).index(0), list(blist).index(0)] if mutant == 'c_at_r' else C[ia, ib]
            ok = Cv != 0
            Cs = np.where(ok, Cv, 1.0)
            Lc = np.where(ok, E - B[ia, ib] * B[ia, ib] / Cs, E if mutant == 'skip_as_E' else np.nan)
            Tc = np.where(ok, B[ia, ib] / Cs, 0.0)
            if mutant == 'chunk' and ib % nb == 0:
                last = nan.copy()
            Lap = np.where((ba == a - 1) & (bb == b), Lc, Lap)
            Lbp = np.where((ba == a) & (bb == b - 1), Lc, Lbp)
            with np.errstate(invalid='ignore'):
                new = (Lc <= bestL) if mutant == 'last' else (Lc < bestL)
            bestL, bestT = np.where(new, Lc, bestL), np.where(new, Tc, bestT)
            ba, bb = np.where(new, a, ba), np.where(new, b, bb)
            Lam, Lbm = np.where(new, prev[ib], Lam), np.where(new, last, Lbm)
            Lap, Lbp = np.where(new, np.nan, Lap), np.where(new, np.nan, Lbp)
            prev[ib] = Lc
            last = Lc

    def refine(Lm, Lp):
        with np.errstate(invalid='ignore', divide='ignore'):
            den = Lm - 2.0 * bestL + Lp
            ok = ~np.isnan(Lm) & ~np.isnan(Lp) & (den > 0)
            return np.where(ok, np.clip(0.5 * (Lm - Lp) / np.where(ok, den, 1.0), -0.5, 0.5), 0.0)

    live = (ba != -100) & (bestT > 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        vals = (np.where(live, bestT, 1.0), np.where(live, ba + refine(Lam, Lap), 0.0),
                np.where(live, bb + refine(Lbm, Lbp), 0.0), np.where(live, np.maximum(bestL, 0) / E, 0.0))
    return [v.astype(np.float32) for v in vals]


def _restated(S, R, w, s, mutant=None):
    """{'transmission', 'dx', 'dy', 'residual'} of the scan, whole images.  'surplus' admits the candidate b = s+1: a cost volume
    of half-width s+1, cropped to |a| <= s and b >= -s; it exists one pixel further from the border, and the ring in
    between keeps the oracle's values."""
    n, m = S[0].shape
    nc = 2 * s + 1
    band = w + s
    fills = dict(zip(ou.KEYS, (1.0, 0.0, 0.0, 0.0)))
    out = {k: np.full((n, m), fills[k], np.float32) for k in ou.KEYS}
    if mutant == 'surplus':
        o = ou.umpa(S, R, w, s)
        out = {k: o[k].copy() for k in ou.KEYS}
        E, B, C = ou.cost_volume(S, R, w, s + 1)
        B, C = (X.reshape((nc + 2, nc + 2) + E.shape)[1:-1, 1:] for X in (B, C))
        vals = _scan(E, B, C, range(-s, s + 1), range(-s, s + 2), s)
        band += 1
    else:
        E, B, C = ou.cost_volume(S, R, w, s)
        B, C = (X.reshape((nc, nc) + E.shape) for X in (B, C))
        vals = _scan(E, B, C, range(-s, s + 1), range(-s, s + 1), s, mutant)
    for k, v in zip(ou.KEYS, vals):
        out[k][band:n - band, band:m - band] = v
    return out


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ou.KEYS)


def test_oracle_is_exact_on_integer_images():
    """umpa() == umpa_brute() bit for bit on all four maps: 25 x 43, K = 2, w = 1, s = 2 with both planted blocks (all-skipped,
    partly skipped and T <= 0 pixels among them), and a periodic instance in which every interior pixel is an exact tie."""
    for w, s, K, period in ((1, 2, 2, None), (2, 2, 1, (2, 3))):
        S, R = ou.integer_model(w, s, K, seed=5, period=period, shape=None if period is None else (15, 17))
        o = ou.umpa(S, R, w, s)
        assert o['fallback'].any() == (period is None)
        assert (o['gap'][o['interior']] == 0).all() == (period is not None)
        brute = ou.umpa_brute(S, R, w, s)
        for key, b in zip(ou.KEYS, brute):
            assert np.array_equal(o[key], b.astype(np.float32)), key
        ou.compare_exact(o, o, ties=period is not None, label="oracle on itself")
        with pytest.raises(AssertionError):
            wrong = {k: o[k].copy() for k in ou.KEYS}
            wrong['dy'][w + s, w + s] = np.nextafter(wrong['dy'][w + s, w + s], np.float32(9))
            ou.compare_exact(wrong, o, ties=True)
    with pytest.raises(AssertionError, match="exact ties"):
        ou.compare_exact(o, o)


@pytest.mark.parametrize("w", range(1, 9))
def test_integer_sweep_holds_every_class_and_wrong_kernels_show(w):
    """For s = 1..8 at this w, on the very inputs of test_umpa_every_window_and_search_exact: all-skipped pixels, partly
    skipped pixels whose best candidate lacks a parabola neighbour, T <= 0 pixels, ordinary pixels in two tile rows and two
    tile columns, no exact tie; the scan restatement equals the oracle bit for bit, and each wrong kernel that applies at
    (w, s) changes at least one output value."""
    for s in range(1, 9):
        S, R = ou.sweep_instance(w, s)
        n, m = S[0].shape
        assert max(n, m) <= 100 and n % ou.TILE_H and m % ou.tile_width(w)
        o = ou.umpa(S, R, w, s)
        c = ou.classes(S, R, w, s)
        count = {k: int(c[k].sum()) for k in c if c[k].dtype == bool}
        print("w=%d s=%d K=%d %dx%d: %s" % (w, s, len(S), n, m, count))
        assert count['all_skipped'] == 9 and count['lacks_neighbour'] >= 1 and count['nonpositive'] >= 1, (s, count)
        assert len(set(c['tile_row'][c['ordinary']])) >= 2 and len(set(c['tile_col'][c['ordinary']])) >= 2, s
        assert sum(count[k] for k in ('all_skipped', 'some_skipped', 'ordinary')) \
            + int((c['nonpositive'] & ~c['some_skipped']).sum()) == o['interior'].sum()
        assert not (o['gap'][o['interior']] == 0).any(), s
        assert np.array_equal(o['fallback'], c['all_skipped'] | c['nonpositive'])
        assert not _differs(_restated(S, R, w, s), o), s
        mutants = ['c_at_r', 'skip_as_E'] + (['chunk'] if s >= 4 else []) + (['surplus'] if s in (4, 5, 6, 8) else [])
        for mu in mutants:
            wrong = _restated(S, R, w, s, mu)
            assert _differs(wrong, o), (s, mu)
            with pytest.raises(AssertionError):
                ou.compare_exact(wrong, o)


def test_periodic_references_tie_everywhere_and_the_last_minimum_shows():
    """The inputs of test_umpa_ties_take_the_first_minimum: every interior pixel is an exact tie, first minima lie strictly
    inside the search range, and a kernel keeping the last of equal minima differs from the oracle at every interior pixel."""
    for w, s, period in ou.TIE_CASES:
        S, R = ou.tie_instance(w, s, period)
        o = ou.umpa(S, R, w, s)
        inner = o['interior']
        assert (o['gap'][inner] == 0).all() and not o['fallback'].any(), (w, s)
        inside = inner & (np.abs(o['a']) < s) & (np.abs(o['b']) < s)
        moved = inside & ((o['dx'] != o['a']) | (o['dy'] != o['b']))         # a parabola term that is not zero
        print("w=%d s=%d period %s: %d tie pixels, %d with u* inside the range on both axes, %d of them refined"
              % (w, s, period, inner.sum(), inside.sum(), moved.sum()))
        assert inside.sum() >= 10, (w, s)
        # along an axis of period 2 the two neighbours are the same candidate, Lm == Lp, and the term is exactly 0
        assert moved.sum() >= 10 or period == (2, 2), (w, s)
        assert not _differs(_restated(S, R, w, s), o), (w, s)
        wrong = _restated(S, R, w, s, 'last')
        assert (wrong['dx'] != o['dx'])[inner].all() or (wrong['dy'] != o['dy'])[inner].all(), (w, s)
        with pytest.raises(AssertionError):
            ou.compare_exact(wrong, o, ties=True)
    assert {ou.tile_width(w) for w, s, p in ou.TIE_CASES} == {16, 32}
    assert {_chunk(s)[1] for w, s, p in ou.TIE_CASES} == {1, 2, 3} and any(s in (4, 5, 6) for w, s, p in ou.TIE_CASES)


def test_last_minimum_passes_the_tolerance_rule():
    """Why the exact comparison: a kernel that keeps the last of equal minima passes compare() on the warped inputs of every
    shape of test_umpa_matches_oracle (float data never ties exactly)."""
    from tests.test_gpu_umpa import SHAPES, _warped
    for n, m, K, w, s, dmax in SHAPES:
        S, R = _warped(n, m, K, dmax)[3:]
        f = ou.compare(_restated(S, R, w, s, 'last'), ou.umpa(S, R, w, s), w, s, label="last minimum, %dx%d" % (n, m))
        assert f['ties'] == 0 and f['compared'] > 0


def test_warped_sweep_excludes_no_pixel():
    """The oracle alone stays inside compare()'s cap at every (w, s) of test_umpa_every_window_and_search_warped: no interior
    pixel has its two best costs within GAP_MIN."""
    ties = 0
    for w, s in ou.PAIRS:
        S, R = ou.warped_instance(w, s)
        o = ou.umpa(S, R, w, s)
        assert max(S[0].shape) <= 100 and not o['fallback'].any(), (w, s)
        ties += int((o['gap'][o['interior']] < ou.GAP_MIN).sum())
    assert ties == 0
