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
