"""UMPA's dark-field term on the GPU (csrc/umpa.hip: k_umpa<TW, S, true>; ops.umpa_df, retrieval.umpa(dark_field=True) /
retrieve(method='umpa-df'), main.py --method umpa-df) against the float64 numpy oracle of tests/_umpa_df_oracle.py: bit for
bit on integer images at every (window, search), under compare_df()'s rule on float images."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import _umpa_df_oracle as od
from tests import _umpa_oracle as ou

pytestmark = pytest.mark.gpu

TIES = [(2, 3, (2, 3)), (8, 5, (4, 5))]                              # of _umpa_oracle.TIE_CASES: tile width 32 and 16


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _gpu(S, R, mu, w, s):
    from paresis_amd import retrieval
    r = retrieval.umpa(_cuda(np.stack(S)), _cuda(np.stack(R)), window=w, search=s, dark_field=True,
                       mean=None if mu is None else list(mu))
    assert sorted(r) == sorted(od.KEYS)
    return {k: _np(v) for k, v in r.items()}


# The host picks one of 16 dark-field kernels and an LDS layout with the second map Gb; the prologue's rows per thread, the
# chunks of a candidate row and the surplus candidate vary with (w, s): all 64 pairs run.  On integer images the contract's
# sums are exact and every later step is one IEEE operation, so the five maps are compared with np.array_equal over the
# whole image: a contracted fma anywhere in the 2 x 2 solve would show.  tests/test_umpa_df_host.py shows what these inputs hold.
@pytest.mark.parametrize("w,s", ou.PAIRS)
def test_umpa_df_every_window_and_search_exact(w, s):
    S, R, mu = od.sweep_instance(w, s)
    o = od.umpa_df(S, R, mu, w, s)
    assert o['fallback'].sum() > 18                                  # the two all-skipped blocks and the T <= 0 block
    od.compare_exact_df(_gpu(S, R, mu, w, s), o, label="w=%d s=%d K=%d %dx%d" % ((w, s, len(S)) + S[0].shape))


@pytest.mark.parametrize("w,s", [(4, 8), (5, 1), (8, 7)])
def test_umpa_df_many_positions_exact(w, s):
    """K = 64 (the most) and 63: E <= 64 * 17^2 * 16387^2 = 5.0e12 at w = 8, exact in float64."""
    for K in (64, 63):
        S, R, mu = od.integer_df_model(w, s, K, seed=5000 + K)
        od.compare_exact_df(_gpu(S, R, mu, w, s), od.umpa_df(S, R, mu, w, s), label="w=%d s=%d K=%d" % (w, s, K))


@pytest.mark.parametrize("w,s,period", TIES)
def test_umpa_df_ties_take_the_first_minimum(w, s, period):
    S, R, mu = od.tie_instance(w, s, period)
    o = od.umpa_df(S, R, mu, w, s)
    f = od.compare_exact_df(_gpu(S, R, mu, w, s), o, ties=True, label="period %s w=%d s=%d" % (period, w, s))
    assert f['ties'] == f['interior'] > 0


@pytest.mark.parametrize("w,s,K", od.NEAR_FLAT_CASES)
def test_umpa_df_near_flat_windows_are_skipped(w, s, K):
    """Windows with 0 < det <= 1e-12 p (tests/test_umpa_df_host.py): only the relative skip test gives the oracle's maps."""
    S, R, mu = od.near_flat_instance(w, s, K)
    o = od.umpa_df(S, R, mu, w, s)
    od.compare_exact_df(_gpu(S, R, mu, w, s), o, label="near flat w=%d s=%d K=%d" % (w, s, K))


@pytest.mark.parametrize("w,s", ou.PAIRS)
def test_umpa_df_every_window_and_search_warped(w, s):
    """Float images with displacements up to about s - 1/2 and V = 0.6 in half the image, under compare()'s rule on T, dx, dy
    and the residual plus |dV| <= 1e-5; cap 1e-4 on excluded near-ties (the oracle alone excludes none:
    tests/test_umpa_df_host.py)."""
    S, R, mu = od.warped_instance(w, s)
    f = od.compare_df(_gpu(S, R, mu, w, s), od.umpa_df(S, R, mu, w, s), w, s, label="warped %dx%d K=%d" % (S[0].shape + (len(S),)))
    assert f['compared'] > 0


@pytest.mark.parametrize("w,s", ou.PAIRS)
def test_umpa_df_smallest_image(w, s):
    """2(w+s)+1 on a side: one interior pixel."""
    q = 2 * (w + s) + 1
    S, R, mu = od.integer_df_model(w, s, ou.sweep_K(w, s), seed=4000 + 100 * w + s, shape=(q, q))
    o = od.umpa_df(S, R, mu, w, s)
    assert o['interior'].sum() == 1
    od.compare_exact_df(_gpu(S, R, mu, w, s), o, label="w=%d s=%d %dx%d" % (w, s, q, q))


def test_umpa_df_means_streams_and_no_allocation_on_reuse():
    from paresis_amd import ops
    S, R, mu = od.warped_instance(2, 3)
    K = len(S)
    St, Rt = _cuda(np.stack(S)), _cuda(np.stack(R))
    a = ops.umpa_df(St, Rt, mean=list(mu))
    assert len(a) == 5
    # mean=None: the float64 device mean of float32 images is the host's to a few units in the last place
    b = ops.umpa_df(St, Rt)
    dev_mu = np.array([float(Rt[k].mean(dtype=torch.float64)) for k in range(K)])
    assert np.abs(dev_mu - mu).max() <= 1e-12 * np.abs(mu).max()
    c = ops.umpa_df(St, Rt, mean=list(dev_mu))
    for u, v in zip(b, c):
        assert torch.equal(u, v)
    od.compare_df({k: _np(v) for k, v in zip(od.KEYS, b)}, od.umpa_df(S, R, mu, 2, 3), 2, 3, label="mean=None")
    d = ops.umpa_df([St[k].clone() for k in range(K)], [Rt[k].clone() for k in range(K)], mean=tuple(mu))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e = ops.umpa_df(St, Rt, mean=list(mu))
    torch.cuda.current_stream().wait_stream(side)
    for x in (d, e):
        for u, v in zip(a, x):
            assert torch.equal(u, v)
    # the four maps it shares with ops.umpa differ from it where V != 1, and ops.umpa is unchanged by having run it
    plain = ops.umpa(St, Rt)
    assert not torch.equal(plain[0], a[0])
    outs = tuple(torch.full_like(a[0], 7.0) for _ in range(5))
    got = ops.umpa_df(St, Rt, mean=list(mu), out=outs)
    torch.cuda.synchronize()
    assert all(x is y for x, y in zip(got, outs))
    mem = torch.cuda.memory_allocated()
    ops.umpa_df(St, Rt, mean=list(mu), out=outs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    for u, v in zip(a, outs):
        assert torch.equal(u, v)
    for u, v in zip(plain, ops.umpa(St, Rt)):
        assert torch.equal(u, v)


def test_umpa_df_argument_errors():
    from paresis_amd import ops
    from paresis_amd._lib import PsxError
    img = lambda K, n=16, m=16, dt=torch.float32: torch.ones((K, n, m), dtype=dt, device="cuda")
    with pytest.raises(PsxError, match="one value per position"):
        ops.umpa_df(img(2), img(2), mean=[1.0])
    with pytest.raises(PsxError, match="finite"):
        ops.umpa_df(img(2), img(2), mean=[1.0, float('nan')])
    with pytest.raises(PsxError, match="float32"):
        ops.umpa_df(img(2, dt=torch.float64), img(2, dt=torch.float64))
    with pytest.raises(PsxError, match="out must hold five"):
        ops.umpa_df(img(2), img(2), out=[torch.empty(16, 16, device="cuda")] * 4)
    # the C entry point checks for itself
    import ctypes
    lib = ops.lib()
    x, o = img(1), torch.empty(16, 16, device="cuda")
    ptr = (ctypes.c_void_p * 1)(x.data_ptr())
    po = ctypes.c_void_p(o.data_ptr())
    mu = (ctypes.c_double * 1)(1.0)
    for K, n, w, s in ((0, 16, 2, 3), (65, 16, 2, 3), (1, 16, 0, 3), (1, 16, 9, 3), (1, 16, 2, 0), (1, 16, 2, 9), (1, 10, 2, 3)):
        assert lib.psx_umpa_df_f32(ptr, ptr, mu, K, n, 16, w, s, po, po, po, po, po, None) != 0, (K, n, w, s)
        assert b"psx_umpa_df_f32" in lib.psx_last_error()
    assert lib.psx_umpa_df_f32(ptr, ptr, None, 1, 16, 16, 2, 3, po, po, po, po, po, None) != 0
    assert lib.psx_umpa_df_f32(ptr, ptr, (ctypes.c_double * 1)(float('inf')), 1, 16, 16, 2, 3, po, po, po, po, po, None) != 0
    assert b"not finite" in lib.psx_last_error()
    assert lib.psx_umpa_df_f32(ptr, ptr, mu, 1, 16, 16, 2, 3, po, po, po, None, po, None) != 0
    # a constant reference is proportional to its mean: every candidate skipped, the fallback everywhere
    t, dx, dy, v, r = ops.umpa_df(img(2), img(2), mean=[1.0, 1.0])
    assert bool((t == 1).all() and (dx == 0).all() and (dy == 0).all() and (v == 1).all() and (r == 0).all())


def _run(K, tmp_path, name, **kw):
    from paresis_amd import main
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": str(tmp_path) + "/" + name + "/", "overSampling": 2,
          "nbExpPoints": K, "simulation_type": "RayT", "noise": False, "seed": 3}
    os.makedirs(ed["filepath"], exist_ok=True)
    return ed, main.run(ed, **kw)


def test_main_retrieve_umpa_df_writes_maps(tmp_path):
    from paresis_amd import retrieval
    from paresis_amd.InputOutput.pagailleIO import openImage
    ed, res = _run(3, tmp_path, "three", save=True, saving_format=".tif", retrieve=True, method='umpa-df')
    files = sorted(glob.glob(ed["filepath"] + "*/retrieval/*.tif"))
    name = lambda f: os.path.basename(f).split("_")[0]
    assert sorted(name(f) for f in files) == ["dx", "dy", "phi", "residual", "transmission", "visibility"], files
    maps = {name(f): openImage(f) for f in files}
    S = [_np(res[p][0])[0] for p in sorted(res)]
    R = [_np(res[p][1])[0] for p in sorted(res)]
    mu = [float(r.astype(np.float64).mean()) for r in R]
    o = od.umpa_df(S, R, mu, 2, 3)
    od.compare_df({k: np.asarray(maps[k], dtype=np.float32) for k in od.KEYS}, o, 2, 3, label="the chain's images")
    assert np.isfinite(maps['phi']).all() and np.abs(maps['phi']).max() > 0
    got = retrieval.retrieve(res, ed['retrievalParams'], method='umpa-df')[0]
    assert set(got) == {'transmission', 'dx', 'dy', 'visibility', 'residual', 'phi'}
    for k in od.KEYS:
        assert np.array_equal(_np(got[k]), maps[k]), k
    # the CLI on the run's directory writes the same bytes
    run_dir = os.path.dirname(os.path.dirname(files[0]))
    p = ed['retrievalParams']
    before = {f: open(f, "rb").read() for f in files}
    for f in files:
        os.remove(f)
    retrieval.main([run_dir, "--method", "umpa-df", "--energy", repr(p['energy_keV']), "--pixel-um", repr(p['pixel_um']),
                    "--distance", repr(p['distance_m']), "--magnification", repr(p['magnification'])])
    for f in files:
        assert open(f, "rb").read() == before[f], f


# --------------------------------------------------------------------------------------------------------- end to end
# The Lung cylinder of tests/_retrieval_df_e2e.py (radius 250 um at 30 degrees, delta 1e-7, beta 1e-10 at 52 keV; ray tracing,
# 12 positions, ov = 2, mono, no noise; theta <= 1.93e-6 rad, a re-splat of sigma <= 0.58 detector px).  CPU calibration, as
# for LCS-DF: oracle.compute_rt (fastRefractionDF) over 12 positions -- shifted copies of one synthetic sphere membrane --
# then the numpy oracle umpa_df at w = 2, s = 3 with the float64 means of the reference images (the oracle LCS-DF of the same
# images reproduces that test's calibration: corr 0.582, slope 0.528):
#   median 1 - V inside the sample (dfe.masks' inside set, 16494 px) 0.338; empty field (11865 px) 1 - V = 0 exactly at every
#   pixel (S == R there: u = 0 fits with alpha = 1, beta = 0); Pearson correlation of 1 - V with df_truth on the inside set
#   0.682 (LCS-DF's df: 0.582), with the transposed truth 0.018; Fil_Nylon_ID17 control: median |1 - V| inside the wire
#   (33581 px) 0.0147 = 0.044 of the Lung run's.
# Asserted: correlation >= 0.45 (two thirds of 0.682) and above the transposed truth's; median 1 - V inside >= 0.17 (half the
# calibration: the signal is there and positive); empty field median |1 - V| <= 0.02 of the inside median and max |1 - V| <=
# 1e-6 (V = 1 to the float32 rounding of the map, 6e-8); control <= 0.2 of the Lung run (4.5 x the calibration).  1 - V is not
# converted to an angle, so no slope is asserted.
VIS_MIN_CORR = 0.45
VIS_MIN_INSIDE = 0.17
VIS_EMPTY_FRACTION = 0.02
VIS_EMPTY_MAX = 1e-6
VIS_CONTROL_FRACTION = 0.2


def _e2e_run(name, root, xml_dir):
    from paresis_amd import main
    ed = {"experimentName": name, "filepath": str(root) + "/" + name + "/", "overSampling": 2, "nbExpPoints": 12,
          "simulation_type": "RayT", "noise": False, "seed": 3, "xmlDir": xml_dir}
    os.makedirs(ed["filepath"], exist_ok=True)
    return ed, main.run(ed, save=False, retrieve=True, method='umpa-df')


@pytest.fixture(scope="module")
def lung_visibility(tmp_path_factory):
    """The Lung run retrieved with method='umpa-df': 1 - V, the truth df_true and the masks (inside, empty field)."""
    from paresis_amd import retrieval
    from paresis_amd.Experiment import Experiment
    from tests import _retrieval_df_e2e as dfe
    root = tmp_path_factory.mktemp("lung_umpa")
    xml_dir = dfe.write_xml(str(root / "xml"))
    with dfe.lung_material():
        ed, res = _e2e_run(dfe.EXPERIMENT, root, xml_dir)
        exp = Experiment(dict(ed, filepath=str(root) + "/probe/"))
        h = float(exp.exp_dict['studyPixelSize']) * 1e-6
        flux = sum(f for _, f in exp.mySource.mySpectrum)
    params = ed['retrievalParams']
    out = retrieval.retrieve(res, params, method='umpa-df')[0]
    theta = _np(res[0][6]) / flux
    df_t, th_t = dfe.df_truth(theta, params['distance_m'], h, params['magnification'], ed['overSampling'])
    inside, far = dfe.masks(_np(res[0][4]), _np(res[0][5]), th_t, theta.shape)
    return 1.0 - _np(out['visibility']).astype(np.float64), df_t, inside, far


def test_end_to_end_visibility(lung_visibility):
    from tests import _retrieval_df_e2e as dfe
    d, df_t, inside, far = lung_visibility
    med_in, med_far, max_far = np.median(d[inside]), np.median(np.abs(d[far])), np.abs(d[far]).max()
    corr = dfe.e2e.figures(d, df_t, inside)[0]
    corr_t = dfe.e2e.figures(d.T, df_t, inside.T)[0]
    print("e2e visibility: inside %d px median 1-V %.4f; empty %d px median |1-V| %.3e max %.3e; corr %.3f, transposed %.3f"
          % (inside.sum(), med_in, far.sum(), med_far, max_far, corr, corr_t))
    assert inside.sum() > 2000 and far.sum() > 2000
    assert corr >= VIS_MIN_CORR and corr_t < corr
    assert med_in >= VIS_MIN_INSIDE
    assert med_far <= VIS_EMPTY_FRACTION * med_in
    assert max_far <= VIS_EMPTY_MAX


def test_non_scattering_control_visibility(tmp_path, lung_visibility):
    from paresis_amd import retrieval
    from paresis_amd.Experiment import Experiment
    from tests import _retrieval_df_e2e as dfe
    d_l, _, inside_l, _ = lung_visibility
    lung_med = float(np.median(np.abs(d_l[inside_l])))
    ed, res = _e2e_run("Fil_Nylon_ID17", tmp_path, None)
    out = retrieval.retrieve(res, ed['retrievalParams'], method='umpa-df')[0]
    exp = Experiment(dict(ed, filepath=str(tmp_path) + "/probe/"))
    T = _np(exp.mySampleofInterest.myGeometry)[0]
    inside, _ = dfe.masks(_np(res[0][4]), _np(res[0][5]), dfe.e2e.bin2(T), T.shape)
    med = float(np.median(np.abs(1.0 - _np(out['visibility']).astype(np.float64))[inside]))
    print("control: median |1-V| in the wire %.4f, Lung run %.4f (ratio %.3f), mask %d" % (med, lung_med, med / lung_med,
                                                                                         int(inside.sum())))
    assert inside.sum() > 2000
    assert med <= VIS_CONTROL_FRACTION * lung_med
