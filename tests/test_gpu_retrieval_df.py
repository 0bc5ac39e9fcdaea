"""Dark-field retrieval on the GPU (csrc/retrieve.hip k_lcs_df, ops.lcs_df, retrieval.lcs / retrieve(dark_field=True),
main.py --retrieve --dark-field) against the float64 oracle of tests/_retrieval_df_oracle.py, and end to end against the
ray-tracing chain's own dark-field map (tests/_retrieval_df_e2e.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import _retrieval_df_e2e as dfe
from tests import _retrieval_df_oracle as odf
from tests import _retrieval_oracle as orl

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _inputs(n, m, K, seed, dmax=0.5, dfmax=0.3):
    """float32 S_k, R_k of the exact model (T in [0.6, 1], |D| <= dmax, Df in (0, dfmax])."""
    T, Dx, Dy, Df, S, R = odf.exact_model(n, m, K, seed=seed, dmax=dmax, dfmax=dfmax)
    return T, Dx, Dy, Df, [s.astype(np.float32) for s in S], R


def _gpu_lcs_df(S, R, max_shift=None):
    from paresis_amd import retrieval
    r = retrieval.lcs(_cuda(np.stack(S)), _cuda(np.stack(R)), max_shift=max_shift, dark_field=True)
    return {k: _np(v) for k, v in r.items()}


@pytest.mark.parametrize("n,m,K", [(200, 200, 4), (301, 173, 64), (3, 3, 7), (2048, 2048, 7)])
def test_lcs_df_matches_oracle(n, m, K):
    T, Dx, Dy, Df, S, R = _inputs(n, m, K, seed=n + m + K)
    g = _gpu_lcs_df(S, R)
    o = odf.lcs_df(S, R, return_mask=True)
    fb = o['fallback']
    gfb = (g['transmission'] == 1.0) & (g['dx'] == 0.0) & (g['dy'] == 0.0) & (g['df'] == 0.0)
    assert np.array_equal(gfb, fb), (int(gfb.sum()), int(fb.sum()))
    ok = ~fb
    dmax = max(np.abs(o['dx'])[ok].max(), np.abs(o['dy'])[ok].max())
    fmax = np.abs(o['df'])[ok].max()
    ex = np.abs(g['dx'] - o['dx'])[ok].max()
    ey = np.abs(g['dy'] - o['dy'])[ok].max()
    ef = np.abs(g['df'] - o['df'])[ok].max()
    et = (np.abs(g['transmission'] - o['transmission']) / np.abs(o['transmission']))[ok].max()
    print("lcs_df %dx%d K=%d: fallback %d, |ddx| %.2e |ddy| %.2e (max|D| %.3f), |ddf| %.2e (max|df| %.3f), rel dT %.2e"
          % (n, m, K, int(fb.sum()), ex, ey, dmax, ef, fmax, et))
    assert ex <= 1e-5 * dmax and ey <= 1e-5 * dmax and ef <= 1e-5 * fmax and et <= 1e-5


def test_lcs_df_exact_model_known_answer():
    """As test_lcs_exact_model_known_answer, with df: the float64 oracle on the SAME float32 inputs measures the displacement
    E_round that rounding S_k to float32 causes; |GPU - truth| <= 2*E_round + 1e-6 (the output's own float32 rounding)."""
    T, Dx, Dy, Df, S, R = _inputs(256, 192, 9, seed=11)
    g = _gpu_lcs_df(S, R)
    o = odf.lcs_df(S, R, dtype=np.float64, return_mask=True)
    ok = ~o['fallback']
    assert int(o['fallback'].sum()) == 4                      # the corners: L = g0 + g1 there
    for key, truth, scale in (('transmission', T, np.abs(T).max()), ('dx', Dx, max(np.abs(Dx).max(), np.abs(Dy).max())),
                              ('dy', Dy, max(np.abs(Dx).max(), np.abs(Dy).max())), ('df', Df, np.abs(Df).max())):
        e_round = np.abs(o[key] - truth)[ok].max()
        e_gpu = np.abs(g[key].astype(np.float64) - truth)[ok].max()
        bound = 2 * e_round + 1e-6 * scale
        print("exact model %s: |gpu-truth| %.2e, float32 rounding alone %.2e, bound %.2e" % (key, e_gpu, e_round, bound))
        assert e_gpu <= bound


def test_lcs_df_fallback_and_clamp_bits():
    T, Dx, Dy, Df, S, R = _inputs(64, 80, 5, seed=5, dmax=2.0, dfmax=1.5)
    for k in range(5):
        R[k][20:30, 30:45] = 5000.0                     # flat reference: zero gradient and Laplacian columns
        S[k][20:30, 30:45] = 4000.0
        S[k][40:44, 10:14] = 0.0                        # dark sample pixels: zero S column
        S[k][50, 60] = -S[k][50, 60]                    # the negated model: x0 = -1/T < 0
    g = _gpu_lcs_df(S, R)
    o = odf.lcs_df(S, R, return_mask=True)
    inner = np.zeros(o['fallback'].shape, bool)
    inner[21:29, 31:44] = True
    inner[40:44, 10:14] = True
    inner[50, 60] = True
    inner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    assert o['fallback'][inner].all()
    for key, v in (('transmission', 1.0), ('dx', 0.0), ('dy', 0.0), ('df', 0.0)):
        assert np.array_equal(g[key][inner], np.full(inner.sum(), v, np.float32)), key
    gfb = (g['transmission'] == 1.0) & (g['dx'] == 0.0) & (g['dy'] == 0.0) & (g['df'] == 0.0)
    assert np.array_equal(gfb, o['fallback'])
    ms = 0.75
    c = _gpu_lcs_df(S, R, max_shift=ms)
    oc = odf.lcs_df(S, R, max_shift=ms)
    for key in ('dx', 'dy'):
        clamped = np.abs(oc[key]) == np.float32(ms)
        assert clamped.sum() > 100
        assert np.array_equal(c[key][clamped], oc[key][clamped])          # exactly +-max_shift, same bits
        assert np.all(np.abs(c[key]) <= np.float32(ms))
    assert np.abs(g['df']).max() > ms                                      # df is not clamped
    assert np.array_equal(c['df'], g['df']) and np.array_equal(c['transmission'], g['transmission'])


def test_input_forms_streams_and_no_allocation_on_reuse():
    from paresis_amd import ops
    T, Dx, Dy, Df, S, R = _inputs(120, 96, 6, seed=21)
    St, Rt = _cuda(np.stack(S)), _cuda(np.stack(R))
    a = ops.lcs_df(St, Rt)
    assert len(a) == 4
    b = ops.lcs_df([St[k].clone() for k in range(6)], [Rt[k].clone() for k in range(6)])
    stacks_s = [torch.stack([St[k] * 0.5, St[k], St[k] * 2]) for k in range(6)]
    stacks_r = [torch.stack([Rt[k] * 0.5, Rt[k], Rt[k] * 2]) for k in range(6)]
    c = ops.lcs_df([s[1] for s in stacks_s], [r[1] for r in stacks_r])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = ops.lcs_df(St, Rt)
    torch.cuda.current_stream().wait_stream(side)
    for x in (b, c, d):
        for u, v in zip(a, x):
            assert torch.equal(u, v)
    outs = tuple(torch.empty_like(a[0]) for _ in range(4))
    r1 = ops.lcs_df(St, Rt, out=outs)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    r2 = ops.lcs_df(St, Rt, out=outs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    assert all(u is v for u, v in zip(r1, outs)) and all(u is v for u, v in zip(r2, outs))
    for u, v in zip(a, outs):
        assert torch.equal(u, v)


def test_lcs_unchanged_by_lcs_df():
    """psx_lcs_f32 gives the same bits on a seeded input whether or not psx_lcs_df_f32 ran before it: no shared state."""
    from paresis_amd import ops
    T, Dx, Dy, S, R = orl.exact_model(150, 130, 7, seed=33)
    St, Rt = _cuda(np.stack(S)), _cuda(np.stack(R))
    before = [t.clone() for t in ops.lcs(St, Rt)]
    torch.cuda.synchronize()
    ops.lcs_df(St * 1.5, Rt, max_shift=0.25)
    ops.lcs_df(St, Rt)
    after = ops.lcs(St, Rt)
    torch.cuda.synchronize()
    for u, v in zip(before, after):
        assert torch.equal(u, v)
    o = orl.lcs(S, R)                                  # and they are still the three-unknown oracle's
    assert np.abs(_np(after[1]) - o['dx']).max() <= 1e-5 * np.abs(o['dx']).max()


# ------------------------------------------------------------------- against the exact and the restated references
@pytest.mark.parametrize("n,m,K,seed,max_shift", odf.LCS_DF_CASES)
def test_lcs_df_matches_exact_reference(n, m, K, seed, max_shift):
    """k_lcs_df against the contract solved in exact rational arithmetic, as tests/test_gpu_retrieval.py
    test_lcs_matches_exact_reference: every pixel within 2^-24 |x*| + 8 Y scale, the four corners (structural fallbacks)
    exactly (1, 0, 0, 0) and the only fallbacks.  tests/test_retrieval_df_host.py holds 8 Y <= 2^-24 and shows that the wrong
    kernels, a zero-padded Laplacian among them, exceed the bound 10 times and more."""
    S, R, ref, f64, Y = odf.lcs_df_parity(n, m, K, seed)
    got = _gpu_lcs_df(S, R, max_shift=max_shift)
    assert np.array_equal(ref['fallback'], odf.corners(n, m))
    orl.check_parity("lcs_df %dx%d K=%d max_shift %s" % (n, m, K, max_shift), got, ref, Y, odf.MAPS, max_shift)
    if max_shift is not None:
        assert np.array_equal(got['df'], _gpu_lcs_df(S, R)['df'])                      # df is not clamped


def test_lcs_df_matches_exact_reference_on_steep_images():
    """tests/test_gpu_retrieval.py test_lcs_matches_exact_reference_on_steep_images for k_lcs_df."""
    n, m, K, seed = orl.LCS_STEEP_CASE
    S, R, ref, f64, Y = odf.lcs_df_parity(n, m, K, seed, steep=True)
    orl.check_parity("lcs_df %dx%d K=%d steep" % (n, m, K), _gpu_lcs_df(S, R), ref, Y, odf.MAPS)


def test_lcs_df_nonfinite_pixels_fall_back():
    """tests/test_gpu_retrieval.py test_lcs_nonfinite_pixels_fall_back for k_lcs_df: (1, 0, 0, 0) where a NaN or an infinity
    is read (and at the corners), the clean run's bits everywhere else."""
    S, R = orl.case_inputs(odf.exact_model, 9, 66, 5, 2)
    Sb, Rb = orl.nonfinite_inputs(S, R)
    mask = orl.nonfinite_pixels(Sb, Rb) | odf.corners(9, 66)
    clean, dirty = _gpu_lcs_df(S, R), _gpu_lcs_df(Sb, Rb)
    for k, v in zip(odf.MAPS, (1.0, 0.0, 0.0, 0.0)):
        assert np.array_equal(dirty[k][mask], np.full(mask.sum(), v, np.float32)), (k, dirty[k][mask])
        assert np.array_equal(dirty[k][~mask].view(np.uint32), clean[k][~mask].view(np.uint32)), k


@pytest.mark.parametrize("k,i,j", [(0, 4, 30), (4, 0, 1), (2, 8, 64), (3, 3, 65)])
def test_lcs_df_one_pixel_reaches_its_neighbours_only(k, i, j):
    S, R = orl.case_inputs(odf.exact_model, 9, 66, 5, 2)
    orl.check_isolation(_gpu_lcs_df, S, R, k, i, j)


# --------------------------------------------------------------------------------------------------------- end to end
def _run(name, K, root, xml_dir, **kw):
    from paresis_amd import main
    ed = {"experimentName": name, "filepath": str(root) + "/" + name + "/", "overSampling": 2, "nbExpPoints": K,
          "simulation_type": "RayT", "noise": False, "seed": 3, "xmlDir": xml_dir}
    os.makedirs(ed["filepath"], exist_ok=True)
    return ed, main.run(ed, **kw)


@pytest.fixture(scope="module")
def lung_run(tmp_path_factory):
    """The Lung cylinder run: RayT, 12 positions, ov = 2, no noise, the mono id17 source, saved as .tif, retrieved with
    dark_field.  Lung's delta/beta are registered for the run only."""
    root = tmp_path_factory.mktemp("lung")
    xml_dir = dfe.write_xml(str(root / "xml"))
    with dfe.lung_material():
        ed, res = _run(dfe.EXPERIMENT, 12, root, xml_dir, save=True, saving_format=".tif", retrieve=True, dark_field=True)
        from paresis_amd.Experiment import Experiment
        exp = Experiment(dict(ed, filepath=str(root) + "/probe/"))
        h = float(exp.exp_dict['studyPixelSize']) * 1e-6
        flux = sum(f for _, f in exp.mySource.mySpectrum)
    from paresis_amd import materials
    assert "Lung" not in materials._REGISTRY
    return ed, res, h, flux


# Thresholds from the CPU calibration: oracle.compute_rt (fastRefractionDF) over 12 positions -- shifted copies of one synthetic
# sphere membrane -- in the Lung_Cylinder_ID17 configuration (ov = 2, mono 52 keV, no noise), then the oracle LCS-DF and
# tests/_retrieval_df_e2e.figures: df against df_true corr 0.589, slope 0.528; scattering against theta corr 0.589, slope
# 0.497; median |df| inside 0.144 against the median df_true 0.148 (ratio 0.97); empty field median |df| 2.5e-17 (S = R
# there, no noise); theta max 1.93e-6 rad, sigma_study max 1.16.  The first-order model flattens the variation of the blur
# across the cylinder (slopes ~0.5) but gets its level right.  Margins: correlations >= 0.4; df slope in [0.25, 1.0] and the
# median ratio in [0.75, 1.35] -- a factor ov^2 moves both by 4 or 1/4, a factor 2 by 2 or 1/2, sqrt 2 the ratio to 0.69 /
# 1.37; a wrong sign makes the slope and the median negative; a swapped axis (the transposed truth: the 30 degree cylinder
# is not symmetric under it) drops the correlation below 0.4.
# Control (Fil_Nylon_ID17, dark_field=True, the same calibration): median |df| inside the wire 0.0066 = 0.046 of the Lung
# run's median |df|; the threshold is 0.2.
DF_MIN_CORR = 0.4
DF_SLOPE = (0.25, 1.0)
DF_MEDIAN_RATIO = (0.75, 1.35)
EMPTY_FRACTION = 0.02
CONTROL_FRACTION = 0.2


def _lung_figures(lung_run):
    from paresis_amd import retrieval
    ed, res, h, flux = lung_run
    params = ed['retrievalParams']
    out = retrieval.retrieve(res, params, dark_field=True)[0]
    theta = _np(res[0][6]) / flux
    df_t, th_t = dfe.df_truth(theta, params['distance_m'], h, params['magnification'], ed['overSampling'])
    inside, far = dfe.masks(_np(res[0][4]), _np(res[0][5]), th_t, theta.shape)
    return out, df_t, th_t, inside, far


def test_end_to_end_dark_field(lung_run):
    ed, res, h, flux = lung_run
    out, df_t, th_t, inside, far = _lung_figures(lung_run)
    S = [_np(res[p][0])[0] for p in sorted(res)]
    R = [_np(res[p][1])[0] for p in sorted(res)]
    o = odf.lcs_df(S, R, return_mask=True)               # the GPU's LCS-DF of the chain's images == the oracle's
    ok = ~o['fallback']
    assert np.abs(_np(out['df']) - o['df'])[ok].max() <= 1e-5 * np.abs(o['df'])[ok].max()
    fig = dfe.figures(_np(out['df']), _np(out['scattering']), df_t, th_t, inside, far)
    print("e2e dark field:", fig, "theta max %.3e" % th_t.max())
    assert fig['npix'] > 2000 and fig['nempty'] > 2000
    for key in ('df', 'scattering'):
        assert fig[key][0] >= DF_MIN_CORR, (key, fig[key])
    assert DF_SLOPE[0] <= fig['df'][1] <= DF_SLOPE[1], fig['df']
    ratio = fig['inside_med_abs_df'] / fig['sample_med_df_true']
    assert DF_MEDIAN_RATIO[0] <= ratio <= DF_MEDIAN_RATIO[1], ratio
    assert np.median(_np(out['df'])[inside]) > 0
    assert fig['empty_med_abs_df'] <= EMPTY_FRACTION * fig['sample_med_df_true'], fig
    # the transposed truth does not fit
    assert dfe.e2e.figures(_np(out['df']).T, df_t, inside.T)[0] < fig['df'][0]


def test_non_scattering_control(tmp_path, lung_run):
    from paresis_amd import retrieval
    from paresis_amd.Experiment import Experiment
    out_l, df_t, th_t, inside_l, _ = _lung_figures(lung_run)
    lung_med = float(np.median(np.abs(_np(out_l['df'])[inside_l])))
    ed, res = _run("Fil_Nylon_ID17", 12, tmp_path, None, save=False, retrieve=True, dark_field=True)
    out = retrieval.retrieve(res, ed['retrievalParams'], dark_field=True)[0]
    assert set(out) == {'transmission', 'dx', 'dy', 'phi', 'df', 'scattering'}
    exp = Experiment(dict(ed, filepath=str(tmp_path) + "/probe/"))
    T = _np(exp.mySampleofInterest.myGeometry)[0]
    inside, _ = dfe.masks(_np(res[0][4]), _np(res[0][5]), dfe.e2e.bin2(T), T.shape)
    med = float(np.median(np.abs(_np(out['df'])[inside])))
    print("control: median |df| in the wire %.4f, Lung run %.4f (ratio %.3f), mask %d" % (med, lung_med, med / lung_med,
                                                                                          int(inside.sum())))
    assert inside.sum() > 2000
    assert med <= CONTROL_FRACTION * lung_med


def test_outputs_on_disk_and_cli(lung_run):
    from paresis_amd import main, retrieval
    from paresis_amd.InputOutput.pagailleIO import openImage
    ed, res, h, flux = lung_run
    files = sorted(glob.glob(ed["filepath"] + "*/retrieval/*.tif"))
    names = sorted(os.path.basename(f).split("_")[0] for f in files)
    assert names == ["df", "dx", "dy", "phi", "scattering", "transmission"], files
    want = retrieval.retrieve(res, ed['retrievalParams'], dark_field=True)[0]
    for f in files:
        img = openImage(f)
        assert img.shape == (200, 200)
        assert np.array_equal(img, _np(want[os.path.basename(f).split("_")[0]])), f
    run_dir = os.path.dirname(os.path.dirname(files[0]))
    p = ed['retrievalParams']
    before = {f: open(f, "rb").read() for f in files}
    retrieval.main([run_dir, "--energy", repr(p['energy_keV']), "--pixel-um", repr(p['pixel_um']), "--distance",
                    repr(p['distance_m']), "--magnification", repr(p['magnification']), "--dark-field"])
    for f in files:
        assert open(f, "rb").read() == before[f], f
    with pytest.raises(ValueError, match="at least 4"):
        main.run(dict(ed, nbExpPoints=3), save=False, retrieve=True, dark_field=True)
    with pytest.raises(ValueError, match="at least 4"):
        retrieval.retrieve({q: res[q] for q in sorted(res)[:3]}, p, dark_field=True)
