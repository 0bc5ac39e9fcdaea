"""Phase retrieval on the GPU (csrc/retrieve.hip, ops.lcs / ops.IntegratePlan, paresis_amd.retrieval, main.py --retrieve)
against the float64 numpy oracle of tests/_retrieval_oracle.py, and end to end against the chain's own ground truth."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import _retrieval_e2e as e2e
from tests import _retrieval_oracle as orl

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _inputs(n, m, K, seed, dmax=0.5):
    """float32 S_k, R_k of the exact model (T in [0.6, 1], |D| <= dmax): well away from the fallback threshold."""
    T, Dx, Dy, S, R = orl.exact_model(n, m, K, seed=seed, dmax=dmax)
    return T, Dx, Dy, [s.astype(np.float32) for s in S], R


def _gpu_lcs(S, R, max_shift=None):
    from paresis_amd import retrieval
    r = retrieval.lcs(_cuda(np.stack(S)), _cuda(np.stack(R)), max_shift=max_shift)
    return {k: _np(v) for k, v in r.items()}


@pytest.mark.parametrize("n,m,K", [(200, 200, 3), (301, 173, 64), (3, 3, 7), (2048, 2048, 7)])
def test_lcs_matches_oracle(n, m, K):
    T, Dx, Dy, S, R = _inputs(n, m, K, seed=n + m + K)
    g = _gpu_lcs(S, R)
    o = orl.lcs(S, R, return_mask=True)
    fb = o['fallback']
    assert np.array_equal(g['transmission'] == 1.0, fb | (o['transmission'] == 1.0))
    ok = ~fb
    dmax = max(np.abs(o['dx']).max(), np.abs(o['dy']).max())
    ex = np.abs(g['dx'] - o['dx'])[ok].max()
    ey = np.abs(g['dy'] - o['dy'])[ok].max()
    et = (np.abs(g['transmission'] - o['transmission']) / np.abs(o['transmission']))[ok].max()
    print("lcs %dx%d K=%d: |ddx| %.2e |ddy| %.2e (max|D| %.3f), rel dT %.2e" % (n, m, K, ex, ey, dmax, et))
    assert ex <= 1e-5 * dmax and ey <= 1e-5 * dmax and et <= 1e-5


def test_lcs_exact_model_known_answer():
    """The GPU recovers T, Dx, Dy of the exact model from its float32-rounded inputs.  Bound: rounding S_k to float32 (the
    only inexact step; R_k and its gradients are float32 already) moves the least-squares solution; the float64 oracle on
    the SAME float32 inputs measures that displacement E_round exactly, and the kernel's float64 arithmetic adds nothing
    comparable, so |GPU - truth| <= 2*E_round + 1e-6 (the float32 rounding of the outputs themselves)."""
    T, Dx, Dy, S, R = _inputs(256, 192, 9, seed=11)
    g = _gpu_lcs(S, R)
    o = orl.lcs(S, R, dtype=np.float64)
    for key, truth, rel in (('transmission', T, True), ('dx', Dx, False), ('dy', Dy, False)):
        e_round = np.abs(o[key] - truth).max()
        e_gpu = np.abs(g[key].astype(np.float64) - truth).max()
        bound = 2 * e_round + 1e-6 * (np.abs(truth).max() if rel else max(np.abs(Dx).max(), np.abs(Dy).max()))
        print("exact model %s: |gpu-truth| %.2e, float32 rounding alone %.2e, bound %.2e" % (key, e_gpu, e_round, bound))
        assert e_gpu <= bound


def test_lcs_fallback_and_clamp_bits():
    T, Dx, Dy, S, R = _inputs(64, 80, 5, seed=5, dmax=2.0)
    for k in range(5):
        R[k][20:30, 30:45] = 5000.0                     # flat reference: zero gradient columns
        S[k][20:30, 30:45] = 4000.0
        S[k][40:44, 10:14] = 0.0                        # dark sample pixels: zero S column
    g = _gpu_lcs(S, R)
    o = orl.lcs(S, R, return_mask=True)
    inner = np.zeros(o['fallback'].shape, bool)
    inner[21:29, 31:44] = True
    inner[40:44, 10:14] = True
    assert o['fallback'][inner].all()
    for key, v in (('transmission', 1.0), ('dx', 0.0), ('dy', 0.0)):
        assert np.array_equal(g[key][inner], np.full(inner.sum(), v, np.float32))
    assert np.array_equal(g['transmission'] == 1.0, o['fallback'] | (o['transmission'] == 1.0))
    ms = 0.75
    c = _gpu_lcs(S, R, max_shift=ms)
    oc = orl.lcs(S, R, max_shift=ms)
    for key in ('dx', 'dy'):
        clamped = np.abs(oc[key]) == np.float32(ms)
        assert clamped.sum() > 100
        assert np.array_equal(c[key][clamped], oc[key][clamped])          # exactly +-max_shift, same bits
        assert np.all(np.abs(c[key]) <= np.float32(ms))


def test_input_forms_streams_and_no_allocation_on_reuse():
    from paresis_amd import ops, retrieval
    T, Dx, Dy, S, R = _inputs(120, 96, 6, seed=21)
    St, Rt = _cuda(np.stack(S)), _cuda(np.stack(R))
    a = ops.lcs(St, Rt)
    b = ops.lcs([St[k].clone() for k in range(6)], [Rt[k].clone() for k in range(6)])
    # bin slices of [nbins, n, m] stacks, as the chains return them: the retrieved bin is 1 of 3
    stacks_s = [torch.stack([St[k] * 0.5, St[k], St[k] * 2]) for k in range(6)]
    stacks_r = [torch.stack([Rt[k] * 0.5, Rt[k], Rt[k] * 2]) for k in range(6)]
    c = ops.lcs([s[1] for s in stacks_s], [r[1] for r in stacks_r])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = ops.lcs(St, Rt)
    torch.cuda.current_stream().wait_stream(side)
    for x in (b, c, d):
        for u, v in zip(a, x):
            assert torch.equal(u, v)
    # out= and a second call of the same shape: no plan, no allocation
    retrieval._plans.clear()
    outs = tuple(torch.empty_like(a[0]) for _ in range(3))
    phi = torch.empty_like(a[0])
    ops.lcs(St, Rt, out=outs)
    retrieval.integrate(outs[1], outs[2], out=phi)
    torch.cuda.synchronize()
    plan = next(iter(retrieval._plans.values()))
    mem, nbytes = torch.cuda.memory_allocated(), plan.bytes
    ops.lcs(St, Rt, out=outs)
    phi2 = retrieval.integrate(outs[1], outs[2], out=phi)
    torch.cuda.synchronize()
    assert phi2 is phi
    assert torch.cuda.memory_allocated() == mem and len(retrieval._plans) == 1
    assert plan.bytes == nbytes and ops.lib().psx_integrate_plan_bytes(plan._h) == nbytes
    assert nbytes >= 8 * 4 * 120 * 96


def _smooth_gradients(n, m, seed):
    rng = np.random.default_rng(seed)
    return orl.smooth_field(n, m, rng, 0.3), orl.smooth_field(n, m, rng, 0.2)


@pytest.mark.parametrize("n,m", [(200, 200), (301, 173), (3, 3), (2048, 2048)])
def test_integrate_matches_oracle(n, m):
    from paresis_amd import retrieval
    gx, gy = _smooth_gradients(n, m, seed=n * 7 + m)
    gx, gy = gx.astype(np.float32), gy.astype(np.float32)
    ref = orl.integrate(gx, gy)
    got = _np(retrieval.integrate(_cuda(gx), _cuda(gy)))
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("integrate %dx%d: max|gpu-oracle|/max|phi| = %.2e" % (n, m, err))
    assert err <= 1e-4


def test_integrate_known_answer():
    """phi evenly extended (a cosine series on the 2n x 2m grid) and its gradients formed spectrally: the GPU returns
    phi - mean(phi) within float32 transform accuracy."""
    from paresis_amd import retrieval
    n, m = 96, 80
    rng = np.random.default_rng(4)
    i = np.arange(n)[:, None] + 0.5
    j = np.arange(m)[None, :] + 0.5
    phi = np.zeros((n, m))
    for _ in range(6):
        a, b = rng.integers(0, 8, 2)
        phi += rng.standard_normal() * np.cos(np.pi * a * i / n) * np.cos(np.pi * b * j / m)
    E = np.concatenate([phi, phi[::-1, :]], 0)
    E = np.concatenate([E, E[:, ::-1]], 1)
    kx = 2 * np.pi * np.fft.fftfreq(2 * n)[:, None]
    ky = 2 * np.pi * np.fft.fftfreq(2 * m)[None, :]
    F = np.fft.fft2(E)
    gx = np.fft.ifft2(1j * kx * F).real[:n, :m]
    gy = np.fft.ifft2(1j * ky * F).real[:n, :m]
    got = _np(retrieval.integrate(_cuda(gx), _cuda(gy)))
    want = phi - phi.mean()
    err = np.abs(got - want).max() / np.abs(want).max()
    print("integrate known answer: %.2e" % err)
    assert err <= 1e-4


# ------------------------------------------------------------------- against the exact and the restated references
@pytest.mark.parametrize("n,m,K,seed,max_shift", orl.LCS_CASES)
def test_lcs_matches_exact_reference(n, m, K, seed, max_shift):
    """k_lcs against the contract solved in exact rational arithmetic, no pixel left out.  The bound is the float32 output's
    rounding plus 8 times what float64 costs on the input (Y, measured on the CPU between the kernel's restatement and the
    exact solution; tests/test_retrieval_host.py holds 8 Y <= 2^-24 and shows that float32 sums, a wrong border spacing, a
    wrapped neighbour and a dropped last position exceed the bound 10 times and more)."""
    S, R, ref, f64, Y = orl.lcs_parity(n, m, K, seed)
    got = _gpu_lcs(S, R, max_shift=max_shift)
    orl.check_parity("lcs %dx%d K=%d max_shift %s" % (n, m, K, max_shift), got, ref, Y, orl.MAPS, max_shift)


def test_lcs_matches_exact_reference_on_steep_images():
    """The same bound on images whose neighbours differ by more than a factor of two: there the float32 difference of the
    gradient rounds, and differences formed in float64 miss the bound (tests/test_retrieval_host.py: 10 times and more)."""
    n, m, K, seed = orl.LCS_STEEP_CASE
    S, R, ref, f64, Y = orl.lcs_parity(n, m, K, seed, steep=True)
    orl.check_parity("lcs %dx%d K=%d steep" % (n, m, K), _gpu_lcs(S, R), ref, Y, orl.MAPS)


def test_lcs_nonfinite_pixels_fall_back():
    """A NaN, a +inf and a -inf in S_k and in R_k at interior, edge and corner pixels: the pixels that read one return
    (1, 0, 0), every other pixel keeps the bits of the run on the clean images (include/paresis_hip.h)."""
    S, R = orl.case_inputs(orl.exact_model, 9, 66, 5, 2)
    Sb, Rb = orl.nonfinite_inputs(S, R)
    mask = orl.nonfinite_pixels(Sb, Rb)
    clean, dirty = _gpu_lcs(S, R), _gpu_lcs(Sb, Rb)
    for k, v in zip(orl.MAPS, (1.0, 0.0, 0.0)):
        assert np.array_equal(dirty[k][mask], np.full(mask.sum(), v, np.float32)), (k, dirty[k][mask])
        assert np.array_equal(dirty[k][~mask].view(np.uint32), clean[k][~mask].view(np.uint32)), k
    c = _gpu_lcs(Sb, Rb, max_shift=0.2)
    for k in ('dx', 'dy'):
        assert np.all(c[k][mask] == 0.0) and np.all(np.abs(c[k]) <= np.float32(0.2))


@pytest.mark.parametrize("k,i,j", [(0, 4, 30), (4, 0, 0), (2, 8, 64), (3, 3, 65)])
def test_lcs_one_pixel_reaches_its_neighbours_only(k, i, j):
    S, R = orl.case_inputs(orl.exact_model, 9, 66, 5, 2)
    orl.check_isolation(_gpu_lcs, S, R, k, i, j)


def _gpu_integrate(plan, gx, gy, scale=1.0):
    return _np(plan.integrate(_cuda(gx), _cuda(gy), scale=scale))


@pytest.mark.parametrize("n,m", orl.INTEGRATE_SHAPES)
def test_integrate_matches_restatement_yardstick(n, m):
    """psx_integrate_f32 on white-noise gradients (independent gx and gy: not integrable) and on single-pixel impulses of gx
    and of gy at a corner and inside, and with scale = -2.5 and 1e-3 on the noise:
        max|gpu - contract| <= 8 * max|integrate_f32 - contract|,
    the contract in float64 on the pack's own float32 input, integrate_f32 the kernels restated in their number formats
    on the CPU (not zero, below 2e-6 of the peak).  |mean(phi)| over the n x m result stays within the same bound."""
    from paresis_amd import ops
    plan = ops.IntegratePlan(n, m)
    worst = 0.0
    for name, gx, gy in orl.integrate_inputs(n, m):
        for scale in (1.0,) if name != "noise" else (1.0, -2.5, 1e-3):
            ref, y, peak = orl.integrate_yardstick(gx, gy, scale)
            got = _gpu_integrate(plan, gx, gy, scale).astype(np.float64)
            err, mean = np.abs(got - ref).max(), abs(got.mean())
            print("integrate %dx%d %s scale %g: yardstick %.2e (%.2e of the peak), error / bound %.3f, |mean| / bound %.3f"
                  % (n, m, name, scale, y, y / peak, err / (8 * y), mean / (8 * y)))
            assert 0.0 < y < 2e-6 * peak
            worst = max(worst, err / (8 * y), mean / (8 * y))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n,m", [(33, 47), (32, 48)])
def test_one_plan_serves_integrate_and_paganin_in_turn(n, m):
    """integrate, paganin, integrate, a pair of Paganin images on ONE plan, as retrieval._plan hands it out: every result has
    the bits of the same call on a fresh plan (the calls share the plan's buffer and transforms, and leave nothing in them)."""
    from paresis_amd import ops
    rng = np.random.default_rng(n * m)
    g = [_cuda(rng.standard_normal((n, m))) for _ in range(4)]
    I = [_cuda(1.0 + 0.1 * rng.standard_normal((n, m))) for _ in range(3)]
    calls = [lambda p: [p.integrate(g[0], g[1])],
             lambda p: list(ops.paganin([I[0]], None, 3.0, 50.0, p)),
             lambda p: [p.integrate(g[2], g[3], scale=-0.5)],
             lambda p: list(ops.paganin(I[1:], None, [0.5, 20.0], [40.0, 80.0], p))]
    shared = ops.IntegratePlan(n, m)
    for call in calls:
        a, b = call(shared), call(ops.IntegratePlan(n, m))
        torch.cuda.synchronize()
        assert len(a) == len(b)
        for u, v in zip(a, b):
            assert torch.isfinite(u).all() and torch.equal(u.view(torch.int32), v.view(torch.int32))


def _run(sim, K, tmp_path, **kw):
    from paresis_amd import main
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": str(tmp_path) + "/" + sim + "/", "overSampling": 2,
          "nbExpPoints": K, "simulation_type": sim, "noise": False, "seed": 3}
    os.makedirs(ed["filepath"], exist_ok=True)
    res = main.run(ed, **kw)
    return ed, res


def _sample_truth():
    """The sample's thickness and delta as the experiment builds them (host), for the true phase -k*delta*T."""
    from paresis_amd.Experiment import Experiment
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": "/tmp/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": "RayT", "noise": False}
    exp = Experiment(ed)
    g = exp.mySampleofInterest.myGeometry
    T = _np(g)[0]
    return T, exp.mySampleofInterest.delta[0][0][1]


# Thresholds from the CPU calibration (tests/_retrieval_e2e.evaluate on oracle.compute_rt / compute_fresnel over 12 membrane
# positions: shifted copies of one synthetic sphere membrane in the configuration of Fil_Nylon_ID17, ov = 2, no noise).
# Calibration, ray tracing: corr dx 0.695, dy 0.843, phi 0.9996; slope dx 1.237, dy 1.260, phi 1.276.  Fresnel: corr dx
# 0.741, dy 0.878, phi 0.9997; slope 1.522, 1.541, 1.556 (central differences on 2-3 pixel grains overestimate D).  Margins:
# correlations 0.15-0.2 below (0.03 for phi), ray-tracing slopes within [1.0, 1.6] -- a swapped axis scales the slopes by
# tan 30 = 0.58 / cot 30 = 1.73, a factor ov by 2 or 1/2, a wrong sign flips them.
RT_MIN_CORR = {'dx': 0.5, 'dy': 0.65, 'phi': 0.97}
SLOPE_RANGE = (1.0, 1.6)
FRESNEL_MIN_PHI_CORR = 0.97


def test_end_to_end_ray_tracing(tmp_path):
    from paresis_amd import retrieval
    ed, res = _run("RayT", 12, tmp_path, save=False, retrieve=True)
    params = ed['retrievalParams']
    out = retrieval.retrieve(res, params)[0]
    S = [_np(res[p][0])[0] for p in sorted(res)]
    R = [_np(res[p][1])[0] for p in sorted(res)]
    o = orl.lcs(S, R, return_mask=True)                     # the GPU's LCS of the chain's images == the oracle's
    ok = ~o['fallback']
    dmax = max(np.abs(o['dx']).max(), np.abs(o['dy']).max())
    assert np.abs(_np(out['dx']) - o['dx'])[ok].max() <= 1e-5 * dmax
    assert np.abs(_np(out['dy']) - o['dy'])[ok].max() <= 1e-5 * dmax
    T, delta = _sample_truth()
    dx_t, dy_t, phi_t = e2e.truths(_np(res[0][4]), _np(res[0][5]), T, delta, params['energy_keV'])
    m = e2e.mask(dx_t, dy_t)
    fig = {k: e2e.figures(_np(out[k]), t, m) for k, t in (('dx', dx_t), ('dy', dy_t), ('phi', phi_t))}
    print("e2e ray tracing (corr, slope):", fig, "mask", int(m.sum()))
    for k, (corr, slope) in fig.items():
        assert corr >= RT_MIN_CORR[k], (k, corr)
        assert SLOPE_RANGE[0] <= slope <= SLOPE_RANGE[1], (k, slope)


def test_end_to_end_fresnel(tmp_path):
    from paresis_amd import retrieval
    ed, res = _run("Fresnel", 12, tmp_path, save=False, retrieve=True)
    params = ed['retrievalParams']
    out = retrieval.retrieve(res, params)[0]
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    _, rt = _run("RayT", 1, tmp_path, save=False)             # the truth's displacements for the mask
    T, delta = _sample_truth()
    dx_t, dy_t, phi_t = e2e.truths(_np(rt[0][4]), _np(rt[0][5]), T, delta, params['energy_keV'])
    m = e2e.mask(dx_t, dy_t)
    corr, slope = e2e.figures(_np(out['phi']), phi_t, m)
    print("e2e Fresnel phi (corr, slope):", corr, slope)
    assert corr >= FRESNEL_MIN_PHI_CORR


def test_main_retrieve_writes_maps(tmp_path):
    from paresis_amd import main, retrieval
    from paresis_amd.InputOutput.pagailleIO import openImage
    ed, res = _run("RayT", 3, tmp_path, save=True, saving_format=".tif", retrieve=True)
    files = sorted(glob.glob(ed["filepath"] + "*/retrieval/*.tif"))
    names = sorted(os.path.basename(f).split("_")[0] for f in files)
    assert names == ["dx", "dy", "phi", "transmission"], files
    want = retrieval.retrieve(res, ed['retrievalParams'])[0]
    for f in files:
        img = openImage(f)
        assert img.shape == (200, 200)
        assert np.array_equal(img, _np(want[os.path.basename(f).split("_")[0]]))
    with pytest.raises(ValueError, match="at least 3"):
        main.run(dict(ed, nbExpPoints=2), save=False, retrieve=True)
    # the CLI on the run's directory writes the same maps
    run_dir = os.path.dirname(os.path.dirname(files[0]))
    p = ed['retrievalParams']
    before = {f: openImage(f) for f in files}
    retrieval.main([run_dir, "--energy", repr(p['energy_keV']), "--pixel-um", repr(p['pixel_um']), "--distance",
                    repr(p['distance_m']), "--magnification", repr(p['magnification'])])
    for f in files:
        assert np.array_equal(openImage(f), before[f]), f
