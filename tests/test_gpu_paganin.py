"""Paganin retrieval of the propagation image on the GPU (csrc/retrieve.hip psx_paganin_f32, ops.paganin,
paresis_amd.retrieval, main.py --retrieve-propagation) against the float64 numpy oracle of tests/_paganin_oracle.py, and end
to end against the chains' own sample."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import _paganin_oracle as po

pytestmark = pytest.mark.gpu

ALPHAS, MUS = (0.0, 3.0, 400.0), (22.0, 35.0, 50.0)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _plan(n, m):
    from paresis_amd import retrieval
    return retrieval._plan(torch.device("cuda", torch.cuda.current_device()), n, m)


def _ratios(got, o, mu):
    """(contact error, thickness error) of one image over the issue's parity bounds."""
    bc, bt = po.bounds(o, mu)
    ec = np.abs(_np(got[0]).astype(np.float64) - o['contact']).max()
    et = np.abs(_np(got[1]).astype(np.float64) - o['thickness']).max()
    return ec / bc, et / bt


@pytest.mark.parametrize("n,m", [(2, 2), (3, 5), (64, 48), (301, 173), (2048, 2048)])
def test_paganin_matches_oracle(n, m):
    """Three images, image i with (ALPHAS[i], MUS[i]): each alone (B = 1), the first two together (B = 2, one transform), all
    three in one call (B = 3, the last with a zero imaginary part), and the first two in the other order (each alpha in
    either half of the transform).  Bound (the issue's): max|contact - oracle| <= 5e-6*max|r - 1| + 1.2e-7*max|c|, and the
    same over mu*c_min for thickness."""
    from paresis_amd import ops
    pairs = [po.image_pair(n, m, seed=n * 7 + m + i) for i in range(3)]
    orc = [po.paganin(I, I0, a, u) for (I, I0), a, u in zip(pairs, ALPHAS, MUS)]
    I = _cuda(np.stack([p[0] for p in pairs]))
    W = _cuda(np.stack([p[1] for p in pairs]))
    plan = _plan(n, m)
    worst = 0.0
    for idx in ([0], [1], [2], [0, 1], [0, 1, 2], [1, 0], [2, 1]):
        c, t = ops.paganin([I[i] for i in idx], [W[i] for i in idx], [ALPHAS[i] for i in idx], [MUS[i] for i in idx], plan)
        assert c.shape == t.shape == (len(idx), n, m) and c.dtype == t.dtype == torch.float32
        for b, i in enumerate(idx):
            rc, rt = _ratios((c[b], t[b]), orc[i], MUS[i])
            worst = max(worst, rc, rt)
            assert rc <= 1.0 and rt <= 1.0, (idx, i, rc, rt)
    print("paganin %dx%d: worst error / bound = %.3f" % (n, m, worst))


def test_no_cross_talk_within_a_transform():
    """B = 2: image 0 with strong structure and alpha = 400, image 1 with r == 1 and alpha = 3.  Image 1's contact stays within
    its own bound of 1 (5e-6*0 + 1.2e-7*1: one float32 step), in either half of the transform."""
    from paresis_amd import ops
    n, m = 64, 48
    I, I0 = po.image_pair(n, m, seed=9, contrast=0.5)
    flat = I0.copy()
    o = po.paganin(I, I0, 400.0, 22.0)
    plan = _plan(n, m)
    for order in ((0, 1), (1, 0)):
        imgs, whites, alpha = [(I, flat)[k] for k in order], [I0, I0], [(400.0, 3.0)[k] for k in order]
        c, t = ops.paganin(_cuda(np.stack(imgs)), _cuda(np.stack(whites)), alpha, 22.0, plan)
        quiet, busy = order.index(1), order.index(0)
        e = float((c[quiet] - 1.0).abs().max())
        print("cross-talk, flat image in half %d: max|contact - 1| = %.3e" % (quiet, e))
        assert e <= 1.2e-7
        assert float(t[quiet].abs().max()) <= 1.2e-7 / 22.0
        rc, rt = _ratios((c[busy], t[busy]), o, 22.0)
        assert rc <= 1.0 and rt <= 1.0


def test_known_answer():
    """t a cosine series on the extension, c0 = exp(-mu t), r = ifft2((1 + alpha k^2) fft2(ext c0)): the GPU returns t within the
    parity bound (rounding r to float32 alone moves the float64 oracle by 0.5 % of it)."""
    from paresis_amd import ops
    n, m, alpha, mu = 96, 80, 30.0, 22.0
    t, r = po.known_answer(n, m, alpha, mu)
    r32 = r.astype(np.float32)
    o = po.paganin(r32, None, alpha, mu)
    bc, bt = po.bounds(o, mu)
    c, th = ops.paganin(_cuda(r32)[None], None, alpha, mu, _plan(n, m))
    et = np.abs(_np(th[0]).astype(np.float64) - t).max()
    ec = np.abs(_np(c[0]).astype(np.float64) - np.exp(-mu * t)).max()
    print("paganin known answer: thickness error / bound %.3f, contact %.3f" % (et / bt, ec / bc))
    assert et <= bt and ec <= bc


def test_guards_leave_every_output_finite():
    """Flat-field pixels that are 0, negative, NaN or inf and an image pixel that is NaN enter as r = 1, as in the oracle; a
    region with c <= 0 (no filter) takes the finite floor -log(FLT_MIN)/mu."""
    from paresis_amd import ops
    n, m = 40, 36
    I, I0 = po.image_pair(n, m, seed=2)
    I0[3, 4], I0[10, 10], I0[20, 7], I0[30, 30] = 0.0, -5.0, np.nan, np.inf
    I0[0, 0] = -np.inf
    I[15, 15], I[n - 1, m - 1] = np.nan, np.inf
    dark = np.ones((n, m), np.float32)
    dark[5:9, 6:12] = -0.5                       # c = -0.5
    dark[20:24, 20:30] = 0.0                     # c = 0 to rounding: either branch, both finite
    plan = _plan(n, m)
    c, t = ops.paganin([_cuda(I), _cuda(dark)], [_cuda(I0), None], [3.0, 0.0], [22.0, 35.0], plan)
    assert torch.isfinite(c).all() and torch.isfinite(t).all()
    o = po.paganin(I, I0, 3.0, 22.0)
    assert all(o['r'][p] == 1.0 for p in ((3, 4), (10, 10), (20, 7), (30, 30), (0, 0), (15, 15), (n - 1, m - 1)))
    rc, rt = _ratios((c[0], t[0]), o, 22.0)
    print("guards: error / bound contact %.3f thickness %.3f" % (rc, rt))
    assert rc <= 1.0 and rt <= 1.0
    od = po.paganin(dark, None, 0.0, 35.0)
    bc, _ = po.bounds(od, 35.0)
    assert np.abs(_np(c[1]).astype(np.float64) - od['contact']).max() <= bc
    floor = np.float32(-np.log(po.FLT_MIN) / 35.0)
    assert np.all(_np(t[1])[5:9, 6:12] == floor)
    lit = dark == 1.0
    assert np.abs(_np(t[1])[lit]).max() <= bc / 35.0
    # the same image alone, without a flat field at all: white = None as an array
    c1, t1 = ops.paganin(_cuda(dark)[None], None, 0.0, 35.0, plan)
    assert torch.isfinite(c1).all() and torch.isfinite(t1).all()
    assert np.abs(_np(c1[0]).astype(np.float64) - od['contact']).max() <= bc and np.all(_np(t1[0])[5:9, 6:12] == floor)


def test_input_forms_streams_and_no_allocation_on_reuse():
    from paresis_amd import ops, retrieval
    from paresis_amd._lib import PsxError
    n, m = 120, 96
    pairs = [po.image_pair(n, m, seed=30 + i) for i in range(3)]
    I = _cuda(np.stack([p[0] for p in pairs]))
    W = _cuda(np.stack([p[1] for p in pairs]))
    retrieval._plans.clear()
    gx = torch.zeros((n, m), dtype=torch.float32, device="cuda")
    retrieval.integrate(gx, gx)                                   # the plan integrate() made is the one paganin() takes
    kw = dict(delta=9.5e-8, beta=4.2e-11, energy_keV=52.0, pixel_um=6.0, distance_m=3.6, magnification=1.0254)
    r = retrieval.paganin(I, W, **kw)
    assert len(retrieval._plans) == 1
    plan = next(iter(retrieval._plans.values()))
    alpha, mu = retrieval.paganin_alpha(**kw)
    a = ops.paganin(I, W, alpha, mu, plan)
    assert torch.equal(a[0], r['contact']) and torch.equal(a[1], r['thickness'])
    from paresis_amd.getk import getk
    assert torch.equal(r['phi'], r['thickness'] * torch.tensor(-getk(52e3) * 9.5e-8, dtype=torch.float32, device="cuda"))
    one = retrieval.paganin(I[2], W[2], **kw)                     # one image: n x m maps; the third of three is alone in its
    assert one['thickness'].shape == (n, m)                       # transform too, so the same bits
    assert all(torch.equal(one[k], r[k][2]) for k in ('contact', 'thickness', 'phi'))
    b = ops.paganin([I[k].clone() for k in range(3)], [W[k].clone() for k in range(3)], [alpha] * 3, [mu] * 3, plan)
    # bin slices of [nbins, n, m] stacks, as the chains return them
    c = ops.paganin([torch.stack([I[k] * 0.5, I[k]])[1] for k in range(3)], [torch.stack([W[k] * 2, W[k]])[1] for k in range(3)],
                    alpha, mu, plan)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = ops.paganin(I, W, alpha, mu, plan)
    torch.cuda.current_stream().wait_stream(side)
    for x in (b, c, d):
        for u, v in zip(a, x):
            assert torch.equal(u, v)
    # out=: stacks, lists, one map only; a second call of the same shape allocates nothing
    outs = (torch.empty_like(a[0]), [torch.empty((n, m), dtype=torch.float32, device="cuda") for _ in range(3)])
    got = ops.paganin(I, W, alpha, mu, plan, out=outs)
    torch.cuda.synchronize()
    assert got[0] is outs[0] and got[1] is outs[1]
    mem, nbytes = torch.cuda.memory_allocated(), plan.bytes
    ops.paganin(I, W, alpha, mu, plan, out=outs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem and len(retrieval._plans) == 1
    assert plan.bytes == nbytes and ops.lib().psx_integrate_plan_bytes(plan._h) == nbytes
    assert torch.equal(outs[0], a[0]) and all(torch.equal(outs[1][k], a[1][k]) for k in range(3))
    only = ops.paganin(I, W, alpha, mu, plan, out=(None, torch.empty_like(a[1])))
    assert only[0] is None and torch.equal(only[1], a[1])
    with pytest.raises(PsxError, match="neither contact nor thickness"):
        ops.paganin(I, W, alpha, mu, plan, out=(None, None))
    with pytest.raises(PsxError, match="shape"):
        ops.paganin(I[:, :-1].contiguous(), None, alpha, mu, plan)
    # the C entry's own checks
    from ctypes import c_double
    lib = ops.lib()
    p3, ok = ops._ptrs([I[0]]), (c_double * 1)(1.0)
    for args, msg in (((None, 1, p3, None, ok, ok, ops._ptrs([outs[0][0]]), None), "null plan"),
                      ((plan._h, 0, p3, None, ok, ok, ops._ptrs([outs[0][0]]), None), "B=0"),
                      ((plan._h, 65, p3, None, ok, ok, ops._ptrs([outs[0][0]]), None), "B=65"),
                      ((plan._h, 1, p3, None, (c_double * 1)(-1.0), ok, ops._ptrs([outs[0][0]]), None), "alpha"),
                      ((plan._h, 1, p3, None, ok, (c_double * 1)(0.0), ops._ptrs([outs[0][0]]), None), "mu"),
                      ((plan._h, 1, p3, None, ok, (c_double * 1)(float("nan")), ops._ptrs([outs[0][0]]), None), "mu"),
                      ((plan._h, 1, ops._ptrs([None]), None, ok, ok, ops._ptrs([outs[0][0]]), None), "image 0 is null"),
                      ((plan._h, 1, p3, None, ok, ok, None, None), "neither"),
                      ((plan._h, 1, p3, None, ok, ok, ops._ptrs([None]), None), "neither")):
        assert lib.psx_paganin_f32(*args, None) != 0
        assert msg in lib.psx_last_error().decode()


def _blob_run(sim):
    """The blob experiment (tests/_paganin_oracle.blob_cfg) through the GPU chain -> (Propag, White) of bin 0, cfg, T."""
    from tests._build import build_experiment
    cfg, T = po.blob_cfg()
    exp = build_experiment(cfg, sim)
    exp.myMembrane.myGeometry = np.zeros((2, 400, 400), dtype=np.float32)
    exp.exp_dict["meanEnergy"] = 0
    out = exp.computeSampleAndReferenceImages(0)
    return out[2][0].float().contiguous(), out[3][0].float().contiguous(), cfg, T


@pytest.mark.parametrize("sim", ["RT", "Fresnel"])
def test_end_to_end_blob_pins_alpha(sim):
    """Magnification 2, no membrane, a Gaussian blob of nylon: max|thickness - bin2(T)|/max T <= 0.08 with alpha = z*M*delta/
    (mu*p^2).  CPU calibration (tests/test_paganin_host.py): ray tracing 0.042, Fresnel 0.034; with z in place of z*M 0.13 and
    0.18, with z/M 0.22 and 0.28, without a filter 0.36 and 0.96 -- every wrong power of M misses the cap."""
    from paresis_amd import retrieval
    P, W, cfg, T = _blob_run(sim)
    kw = po.blob_params(cfg)
    r = retrieval.paganin(P, W, **kw)
    err = po.blob_error(_np(r['thickness']), T)
    from paresis_amd.getk import getk
    phi_t = -getk(kw['energy_keV'] * 1e3) * kw['delta'] * po.bin2(T)
    ephi = float(np.abs(_np(r['phi']) - phi_t).max() / np.abs(phi_t).max())
    wrong = po.blob_error(_np(retrieval.paganin(P, W, **dict(kw, magnification=1.0))['thickness']), T)
    print("blob %s on the GPU: thickness error %.4f, phi %.4f; with M = 1 in alpha %.4f" % (sim, err, ephi, wrong))
    assert err <= 0.08 and ephi <= 0.08
    assert wrong > 0.08
    o = po.paganin(_np(P), _np(W), *retrieval.paganin_alpha(**kw))          # and the kernel is the oracle on the chain's images
    rc, rt = _ratios((r['contact'], r['thickness']), o, retrieval.paganin_alpha(**kw)[1])
    assert rc <= 1.0 and rt <= 1.0


def _wire_truth():
    from paresis_amd.Experiment import Experiment
    exp = Experiment({"experimentName": "Fil_Nylon_ID17", "filepath": "/tmp/", "overSampling": 2, "nbExpPoints": 1,
                      "simulation_type": "RayT", "noise": False})
    return po.bin2(np.asarray(_np(exp.mySampleofInterest.myGeometry)[0], dtype=np.float64))


@pytest.mark.parametrize("sim", ["RayT", "Fresnel"])
def test_main_retrieve_propagation_writes_maps(sim, tmp_path):
    """main.run(propagation=True) on Fil_Nylon_ID17, one position, ov 2, no noise: the three files, the API's bits, the CLI's
    bits, and rms thickness error over max T <= 0.12 (CPU reference 0.078 ray tracing, 0.057 Fresnel; 1.07 and 1.64 without
    the filter).  The wire is not in the near field (I/I0 reaches 2 to 3): a plumbing check, not an accuracy claim."""
    from paresis_amd import main, retrieval
    from paresis_amd.InputOutput.pagailleIO import openImage
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": str(tmp_path) + "/" + sim + "/", "overSampling": 2,
          "nbExpPoints": 1, "simulation_type": sim, "noise": False, "seed": 3}
    os.makedirs(ed["filepath"], exist_ok=True)
    res = main.run(ed, save=True, saving_format=".tif", propagation=True)
    files = sorted(glob.glob(ed["filepath"] + "*/propag/retrieval/*.tif"))
    assert sorted(os.path.basename(f).split("_")[0] for f in files) == ["contact", "phi", "thickness"], files
    assert not glob.glob(ed["filepath"] + "*/retrieval")                           # the trackers' directory: --retrieve only
    pp = ed['propagationParams']
    assert pp['material'] == "Nylon"
    assert (pp['alpha'], pp['mu']) == retrieval.paganin_alpha(pp['delta'], pp['beta'], pp['energy_keV'], pp['pixel_um'],
                                                              pp['distance_m'], pp['magnification'])
    params = {k: pp[k] for k in ('energy_keV', 'pixel_um', 'distance_m', 'magnification')}
    for want in (retrieval.retrieve_propagation(res, params, "Nylon")[0],
                 retrieval.retrieve_propagation(res, params, (pp['delta'], pp['beta']))[0]):
        for f in files:
            img = openImage(f)
            assert img.shape == (200, 200)
            assert np.array_equal(img, _np(want[os.path.basename(f).split("_")[0]])), f
    T = _wire_truth()
    th = {os.path.basename(f).split("_")[0]: openImage(f) for f in files}['thickness']
    rms = float(np.sqrt(np.mean((th.astype(np.float64) - T) ** 2)) / T.max())
    print("main.run(propagation=True) %s: rms thickness error / max T = %.4f" % (sim, rms))
    assert rms <= 0.12
    # the CLI on the run's directory rewrites the same bits
    run_dir = os.path.dirname(os.path.dirname(os.path.dirname(files[0])))
    before = {f: openImage(f) for f in files}
    for f in files:
        os.remove(f)
    retrieval.main([run_dir, "--propagation", "--delta", repr(pp['delta']), "--beta", repr(pp['beta']),
                    "--energy", repr(pp['energy_keV']), "--pixel-um", repr(pp['pixel_um']), "--distance",
                    repr(pp['distance_m']), "--magnification", repr(pp['magnification'])])
    assert sorted(glob.glob(ed["filepath"] + "*/propag/retrieval/*.tif")) == files
    for f in files:
        assert np.array_equal(openImage(f), before[f]), f
    if sim == "RayT":
        # the default run writes no such directory; a wrong material fails before any image is computed
        ed2 = {"experimentName": "Fil_Nylon_ID17", "filepath": str(tmp_path) + "/default/", "overSampling": 2,
               "nbExpPoints": 1, "simulation_type": sim, "noise": False, "seed": 3}
        os.makedirs(ed2["filepath"], exist_ok=True)
        main.run(ed2, save=True, saving_format=".tif")
        assert glob.glob(ed2["filepath"] + "*/propag/PropagImage_*") and not glob.glob(ed2["filepath"] + "*/propag/retrieval")
        assert 'propagationParams' not in ed2
        with pytest.raises(ValueError, match="not one of the sample of interest's"):
            main.run(dict(ed, filepath=str(tmp_path) + "/bad/"), save=False, propagation=True, material="PMMA")
