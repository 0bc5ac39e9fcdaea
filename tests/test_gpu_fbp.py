"""Filtered back-projection on the GPU (csrc/fbp.hip, ops.FbpPlan / ops.fbp, paresis_amd.tomography)
against the float64 numpy oracle of tests/_fbp_oracle.py, on the phantom's own projections, and through the chain."""
import numpy as np
import pytest
import torch

from tests import _fbp_oracle as fo
from tests._fbp_oracle import F32_ERROR, PHANTOM_DELTA

pytestmark = pytest.mark.gpu

# beta at 52 keV of the 13 materials, the stand-ins of tests/test_gpu_phantom.py (ID17_DELTA_BETA_52KEV), copied
PHANTOM_BETA = (1.9e-10, 1.6e-10, 1.75e-10, 6.0e-11, 5.2e-11, 7.5e-11, 5.6e-11, 6.4e-11, 1.5e-10, 6.1e-11, 7.0e-14, 7.0e-14, 6.0e-11)
DIMX, DIMY, PIX_UM, E_KEV = 24, 64, 500.0, 52.0


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# -------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("which_center", [0, 1])
@pytest.mark.parametrize("flt", fo.FILTERS)
@pytest.mark.parametrize("shape", fo.SHAPES)
def test_fbp_matches_oracle(shape, flt, which_center):
    """max|vol - oracle| <= 8 * F32_ERROR[shape] * max|oracle|, F32_ERROR the distance of the contract's float32 restatement
    from the oracle on the CPU (tests/test_fbp_host.py).  circle on and off (the oracle's slice times the mask: one
    reference for both), then a second call on each plan with one row less (n = 1: once more with the same)."""
    from paresis_amd import ops
    A, n, m = shape
    theta, sino = fo.case_angles(A), fo.case_sino(A, n, m)
    center = fo.case_centers(m)[which_center]
    ref = fo.fbp(sino, theta, center, flt, circle=False)
    bound = 8 * F32_ERROR[shape] * np.abs(ref).max()
    mask = fo.circle_mask(m)
    s = _cuda(sino)
    n2 = max(1, n - 1)
    s2 = s[:, :n2].contiguous()
    worst = 0.0
    for circle in (False, True):
        plan = ops.FbpPlan(theta, m, center=center, filter=flt, circle=circle)
        assert plan.bytes > 0
        want = ref * mask if circle else ref
        vol = ops.fbp(s, plan)
        assert vol.shape == (n, m, m) and vol.dtype == torch.float32
        e1 = np.abs(_np(vol) - want).max()
        e2 = np.abs(_np(plan.fbp(s2)) - want[:n2]).max()
        worst = max(worst, e1, e2)
        if circle:
            assert np.all(_np(vol)[:, ~mask] == 0)
        plan.close()
    print("fbp %s %s center %.2f: worst error / bound = %.3f (bound %.3e)" % (shape, flt, center, worst / bound, bound))
    assert worst <= bound


def test_row_blocks_and_plan_cache():
    """A plan capped at 2 rows per pass walks 5 rows in three blocks and gives the bits of the uncapped plan; the module keeps
    one plan per (device, A, m, angles, center, filter, circle); a sequence of maps is a stack."""
    from paresis_amd import ops, tomography
    A, n, m = 33, 5, 301
    theta, s = fo.case_angles(A), _cuda(fo.case_sino(A, n, m))
    whole = ops.fbp(s, ops.FbpPlan(theta, m, filter="hann"))
    capped = ops.FbpPlan(theta, m, filter="hann", max_rows=2)
    assert capped.bytes < ops.FbpPlan(theta, m, filter="hann", max_rows=6).bytes
    assert torch.equal(ops.fbp(s, capped), whole)
    out = torch.empty_like(whole)
    assert ops.fbp(s, capped, out=out) is out and torch.equal(out, whole)
    tomography._plans.clear()
    a = tomography.fbp(s, theta, filter="hann")
    b = tomography.fbp([s[k] for k in range(A)], list(theta), center=m // 2, filter="hann")
    assert len(tomography._plans) == 1 and torch.equal(a, whole) and torch.equal(b, whole)
    tomography.fbp(s, theta, filter="hann", circle=False)
    tomography.fbp(s, theta, center=m / 2 - 0.25, filter="hann")
    assert len(tomography._plans) == 3
    with pytest.raises(ops.PsxError, match="shape"):
        ops.fbp(s[:, :, :-1].contiguous(), capped)
    with pytest.raises(ops.PsxError, match="projections"):
        tomography.fbp(s, theta[:-1])


# ----------------------------------------------------------------------------------- the phantom's own data
@pytest.fixture(scope="module")
def angles90():
    return np.arange(90) * 2.0


def test_phantom_round_trip(angles90):
    """contrast_phantom_lines' thickness maps (one detector row of the 13 materials, metres) at 90 angles -> fbp: vol > 0.5*pix
    is contrast_phantom_slices on all but 0.1 % of the pixels at most, per material; first for the oracle on the same lines."""
    from paresis_amd import tomography
    from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_lines, contrast_phantom_slices
    row = DIMX // 2                                                # inside the tubes' and the support's rows
    sino = torch.stack([contrast_phantom_lines(DIMX, DIMY, PIX_UM, a)[0][:, row, :] for a in angles90]).contiguous()
    assert sino.shape == (90, 13, DIMY)
    slices = contrast_phantom_slices(DIMX, DIMY, PIX_UM, 30).cpu().numpy().astype(bool)
    assert np.array_equal(slices, fo.phantom_slices(DIMY, PIX_UM))          # the host tests' restatement is the kernel's
    half, cap = 0.5 * PIX_UM * 1e-6, int(0.001 * DIMY * DIMY)
    ref = fo.fbp(_np(sino), angles90)
    wrong_ref = [int(((ref[k] > half) != slices[k]).sum()) for k in range(13)]
    vol = _np(tomography.fbp(sino, angles90))
    wrong = [int(((vol[k] > half) != slices[k]).sum()) for k in range(13)]
    print("phantom round trip: misclassified pixels per material, oracle %s, GPU %s (cap %d)" % (wrong_ref, wrong, cap))
    assert max(wrong_ref) <= cap
    assert max(wrong) <= cap


def _phantom_sample():
    from paresis_amd.Sample import AnalyticalSample
    s = AnalyticalSample()
    s.myName, s.myType, s.myMaterials = "phantom", "sample_of_interest", ["m%d" % i for i in range(13)]
    s.myGeometryFunction = "generateContrastPhantom"
    s.delta = [[(E_KEV, d)] for d in PHANTOM_DELTA]
    s.beta = [[(E_KEV, b)] for b in PHANTOM_BETA]
    return s


def test_delta_known_answer(angles90):
    """project -> fbp -> delta_volume: in rows [12, 22) (tubes and support), the mean over each material's interior pixels is
    within 1 % of the largest delta of that material's delta (three times the float64 oracle's 0.3 % on a restated phantom;
    the oracle's figure on this sinogram is printed beside it); rows whose sinogram is zero reconstruct to exactly 0.
    Pins the sign, k and the voxel size."""
    from paresis_amd import tomography
    s = _phantom_sample()
    p = tomography.project(s, E_KEV, angles90, (DIMX, DIMY), PIX_UM)
    assert p['phi'].shape == p['logT'].shape == (90, DIMX, DIMY) and s.myAngle == 178.0
    assert float(p['phi'].min()) < -100 and float(p['logT'].max()) > 0.1
    vol = tomography.fbp(p['phi'], angles90)
    delta = _np(tomography.delta_volume(vol, E_KEV, PIX_UM * 1e-6))
    slices = fo.phantom_slices(DIMY, PIX_UM)
    dmax = max(PHANTOM_DELTA)
    err = max(abs(delta[r][fo.interior(slices[k])].mean() - PHANTOM_DELTA[k]) / dmax for r in range(12, 22) for k in range(13))
    oref = fo.fbp(_np(p['phi'][:, 12:13]), angles90)[0] * (-1.0 / (2 * np.pi * E_KEV * 1e3 * 1.6e-19 / (6.626e-34 * 2.998e8) * PIX_UM * 1e-6))
    eref = max(abs(oref[fo.interior(slices[k])].mean() - PHANTOM_DELTA[k]) / dmax for k in range(13))
    print("delta known answer: worst interior mean error / max delta: GPU %.4f, oracle on the same sinogram %.4f" % (err, eref))
    assert err <= 0.01
    empty = [r for r in range(DIMX) if float(p['phi'][:, r].abs().max()) == 0.0]
    assert empty == [0, 1, 22, 23]
    assert float(vol[empty].abs().max()) == 0.0
    mu = _np(tomography.mu_volume(tomography.fbp(p['logT'], angles90), PIX_UM * 1e-6))
    k = 2 * np.pi * E_KEV * 1e3 * 1.6e-19 / (6.626e-34 * 2.998e8)
    emu = max(abs(mu[15][fo.interior(slices[m])].mean() - 2 * k * PHANTOM_BETA[m]) for m in range(13)) / (2 * k * max(PHANTOM_BETA))
    print("mu known answer: worst interior mean error / max mu %.4f" % emu)
    assert emu <= 0.01


# -------------------------------------------------------------------------------------------------- chain
def _membrane_maps(point):
    """The two membrane layers at position `point`: a smooth pattern that differs from position to position."""
    i, j = np.mgrid[0:DIMX, 0:DIMY]
    pattern = np.sin(0.9 * i + 0.3 + 1.7 * point) * np.cos(0.7 * j + 0.9 * point)
    return np.stack([2e-6 * (1 + 0.5 * pattern), np.full((DIMX, DIMY), 1e-4)]).astype(np.float32)


def _phantom_experiment(npos):
    """A 24 x 64 study grid of 500 um pixels (oversampling 2: a 12 x 32 detector), monochromatic, in vacuum, no plate, no
    blur, the contrast phantom as the sample, and a two-layer membrane whose geometry function hands out _membrane_maps
    per position, as a membrane read from a file does in main.run."""
    from oracle import paresis_oracle as orc
    from tests._build import build_experiment
    M = (140.0 + 1.6 + 3.6) / (140.0 + 1.6)
    cfg = dict(scintillator=None, dSM=140.0, dMO=1.6, dOD=3.6, meanShotCount=30000.0, ov=2, pix_um=PIX_UM, M=M,
               inVacuum=True, N=(DIMX, DIMY), spectrum=[(E_KEV, 1.0)], source_size_um=0.0, energy_sampling=1.0,
               det_dims=(DIMX // 2, DIMY // 2), det_pix_um=PIX_UM * 2 * M, psf=0.0, bins=[],
               membrane=orc.Obj(_membrane_maps(0), [[5.0e-7], [9.9e-8]], [[3.0e-9], [5.3e-11]]),
               sample=orc.Obj(np.zeros((13, DIMX, DIMY)), [[d] for d in PHANTOM_DELTA], [[b] for b in PHANTOM_BETA]),
               air=None, plate=None)
    exp = build_experiment(cfg, "RT", sample_materials=["m%d" % k for k in range(13)])
    exp.exp_dict["nbExpPoints"] = npos
    exp.mySampleofInterest.myGeometryFunction = "generateContrastPhantom"
    mem = exp.myMembrane
    mem.myGeometryFunction, mem.membranePixelSize = "testPattern", PIX_UM

    def get_geometry(dims, pix, ov, pointNum=0, number_of_positions=0):
        mem.myGeometry = _membrane_maps(pointNum)

    mem.getMyGeometry = get_geometry
    return exp


def test_scan_attenuation_puts_the_tube_where_the_slice_has_it():
    """scan(modality='attenuation'), 30 angles, one position, ray tracing, no noise -> mu_volume: the centroid of the most
    attenuating tube (weights mu - mu_support, clipped at 0, within 3.5 detector pixels of where it should be: the next tube
    starts at 4) lies within 0.5 detector pixel of the slice's centroid, study pixel x -> voxel m // 2 + (x - dimY // 2)/ov."""
    from paresis_amd import tomography
    exp = _phantom_experiment(1)
    angles = np.arange(30) * 6.0
    sc = tomography.scan(exp, angles)
    assert sc['center'] == tomography.rotation_center(exp) == 15.75 and sc['modality'] == 'attenuation'
    assert sc['voxel_m'] == pytest.approx(PIX_UM * 2e-6, rel=1e-12) and sc['energy_keV'] == pytest.approx(E_KEV, rel=1e-6)
    assert list(sc['sinograms']) == [0] and sc['sinograms'][0].shape == (30, DIMX // 2, DIMY // 2)
    mu = _np(tomography.reconstruct(sc)[0])
    k = 2 * np.pi * E_KEV * 1e3 * 1.6e-19 / (6.626e-34 * 2.998e8)
    tube = int(np.argmax(PHANTOM_BETA))
    si, sj = np.nonzero(fo.phantom_slices(DIMY, PIX_UM)[tube])
    m = DIMY // 2
    ci, cj = m // 2 + (si.mean() - DIMY // 2) / 2, m // 2 + (sj.mean() - DIMY // 2) / 2
    i, j = np.mgrid[0:m, 0:m]
    row = mu[8]                                                   # detector row 8 = study rows 16, 17: tubes and support
    w = np.clip(row - 2 * k * PHANTOM_BETA[12], 0, None) * (np.hypot(i - ci, j - cj) <= 3.5)
    gi, gj = (w * i).sum() / w.sum(), (w * j).sum() / w.sum()
    print("tube %d: expected (%.3f, %.3f), centroid (%.3f, %.3f), peak mu %.1f of %.1f 1/m"
          % (tube, ci, cj, gi, gj, row[int(round(ci)), int(round(cj))], 2 * k * PHANTOM_BETA[tube]))
    assert np.hypot(gi - ci, gj - cj) <= 0.5


def test_scan_phase_is_retrieve_per_angle():
    """modality='phase', 4 angles, 3 positions: every map of the sinogram is retrieval.retrieve's phi of that angle's run, bit
    for bit."""
    from paresis_amd import retrieval, tomography
    angles = [0.0, 45.0, 90.0, 135.0]
    sc = tomography.scan(_phantom_experiment(3), angles, modality='phase', max_shift=2.0)
    assert sc['sinograms'][0].shape == (4, DIMX // 2, DIMY // 2) and sc['modality'] == 'phase'
    exp = _phantom_experiment(3)
    ed = exp.exp_dict
    for a, angle in enumerate(angles):
        exp.mySampleofInterest.myAngle = angle
        exp.mySampleofInterest.getMyGeometry(ed['studyDimensions'], ed['studyPixelSize'], ed['overSampling'])
        ed['meanEnergy'] = 0
        results = {}
        for p in range(3):
            exp.myMembrane.getMyGeometry(ed['studyDimensions'], PIX_UM, 2, p, 3)
            results[p] = exp.computeSampleAndReferenceImages(p)
        exp.resolve_mean_energy()
        want = retrieval.retrieve(results, retrieval.params_from_experiment(exp), max_shift=2.0)[0]['phi']
        assert torch.equal(sc['sinograms'][0][a], want), angle
    assert float(sc['sinograms'][0].abs().max()) > 0                   # three distinct positions: LCS has something to solve


def test_main_tomography_writes_the_volumes(tmp_path, monkeypatch):
    """main.run(tomography=6) on the phantom experiment: <run dir>/tomography/mu_<expID>.npy holds the bits of scan +
    reconstruct through the API, which exp_dict['tomographyVolumes'] holds too; the sample's other outputs are written as always."""
    import glob
    import os
    from paresis_amd import Experiment as experiment_module
    from paresis_amd import main, tomography

    exp = _phantom_experiment(1)
    exp.mySampleofInterest.getMyGeometry(exp.exp_dict['studyDimensions'], exp.exp_dict['studyPixelSize'], 2)

    def injected(exp_dict):
        for k, v in exp.exp_dict.items():
            exp_dict.setdefault(k, v)
        exp.exp_dict = exp_dict                                      # main.run and the experiment share one dictionary
        return exp

    ed = {"experimentName": "injected", "filepath": str(tmp_path) + "/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": "RayT", "noise": False}
    with monkeypatch.context() as mp:
        mp.setattr(experiment_module, "Experiment", injected)
        main.run(ed, save=True, saving_format=".npy", tomography=6)
    files = sorted(glob.glob(str(tmp_path) + "/*/tomography/*.npy"))
    assert [os.path.basename(f) for f in files] == ["mu_%s.npy" % ed['expID']], files
    assert glob.glob(str(tmp_path) + "/*/sample/sampleImage_*") and glob.glob(str(tmp_path) + "/*/propag/PropagImage_*")
    tp = ed['tomographyParams']
    assert tp['angles'] == [0.0, 30.0, 60.0, 90.0, 120.0, 150.0] and tp['center'] == 15.75 and tp['modality'] == 'attenuation'
    want = tomography.reconstruct(tomography.scan(_phantom_experiment(1), tp['angles']))[0]
    got = np.load(files[0])
    assert got.shape == (DIMX // 2, DIMY // 2, DIMY // 2) and got.dtype == np.float32
    assert np.array_equal(got, want.cpu().numpy()) and torch.equal(ed['tomographyVolumes'][0], want)
    assert float(np.abs(got).max()) > 10                              # 1/m: the support alone is 31.6
    with pytest.raises(ValueError, match="tomography_modality is an option"):
        main.run(dict(ed), save=False, tomography_modality="phase")
    with pytest.raises(ValueError, match="at least 3 positions"):
        main.run(dict(ed), save=False, tomography=4, tomography_modality="phase")
