"""Differential phase tomography on the GPU (csrc/fbp.hip's Hilbert filter step, ops.FbpPlan(filter='hilbert' |
'hilbert-hann'), tomography.fbp / scan(differential=True) / reconstruct, main.run) against the float64 oracle of
tests/_hilbert_oracle.py, against the ramp on analytic sinograms, on the phantom's own projections, and through the chain."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import _fbp_oracle as fo
from tests import _hilbert_oracle as ho
from tests._fbp_oracle import PHANTOM_DELTA
from tests._hilbert_oracle import F32_ERROR_HILBERT

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
@pytest.mark.parametrize("flt", ho.FILTERS)
@pytest.mark.parametrize("shape", ho.SHAPES)
def test_hilbert_fbp_matches_oracle(shape, flt, which_center):
    """max|vol - oracle| <= 8 * F32_ERROR_HILBERT[shape] * max|oracle|, the table the distance of the contract's float32
    restatement from the oracle on the CPU (tests/test_hilbert_host.py).  circle on and off (the oracle's slice times the
    mask: one reference for both; outside the circle exactly 0), then a second call on each plan with one row less: odd n
    and an unpaired last row (n = 1: once more with the same)."""
    from paresis_amd import ops
    A, n, m = shape
    theta, sino = fo.case_angles(A), fo.case_sino(A, n, m)
    center = fo.case_centers(m)[which_center]
    ref = ho.fbp(sino, theta, center, flt, circle=False)
    bound = 8 * F32_ERROR_HILBERT[shape] * np.abs(ref).max()
    mask = fo.circle_mask(m)
    s = _cuda(sino)
    n2 = max(1, n - 1)
    s2 = s[:, :n2].contiguous()
    worst = 0.0
    for circle in (False, True):
        plan = ops.FbpPlan(theta, m, center=center, filter=flt, circle=circle)
        assert plan.bytes > 0 and plan.filter == flt
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


# -------------------------------------------------------------------------------------------------- bits
def test_same_bits_twice_in_row_blocks_and_the_pair_ignores_the_filter():
    """Two calls give the same bits; a plan capped at 2 rows per pass walks 5 rows in three blocks and gives the bits of the
    uncapped plan at (33, 5, 301); ops.fbp_adjoint on a 'hilbert' plan is the 'none' plan's, bit for bit, and so is
    ops.fbp_project: the pair ignores the plan's filter."""
    from paresis_amd import ops, tomography
    A, n, m = 33, 5, 301
    theta, s = fo.case_angles(A), _cuda(fo.case_sino(A, n, m))
    for flt in ho.FILTERS:
        plan = ops.FbpPlan(theta, m, filter=flt)
        whole = ops.fbp(s, plan)
        assert torch.equal(ops.fbp(s, plan), whole) and float(whole.abs().max()) > 0
        capped = ops.FbpPlan(theta, m, filter=flt, max_rows=2)
        assert capped.bytes < plan.bytes
        assert torch.equal(ops.fbp(s, capped), whole)
        assert torch.equal(tomography.fbp(s, theta, filter=flt), whole)
    none, hilbert = ops.FbpPlan(theta, m, filter="none"), ops.FbpPlan(theta, m, filter="hilbert")
    back = ops.fbp_adjoint(s, none)
    assert torch.equal(ops.fbp_adjoint(s, hilbert), back) and float(back.abs().max()) > 0
    assert torch.equal(ops.fbp_project(back, hilbert), ops.fbp_project(back, none))
    assert not torch.equal(ops.fbp(s, hilbert), ops.fbp(s, ops.FbpPlan(theta, m, filter="ramp")))


# ----------------------------------------------------------------------------------- the right operator
@pytest.mark.parametrize("case", [ho.BLOB_CASES[0], ho.BLOB_CASES[3]], ids=lambda c: "m%d-A%d" % c[:2])
def test_hilbert_of_the_derivative_is_the_ramp_on_the_device(case):
    """Analytic p and dp/du of three Gaussian blobs: max|fbp(dp/du, 'hilbert') - fbp(p, 'ramp')| on the GPU within the float64
    oracles' own gap on these (float32) inputs plus 8 times the float32 yardstick of either side, all times max|ramp|.  The
    yardsticks are the two restatements' distances from their oracles on these inputs."""
    from paresis_amd import tomography
    m, A, center, _ = case
    theta, p, dp = ho.blob_sinograms(m, A, center)
    p, dp = p.astype(np.float32), dp.astype(np.float32)
    ramp64, hilb64 = fo.fbp(p, theta, center, "ramp"), ho.fbp(dp, theta, center, "hilbert")
    peak = np.abs(ramp64).max()
    gap = np.abs(hilb64 - ramp64).max() / peak
    y_ramp = np.abs(fo.fbp_f32(p, theta, center, "ramp") - ramp64).max() / peak
    y_hilb = np.abs(ho.fbp_f32(dp, theta, center, "hilbert") - hilb64).max() / np.abs(hilb64).max()
    bound = (gap + 8 * (y_ramp + y_hilb)) * peak
    ramp = _np(tomography.fbp(_cuda(p), theta, center=center, filter="ramp"))
    hilb = _np(tomography.fbp(_cuda(dp), theta, center=center, filter="hilbert"))
    err = np.abs(hilb - ramp).max()
    print("blobs m=%d A=%d: oracles' gap %.3e, yardsticks ramp %.3e hilbert %.3e; GPU error / bound = %.3f (bound %.3e, "
          "peak %.3f)" % (m, A, gap, y_ramp, y_hilb, err / bound, bound, peak))
    assert 0 < y_ramp < 1e-5 and 0 < y_hilb < 1e-5
    assert err <= bound
    assert np.abs(hilb + ramp).max() > 1.9 * peak                    # the other sign would have missed by the whole volume


# ----------------------------------------------------------------------------------- the phantom's own data
def _phantom_sample():
    from paresis_amd.Sample import AnalyticalSample
    s = AnalyticalSample()
    s.myName, s.myType, s.myMaterials = "phantom", "sample_of_interest", ["m%d" % i for i in range(13)]
    s.myGeometryFunction = "generateContrastPhantom"
    s.delta = [[(E_KEV, d)] for d in PHANTOM_DELTA]
    s.beta = [[(E_KEV, b)] for b in PHANTOM_BETA]
    return s


def test_delta_known_answer_from_the_gradient():
    """project -> central differences of phi along axis 2 (torch) -> fbp(filter='hilbert') -> delta_volume: in rows [12, 22)
    the mean over each material's interior pixels is within 3 % of the largest delta of that material's delta -- twice the
    1.48 % of the float64 oracle on the restated phantom (tests/test_hilbert_host.py) --, first for the oracle on this
    differentiated sinogram, then for the GPU; rows whose sinogram is zero reconstruct to exactly 0."""
    from paresis_amd import tomography
    angles = np.arange(90) * 2.0
    phi = tomography.project(_phantom_sample(), E_KEV, angles, (DIMX, DIMY), PIX_UM)['phi']
    pad = torch.nn.functional.pad(phi, (1, 1))
    dphi = (0.5 * (pad[:, :, 2:] - pad[:, :, :-2])).contiguous()
    assert dphi.shape == (90, DIMX, DIMY) and dphi.dtype == torch.float32
    vol = tomography.fbp(dphi, angles, filter='hilbert')
    delta = _np(tomography.delta_volume(vol, E_KEV, PIX_UM * 1e-6))
    slices = fo.phantom_slices(DIMY, PIX_UM)
    dmax = max(PHANTOM_DELTA)
    k = 2 * np.pi * E_KEV * 1e3 * 1.6e-19 / (6.626e-34 * 2.998e8)
    oref = ho.fbp(_np(dphi[:, 12:22]), angles) * (-1.0 / (k * PIX_UM * 1e-6))
    eref = max(abs(oref[r][fo.interior(slices[m])].mean() - PHANTOM_DELTA[m]) / dmax for r in range(10) for m in range(13))
    err = max(abs(delta[r][fo.interior(slices[m])].mean() - PHANTOM_DELTA[m]) / dmax for r in range(12, 22) for m in range(13))
    print("delta from the gradient: worst interior mean error / max delta: oracle %.4f, GPU %.4f" % (eref, err))
    assert eref <= 0.03
    assert err <= 0.03
    empty = [r for r in range(DIMX) if float(dphi[:, r].abs().max()) == 0.0]
    assert empty == [0, 1, 22, 23]
    assert float(vol[empty].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------------- chain
def _membrane_maps(point):
    """The two membrane layers at position `point`: a smooth pattern that differs from position to position."""
    i, j = np.mgrid[0:DIMX, 0:DIMY]
    pattern = np.sin(0.9 * i + 0.3 + 1.7 * point) * np.cos(0.7 * j + 0.9 * point)
    return np.stack([2e-6 * (1 + 0.5 * pattern), np.full((DIMX, DIMY), 1e-4)]).astype(np.float32)


def _phantom_experiment(npos):
    """tests/test_gpu_fbp.py's, restated: a 24 x 64 study grid of 500 um pixels (oversampling 2: a 12 x 32 detector),
    monochromatic, in vacuum, no plate, no blur, the contrast phantom as the sample, and a two-layer membrane whose geometry
    function hands out _membrane_maps per position."""
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


def test_differential_scan_is_the_tracked_gradient_per_angle():
    """scan(modality='phase', differential=True), 4 angles, 3 positions: every map is the dy of retrieval.retrieve without
    parameters (no integration) times gradient_scale for that angle's run, bit for bit; reconstruct is delta_volume of the
    'hilbert' back-projection about the scan's centre, bit for bit."""
    from paresis_amd import retrieval, tomography
    angles = [0.0, 45.0, 90.0, 135.0]
    sc = tomography.scan(_phantom_experiment(3), angles, modality='phase', differential=True, max_shift=2.0)
    sino = sc['sinograms'][0]
    assert sino.shape == (4, DIMX // 2, DIMY // 2) and sc['modality'] == 'phase' and sc['differential'] is True
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
        r = retrieval.retrieve(results, None, max_shift=2.0)[0]
        assert 'phi' not in r
        want = r['dy'] * retrieval.gradient_scale(**retrieval.params_from_experiment(exp))
        assert torch.equal(sino[a], want), angle
    assert float(sino.abs().max()) > 0
    vol = tomography.reconstruct(sc)[0]
    want = tomography.delta_volume(tomography.fbp(sino, angles, center=sc['center'], filter='hilbert'), sc['energy_keV'], sc['voxel_m'])
    assert torch.equal(vol, want) and float(vol.abs().max()) > 0
    hann = tomography.delta_volume(tomography.fbp(sino, angles, center=sc['center'], filter='hilbert-hann'), sc['energy_keV'],
                                   sc['voxel_m'])
    assert torch.equal(tomography.reconstruct(sc, filter='hann')[0], hann) and not torch.equal(hann, want)
    integral = tomography.scan(_phantom_experiment(3), angles[:1], modality='phase', max_shift=2.0)
    assert integral['differential'] is False


# ------------------------------------------------------------------------------------- run and command line
def _injected(mp, seen):
    """main's Experiment -> the phantom experiment of 3 positions, sharing main's dictionary (kept in `seen`)."""
    from paresis_amd import Experiment as experiment_module
    exp = _phantom_experiment(3)
    exp.mySampleofInterest.getMyGeometry(exp.exp_dict['studyDimensions'], exp.exp_dict['studyPixelSize'], 2)

    def injected(exp_dict):
        for k, v in exp.exp_dict.items():
            exp_dict.setdefault(k, v)
        exp.exp_dict = exp_dict
        seen.append(exp_dict)
        return exp

    mp.setattr(experiment_module, "Experiment", injected)


def _want(angles):
    from paresis_amd import tomography
    return tomography.reconstruct(tomography.scan(_phantom_experiment(3), angles, modality='phase', differential=True))[0]


def _check_run(tmp_path, ed):
    files = sorted(glob.glob(str(tmp_path) + "/*/tomography/*"))
    assert [os.path.basename(f) for f in files] == ["delta_%s.npy" % ed['expID']], files
    tp = ed['tomographyParams']
    assert tp['differential'] is True and tp['modality'] == 'phase' and tp['method'] == 'fbp' and len(tp['angles']) == 6
    got = np.load(files[0])
    assert got.shape == (DIMX // 2, DIMY // 2, DIMY // 2) and got.dtype == np.float32
    assert np.array_equal(got, _want(tp['angles']).cpu().numpy()) and float(np.abs(got).max()) > 0


def test_main_run_differential_writes_delta(tmp_path, monkeypatch):
    """main.run(tomography=6, tomography_modality='phase', tomography_differential=True) writes tomography/delta_<expID>, the
    bits of scan(differential=True) + reconstruct through the API, and tomographyParams carries 'differential'."""
    from paresis_amd import main
    ed = {"experimentName": "injected", "filepath": str(tmp_path) + "/", "overSampling": 2, "nbExpPoints": 3,
          "simulation_type": "RayT", "noise": False}
    with monkeypatch.context() as mp:
        _injected(mp, [])
        main.run(ed, save=True, saving_format=".npy", tomography=6, tomography_modality='phase', tomography_differential=True)
    _check_run(tmp_path, ed)
    assert torch.equal(ed['tomographyVolumes'][0], _want(ed['tomographyParams']['angles']))


def test_cli_differential_writes_delta(tmp_path, monkeypatch):
    """--tomography 6 --tomography-modality phase --tomography-differential: the same through the command line."""
    from paresis_amd import main
    seen = []
    with monkeypatch.context() as mp:
        _injected(mp, seen)
        main.main(["--experiment", "injected", "--out", str(tmp_path), "--format", ".npy", "--no-noise", "--points", "3",
                   "--tomography", "6", "--tomography-modality", "phase", "--tomography-differential"])
    assert len(seen) == 1
    _check_run(tmp_path, seen[0])
