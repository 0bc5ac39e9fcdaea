"""FDK on the GPU (csrc/fbp.hip: k_fdk_backproject behind ops.FdkPlan / ops.fdk / tomography.fdk) against the float64 oracle
of tests/_fdk_oracle.py, against the parallel back-projection at a far source, on the analytic ball, and through the chain:
scan(beam='cone') -> reconstruct, main.run and the command line."""
import glob

import numpy as np
import pytest
import torch

from tests import _fbp_oracle as fo
from tests import _fdk_oracle as fk
from tests import _volume_oracle as vo

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# -------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("flt", fk.FILTERS)
@pytest.mark.parametrize("shape", fk.SHAPES)
def test_fdk_matches_oracle(shape, flt):
    """max|vol - oracle| <= 8 * F32_ERROR[shape, dso / m] * max|oracle|, F32_ERROR the distance of the contract's float32
    restatement from the oracle on the CPU (tests/test_cone_host.py): at dso = m, 2.5 m and 1e6 m, the optical axis on the
    middle row, on a fractional row and off the detector, two centres, circle on and off in turn (masked voxels exactly 0); a
    second call returns the same bits."""
    from paresis_amd import ops
    A, n, m = shape
    theta, sino = fk.case_angles(A), fo.case_sino(A, n, m)
    s = _cuda(sino)
    mask = fo.circle_mask(m)
    worst = 0.0
    for i_f, factor in enumerate(fk.DSO_FACTORS):
        for i_v, vc in enumerate(fk.case_vcenters(n)):
            for i_c, center in enumerate(fo.case_centers(m)):
                ref = fk.fdk(sino, theta, factor * m, center, vc, flt, circle=False)
                bound = 8 * fk.F32_ERROR[shape, factor] * np.abs(ref).max()
                for circle in ((i_f + i_v + i_c) % 2 == 1,):          # on and off in turn: nine combinations each
                    plan = ops.FdkPlan(theta, n, m, factor * m, center=center, vcenter=vc, filter=flt, circle=circle)
                    assert plan.bytes >= 4 * A * n * m
                    vol = ops.fdk(s, plan)
                    assert vol.shape == (n, m, m) and vol.dtype == torch.float32
                    err = np.abs(_np(vol) - (ref * mask if circle else ref)).max()
                    worst = max(worst, err / bound)
                    assert err <= bound, (shape, flt, factor, vc, center, circle, err / bound)
                    if circle:
                        assert np.all(_np(vol)[:, ~mask] == 0)
                    assert torch.equal(plan.fdk(s), vol)
                    plan.close()
    print("fdk %s %s: worst error / bound = %.3f" % (shape, flt, worst))


FAR_SHAPES = [(36, 5, 33), (60, 9, 64)]


def _far_source_against_fbp(shape, sino, factor):
    """worst |ops.fdk at dso = factor * m - ops.fbp| / (8 * F32_ERROR[shape, 1e6] * max|ops.fbp|) over the three filters, the
    two centres and the three optical rows; the float32 cost of the far source does not depend on how far it is."""
    from paresis_amd import ops
    A, n, m = shape
    theta, s = fk.case_angles(A), _cuda(sino)
    worst = 0.0
    for flt in fk.FILTERS:
        for center in fo.case_centers(m):
            want = _np(ops.fbp(s, ops.FbpPlan(theta, m, center=center, filter=flt, circle=False)))
            bound = 8 * fk.F32_ERROR[shape, 1e6] * np.abs(want).max()
            for vc in fk.case_vcenters(n):
                got = _np(ops.fdk(s, ops.FdkPlan(theta, n, m, factor * m, center=center, vcenter=vc, filter=flt, circle=False)))
                worst = max(worst, np.abs(got - want).max() / bound)
    return worst


@pytest.mark.parametrize("shape", FAR_SHAPES)
def test_far_source_is_the_parallel_back_projection(shape):
    """At dso = 1e6 m the volume is ops.fbp's on the same sinogram, within the parity bound -- on fk.smooth_sino, where the
    geometry's own difference at that distance is a third of the bound (see there)."""
    worst = _far_source_against_fbp(shape, fk.smooth_sino(*shape), 1e6)
    print("fdk at 1e6 m against fbp %s, smooth sinogram: worst difference / bound = %.3f" % (shape, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("shape", FAR_SHAPES)
def test_far_source_on_the_parity_sinogram(shape):
    """The same on the parity cases' own fo.case_sino, whose filtered lines jump from sample to sample: there the geometry's
    own difference from the parallel beam is 5.3e-6 and 1.5e-5 of the peak at dso = 1e6 m (the oracle pair on the CPU, at
    the two shapes), above the parity bound of 2.7e-6 and 3.3e-6.  It falls as 1/dso, so at dso = 1e8 m it is 5.3e-8 and
    1.5e-7, a twentieth of the bound, and the volume is ops.fbp's within the bound; at 1e6 m it stays within 8 times the
    bound (the geometric term is 4.6 times it at most, the float32 terms of the two kernels below one each)."""
    sino = fo.case_sino(*shape)
    far, nearer = _far_source_against_fbp(shape, sino, 1e8), _far_source_against_fbp(shape, sino, 1e6)
    print("fdk against fbp %s, parity sinogram: worst difference / bound = %.3f at 1e8 m, %.3f at 1e6 m" % (shape, far, nearer))
    assert far <= 1.0 and nearer <= 8.0


def test_repeatability_row_blocks_and_plan_cache():
    """Two calls and a call into `out` give the same bits; 70 detector rows go through the filter in two row blocks and
    through the back-projector in nine slice blocks, within 8 times the float32 restatement's distance from the oracle,
    measured here; tomography.fdk keeps one plan per geometry and takes a sequence of maps."""
    from paresis_amd import ops, tomography
    A, n, m = 3, 70, 8
    theta, sino = fk.case_angles(A), fo.case_sino(A, n, m)
    s = _cuda(sino)
    plan = ops.FdkPlan(theta, n, m, 2.0 * m, vcenter=33.3, filter="hann")
    vol = ops.fdk(s, plan)
    out = torch.empty_like(vol)
    assert ops.fdk(s, plan, out=out) is out and torch.equal(out, vol) and torch.equal(plan.fdk(s), vol)
    ref = fk.fdk(sino, theta, 2.0 * m, None, 33.3, "hann")
    yard = np.abs(fk.fdk_f32(sino, theta, 2.0 * m, None, 33.3, "hann") - ref).max()
    err = np.abs(_np(vol) - ref).max()
    print("70 rows: error / (8 * float32 restatement's) = %.3f (restatement %.2e of the peak)" % (err / (8 * yard), yard / np.abs(ref).max()))
    assert 0 < yard and err <= 8 * yard
    for lo in range(0, n, 8):                                         # every slice block, and both row blocks, hold data
        assert np.abs(_np(vol)[lo:lo + 8]).max() > 0.1 * np.abs(ref).max()
    tomography._fdk_plans.clear()
    a = tomography.fdk(s, theta, 2.0 * m, row_center=33.3, filter="hann")
    assert torch.equal(a, vol) and len(tomography._fdk_plans) == 1
    assert torch.equal(tomography.fdk(list(s), theta, 2.0 * m, row_center=33.3, filter="hann"), vol) and len(tomography._fdk_plans) == 1
    tomography.fdk(s, theta, 2.5 * m, row_center=33.3, filter="hann")
    assert len(tomography._fdk_plans) == 2
    with pytest.raises(ops.PsxError, match="expected"):
        ops.fdk(s[:, :5].contiguous(), plan)
    with pytest.raises(ops.PsxError, match="dso="):
        ops.FdkPlan(theta, n, m, m - 0.5)


@pytest.mark.parametrize("flt", fk.FILTERS)
def test_a_voxel_keeps_its_bits_in_any_slice_block(flt):
    """Zero rows appended to the sinogram (n -> n + k at the same centre, optical row and distance; n and k even, so that the
    appended rows fill row pairs of their own and filter to exact zeros) leave the pre-weights, the filtered rows and the
    taps of slices 0 .. n - 1 what they were, and a zero sample adds +0 to a sum: vol[:n] has to keep its bits.  What
    changes is the back-projector's launch: the last slices sit in a tail block of 6 (n = 70), in a full block (72), in
    tails of 4 (76) and 2 (66, the sinogram's last four rows zeroed for both), and 136 rows take a third filter row block."""
    from paresis_amd import ops
    A, n, m = 5, 70, 17
    theta, sino = fk.case_angles(A), fo.case_sino(A, n, m)

    def run(rows, keep=n):
        padded = np.zeros((A, rows, m), dtype=np.float32)
        padded[:, :min(keep, rows)] = sino[:, :min(keep, rows)]
        plan = ops.FdkPlan(theta, rows, m, 1.5 * m, center=m / 2 - 0.25, vcenter=33.3, filter=flt, circle=False)
        return ops.fdk(_cuda(padded), plan)

    base = run(n)
    assert float(base[64:].abs().max()) > 0 and float(base[:8].abs().max()) > 0
    for rows in (72, 76, 80, 136):
        assert torch.equal(run(rows)[:n], base), (flt, rows)
    short = run(66, keep=66)
    assert torch.equal(run(n, keep=66)[:66], short) and not torch.equal(base[:66], short)


def test_ball():
    """The analytic ball of tests/test_cone_host.py through tomography.fdk: the same figure, the same bound."""
    from paresis_amd import tomography
    from tests.test_cone_host import BALL_ERROR
    sino, theta = fk.ball_cone_sino(), fk.full_turn(fk.BALL_ANGLES)
    vol = tomography.fdk(_cuda(sino), theta, fk.BALL_DSO)
    err = fk.ball_error(_np(vol))
    print("ball through tomography.fdk: %.3e (oracle %.3e, bound %.3e)" % (err, BALL_ERROR, 2 * BALL_ERROR))
    assert err <= 2 * BALL_ERROR


# --------------------------------------------------------------------------------------------------- chain
CH_DIMX, CH_M, CH_OV, PIX_UM, E_KEV = 32, 64, 2, 500.0, 52.0
CH_DELTA, CH_BETA = (8.7e-8, 1.4e-7), (6.0e-11, 1.5e-10)            # beta in the ratio of vo.CHIRAL_VALUES
CH_ROWS = (8, 24)                                                    # the slices that hold the chiral slice
CH_ANGLES = 60
CH_SOURCE = (0.08, 0.016, 0.0036)                                    # source-membrane, membrane-object, object-detector (m)


def _chiral_volume():
    vol = np.zeros((CH_DIMX, CH_M, CH_M), dtype=np.uint8)
    vol[CH_ROWS[0]:CH_ROWS[1]] = vo.chiral_slice(CH_M)
    return vol


def _close_experiment():
    """tests/test_gpu_volume.py's chiral experiment with the source 0.096 m from the axis: 192 study voxels of 500 um, three
    times the slice's width (96 voxels of the 16 x 32 detector's 1 mm); M = 1.0375."""
    from oracle import paresis_oracle as orc
    from tests._build import build_experiment
    from tests.test_gpu_volume import _membrane_maps
    dSM, dMO, dOD = CH_SOURCE
    M = (dSM + dMO + dOD) / (dSM + dMO)
    cfg = dict(scintillator=None, dSM=dSM, dMO=dMO, dOD=dOD, meanShotCount=30000.0, ov=CH_OV, pix_um=PIX_UM, M=M,
               inVacuum=True, N=(CH_DIMX, CH_M), spectrum=[(E_KEV, 1.0)], source_size_um=0.0, energy_sampling=1.0,
               det_dims=(CH_DIMX // 2, CH_M // 2), det_pix_um=PIX_UM * 2 * M, psf=0.0, bins=[],
               membrane=orc.Obj(_membrane_maps(0), [[5.0e-7], [9.9e-8]], [[3.0e-9], [5.3e-11]]),
               sample=orc.Obj(np.zeros((2, CH_DIMX, CH_M)), [[d] for d in CH_DELTA], [[b] for b in CH_BETA]),
               air=None, plate=None)
    exp = build_experiment(cfg, "RT", sample_materials=["square", "ell"])
    exp.exp_dict["nbExpPoints"] = 1
    s = exp.mySampleofInterest
    s.myGeometryFunction, s.myVolume, s.myVoxelSize = "getVolumeFromFile", _chiral_volume(), PIX_UM
    return exp


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_cone_scan_comes_back_through_fdk():
    """scan(beam='cone') (attenuation, ray tracing, 60 angles on the full turn, one position, dso = 3 m) -> reconstruct: the
    slice of detector row 8 correlates with the block-averaged labels, and more strongly than ops.fbp's parallel
    reconstruction of the same cone sinograms.  The oracle pair on the CPU (tests/_cone_oracle.py's projection of the same
    volume, block-averaged to the detector, through fk.fdk and fo.fbp) gives 0.9571 and 0.9488 at that row: the threshold
    is set below the first, and the order is asserted."""
    from paresis_amd import tomography
    exp = _close_experiment()
    angles = np.arange(CH_ANGLES) * (360.0 / CH_ANGLES)
    sample = exp.mySampleofInterest
    assert sample.mySourceDistance is None
    sc = tomography.scan(exp, angles, beam='cone')
    assert sample.mySourceDistance is None                            # restored
    m = CH_M // CH_OV
    assert sc['beam'] == 'cone' and sc['center'] == 15.75 and sc['row_center'] == tomography.optical_row(exp) == 7.75
    assert abs(sc['source_px'] - 3.0 * m) < 1e-9 and abs(tomography.source_distance(exp) - 0.096) < 1e-15
    assert sc['sinograms'][0].shape == (CH_ANGLES, CH_DIMX // 2, m)
    flat = tomography.scan(exp, angles[:2])
    assert 'beam' not in flat and 'source_px' not in flat and not torch.equal(flat['sinograms'][0], sc['sinograms'][0][:2])
    mu = _np(tomography.reconstruct(sc)[0])
    assert mu.shape == (CH_DIMX // 2, m, m)
    parallel = _np(tomography.fbp(sc['sinograms'][0], angles, center=sc['center']))
    k = 2 * np.pi * E_KEV * 1e3 * 1.6e-19 / (6.626e-34 * 2.998e8)
    mu_true = 2 * k * np.array((0.0,) + CH_BETA)
    truth = mu_true[vo.chiral_slice(CH_M)].reshape(m, CH_OV, m, CH_OV).mean(axis=(1, 3))
    own, flat_beam = _corr(mu[8], truth), _corr(parallel[8], truth)
    print("correlation with the truth: FDK %.4f (oracle 0.9571), parallel fbp of the same sinograms %.4f (oracle 0.9488); "
          "mu of the ell %.1f of %.1f 1/m" % (own, flat_beam, mu[8][23, 11], mu_true[2]))
    assert own > 0.94 and own > flat_beam
    assert np.abs(mu[0]).max() < 0.1 * mu_true[1]                     # study rows 0, 1: no label, and none seen from there
    # the rules
    with pytest.raises(ValueError, match="no differential form"):
        tomography.scan(exp, angles, modality='phase', differential=True, beam='cone')
    with pytest.raises(ValueError, match="method 'sirt' has no cone-beam form"):
        tomography.reconstruct(sc, method='sirt', iterations=2)
    sample.myGeometryFunction = "generateContrastPhantom"
    with pytest.raises(ValueError, match="a diverging beam needs a getVolumeFromFile sample"):
        tomography.scan(exp, angles[:1], beam='cone')
    sample.myGeometryFunction = "getVolumeFromFile"


def test_project_from_a_point_source():
    """tomography.project(source_distance_m=...) is the divergent kernel's projection, and leaves the sample parallel."""
    from paresis_amd import ops, tomography
    exp = _close_experiment()
    s = exp.mySampleofInterest
    got = tomography.project(s, E_KEV, [30.0], (CH_DIMX, CH_M), PIX_UM, source_distance_m=0.096)
    assert s.mySourceDistance is None
    lab = torch.from_numpy(_chiral_volume()).cuda()
    geom = ops.volume_project(lab, 2, 30.0, (CH_DIMX, CH_M), 1.0, PIX_UM * 1e-6, dso=0.096 * 1e6 / PIX_UM)
    from paresis_amd.getk import getk
    k = getk(E_KEV * 1e3)
    want = 2 * k * (CH_BETA[0] * _np(geom[0]) + CH_BETA[1] * _np(geom[1]))
    assert np.abs(_np(got['logT'][0]) - want).max() <= 1e-3 * want.max() and want.max() > 0
    flat = tomography.project(s, E_KEV, [30.0], (CH_DIMX, CH_M), PIX_UM)
    assert np.abs(_np(flat['logT'][0]) - want).max() > 0.05 * want.max()


def test_main_and_command_line_write_the_cone_volume(tmp_path):
    """main.run(tomography=6, tomography_beam='cone') on tests/test_gpu_volume.py's XML directory (the ID17 distances: a
    source 141.6 m away, 4.9e7 voxels): the angles lie on the full turn, exp_dict['tomographyVolumes'] and mu_<expID>.npy
    hold the bits of scan(beam='cone') + reconstruct through the API, and the command line writes the same file."""
    from paresis_amd import main, tomography
    from paresis_amd.Experiment import Experiment
    from tests.test_gpu_volume import _write_xml
    M = (140.0 + 1.6 + 3.6) / (140.0 + 1.6)
    voxel_um = 6.0 / CH_OV / M
    np.save(str(tmp_path / "chiral.npy"), _chiral_volume())
    xml = _write_xml(tmp_path, str(tmp_path / "chiral.npy"), voxel_um)

    def exp_dict(out):
        return {"experimentName": "Chiral_volume_ID17", "filepath": str(tmp_path / out) + "/", "overSampling": CH_OV,
                "nbExpPoints": 1, "simulation_type": "RayT", "noise": False, "xmlDir": xml}

    ed = exp_dict("run")
    main.run(ed, save=True, saving_format=".npy", tomography=6, tomography_beam='cone')
    tp = ed['tomographyParams']
    assert tp['angles'] == [0.0, 60.0, 120.0, 180.0, 240.0, 300.0] and tp['beam'] == 'cone' and tp['row_center'] == 7.75
    assert abs(tp['source_px'] - 141.6 / (6e-6 / M)) < 1e-3
    exp = Experiment(exp_dict("api"))
    want = tomography.reconstruct(tomography.scan(exp, tp['angles'], beam='cone'))[0]
    assert want.shape == (CH_DIMX // 2, CH_M // 2, CH_M // 2) and float(want.abs().max()) > 0
    assert torch.equal(ed['tomographyVolumes'][0], want)
    files = glob.glob(str(tmp_path / "run") + "/*/tomography/mu_%s.npy" % ed['expID'])
    assert len(files) == 1 and np.array_equal(np.load(files[0]), want.cpu().numpy())
    main.main(["--experiment", "Chiral_volume_ID17", "--out", str(tmp_path / "cli"), "--xml", xml, "--oversampling", str(CH_OV),
               "--no-noise", "--format", ".npy", "--tomography", "6", "--tomography-beam", "cone"])
    files = glob.glob(str(tmp_path / "cli") + "/*/tomography/mu_*.npy")
    assert len(files) == 1 and np.array_equal(np.load(files[0]), want.cpu().numpy())
