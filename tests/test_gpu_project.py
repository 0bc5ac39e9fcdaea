"""The matched projector pair on the GPU (csrc/fbp.hip k_fbp_project, ops.fbp_project / ops.fbp_adjoint) and SIRT / CGLS on
it (paresis_amd.tomography) against the float64 numpy oracle of tests/_project_oracle.py, on the phantom's own lines, and
through reconstruct, main.run and the command line.  Every bound is 8 times the float32 restatement's distance from the
oracle, measured on the CPU (tests/test_project_host.py)."""
import numpy as np
import pytest
import torch

from tests import _fbp_oracle as fo
from tests import _project_oracle as po

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# -------------------------------------------------------------------------------------------------- the projector
@pytest.mark.parametrize("which_center", [0, 1])
@pytest.mark.parametrize("shape", po.SHAPES)
def test_project_matches_oracle(shape, which_center):
    """max|sino - oracle| <= 8 * F32_ERROR[shape] * max|oracle|, circle off and on (the oracle of the masked volume: one
    call for both); a second call returns the same bits."""
    from paresis_amd import ops
    A, n, m = shape
    theta, vol = po.case_angles(A), po.case_vol(A, n, m)
    center = fo.case_centers(m)[which_center]
    both = po.project(np.concatenate([vol, vol * fo.circle_mask(m)]), theta, center, circle=False)
    v = _cuda(vol)
    worst = 0.0
    for circle in (False, True):
        ref = both[:, n:] if circle else both[:, :n]
        bound = 8 * po.F32_ERROR[shape] * np.abs(ref).max()
        plan = ops.FbpPlan(theta, m, center=center, filter="none", circle=circle)
        sino = ops.fbp_project(v, plan)
        assert sino.shape == (A, n, m) and sino.dtype == torch.float32
        e = np.abs(_np(sino) - ref).max()
        print("project %s center %.2f circle %d: error / bound = %.3f (bound %.3e)" % (shape, center, circle, e / bound, bound))
        worst = max(worst, e / bound)
        out = torch.full_like(sino, float("nan"))
        assert plan.project(v, out=out) is out and torch.equal(out, sino)
        plan.close()
    assert worst <= 1.0


def test_project_ignores_the_filter_and_the_row_blocks():
    """A plan capped at 2 rows per pass gives the uncapped bits over 5 rows, for the projector and for the adjoint (which
    walks three blocks), on a filtered plan as on a 'none' one; one row alone gives the bits it has in the stack."""
    from paresis_amd import ops
    A, n, m = 33, 5, 301
    theta, v, s = po.case_angles(A), _cuda(po.case_vol(A, n, m)), _cuda(fo.case_sino(A, n, m))
    plain = ops.FbpPlan(theta, m, filter="none")
    sino, vol = ops.fbp_project(v, plain), ops.fbp_adjoint(s, plain)
    for flt in ("none", "hann"):
        capped = ops.FbpPlan(theta, m, filter=flt, max_rows=2)
        assert torch.equal(ops.fbp_project(v, capped), sino) and torch.equal(ops.fbp_adjoint(s, capped), vol)
        assert torch.equal(capped.adjoint(s), vol)
    assert torch.equal(ops.fbp_project(v[3:4].contiguous(), plain)[:, 0], sino[:, 3])
    assert torch.equal(ops.fbp_adjoint(s[:, 2:3].contiguous(), plain)[0], vol[2])
    with pytest.raises(ops.PsxError, match="shape"):
        ops.fbp_project(v[:, :, :-1].contiguous(), plain)
    with pytest.raises(ops.PsxError, match="shape"):
        ops.fbp_project(s, plain)
    with pytest.raises(ops.PsxError, match="shape"):
        ops.fbp_adjoint(v, plain)
    with pytest.raises(ops.PsxError, match="expected"):
        ops.fbp_project(v, plain, out=torch.empty((A, n, m + 1), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("shape", [(3, 2, 5), (90, 3, 64), (33, 5, 301)])
def test_adjoint_is_the_unscaled_unfiltered_back_projection(shape):
    """On a 'none' plan ops.fbp is float32(pi/(2A)) times fbp_adjoint, bit for bit; and it is the oracle's B within the FBP
    suite's bound."""
    from paresis_amd import ops
    A, n, m = shape
    theta, sino = fo.case_angles(A), fo.case_sino(A, n, m)            # the FBP suite's case: its table is the bound
    s = _cuda(sino)
    for circle in (False, True):
        plan = ops.FbpPlan(theta, m, center=m / 2 - 0.25, filter="none", circle=circle)
        adj = ops.fbp_adjoint(s, plan)
        assert adj.shape == (n, m, m)
        assert torch.equal(adj * float(np.float32(np.pi / (2.0 * A))), ops.fbp(s, plan))
        ref = po.adjoint(sino, theta, m / 2 - 0.25, circle)
        assert np.abs(_np(adj) - ref).max() <= 8 * fo.F32_ERROR[shape] * np.abs(ref).max()
        plan.close()


@pytest.mark.parametrize("shape", po.DOT_SHAPES)
def test_the_pair_is_adjoint(shape):
    """<project(x), y> and <x, adjoint(y)>, summed on the host in float64 from the GPU's outputs with positive random x and
    y, agree within 8 times the mismatch of the float32 restatements (DOT_F32_ERROR)."""
    from paresis_amd import ops
    A, n, m = shape
    theta, x, y = po.case_angles(A), po.case_vol(A, n, m), fo.case_sino(A, n, m)
    worst = 0.0
    for center in fo.case_centers(m):
        for circle in (False, True):
            plan = ops.FbpPlan(theta, m, center=center, filter="none", circle=circle)
            e = po.dot_mismatch(_np(plan.project(_cuda(x))), y, x, _np(plan.adjoint(_cuda(y))))
            worst = max(worst, e)
            plan.close()
    print("adjointness %s: mismatch %.3e, float32 restatement %.3e" % (shape, worst, po.DOT_F32_ERROR[shape]))
    assert worst <= 8 * po.DOT_F32_ERROR[shape]


@pytest.mark.parametrize("m", [2, 5, 64, 301])
def test_nothing_outside_the_circle_is_projected(m):
    """A volume that is zero inside the circle and not outside projects to exactly 0 with circle=True, and to something
    without; forward_project and back_project are the two operators on the module's 'none' plan."""
    from paresis_amd import ops, tomography
    A = 7
    theta = po.case_angles(A)
    vol = np.where(fo.circle_mask(m), 0.0, 3.0 + np.arange(m)[None, :])[None].astype(np.float32)
    tomography._plans.clear()
    lit = tomography.forward_project(_cuda(vol), theta)
    assert lit.shape == (A, 1, m) and float(lit.abs().max()) == 0.0
    dark = tomography.forward_project(_cuda(vol), theta, circle=False)
    assert float(dark.abs().max()) > 0
    back = tomography.back_project(dark, theta, circle=False)
    assert back.shape == (1, m, m) and len(tomography._plans) == 2
    assert all(k[5] == "none" for k in tomography._plans)
    plan = ops.FbpPlan(theta, m, filter="none", circle=False)
    assert torch.equal(back, ops.fbp_adjoint(dark, plan)) and torch.equal(dark, ops.fbp_project(_cuda(vol), plan))


# -------------------------------------------------------------------------------------------------- the solvers
@pytest.fixture(scope="module", params=po.SOLVER_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def solver_case(request):
    theta, center, sino = po.solver_case(*request.param)
    return request.param, theta, center, sino


@pytest.mark.parametrize("iterations", po.SOLVER_ITERATIONS)
def test_sirt_matches_oracle(solver_case, iterations):
    """Against the float64 oracle within 8 times SIRT_F32_ERROR, with and without the clamp; the zero sinogram row comes
    back exactly 0."""
    from paresis_amd import tomography
    case, theta, center, sino = solver_case
    for nonneg in (False, True):
        ref = po.sirt(sino, theta, iterations, center, True, nonneg=nonneg)
        got = tomography.sirt(_cuda(sino), theta, iterations, center=center, nonneg=nonneg)
        e = np.abs(_np(got) - ref).max() / np.abs(ref).max()
        print("sirt %s, %d iterations, nonneg %d: error %.3e, table %.3e" % (case, iterations, nonneg, e, po.SIRT_F32_ERROR[(case, iterations)]))
        assert e <= 8 * po.SIRT_F32_ERROR[(case, iterations)]
        assert float(got[1].abs().max()) == 0.0


def test_sirt_clamps_and_continues(solver_case):
    from paresis_amd import tomography
    case, theta, center, sino = solver_case
    s = _cuda(sino)
    assert float(tomography.sirt(-s, theta, 3, center=center, nonneg=True).abs().max()) == 0.0
    x4 = tomography.sirt(s, theta, 4, center=center)
    keep = x4.clone()
    x7 = tomography.sirt(s, theta, 3, center=center, x0=x4)
    assert torch.equal(x4, keep)                                                  # the start is not modified
    assert torch.equal(x7, tomography.sirt(s, theta, 7, center=center))           # a stationary iteration: the same bits
    assert torch.equal(tomography.sirt(s, theta, 0, center=center), torch.zeros_like(x4))


@pytest.mark.parametrize("iterations", po.SOLVER_ITERATIONS)
def test_cgls_matches_oracle(solver_case, iterations):
    """Against the float64 oracle within 8 times CGLS_F32_ERROR (see the table's note on the 10-step figure); the zero
    sinogram row comes back exactly 0; a row alone agrees with the stack within the same bound."""
    from paresis_amd import tomography
    case, theta, center, sino = solver_case
    ref = po.cgls(sino, theta, iterations, center, True)
    got = tomography.cgls(_cuda(sino), theta, iterations, center=center)
    bound = 8 * po.CGLS_F32_ERROR[(case, iterations)] * np.abs(ref).max()
    e = np.abs(_np(got) - ref).max()
    alone = tomography.cgls(_cuda(sino[:, 0:1]), theta, iterations, center=center)
    e1 = np.abs(_np(alone[0]) - _np(got[0])).max()
    print("cgls %s, %d iterations: error / bound %.3f, row alone against the stack / bound %.3g (table %.3e)"
          % (case, iterations, e / bound, e1 / bound, po.CGLS_F32_ERROR[(case, iterations)]))
    assert e <= bound and e1 <= bound
    assert float(got[1].abs().max()) == 0.0


def test_cgls_takes_a_start(solver_case):
    """Started from the float64 oracle's 6-step result, 2 more steps reduce the residual further; the start is not modified."""
    from paresis_amd import tomography
    case, theta, center, sino = solver_case
    s = _cuda(sino)
    x0 = _cuda(po.cgls(sino, theta, 6, center, True))
    keep = x0.clone()
    x = tomography.cgls(s, theta, 2, center=center, x0=x0)
    assert torch.equal(x0, keep)
    res = lambda v: float((s - tomography.forward_project(v, theta, center=center)).double().pow(2).sum())
    assert res(x) < res(x0)
    assert torch.equal(tomography.cgls(s, theta, 0, center=center, x0=x0), x0)


# ------------------------------------------------------------------------------------ few angles, on the phantom's own lines
DIMX, DIMY, PIX_UM = 24, 64, 500.0


def test_few_angles_sirt_beats_fbp():
    """contrast_phantom_lines at 12 angles, the delta-weighted sum of one detector row as a line integral in pixels of the
    slice delta/1.62e-7: 20 SIRT iterations with the clamp leave at most 0.70 of ramp FBP's rms error inside the circle.
    The float64 oracle's figures on the same sinogram are printed beside the GPU's."""
    from paresis_amd import tomography
    from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_lines
    theta = np.arange(12) * 15.0
    w = torch.tensor(fo.PHANTOM_DELTA, dtype=torch.float32, device="cuda") / (1.62e-7 * PIX_UM * 1e-6)
    row = DIMX // 2
    sino = torch.stack([(contrast_phantom_lines(DIMX, DIMY, PIX_UM, a)[0][:, row, :] * w[:, None]).sum(dim=0) for a in theta])
    sino = sino[:, None, :].contiguous()
    truth = np.einsum("kij,k->ij", fo.phantom_slices(DIMY, PIX_UM).astype(np.float64), np.array(fo.PHANTOM_DELTA) / 1.62e-7)
    e_fbp = po.rms_in_circle(_np(tomography.fbp(sino, theta))[0], truth)
    e_sirt = po.rms_in_circle(_np(tomography.sirt(sino, theta, 20, nonneg=True))[0], truth)
    e_cgls = po.rms_in_circle(_np(tomography.cgls(sino, theta, 10))[0], truth)
    s64 = _np(sino)
    o_fbp = po.rms_in_circle(fo.fbp(s64, theta)[0], truth)
    o_sirt = po.rms_in_circle(po.sirt(s64, theta, 20, nonneg=True)[0], truth)
    o_cgls = po.rms_in_circle(po.cgls(s64, theta, 10)[0], truth)
    print("12 angles, rms error / max: GPU FBP %.4f SIRT(20, nonneg) %.4f (ratio %.3f) CGLS(10) %.4f; "
          "oracle FBP %.4f SIRT %.4f (ratio %.3f) CGLS %.4f" % (e_fbp, e_sirt, e_sirt / e_fbp, e_cgls, o_fbp, o_sirt, o_sirt / o_fbp, o_cgls))
    assert e_sirt <= 0.70 * e_fbp


# -------------------------------------------------------------------------------------------------- the public API
def test_reconstruct_converts_the_solvers_volumes():
    """reconstruct(scan, method='sirt', iterations=5) is sirt's bits in physical units (cgls likewise, delta for a phase
    scan); the default call is fbp's."""
    from paresis_amd import tomography
    case, (theta, center, sino) = po.SOLVER_CASES[0], po.solver_case(*po.SOLVER_CASES[0])
    s = _cuda(sino)
    scan = {"sinograms": {0: s}, "angles": list(theta), "center": center, "voxel_m": 1e-3, "modality": "attenuation",
            "energy_keV": 52.0}
    got = tomography.reconstruct(scan, method="sirt", iterations=5)
    assert list(got) == [0]
    assert torch.equal(got[0], tomography.mu_volume(tomography.sirt(s, theta, 5, center=center), 1e-3))
    got = tomography.reconstruct(scan, method="sirt", iterations=5, nonneg=True, circle=False)
    assert torch.equal(got[0], tomography.mu_volume(tomography.sirt(s, theta, 5, center=center, circle=False, nonneg=True), 1e-3))
    phase = dict(scan, modality="phase")
    got = tomography.reconstruct(phase, method="cgls", iterations=3)
    assert torch.equal(got[0], tomography.delta_volume(tomography.cgls(s, theta, 3, center=center), 52.0, 1e-3))
    assert torch.equal(tomography.reconstruct(scan)[0], tomography.mu_volume(tomography.fbp(s, theta, center=center), 1e-3))
    assert torch.equal(tomography.reconstruct(scan, filter="hann", method="fbp")[0],
                       tomography.mu_volume(tomography.fbp(s, theta, center=center, filter="hann"), 1e-3))


def test_main_tomography_method_writes_the_api_bits(tmp_path, monkeypatch):
    """main.run(tomography=6, tomography_method='cgls', tomography_iterations=4) writes scan + reconstruct(method='cgls',
    iterations=4) through the API, and tomographyParams carries the method and its iterations."""
    import glob
    from paresis_amd import Experiment as experiment_module
    from paresis_amd import main, tomography
    from tests.test_gpu_fbp import DIMX as NX, DIMY as NY, _phantom_experiment

    exp = _phantom_experiment(1)
    exp.mySampleofInterest.getMyGeometry(exp.exp_dict['studyDimensions'], exp.exp_dict['studyPixelSize'], 2)

    def injected(exp_dict):
        for k, v in exp.exp_dict.items():
            exp_dict.setdefault(k, v)
        exp.exp_dict = exp_dict
        return exp

    ed = {"experimentName": "injected", "filepath": str(tmp_path) + "/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": "RayT", "noise": False}
    with monkeypatch.context() as mp:
        mp.setattr(experiment_module, "Experiment", injected)
        main.run(ed, save=True, saving_format=".npy", tomography=6, tomography_method="cgls", tomography_iterations=4)
    files = sorted(glob.glob(str(tmp_path) + "/*/tomography/*.npy"))
    assert len(files) == 1
    tp = ed['tomographyParams']
    assert tp['method'] == 'cgls' and tp['iterations'] == 4 and tp['modality'] == 'attenuation' and len(tp['angles']) == 6
    want = tomography.reconstruct(tomography.scan(_phantom_experiment(1), tp['angles']), method='cgls', iterations=4)[0]
    got = np.load(files[0])
    assert got.shape == (NX // 2, NY // 2, NY // 2) and got.dtype == np.float32
    assert np.array_equal(got, want.cpu().numpy()) and torch.equal(ed['tomographyVolumes'][0], want)
    assert float(np.abs(got).max()) > 10                              # 1/m: the support alone is 31.6
    fbp = tomography.reconstruct(tomography.scan(_phantom_experiment(1), tp['angles']))[0]
    assert not torch.equal(fbp, want)


def test_cli_refuses_iterations_without_tomography(capsys, tmp_path):
    from paresis_amd import main
    with pytest.raises(SystemExit):
        main.main(["--out", str(tmp_path / "o"), "--tomography-iterations", "3"])
    assert "--tomography-iterations is an option of --tomography" in capsys.readouterr().err
