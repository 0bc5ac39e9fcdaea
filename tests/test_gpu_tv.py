"""Total-variation reconstruction on the GPU (csrc/fbp.hip k_fbp_tv_step, ops.fbp_tv_step, paresis_amd.tomography.tv /
tv_objective) against the float64 numpy oracle of tests/_tv_oracle.py, on few-angle data of the phantom, and through
reconstruct, main.run and the command line.  Every bound is 8 times the float32 restatement's distance from the oracle: the
step's is measured beside the comparison, the solver's on the CPU (TV_F32_ERROR, tests/test_tv_host.py)."""
import numpy as np
import pytest
import torch

from tests import _fbp_oracle as fo
from tests import _project_oracle as po
from tests import _tv_oracle as to

pytestmark = pytest.mark.gpu

OUTPUTS = ("x", "xbar", "px", "py")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _gpu_step(plan, lam, nonneg, u, c, x, xbar, px, py):
    """One call on fresh device copies of float32 arrays -> (x', xbar', px', py') as device tensors."""
    from paresis_amd import ops
    xd = _cuda(x)
    outs = [torch.full_like(xd, float("nan")) for _ in range(3)]
    got = ops.fbp_tv_step(plan, lam, nonneg, _cuda(u), _cuda(c), xd, _cuda(xbar), outs[0], _cuda(px), _cuda(py), outs[1], outs[2])
    assert got[0] is xd and got[1] is outs[0] and got[2] is outs[1] and got[3] is outs[2]
    return got


# -------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("m", to.STEP_M)
def test_step_matches_oracle(m):
    """One call on random state (tests/_tv_oracle.step_case: flat patches, p on the bound, c = 0, both signs) and three
    more, each from the GPU's own result, against the float64 step applied to the same input; n in {1, 2, 5}, circle off
    and on, lambda zero, middle and large, nonneg off and on.  Per output the bound is 8 times the worst distance of the
    float32 restatement from float64 over this size's calls, relative to the output's largest value.  The oracle must show the middle lambda saturating 10 % to 90 % of the active differences and the clamp catching 5 % to
    95 % of the lit voxels on the first call.  Two calls give the same bits, and a slice alone the bits it has in the stack."""
    from paresis_amd import ops
    plans = {circle: ops.FbpPlan([0.0], m, filter="none", circle=circle) for circle in (False, True)}
    yard, worst = dict.fromkeys(OUTPUTS, 0.0), dict.fromkeys(OUTPUTS, 0.0)
    for n in to.STEP_N:
        for circle in (False, True):
            for kind in to.LAMBDA_KINDS:
                lam, u, c, x, xbar, px, py = to.step_case(n, m, circle, kind)
                for nonneg in (False, True):
                    state = (x, xbar, px, py)
                    for call in range(4):
                        ref = to.step_f64(lam, nonneg, circle, u, c, *state)
                        f32 = to.step_f32(lam, nonneg, circle, u, c, *state)
                        got = _gpu_step(plans[circle], lam, nonneg, u, c, *state)
                        if call == 0:
                            info = ref[4]
                            assert 0.05 <= info["clamped"] <= 0.95, (n, circle, kind, info)
                            assert {"zero": True, "middle": 0.10 <= info["saturated"] <= 0.90,
                                    "large": info["saturated"] == 0}[kind], (n, circle, kind, info)
                            again = _gpu_step(plans[circle], lam, nonneg, u, c, *state)
                            assert all(torch.equal(a, b) for a, b in zip(got, again))
                            r = n - 1
                            alone = _gpu_step(plans[circle], lam, nonneg, *(v[r:r + 1] for v in (u, c) + state))
                            assert all(torch.equal(a[0], b[r]) for a, b in zip(alone, got))
                        for k, name in enumerate(OUTPUTS):
                            scale = max(np.abs(ref[k]).max(), 1e-30)
                            yard[name] = max(yard[name], float(np.abs(f32[k].astype(np.float64) - ref[k]).max() / scale))
                            worst[name] = max(worst[name], float(np.abs(_np(got[k]) - ref[k]).max() / scale))
                            if kind == "zero" and k >= 2:
                                assert float(got[k].abs().max()) == 0.0           # lambda = 0: the dual is exactly 0
                        state = tuple(t.cpu().numpy() for t in got)
    for plan in plans.values():
        plan.close()
    print("tv step m = %d: error (float32 restatement's) " % m
          + ", ".join("%s %.2e (%.2e)" % (name, worst[name], yard[name]) for name in OUTPUTS))
    for name in OUTPUTS:
        assert yard[name] > 0 and worst[name] <= 8 * yard[name], name


def test_step_checks_its_arguments():
    from paresis_amd import ops
    m = 9
    plan = ops.FbpPlan([0.0], m, filter="none")
    t = [torch.zeros((2, m, m), dtype=torch.float32, device="cuda") for _ in range(9)]
    u, c, x, xb, xbo, px, py, pxo, pyo = t
    ops.fbp_tv_step(plan, 0.0, False, u, c, x, xb, xbo, px, py, pxo, pyo)
    for args, msg in (((u, c, x, xb, xb, px, py, pxo, pyo), "xbar_out shares its storage with xbar_in"),
                      ((u, c, x, xb, x, px, py, pxo, pyo), "xbar_out shares its storage with x"),
                      ((u, c, x, xb, xbo, px, py, px, pyo), "px_out shares its storage with px_in"),
                      ((u, c, x, xb, xbo, px, py, pxo, py), "py_out shares its storage with py_in"),
                      ((u, c, x, xb, xbo, px, py, pxo, pxo), "py_out shares its storage with px_out"),
                      ((u, c, x, xb, xbo[:1].contiguous(), px, py, pxo, pyo), "shape"),
                      ((u, c, x[:, :, :-1].contiguous(), xb, xbo, px, py, pxo, pyo), "the plan takes"),
                      ((u.double(), c, x, xb, xbo, px, py, pxo, pyo), "float32")):
        with pytest.raises(ops.PsxError, match=msg):
            ops.fbp_tv_step(plan, 0.1, False, *args)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ops.PsxError, match="weight"):
            ops.fbp_tv_step(plan, bad, False, u, c, x, xb, xbo, px, py, pxo, pyo)
    plan.close()


# -------------------------------------------------------------------------------------------------- the solver
@pytest.fixture(scope="module", params=po.SOLVER_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def solver_case(request):
    theta, center, sino = to.solver_case(*request.param)
    return request.param, theta, center, sino


@pytest.mark.parametrize("iterations", to.SOLVER_ITERATIONS)
def test_tv_matches_oracle(solver_case, iterations):
    """Against the float64 oracle within 8 times TV_F32_ERROR, with lambda = 0.3 and the clamp and with lambda = 0 without;
    the zero sinogram row comes back exactly 0."""
    from paresis_amd import tomography
    case, theta, center, sino = solver_case
    for lam, nonneg in to.SOLVER_SETTINGS:
        ref = to.tv(sino, theta, iterations, lam, center, True, nonneg)
        got = tomography.tv(_cuda(sino), theta, iterations, lam, center=center, nonneg=nonneg)
        assert got.shape == ref.shape and got.dtype == torch.float32
        e = np.abs(_np(got) - ref).max() / np.abs(ref).max()
        table = to.TV_F32_ERROR[(case, iterations, (lam, nonneg))]
        print("tv %s, %d iterations, lambda %.1f, nonneg %d: error %.3e, table %.3e" % (case, iterations, lam, nonneg, e, table))
        assert e <= 8 * table
        assert float(got[1].abs().max()) == 0.0


def test_tv_takes_a_start(solver_case):
    """tv(..., x0=v) differs from tv(...) and matches the oracle started at v; v is not modified; 0 iterations return it."""
    from paresis_amd import tomography
    case, theta, center, sino = solver_case
    v = (po.case_vol(*case[:3], seed=1) - 1.0).astype(np.float32)
    s, x0 = _cuda(sino), _cuda(v)
    got = tomography.tv(s, theta, 10, 0.3, center=center, nonneg=True, x0=x0)
    assert torch.equal(x0, _cuda(v))
    assert not torch.equal(got, tomography.tv(s, theta, 10, 0.3, center=center, nonneg=True))
    ref = to.tv(sino, theta, 10, 0.3, center, True, True, x0=v)
    e = np.abs(_np(got) - ref).max() / np.abs(ref).max()
    print("tv %s from a start, 10 iterations: error %.3e" % (case, e))
    assert e <= 8 * to.TV_F32_ERROR[(case, 10, (0.3, True))]
    assert torch.equal(tomography.tv(s, theta, 0, 0.3, center=center, x0=x0), x0)
    assert torch.equal(tomography.tv(s, theta, 0, 0.3, center=center), torch.zeros_like(x0))


# -------------------------------------------------------------------------------------------------- few angles
DIMX, DIMY, PIX_UM = 24, 64, 500.0


def test_few_angles_tv_beats_sirt_on_consistent_data():
    """The delta-weighted phantom slice through forward_project at 12 angles: 100 TV iterations (lambda = 0.1, clamp) leave
    at most 0.25 of the rms error in the circle of 100 SIRT iterations with the clamp (the float64 oracle: 0.0094 against
    0.0633, 0.15)."""
    from paresis_amd import tomography
    truth = to.phantom_truth(DIMY, PIX_UM)
    theta = to.FEW_ANGLES
    b = tomography.forward_project(_cuda(truth[None]), theta)
    e_tv = po.rms_in_circle(_np(tomography.tv(b, theta, 100, 0.1, nonneg=True))[0], truth)
    e_sirt = po.rms_in_circle(_np(tomography.sirt(b, theta, 100, nonneg=True))[0], truth)
    b64 = _np(b)
    o_tv = po.rms_in_circle(to.tv(b64, theta, 100, 0.1, nonneg=True)[0], truth)
    o_sirt = po.rms_in_circle(po.sirt(b64, theta, 100, nonneg=True)[0], truth)
    print("12 angles, consistent data, rms error / max: GPU TV(100, 0.1, nonneg) %.4f SIRT(100, nonneg) %.4f (ratio %.3f); "
          "oracle TV %.4f SIRT %.4f (ratio %.3f)" % (e_tv, e_sirt, e_tv / e_sirt, o_tv, o_sirt, o_tv / o_sirt))
    assert e_tv <= 0.25 * e_sirt


def test_few_angles_tv_beats_sirt_on_the_phantoms_own_lines():
    """The sinogram of test_few_angles_sirt_beats_fbp (contrast_phantom_lines, not consistent with B^T): 100 TV iterations
    with lambda = 1 and the clamp leave at most 0.8 of the error of 20 SIRT iterations with the clamp (the float64 oracle on
    radon_line's data: 0.053 against 0.081, 0.66)."""
    from paresis_amd import tomography
    from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_lines
    theta = to.FEW_ANGLES
    w = torch.tensor(fo.PHANTOM_DELTA, dtype=torch.float32, device="cuda") / (1.62e-7 * PIX_UM * 1e-6)
    row = DIMX // 2
    sino = torch.stack([(contrast_phantom_lines(DIMX, DIMY, PIX_UM, a)[0][:, row, :] * w[:, None]).sum(dim=0) for a in theta])
    sino = sino[:, None, :].contiguous()
    truth = to.phantom_truth(DIMY, PIX_UM)
    e_tv = po.rms_in_circle(_np(tomography.tv(sino, theta, 100, 1.0, nonneg=True))[0], truth)
    e_sirt = po.rms_in_circle(_np(tomography.sirt(sino, theta, 20, nonneg=True))[0], truth)
    s64 = _np(sino)
    o_tv = po.rms_in_circle(to.tv(s64, theta, 100, 1.0, nonneg=True)[0], truth)
    o_sirt = po.rms_in_circle(po.sirt(s64, theta, 20, nonneg=True)[0], truth)
    print("12 angles, the phantom's lines, rms error / max: GPU TV(100, 1.0, nonneg) %.4f SIRT(20, nonneg) %.4f (ratio %.3f); "
          "oracle TV %.4f SIRT %.4f (ratio %.3f)" % (e_tv, e_sirt, e_tv / e_sirt, o_tv, o_sirt, o_tv / o_sirt))
    assert e_tv <= 0.8 * e_sirt


def test_tv_objective():
    """tv_objective equals the oracle's to 1e-5 relative on a random volume (circle on and off) and on tv's result, and is
    lower after 100 iterations than after 10."""
    from paresis_amd import tomography
    case = po.SOLVER_CASES[1]
    theta, center, sino = to.solver_case(*case)
    vol = (po.case_vol(*case[:3]) - 1.5).astype(np.float32)
    s, v = _cuda(sino), _cuda(vol)
    for circle in (False, True):
        got = tomography.tv_objective(v, s, theta, 0.3, center=center, circle=circle)
        want = to.objective(vol, sino, theta, 0.3, center, circle)
        assert got.dtype == torch.float64 and got.shape == (case[1],)
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    obj = []
    for k in (10, 100):
        x = tomography.tv(s, theta, k, 0.3, center=center)
        got = tomography.tv_objective(x, s, theta, 0.3, center=center).cpu().numpy()
        want = to.objective(_np(x), sino, theta, 0.3, center, True)
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
        obj.append(got)
    print("tv objective per row after 10 and 100 iterations: %s, %s" % (obj[0], obj[1]))
    assert obj[1][0] < obj[0][0] and obj[1][2] < obj[0][2] and obj[0][1] == 0 and obj[1][1] == 0


# -------------------------------------------------------------------------------------------------- the public API
def test_reconstruct_scales_the_weight_by_the_sinogram():
    """reconstruct(method='tv', weight=w) is mu_volume(tv(s, ..., weight=w * max|s|)) bit for bit (delta for a phase scan)."""
    from paresis_amd import tomography
    theta, center, sino = to.solver_case(*po.SOLVER_CASES[0])
    s = _cuda(sino)
    scan = {"sinograms": {0: s}, "angles": list(theta), "center": center, "voxel_m": 1e-3, "modality": "attenuation",
            "energy_keV": 52.0}
    lam = 0.02 * float(s.abs().max())
    got = tomography.reconstruct(scan, method="tv", iterations=6, weight=0.02)
    assert list(got) == [0]
    assert torch.equal(got[0], tomography.mu_volume(tomography.tv(s, theta, 6, lam, center=center), 1e-3))
    assert not torch.equal(got[0], tomography.reconstruct(scan, method="tv", iterations=6, weight=0.0)[0])
    got = tomography.reconstruct(dict(scan, modality="phase"), method="tv", iterations=6, weight=0.02, nonneg=True, circle=False)
    assert torch.equal(got[0], tomography.delta_volume(tomography.tv(s, theta, 6, lam, center=center, circle=False, nonneg=True),
                                                       52.0, 1e-3))


def _injected(monkeypatch_context, n_positions=1):
    from paresis_amd import Experiment as experiment_module
    from tests.test_gpu_fbp import _phantom_experiment
    exp = _phantom_experiment(n_positions)
    exp.mySampleofInterest.getMyGeometry(exp.exp_dict['studyDimensions'], exp.exp_dict['studyPixelSize'], 2)

    def injected(exp_dict):
        for k, v in exp.exp_dict.items():
            exp_dict.setdefault(k, v)
        exp.exp_dict = exp_dict
        return exp

    monkeypatch_context.setattr(experiment_module, "Experiment", injected)


def _want(tp):
    from paresis_amd import tomography
    from tests.test_gpu_fbp import _phantom_experiment
    return tomography.reconstruct(tomography.scan(_phantom_experiment(1), tp['angles']), method='tv', iterations=5, weight=0.05)[0]


def test_main_tomography_tv_writes_the_api_bits(tmp_path, monkeypatch):
    """main.run(tomography=6, tomography_method='tv', tomography_iterations=5, tomography_weight=0.05) writes scan +
    reconstruct(method='tv', iterations=5, weight=0.05) through the API, and tomographyParams carries the weight."""
    import glob
    from paresis_amd import main
    from tests.test_gpu_fbp import DIMX as NX, DIMY as NY
    ed = {"experimentName": "injected", "filepath": str(tmp_path) + "/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": "RayT", "noise": False}
    with monkeypatch.context() as mp:
        _injected(mp)
        main.run(ed, save=True, saving_format=".npy", tomography=6, tomography_method="tv", tomography_iterations=5,
                 tomography_weight=0.05)
    files = sorted(glob.glob(str(tmp_path) + "/*/tomography/*.npy"))
    assert len(files) == 1
    tp = ed['tomographyParams']
    assert tp['method'] == 'tv' and tp['iterations'] == 5 and tp['weight'] == 0.05 and len(tp['angles']) == 6
    want = _want(tp)
    got = np.load(files[0])
    assert got.shape == (NX // 2, NY // 2, NY // 2) and got.dtype == np.float32
    assert np.array_equal(got, want.cpu().numpy()) and torch.equal(ed['tomographyVolumes'][0], want)
    assert float(np.abs(got).max()) > 10                              # 1/m: the support alone is 31.6


def test_cli_tomography_tv_writes_the_api_bits(tmp_path, monkeypatch):
    """--tomography 6 --tomography-method tv --tomography-iterations 5 --tomography-weight 0.05 writes the same bits."""
    import glob
    from paresis_amd import main
    with monkeypatch.context() as mp:
        _injected(mp)
        main.main(["--experiment", "injected", "--out", str(tmp_path), "--format", ".npy", "--no-noise", "--tomography", "6",
                   "--tomography-method", "tv", "--tomography-iterations", "5", "--tomography-weight", "0.05"])
    files = sorted(glob.glob(str(tmp_path) + "/*/tomography/*.npy"))
    assert len(files) == 1
    want = _want({'angles': [180.0 * a / 6 for a in range(6)]})
    assert np.array_equal(np.load(files[0]), want.cpu().numpy())
