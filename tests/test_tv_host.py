"""Total-variation reconstruction without a GPU: the float64 oracle of tests/_tv_oracle.py against itself (the difference
operators' adjointness, the preconditioned operator's norm, convergence), the float32 yardsticks of the GPU bounds, the few-
angle figures that motivate the method, the C entry point's argument errors and the host-side checks of the binding, of
paresis_amd.tomography and of the command line."""
import ctypes

import numpy as np
import pytest

from tests import _fbp_oracle as fo
from tests import _project_oracle as po
from tests import _tv_oracle as to


@pytest.mark.parametrize("m", [2, 5, 33])
def test_gradient_and_its_transpose_are_adjoint(m):
    """<grad x, p> = <x, grad^T p> to 1e-12 relative on random data, circle on and off; deg counts grad's entries per voxel."""
    rng = np.random.default_rng(m)
    for circle in (False, True):
        lit, ax, ay, deg = to.masks(m, circle)
        x, px, py = rng.normal(size=(3, m, m)), rng.normal(size=(3, m, m)), rng.normal(size=(3, m, m))
        gx, gy = to.grad(x, ax, ay)
        lhs, rhs = float((gx * px + gy * py).sum()), float((x * to.grad_t(px, py, ax, ay)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (m, circle, lhs, rhs)
        ex, ey = to.grad(np.ones((m, m)), ax, ay)
        assert np.all(ex == 0) and np.all(ey == 0)
        assert deg.min() >= 0 and deg.max() <= 4 and np.all(deg[~lit] == 0)
        assert deg.sum() == 2 * (ax.sum() + ay.sum())                          # every difference has two ends
    assert to.masks(2, True)[3].tolist() == [[0, 1], [1, 2]] and to.masks(2, False)[3].tolist() == [[2, 2], [2, 2]]


def test_preconditioned_operator_has_norm_at_most_one():
    """|S^(1/2) K T^(1/2)| <= 1 for K = [B^T; grad], S = diag(s1, 1/2), T = diag(tau): Pock and Chambolle's Lemma 2 with
    alpha = 1, which is what lets the solver run without an operator norm.  Power iteration, A = 5, m = 16."""
    A, m = 5, 16
    theta = po.case_angles(A)
    rng = np.random.default_rng(3)
    for circle in (False, True):
        for center in fo.case_centers(m):
            lit, ax, ay, deg = to.masks(m, circle)
            P = lambda v: po.project(v, theta, center, circle)
            Bk = lambda q: po.adjoint(q, theta, center, circle)
            s1 = np.sqrt(po._reciprocal(P(np.ones((1, m, m)))))
            cd = Bk(np.ones((A, 1, m))) + deg
            st = np.sqrt(np.where(cd > 1e-6, 1.0 / np.where(cd > 1e-6, cd, 1), 0))

            def MtM(x):
                z = st * x
                gx, gy = to.grad(z, ax, ay)
                return st * (Bk(s1 * (s1 * P(z))) + to.grad_t(0.5 * gx, 0.5 * gy, ax, ay))

            x = rng.normal(size=(1, m, m)) * (st > 0)
            lam = 0.0
            for _ in range(300):
                w = MtM(x)
                lam = float(np.sqrt((w ** 2).sum() / (x ** 2).sum()))
                x = w / np.sqrt((w ** 2).sum())
            print("circle %d centre %.2f: |S^1/2 K T^1/2|^2 = %.12f" % (circle, center, lam))
            assert 0.5 < lam <= 1 + 1e-9


@pytest.fixture(scope="module")
def consistent():
    truth = to.phantom_truth()
    return truth, po.project(truth[None], to.FEW_ANGLES)


def test_tv_converges(consistent):
    """On the consistent 12-angle phantom sinogram with lambda = 0.1 the objective after 400 iterations is within 1 % of the
    objective after 2000 (18.195 against 18.184 here), and it falls on the way there."""
    truth, b = consistent
    obj = [float(to.objective(to.tv(b, to.FEW_ANGLES, k, 0.1), b, to.FEW_ANGLES, 0.1)[0]) for k in (10, 100, 400, 2000)]
    print("objective after 10, 100, 400, 2000 iterations: %s" % obj)
    assert obj[0] > obj[1] > obj[2] > obj[3] > 0
    assert obj[2] - obj[3] <= 0.01 * obj[3]


def test_few_angles_tv_beats_sirt(consistent):
    """The figures that motivate the method, float64: on consistent 12-angle data 100 TV iterations (lambda = 0.1, clamp)
    leave 0.0094 rms error against SIRT's 0.0633 (ratio 0.15, bound 0.25); on the phantom's own lines (radon_line, not
    consistent with B^T) lambda = 1 leaves 0.053 against 0.081 of 20 SIRT iterations (0.66, bound 0.8)."""
    truth, b = consistent
    e_tv = po.rms_in_circle(to.tv(b, to.FEW_ANGLES, 100, 0.1, nonneg=True)[0], truth)
    e_sirt = po.rms_in_circle(po.sirt(b, to.FEW_ANGLES, 100, nonneg=True)[0], truth)
    sino = np.stack([fo.radon_line(truth, a) for a in to.FEW_ANGLES])[:, None, :]
    l_tv = po.rms_in_circle(to.tv(sino, to.FEW_ANGLES, 100, 1.0, nonneg=True)[0], truth)
    l_sirt = po.rms_in_circle(po.sirt(sino, to.FEW_ANGLES, 20, nonneg=True)[0], truth)
    print("consistent: TV %.4f SIRT %.4f (ratio %.3f); lines: TV %.4f SIRT %.4f (ratio %.3f)"
          % (e_tv, e_sirt, e_tv / e_sirt, l_tv, l_sirt, l_tv / l_sirt))
    assert e_tv <= 0.25 * e_sirt and l_tv <= 0.8 * l_sirt


def test_lambda_zero_keeps_the_dual_at_zero():
    theta, center, sino = to.solver_case(*po.SOLVER_CASES[1])
    n, m = sino.shape[1], sino.shape[2]
    z = np.zeros((n, m, m), dtype=np.float32)
    rng = np.random.default_rng(0)
    v = rng.normal(size=(n, m, m)).astype(np.float32)
    for step in (to.step_f64, to.step_f32):
        x, xbar, px, py, info = step(0.0, False, True, v, np.abs(v), v, v[::-1].copy(), z, z)
        assert np.all(px == 0) and np.all(py == 0) and np.array_equal(xbar, 2 * x - v)


@pytest.mark.parametrize("case", po.SOLVER_CASES)
def test_float32_solver_yardsticks(case):
    """TV_F32_ERROR is reproduced (a quarter of slack, as the projector's tables get); the zero sinogram row stays 0; the
    case exercises what it claims: with (0.3, True) the clamp acts at every count, and saturation from 10 iterations on."""
    theta, center, sino = to.solver_case(*case)
    assert np.all(sino[:, 1] == 0) and sino[:, 0].min() < 0 < sino[:, 0].max()
    for lam, nonneg in to.SOLVER_SETTINGS:
        for it in to.SOLVER_ITERATIONS:
            info = []
            ref = to.tv(sino, theta, it, lam, center, True, nonneg, info=info)
            got = to.tv_f32(sino, theta, it, lam, center, True, nonneg)
            e = float(np.abs(got - ref).max() / np.abs(ref).max())
            table = to.TV_F32_ERROR[(case, it, (lam, nonneg))]
            print("float32 tv at %s, %d iterations, lambda %.1f, nonneg %d: %.3e (table %.3e); saturated %.3f, clamped %.3f"
                  % (case, it, lam, nonneg, e, table, info[-1]["saturated"], info[-1]["clamped"]))
            assert got.dtype == np.float32 and 0 < e <= 1.25 * table
            assert np.all(ref[1] == 0) and np.all(got[1] == 0)
            if nonneg:
                assert 0.05 <= info[-1]["clamped"] <= 0.95 and ref.min() == 0
                assert info[-1]["saturated"] == 0 if it == 4 else 0.05 <= info[-1]["saturated"] <= 0.9


def test_solver_takes_a_start():
    case = po.SOLVER_CASES[1]
    theta, center, sino = to.solver_case(*case)
    v = po.case_vol(*case[:3], seed=1) - 1.0
    keep = v.copy()
    a, b = to.tv(sino, theta, 5, 0.3, center, x0=v), to.tv(sino, theta, 5, 0.3, center)
    assert np.array_equal(v, keep) and np.abs(a - b).max() > 1e-3
    assert np.array_equal(to.tv(sino, theta, 0, 0.3, center, x0=v), v)
    lit = fo.circle_mask(case[2])
    assert np.array_equal(a[:, ~lit], v.astype(np.float64)[:, ~lit])           # tau = 0 outside the circle: the start stays


def test_step_cases_hold_what_they_claim():
    """Every step case of the GPU suite has its flat patch, p on the bound, c = 0 and, for the middle lambda, between 10 %
    and 90 % of the active differences saturated and between 5 % and 95 % of the lit voxels below 0 before the clamp."""
    for m in to.STEP_M[:-1]:
        for n in to.STEP_N:
            for circle in (False, True):
                for kind in to.LAMBDA_KINDS:
                    lam, u, c, x, xbar, px, py = to.step_case(n, m, circle, kind)
                    _, ax, ay, _ = to.masks(m, circle)
                    gx, gy = to.grad(xbar, ax, ay)
                    assert np.all(gx[:, 0, 0] == 0) and np.all(gy[:, 0, 0] == 0) and np.any(c == 0)
                    assert np.all(np.hypot(px[:, 0, 0].astype(np.float64), py[:, 0, 0]) == lam)
                    info = to.step_f64(lam, True, circle, u, c, x, xbar, px, py)[4]
                    assert 0.05 <= info["clamped"] <= 0.95, (m, n, circle, kind, info)
                    if kind == "middle":
                        assert 0.10 <= info["saturated"] <= 0.90, (m, n, circle, kind, info)
                    elif kind == "large":
                        assert info["saturated"] == 0


# ---------------------------------------------------------------------------------------------- the library and the bindings
def test_argument_errors_without_gpu():
    from paresis_amd import _lib
    lib = _lib.lib()
    f = lib.psx_fbp_tv_step_f32
    bufs = [(ctypes.c_float * 16)() for _ in range(9)]
    fake = (ctypes.c_char * 4096)()                   # stands in for a plan: every refusal comes before it is read
    u, c, x, xb_in, xb_out, px_in, py_in, px_out, py_out = bufs

    def call(plan=fake, n=1, lam=0.5, **kw):
        a = dict(u=u, c=c, x=x, xb_in=xb_in, xb_out=xb_out, px_in=px_in, py_in=py_in, px_out=px_out, py_out=py_out)
        a.update(kw)
        rc = f(plan, n, lam, 0, a["u"], a["c"], a["x"], a["xb_in"], a["xb_out"], a["px_in"], a["py_in"], a["px_out"],
               a["py_out"], None)
        return rc, lib.psx_last_error().decode()

    rc, msg = call(plan=None)
    assert rc == -1 and "psx_fbp_tv_step_f32" in msg and "null plan" in msg
    for name in ("u", "c", "x", "xb_in", "xb_out", "px_in", "py_in", "px_out", "py_out"):
        rc, msg = call(**{name: None})
        assert rc == -1 and "psx_fbp_tv_step_f32" in msg and "null" in msg, name
    for n in (0, -3):
        rc, msg = call(n=n)
        assert rc == -1 and "psx_fbp_tv_step_f32" in msg and "n=%d" % n in msg
    for lam in (-1.0, float("nan"), float("inf"), -float("inf")):
        rc, msg = call(lam=lam)
        assert rc == -1 and "psx_fbp_tv_step_f32" in msg and "lambda" in msg, lam
    for kw in (dict(xb_out=xb_in), dict(px_out=px_in), dict(py_out=py_in)):
        rc, msg = call(**kw)
        assert rc == -1 and "psx_fbp_tv_step_f32" in msg and "own inputs" in msg
    rc, msg = call(xb_out=x)
    assert rc == -1 and "psx_fbp_tv_step_f32" in msg and "must not be x" in msg
    assert _lib.ABI_VERSION >= 19 and lib.psx_abi_version() == _lib.ABI_VERSION


def test_binding_checks_come_before_the_device():
    import torch
    from paresis_amd import ops, tomography
    z = torch.zeros((1, 8, 8))
    with pytest.raises(ops.PsxError, match="FbpPlan"):
        ops.fbp_tv_step(None, 0.1, False, z, z, z, z, z, z, z, z, z)
    with pytest.raises(ops.PsxError, match="no CPU path|HBM"):
        tomography.tv(torch.zeros((2, 1, 8)), [0.0, 90.0], 3, 0.1)
    with pytest.raises(ops.PsxError, match="no CPU path|HBM"):
        tomography.tv_objective(z, torch.zeros((2, 1, 8)), [0.0, 90.0], 0.1)
    for bad in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="iterations"):
            tomography.tv(torch.zeros((2, 1, 8)), [0.0, 90.0], bad, 0.1)
    for bad in (-0.5, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError, match="weight"):
            tomography.tv(torch.zeros((2, 1, 8)), [0.0, 90.0], 3, bad)
        with pytest.raises(ValueError, match="weight"):
            tomography.tv_objective(z, torch.zeros((2, 1, 8)), [0.0, 90.0], bad)


def test_reconstruct_checks_its_method():
    from paresis_amd import main, tomography
    assert tomography.METHODS == ("fbp", "sirt", "cgls") and tomography.REGULARISED_METHODS == ("tv",)
    with pytest.raises(ValueError, match="needs iterations"):
        tomography.reconstruct({}, method="tv", weight=0.1)
    with pytest.raises(ValueError, match="needs weight"):
        tomography.reconstruct({}, method="tv", iterations=3)
    for method, it in (("fbp", None), ("sirt", 3), ("cgls", 3)):
        with pytest.raises(ValueError, match="weight is an option of method 'tv'"):
            tomography.reconstruct({}, method=method, iterations=it, weight=0.1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight must be"):
            tomography.reconstruct({}, method="tv", iterations=3, weight=bad)
    with pytest.raises(ValueError, match="iterations must be"):
        tomography.reconstruct({}, method="tv", iterations=-2, weight=0.1)
    with pytest.raises(ValueError, match="method must be one of fbp, sirt, cgls, tv"):
        tomography.reconstruct({}, method="art", iterations=3)
    with pytest.raises(ValueError, match="nonneg is an option of method 'sirt'"):
        tomography.reconstruct({}, method="cgls", iterations=3, nonneg=True)
    assert tomography.reconstruct({"sinograms": {}}, method="tv", iterations=2, weight=0.0, nonneg=True) == {}
    ed = {"nbExpPoints": 1}
    with pytest.raises(ValueError, match="tomography_weight is an option of tomography"):
        main.run(dict(ed), save=False, tomography_weight=0.1)
    with pytest.raises(ValueError, match="options of tomography"):
        main.run(dict(ed), save=False, tomography_method="tv", tomography_iterations=3, tomography_weight=0.1)
    with pytest.raises(ValueError, match="needs weight"):
        main.run(dict(ed), save=False, tomography=4, tomography_method="tv", tomography_iterations=3)
    with pytest.raises(ValueError, match="needs iterations"):
        main.run(dict(ed), save=False, tomography=4, tomography_method="tv", tomography_weight=0.1)
    with pytest.raises(ValueError, match="weight is an option of method 'tv'"):
        main.run(dict(ed), save=False, tomography=4, tomography_method="sirt", tomography_iterations=3, tomography_weight=0.1)


def test_cli_refuses_the_weight_without_its_method(capsys, tmp_path):
    from paresis_amd import main
    tv = ["--tomography", "4", "--tomography-method", "tv"]
    for argv, msg in ((["--tomography-weight", "0.1"], "--tomography-weight is an option of --tomography"),
                      (["--tomography", "4", "--tomography-weight", "0.1"], "--tomography-weight W >= 0 goes with --tomography-method tv"),
                      (["--tomography", "4", "--tomography-method", "sirt", "--tomography-iterations", "3", "--tomography-weight", "0.1"],
                       "--tomography-weight W >= 0 goes with --tomography-method tv"),
                      (tv + ["--tomography-iterations", "3"], "--tomography-weight W >= 0 goes with --tomography-method tv"),
                      (tv + ["--tomography-iterations", "3", "--tomography-weight", "-1"], "--tomography-weight takes a finite weight >= 0"),
                      (tv + ["--tomography-iterations", "3", "--tomography-weight", "nan"], "--tomography-weight takes a finite weight >= 0"),
                      (tv + ["--tomography-weight", "0.1"], "--tomography-method tv needs --tomography-iterations K >= 1"),
                      (["--tomography-method", "tv"], "--tomography-method is an option of --tomography")):
        with pytest.raises(SystemExit):
            main.main(["--out", str(tmp_path / "o")] + argv)
        assert msg in capsys.readouterr().err, argv
