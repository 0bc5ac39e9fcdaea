"""The tomography operators of csrc/fbp.hip where their index arithmetic decides what is read: rotation axes off the middle,
off the detector and out of reach, sizes one below, at and above the 16-voxel tile, the 64-sample run, the 32-angle chunk
and the pad-length step, angles on the axes and ties of every quadrant and a hair beside them.
  A  the projector and the back-projector as whole matrices, from unit impulses: equal bit for bit, and within 2^-23 of the
     contract's matrix written down in numpy (tests/_project_oracle.py matrix);
  B  dense data at the edge shapes against the float64 oracle, every bound 8 times the float32 restatement's distance from
     the oracle as measured on the CPU (tests/test_project_host.py, tests/test_fbp_host.py);
  C  SIRT and CGLS where the guards of R = B^T 1 and C = B 1 are taken."""
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


# ------------------------------------------------------------------------------------------ A: the operators as matrices
def _where(diff, m):
    """The first differing entry of a [A][m*m][m] comparison, for the assertion's message."""
    if not bool(diff.any()):
        return ""
    a, v, k = (int(t[0]) for t in torch.nonzero(diff)[:1].unbind(dim=1))
    return "%d entries differ, the first at angle %d, voxel (%d, %d), sample %d" % (int(diff.sum()), a, v // m, v % m, k)


def _matrices(ops, eye, imp, theta, m, center, circle, **plan_args):
    """-> (P, B) in the layout [A][m*m][m]: ops.fbp_project of the identity, ops.fbp_adjoint of the impulses."""
    A = len(theta)
    plan = ops.FbpPlan(theta, m, center=center, filter="none", circle=circle, **plan_args)
    P = ops.fbp_project(eye, plan)
    B = ops.fbp_adjoint(imp, plan)
    plan.close()
    assert P.shape == (A, m * m, m) and B.shape == (A * m, m, m)
    return P, B.view(A, m, m * m).permute(0, 2, 1)


def _check_matrices(m, theta, centers, far):
    """Part A for one size.  2^-23: a weight is a float32 rounding of a number in [0, 1], half an ulp (2^-24); the device's
    fused u and numpy's unfused one differ by a few float64 ulps, which moves that rounding by at most one float32 ulp more;
    where the difference flips floor(u) at a tie the weight 1 lands on the same sample either way."""
    from paresis_amd import ops
    theta = np.asarray(theta, dtype=np.float64)
    A = len(theta)
    eye = torch.eye(m * m, dtype=torch.float32, device="cuda").view(m * m, m, m)
    imp = _cuda(po.impulses(A, m))
    worst, entries = 0.0, 0
    for center in centers:
        for circle in (False, True):
            P, B = _matrices(ops, eye, imp, theta, m, center, circle)
            assert torch.equal(P, B), "m %d center %r circle %d: %s" % (m, center, circle, _where(P != B, m))
            if center in far:
                assert int(torch.count_nonzero(P)) == 0 and int(torch.count_nonzero(B)) == 0, (m, center, circle)
                continue
            M = po.matrix(m, theta, center, circle)
            entries += int(np.count_nonzero(M))
            for a in range(A):
                d = np.abs(_np(P[a]) - M[a])
                e = float(d.max())
                assert e <= 2.0 ** -23, "m %d center %r circle %d angle %r: |P - M| = %.3e at voxel, sample %s" % (
                    m, center, circle, theta[a], e, np.unravel_index(int(d.argmax()), d.shape))
                worst = max(worst, e)
            del P, B
    print("matrices m %d, %d angles, %d centres: P == B everywhere; %d non-zero entries, max|P - M| / 2^-23 = %.3g"
          % (m, A, len(centers), entries, worst * 2.0 ** 23))
    del eye, imp
    torch.cuda.empty_cache()


@pytest.mark.parametrize("m", po.MATRIX_M)
def test_the_operators_are_exact_transposes(m):
    """Every angle of EDGE_ANGLES and every centre of edge_centers, circle off and on: the adjoint call passes A*m rows
    through the plan's 64-row blocks, the projector call m*m rows through its four-row blocks.  At the three far centres
    both matrices are exactly zero."""
    centers = fo.edge_centers(m)
    _check_matrices(m, fo.EDGE_ANGLES, centers, centers[-fo.FAR_CENTERS:])


@pytest.mark.parametrize("m", po.MATRIX_LARGE_M)
def test_the_operators_are_exact_transposes_across_runs(m):
    """One sample below a 64-sample run, at it, one sample into the second and one into the third."""
    _check_matrices(m, po.MATRIX_LARGE_ANGLES, po.matrix_large_centers(m), ())


def test_the_matrices_ignore_the_row_blocks():
    """A plan capped at 2 rows per pass walks the 320 impulse rows in 160 blocks: the uncapped bits, the projector's bits."""
    from paresis_amd import ops
    m, theta = 16, np.asarray(fo.EDGE_ANGLES)
    eye = torch.eye(m * m, dtype=torch.float32, device="cuda").view(m * m, m, m)
    imp = _cuda(po.impulses(len(theta), m))
    for center in (-3.5, m / 2 + 7.3):
        P, B = _matrices(ops, eye, imp, theta, m, center, True)
        P2, B2 = _matrices(ops, eye, imp, theta, m, center, True, max_rows=2)
        assert torch.equal(B2, B) and torch.equal(P2, P) and torch.equal(P2, B2), _where(P2 != B2, m)


# ------------------------------------------------------------------------------------------ B: dense data at the edge shapes
@pytest.mark.parametrize("shape", po.EDGE_SHAPES)
def test_project_matches_oracle_at_the_edges(shape):
    """max|sino - oracle| <= 8 * EDGE_F32_ERROR[shape] * max|oracle| at the three truncating centres, circle off and on."""
    from paresis_amd import ops
    A, n, m = shape
    theta, vol = fo.edge_angles(A), po.case_vol(A, n, m)
    v = _cuda(vol)
    worst = 0.0
    for center in fo.dense_centers(m):
        both = po.project(np.concatenate([vol, vol * fo.circle_mask(m)]), theta, center, circle=False)
        for circle in (False, True):
            ref = both[:, n:] if circle else both[:, :n]
            bound = 8 * po.EDGE_F32_ERROR[shape] * np.abs(ref).max()
            plan = ops.FbpPlan(theta, m, center=center, filter="none", circle=circle)
            sino = ops.fbp_project(v, plan)
            plan.close()
            assert sino.shape == (A, n, m)
            e = np.abs(_np(sino) - ref).max()
            print("project %s center %.2f circle %d: error / bound = %.3f (bound %.3e)" % (shape, center, circle, e / bound, bound))
            worst = max(worst, e / bound)
    assert worst <= 1.0


@pytest.mark.parametrize("shape", po.EDGE_SHAPES)
def test_adjoint_matches_oracle_at_the_edges(shape):
    """max|vol - oracle| <= 8 * EDGE_ADJ_F32_ERROR[shape] * max|oracle|, likewise; nothing outside the circle."""
    from paresis_amd import ops
    A, n, m = shape
    theta, sino = fo.edge_angles(A), fo.case_sino(A, n, m)
    s = _cuda(sino)
    mask = fo.circle_mask(m)
    worst = 0.0
    for center in fo.dense_centers(m):
        whole = po.adjoint(sino, theta, center, circle=False)
        for circle in (False, True):
            ref = whole * mask if circle else whole
            bound = 8 * po.EDGE_ADJ_F32_ERROR[shape] * np.abs(ref).max()
            plan = ops.FbpPlan(theta, m, center=center, filter="none", circle=circle)
            vol = _np(ops.fbp_adjoint(s, plan))
            plan.close()
            assert vol.shape == (n, m, m)
            if circle:
                assert np.all(vol[:, ~mask] == 0)
            e = np.abs(vol - ref).max()
            print("adjoint %s center %.2f circle %d: error / bound = %.3f (bound %.3e)" % (shape, center, circle, e / bound, bound))
            worst = max(worst, e / bound)
    assert worst <= 1.0


@pytest.mark.parametrize("shape", po.EDGE_SHAPES)
def test_the_pair_is_adjoint_on_a_truncated_detector(shape):
    """<project(x), y> and <x, adjoint(y)>, summed on the host in float64 from the GPU's outputs, agree within 8 times the
    mismatch of the float32 restatements (EDGE_DOT_F32_ERROR) where the detector cuts the projections off."""
    from paresis_amd import ops
    A, n, m = shape
    theta, x, y = fo.edge_angles(A), po.case_vol(A, n, m), fo.case_sino(A, n, m)
    worst = 0.0
    for center in fo.dense_centers(m):
        for circle in (False, True):
            plan = ops.FbpPlan(theta, m, center=center, filter="none", circle=circle)
            worst = max(worst, po.dot_mismatch(_np(plan.project(_cuda(x))), y, x, _np(plan.adjoint(_cuda(y)))))
            plan.close()
    bound = 8 * po.EDGE_DOT_F32_ERROR[shape]
    print("adjointness %s: mismatch / bound = %.3f (bound %.3e)" % (shape, worst / bound, bound))
    assert worst <= bound


@pytest.mark.parametrize("flt", fo.FILTERS)
@pytest.mark.parametrize("shape", fo.EDGE_FBP_SHAPES)
def test_fbp_matches_oracle_at_the_edges(shape, flt):
    """max|vol - oracle| <= 8 * fo.EDGE_F32_ERROR[shape] * max|oracle| at the three truncating centres, circle off and on;
    a plan capped at 6 rows per pass (blocks of six rows and of one, whose last pair has no second line) gives the same
    bits."""
    from paresis_amd import ops
    A, n, m = shape
    theta, sino = fo.edge_angles(A), fo.case_sino(A, n, m)
    s = _cuda(sino)
    mask = fo.circle_mask(m)
    worst = 0.0
    for center in fo.dense_centers(m):
        ref = fo.fbp(sino, theta, center, flt, circle=False)
        bound = 8 * fo.EDGE_F32_ERROR[shape] * np.abs(ref).max()
        for circle in (False, True):
            plan = ops.FbpPlan(theta, m, center=center, filter=flt, circle=circle)
            vol = ops.fbp(s, plan)
            plan.close()
            capped = ops.FbpPlan(theta, m, center=center, filter=flt, circle=circle, max_rows=6)
            assert torch.equal(ops.fbp(s, capped), vol)
            capped.close()
            e = np.abs(_np(vol) - (ref * mask if circle else ref)).max()
            print("fbp %s %s center %.2f circle %d: error / bound = %.3f (bound %.3e)" % (shape, flt, center, circle, e / bound, bound))
            worst = max(worst, e / bound)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------ C: the solvers' guards
@pytest.fixture(scope="module", params=po.EDGE_SOLVER_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def guarded_case(request):
    """-> (case, angles, centre, sinogram, where R = B^T 1 is 0 [A][m], where C = B 1 is 0 [m][m]), R and C the oracle's;
    tests/test_project_host.py asserts that neither has an entry in (0, 1e-5], so float32 falls on the same side of the
    solvers' 1e-6."""
    A, n, m, _ = request.param
    theta, center, sino = po.solver_case(*request.param)
    R = po.project(np.ones((1, m, m)), theta, center, True)[:, 0]
    C = po.adjoint(np.ones((A, 1, m)), theta, center, True)[0]
    assert (R == 0).any() and (C[fo.circle_mask(m)] == 0).any()
    return request.param, theta, center, sino, R == 0, C == 0


@pytest.mark.parametrize("iterations", po.SOLVER_ITERATIONS)
def test_sirt_matches_oracle_where_the_guards_act(guarded_case, iterations):
    """Against the float64 oracle within 8 times SIRT_F32_ERROR, with and without the clamp; the voxels no ray reaches stay
    exactly 0, as the zero sinogram row does."""
    from paresis_amd import tomography
    case, theta, center, sino, R0, C0 = guarded_case
    for nonneg in (False, True):
        ref = po.sirt(sino, theta, iterations, center, True, nonneg=nonneg)
        got = tomography.sirt(_cuda(sino), theta, iterations, center=center, nonneg=nonneg)
        bound = 8 * po.SIRT_F32_ERROR[(case, iterations)]
        e = np.abs(_np(got) - ref).max() / np.abs(ref).max()
        print("sirt %s, %d iterations, nonneg %d: error / bound = %.3f (bound %.3e)" % (case, iterations, nonneg, e / bound, bound))
        assert e <= bound
        assert float(got[1].abs().max()) == 0.0 and float(got[:, _cuda(C0).bool()].abs().max()) == 0.0


def test_sirt_guards_hold_exactly(guarded_case):
    """A voxel with C = 0 keeps its start, bit for bit; a sample with R = 0 has no influence: set to 1e30 in every row, it
    leaves the volume's bits as they were."""
    from paresis_amd import tomography
    case, theta, center, sino, R0, C0 = guarded_case
    A, n, m = case[:3]
    s, dead = _cuda(sino), _cuda(C0).bool()
    x0 = _cuda(po.case_vol(A, n, m, seed=3))
    for nonneg in (False, True):
        x = tomography.sirt(s, theta, 3, center=center, nonneg=nonneg, x0=x0)
        assert torch.equal(x[:, dead], x0[:, dead]) and not torch.equal(x[:, ~dead], x0[:, ~dead])
        loud = sino.copy()
        loud[np.broadcast_to(R0[:, None, :], loud.shape)] = 1e30
        assert torch.equal(tomography.sirt(_cuda(loud), theta, 3, center=center, nonneg=nonneg, x0=x0), x)
        assert torch.equal(tomography.sirt(_cuda(loud), theta, 3, center=center, nonneg=nonneg), tomography.sirt(s, theta, 3, center=center, nonneg=nonneg))


def test_cgls_matches_oracle_where_the_guards_act(guarded_case):
    """At the smallest iteration count (the table's note: the float32 recurrence drifts from there), against the float64
    oracle within 8 times CGLS_F32_ERROR; the zero sinogram row comes back exactly 0."""
    from paresis_amd import tomography
    case, theta, center, sino, R0, C0 = guarded_case
    iterations = min(po.SOLVER_ITERATIONS)
    ref = po.cgls(sino, theta, iterations, center, True)
    got = tomography.cgls(_cuda(sino), theta, iterations, center=center)
    bound = 8 * po.CGLS_F32_ERROR[(case, iterations)]
    e = np.abs(_np(got) - ref).max() / np.abs(ref).max()
    print("cgls %s, %d iterations: error / bound = %.3f (bound %.3e)" % (case, iterations, e / bound, bound))
    assert e <= bound
    assert float(got[1].abs().max()) == 0.0
