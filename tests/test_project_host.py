"""The matched projector pair and the iterative reconstructions without a GPU: the float64 oracle of tests/_project_oracle.py
against itself (two forms of the projector, adjointness) and against known answers, the float32 yardsticks of the GPU
bounds, the few-angle figure that motivates SIRT, the C entry points' argument errors and the host-side checks of the
bindings and of paresis_amd.tomography."""
import ctypes

import numpy as np
import pytest

from tests import _fbp_oracle as fo
from tests import _project_oracle as po


def test_scatter_and_gather_forms_agree():
    """np.add.at of (w0, w1) and the tent max(0, 1 - |u - s|) are one operator: 1e-12 of the largest sample (2.5e-14 here)."""
    A, n, m = 90, 2, 64
    theta, vol = po.case_angles(A), po.case_vol(A, n, m)
    for center in fo.case_centers(m):
        for circle in (False, True):
            a, b = po.project(vol, theta, center, circle), po.project_tent(vol, theta, center, circle)
            assert a.shape == (A, n, m)
            assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


def test_case_angles_hold_the_tie():
    th = po.case_angles(90)
    assert list(th[:6]) == [0.0, 90.0, -30.0, 270.0, 45.0, 135.0] and len(th) == 90
    assert list(po.case_angles(7)[4:6]) == [45.0, 135.0]
    assert np.array_equal(po.case_angles(3), fo.case_angles(3)) and np.array_equal(po.case_angles(5), fo.case_angles(5))
    assert all(np.all(po.case_vol(*s) != 0) for s in po.SHAPES[:4])


@pytest.mark.parametrize("A,m", [(3, 5), (7, 64), (33, 301)])
def test_projector_is_the_transpose_of_the_back_projector(A, m):
    """<B^T x, y> = <x, B y> to 1e-13 relative (1.8e-16 here), circle on and off, both centres."""
    n = 2
    theta, x, y = po.case_angles(A), po.case_vol(A, n, m).astype(np.float64), fo.case_sino(A, n, m).astype(np.float64)
    for center in fo.case_centers(m):
        for circle in (False, True):
            e = po.dot_mismatch(po.project(x, theta, center, circle), y, x, po.adjoint(y, theta, center, circle))
            assert e <= 1e-13, (center, circle, e)


def test_adjoint_is_the_unscaled_back_projection():
    A, n, m = 7, 2, 64
    theta, sino = po.case_angles(A), fo.case_sino(A, n, m)
    for circle in (False, True):
        want = fo.fbp(sino, theta, 31.75, "none", circle) / (np.pi / (2 * A))
        assert np.abs(po.adjoint(sino, theta, 31.75, circle) - want).max() <= 1e-13 * np.abs(want).max()


def test_centred_disc_projects_to_its_chords():
    """A disc of radius rho about the axis: 2 sqrt(rho^2 - t^2) at every angle.  Pins the unit (a line integral in pixels),
    the centre and the weights' sum.  The tolerance has three parts.  (1) At 0 degrees u is the integer j, so the projection
    is the exact column sum of the pixelised disc: its distance from the chord, e0, is the pixelisation's error, measured
    here.  (2) B^T is voxel-driven: the tents of the voxels are a partition of unity only where their u are spaced by 1/k.
    The worst case is 45 degrees, where every u falls on the lattice of spacing d = 1/sqrt(2) and a sample collects
    d*sum_n tent(n*d - x) in [0.914, 1.1214] of the chord (x = d/2 and x = 0: d*(3 - 2d) = 1.1213), so 12.14 % of the chord
    is allowed at every angle.  (3) The stated margin: one pixel of path length, for the edge of the pixelised disc adding or
    removing a voxel on a ray.  Checked three pixels and more inside the edge, where the chord's slope is finite.  A wrong
    factor (2, sqrt(2), cos) or a centre off by a pixel near the edge misses by far more."""
    m, rho = 65, 20.0
    i, j = np.mgrid[0:m, 0:m]
    disc = (np.hypot(i - m // 2, j - m // 2) <= rho).astype(np.float64)[None]
    theta = np.concatenate([[0.0, 45.0, 90.0, 135.0], np.arange(30) * 6.0 + 1.3])
    t = np.arange(m) - m // 2
    inner = np.abs(t) <= rho - 3
    chord = 2 * np.sqrt(np.maximum(rho ** 2 - t ** 2, 0))
    sino = po.project(disc, theta)[:, 0, :]
    assert np.array_equal(sino[0], disc[0].sum(axis=0))
    e0 = np.abs(sino[0] - chord)[inner].max()
    worst = np.abs(sino - chord)[:, inner].max()
    excess = (np.abs(sino - chord) - 0.1214 * chord)[:, inner].max()
    print("disc: column sums within %.3f of the chords, every angle within %.3f; beyond the ripple allowance %.3f (margin 1)"
          % (e0, worst, excess))
    assert e0 <= 1.0 and excess <= e0 + 1.0
    assert np.abs(sino.sum(axis=1) - disc.sum()).max() <= 1e-9 * disc.sum()       # every voxel's weights sum to 1


@pytest.mark.parametrize("shape", po.SHAPES[:5])
def test_float32_yardstick(shape):
    """project_f32 reproduces the figure the GPU bound is 8 times of (the 512-pixel shape takes 90 s here and was measured
    once: 4.43e-7).  A quarter of slack, as tests/test_fbp_host.py gives."""
    A, n, m = shape
    theta, vol = po.case_angles(A), po.case_vol(A, n, m)
    worst = 0.0
    for c in fo.case_centers(m):
        for circle in (False, True):
            ref = po.project(vol, theta, c, circle)
            worst = max(worst, float(np.abs(po.project_f32(vol, theta, c, circle) - ref).max() / np.abs(ref).max()))
    print("float32 projector at %s: %.3e (table %.3e)" % (shape, worst, po.F32_ERROR[shape]))
    assert 0 < worst <= 1.25 * po.F32_ERROR[shape]


@pytest.mark.parametrize("shape", po.DOT_SHAPES[:2])
def test_float32_adjointness_yardstick(shape):
    """The float32 restatements' <P x, y> against <x, B y> (the 301-pixel shape takes 80 s and was measured once: 7.39e-10)."""
    A, n, m = shape
    theta = po.case_angles(A)
    worst = 0.0
    for seed in (0, 1):
        x, y = po.case_vol(A, n, m, seed), fo.case_sino(A, n, m, seed)
        for c in fo.case_centers(m):
            for circle in (False, True):
                worst = max(worst, po.dot_mismatch(po.project_f32(x, theta, c, circle), y, x, po.adjoint_f32(y, theta, c, circle)))
    print("float32 adjointness at %s: %.3e (table %.3e)" % (shape, worst, po.DOT_F32_ERROR[shape]))
    assert 0 < worst <= 1.25 * po.DOT_F32_ERROR[shape]


@pytest.mark.parametrize("case", po.SOLVER_CASES)
def test_float32_solver_yardsticks(case):
    theta, center, sino = po.solver_case(*case)
    assert np.all(sino[:, 1] == 0) and sino[:, 0].min() >= 0 and sino[:, 0].max() > 10
    for it in po.SOLVER_ITERATIONS:
        for name, f64, f32, table in (("sirt", po.sirt, po.sirt_f32, po.SIRT_F32_ERROR), ("cgls", po.cgls, po.cgls_f32, po.CGLS_F32_ERROR)):
            ref, got = f64(sino, theta, it, center), f32(sino, theta, it, center)
            e = float(np.abs(got - ref).max() / np.abs(ref).max())
            print("float32 %s at %s, %d iterations: %.3e (table %.3e)" % (name, case, it, e, table[(case, it)]))
            assert got.dtype == np.float32 and 0 < e <= 1.25 * table[(case, it)]
            assert np.all(ref[1] == 0) and np.all(got[1] == 0)               # the zero sinogram row


@pytest.mark.parametrize("m", [2, 5, 16, 17])
def test_matrix_builder_is_the_operators_matrix(m):
    """po.matrix, the yardstick of the GPU's matrices, against the operators on unit impulses at every angle of EDGE_ANGLES
    and every centre of edge_centers, circle off and on: the bits of project_f32 of an identity and of adjoint_f32 of the
    impulses (one non-zero term per sum: nothing to round, so the restatements are exact transposes as the kernels must
    be), within 2^-24 -- one rounding of a weight in [0, 1] -- of the float64 project and adjoint, and all zero from the
    three far centres."""
    theta = np.asarray(fo.EDGE_ANGLES)
    A = len(theta)
    eye, imp = np.eye(m * m, dtype=np.float32).reshape(m * m, m, m), po.impulses(A, m)
    assert imp.sum() == A * m and all(imp[a, a * m + k, k] == 1 for a in (0, A - 1) for k in (0, m - 1))
    centers = fo.edge_centers(m)
    worst = 0.0
    for center in centers:
        for circle in (False, True):
            M = po.matrix(m, theta, center, circle)
            assert M.dtype == np.float32 and M.shape == (A, m * m, m)
            P32 = po.project_f32(eye, theta, center, circle)
            B32 = po.as_matrix(po.adjoint_f32(imp, theta, center, circle), A, m)
            assert np.array_equal(P32, B32) and np.array_equal(M, P32), (center, circle)
            P64 = po.project(eye, theta, center, circle)
            B64 = po.as_matrix(po.adjoint(imp, theta, center, circle), A, m)
            assert np.array_equal(P64, B64)
            worst = max(worst, float(np.abs(M - P64).max()))
            if center in centers[-fo.FAR_CENTERS:]:
                assert not M.any() and not P64.any()
            elif center in fo.case_centers(m):
                assert M.any()
    print("matrix m %d: max|float32 - float64| = %.3e (2^-24 = %.3e)" % (m, worst, 2.0 ** -24))
    assert worst <= 2.0 ** -24
    # a voxel's weights sum to 1 where both its samples are on the detector; at most two entries per voxel and angle
    M = po.matrix(m, theta, m // 2, False)
    assert (np.count_nonzero(M, axis=2) <= 2).all() and np.abs(M.sum(axis=2)[:, (m // 2) * m + m // 2] - 1).max() <= 2.0 ** -23


def test_edge_cases_cover_what_they_name():
    assert len(fo.EDGE_ANGLES) == 20 and list(fo.edge_angles(3)) == [0.0, 45.0, 90.0]
    th = fo.edge_angles(65)
    assert tuple(th[:20]) == fo.EDGE_ANGLES and len(th) == 65 and th[20:].min() > 110 and 354 < th[20:].max() < 360
    assert np.cos(np.deg2rad(fo.EDGE_ANGLES[4])) == -1.0                          # 1 / cos < 0 on the j-major branch
    assert set(po.MATRIX_LARGE_ANGLES) <= set(fo.EDGE_ANGLES) and len(po.MATRIX_LARGE_ANGLES) == 10
    for m in po.MATRIX_M + po.MATRIX_LARGE_M:
        c = fo.edge_centers(m)
        assert c[:2] == fo.case_centers(m) and len(c) == 10 and c[-3:] == (3.0 * m, 2.0 ** 20, -2.0 ** 20)
        assert set(fo.dense_centers(m)) <= set(c) and set(po.matrix_large_centers(m)) <= set(c)
    assert {m for _, _, m in po.EDGE_SHAPES} >= {15, 16, 17, 31, 32, 33, 63, 65, 127, 129}
    assert {A for A, _, _ in po.EDGE_SHAPES} >= {31, 32, 33, 63, 64, 65}
    assert set(po.EDGE_SHAPES) == set(po.EDGE_F32_ERROR) == set(po.EDGE_ADJ_F32_ERROR) == set(po.EDGE_DOT_F32_ERROR)


@pytest.mark.parametrize("shape", po.EDGE_SHAPES)
def test_edge_float32_yardsticks(shape):
    """project_f32, adjoint_f32 and their dot-product mismatch reproduce the three figures the GPU's edge bounds are 8 times
    of: the worst over the three truncating centres and circle on and off (the mismatch over the seeds 0 and 1 too)."""
    A, n, m = shape
    theta = fo.edge_angles(A)
    wp = wa = wd = 0.0
    for c in fo.dense_centers(m):
        for circle in (False, True):
            for seed in (0, 1):
                x, y = po.case_vol(A, n, m, seed), fo.case_sino(A, n, m, seed)
                p32, a32 = po.project_f32(x, theta, c, circle), po.adjoint_f32(y, theta, c, circle)
                wd = max(wd, po.dot_mismatch(p32, y, x, a32))
                if seed == 0:
                    p64, a64 = po.project(x, theta, c, circle), po.adjoint(y, theta, c, circle)
                    assert po.dot_mismatch(p64, y, x, a64) <= 1e-13               # truncation leaves the oracle's pair adjoint
                    wp = max(wp, float(np.abs(p32 - p64).max() / np.abs(p64).max()))
                    wa = max(wa, float(np.abs(a32 - a64).max() / np.abs(a64).max()))
    print("float32 at %s: projector %.3e (table %.3e), adjoint %.3e (table %.3e), adjointness %.3e (table %.3e)"
          % (shape, wp, po.EDGE_F32_ERROR[shape], wa, po.EDGE_ADJ_F32_ERROR[shape], wd, po.EDGE_DOT_F32_ERROR[shape]))
    assert 0 < wp <= 1.25 * po.EDGE_F32_ERROR[shape]
    assert 0 < wa <= 1.25 * po.EDGE_ADJ_F32_ERROR[shape]
    assert 0 < wd <= 1.25 * po.EDGE_DOT_F32_ERROR[shape]


@pytest.mark.parametrize("case,r0,c0", [((12, 2, 64, -3.5), 409, 300), ((5, 3, 33, -3.5), 95, 167)])
def test_guarded_solver_cases(case, r0, c0):
    """The axis 3.5 samples below the detector: r0 entries of R = B^T 1 and c0 lit entries of C = B 1 are exactly 0, so both
    of the solvers' guards are taken, and -- the condition of the GPU comparison -- no entry of either lies in (0, 1e-5],
    where a float32 value could fall on the other side of the 1e-6 threshold.  Then the float32 yardsticks."""
    assert case in po.EDGE_SOLVER_CASES
    A, n, m, _ = case
    theta, center, sino = po.solver_case(*case)
    assert center == -3.5 and np.all(sino[:, 1] == 0) and sino[:, 0].max() > 10
    R = po.project(np.ones((1, m, m)), theta, center, True)[:, 0]
    C = po.adjoint(np.ones((A, 1, m)), theta, center, True)[0]
    lit = fo.circle_mask(m)
    print("%s: R = 0 at %d of %d, C = 0 at %d of %d lit voxels, smallest positive R %.3g, C %.3g"
          % (case, (R == 0).sum(), R.size, (C[lit] == 0).sum(), lit.sum(), R[R > 0].min(), C[C > 0].min()))
    assert (R == 0).sum() == r0 and (C[lit] == 0).sum() == c0
    assert not ((R > 0) & (R <= 1e-5)).any() and not ((C > 0) & (C <= 1e-5)).any()
    R32 = po.project_f32(np.ones((1, m, m)), theta, center, True)[:, 0]
    C32 = po.adjoint_f32(np.ones((A, 1, m)), theta, center, True)[0]
    assert np.array_equal(R32 == 0, R == 0) and np.array_equal(C32 == 0, C == 0)
    for it in po.SOLVER_ITERATIONS:
        e = 0.0
        for nonneg in (False, True):
            ref, got = po.sirt(sino, theta, it, center, nonneg=nonneg), po.sirt_f32(sino, theta, it, center, nonneg=nonneg)
            e = max(e, float(np.abs(got - ref).max() / np.abs(ref).max()))
            assert np.all(ref[:, C == 0] == 0) and np.all(got[:, C == 0] == 0) and np.all(got[1] == 0)
        print("float32 sirt at %s, %d iterations: %.3e (table %.3e)" % (case, it, e, po.SIRT_F32_ERROR[(case, it)]))
        assert 0 < e <= 1.25 * po.SIRT_F32_ERROR[(case, it)]
    it = min(po.SOLVER_ITERATIONS)
    ref, got = po.cgls(sino, theta, it, center), po.cgls_f32(sino, theta, it, center)
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("float32 cgls at %s, %d iterations: %.3e (table %.3e)" % (case, it, e, po.CGLS_F32_ERROR[(case, it)]))
    assert 0 < e <= 1.25 * po.CGLS_F32_ERROR[(case, it)]
    # a sample with R = 0 has no influence on the oracle either
    loud = sino.copy()
    loud[np.broadcast_to((R == 0)[:, None, :], loud.shape)] = 1e30
    assert np.array_equal(po.sirt_f32(loud, theta, 3, center), po.sirt_f32(sino, theta, 3, center))


def test_solvers_reduce_the_residual_and_take_a_start():
    """SIRT's residual falls monotonically in the R-weighted norm it descends in; CGLS's falls in the plain norm; a solver
    started from an earlier result continues it (SIRT exactly: it is stationary)."""
    case = po.SOLVER_CASES[0]
    theta, center, sino = po.solver_case(*case)
    b = sino.astype(np.float64)
    Rinv = po._reciprocal(po.project(np.ones((2, 64, 64)), theta, center))
    res_s = [float(np.sum(Rinv * (b - po.project(po.sirt(sino, theta, k, center), theta, center)) ** 2)) for k in (0, 1, 2, 5, 10)]
    res_c = [float(np.sum((b - po.project(po.cgls(sino, theta, k, center), theta, center)) ** 2)) for k in (0, 1, 2, 5, 10)]
    assert all(a > c for a, c in zip(res_s, res_s[1:])) and all(a > c for a, c in zip(res_c, res_c[1:]))
    assert res_c[-1] < res_s[-1] < 0.01 * res_s[0]
    x4 = po.sirt(sino, theta, 4, center)
    assert np.abs(po.sirt(sino, theta, 3, center, x0=x4) - po.sirt(sino, theta, 7, center)).max() <= 1e-12
    neg = po.sirt(-sino, theta, 3, center, nonneg=True)
    assert np.all(neg == 0)


def test_few_angles_sirt_beats_fbp():
    """The restated delta phantom (64 x 64, 500 um) through k_phantom_lines' map at the 12 angles 0, 15, ... 165 degrees:
    20 SIRT iterations with the non-negativity clamp leave at most 0.70 of ramp-filtered back-projection's rms error
    inside the circle (0.0812 against 0.1404 here: 0.58)."""
    slices = fo.phantom_slices(64, 500.0)
    truth = np.einsum("kij,k->ij", slices.astype(np.float64), np.array(fo.PHANTOM_DELTA) / 1.62e-7)
    theta = np.arange(12) * 15.0
    sino = np.stack([fo.radon_line(truth, a) for a in theta])[:, None, :]
    e_fbp = po.rms_in_circle(fo.fbp(sino, theta, 32.0, "ramp")[0], truth)
    e_hann = po.rms_in_circle(fo.fbp(sino, theta, 32.0, "hann")[0], truth)
    e_sirt = po.rms_in_circle(po.sirt(sino, theta, 20, 32.0, True, nonneg=True)[0], truth)
    e_cgls = po.rms_in_circle(po.cgls(sino, theta, 10, 32.0, True)[0], truth)
    print("12 angles, rms error / max: FBP ramp %.4f, FBP Hann %.4f, SIRT(20, nonneg) %.4f (ratio %.2f), CGLS(10) %.4f"
          % (e_fbp, e_hann, e_sirt, e_sirt / e_fbp, e_cgls))
    assert e_sirt <= 0.70 * e_fbp


def test_argument_errors_without_gpu():
    from paresis_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    fake = (ctypes.c_char * 4096)()                   # stands in for a plan: both calls refuse n < 1 before they read it
    for name in ("psx_fbp_project_f32", "psx_fbp_adjoint_f32"):
        f = getattr(lib, name)
        assert f(None, buf, 1, buf, None) == -1 and "null plan" in lib.psx_last_error().decode()
        assert f(fake, None, 1, buf, None) == -1 and "null" in lib.psx_last_error().decode()
        assert f(fake, buf, 1, None, None) == -1 and "null" in lib.psx_last_error().decode()
        assert f(fake, buf, 0, buf, None) == -1 and "n=0" in lib.psx_last_error().decode()
        assert f(fake, buf, -3, buf, None) == -1 and "n=-3" in lib.psx_last_error().decode()
        assert name in lib.psx_last_error().decode()
    assert _lib.ABI_VERSION >= 18 and lib.psx_abi_version() == _lib.ABI_VERSION


def test_binding_checks_come_before_the_device():
    import torch
    from paresis_amd import ops, tomography
    with pytest.raises(ops.PsxError, match="FbpPlan"):
        ops.fbp_project(torch.zeros((1, 8, 8)), None)
    with pytest.raises(ops.PsxError, match="FbpPlan"):
        ops.fbp_adjoint(torch.zeros((2, 1, 8)), None)
    for call in (lambda: tomography.forward_project(torch.zeros((1, 8, 8)), [0.0, 90.0]),
                 lambda: tomography.back_project(torch.zeros((2, 1, 8)), [0.0, 90.0]),
                 lambda: tomography.sirt(torch.zeros((2, 1, 8)), [0.0, 90.0], 3),
                 lambda: tomography.cgls(torch.zeros((2, 1, 8)), [0.0, 90.0], 3)):
        with pytest.raises(ops.PsxError, match="no CPU path|HBM"):
            call()
    for bad in (-1, 2.5, None, True):
        with pytest.raises(ValueError, match="iterations"):
            tomography.sirt(torch.zeros((2, 1, 8)), [0.0, 90.0], bad)
        with pytest.raises(ValueError, match="iterations"):
            tomography.cgls(torch.zeros((2, 1, 8)), [0.0, 90.0], bad)


def test_reconstruct_checks_its_method():
    from paresis_amd import main, tomography
    assert tomography.METHODS == ("fbp", "sirt", "cgls")
    with pytest.raises(ValueError, match="iterations is an option of the iterative methods"):
        tomography.reconstruct({}, method="fbp", iterations=3)
    for method in ("sirt", "cgls"):
        with pytest.raises(ValueError, match="needs iterations"):
            tomography.reconstruct({}, method=method)
    with pytest.raises(ValueError, match="method must be one of"):
        tomography.reconstruct({}, method="art", iterations=3)
    with pytest.raises(ValueError, match="nonneg is an option"):
        tomography.reconstruct({}, method="cgls", iterations=3, nonneg=True)
    with pytest.raises(ValueError, match="nonneg is an option"):
        tomography.reconstruct({}, nonneg=True)
    with pytest.raises(ValueError, match="iterations must be"):
        tomography.reconstruct({}, method="sirt", iterations=-2)
    assert tomography.reconstruct({"sinograms": {}}, method="sirt", iterations=2, nonneg=True) == {}
    ed = {"nbExpPoints": 1}
    with pytest.raises(ValueError, match="options of tomography"):
        main.run(dict(ed), save=False, tomography_method="sirt", tomography_iterations=3)
    with pytest.raises(ValueError, match="options of tomography"):
        main.run(dict(ed), save=False, tomography_iterations=3)
    with pytest.raises(ValueError, match="needs iterations"):
        main.run(dict(ed), save=False, tomography=4, tomography_method="cgls")
    with pytest.raises(ValueError, match="iterations is an option of the iterative methods"):
        main.run(dict(ed), save=False, tomography=4, tomography_iterations=2)


def test_cli_refuses_the_method_options_without_tomography(capsys, tmp_path):
    from paresis_amd import main
    for argv, msg in ((["--tomography-iterations", "3"], "--tomography-iterations is an option of --tomography"),
                      (["--tomography-method", "sirt"], "--tomography-method is an option of --tomography"),
                      (["--tomography", "4", "--tomography-method", "sirt"], "--tomography-iterations K >= 1"),
                      (["--tomography", "4", "--tomography-iterations", "3"], "--tomography-iterations K >= 1")):
        with pytest.raises(SystemExit):
            main.main(["--out", str(tmp_path / "o")] + argv)
        assert msg in capsys.readouterr().err
