"""Cone-beam tomography on the CPU: the divergent projector's oracle (tests/_cone_oracle.py) against the parallel one and
against the geometry it states, FDK's oracle (tests/_fdk_oracle.py) on an analytic ball, the float32 yardstick of the GPU
parity bound, and the host rules of the public interface.  No GPU."""
import argparse
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import _cone_oracle as co
from tests import _fbp_oracle as fo
from tests import _fdk_oracle as fk
from tests import _volume_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ------------------------------------------------------------------------------------- the projector's oracle
@pytest.mark.parametrize("angle", [0.0, 30.0, 135.0, -17.0])
def test_cone_oracle_at_a_far_source_is_the_parallel_oracle(angle):
    """At dso = 2^70 every magnification (dso + w)/dso rounds to 1 and L to 1: the lines are _volume_oracle's bit for bit
    (s = 1; study grids smaller and larger than the volume)."""
    n, m, nmat = 3, 33, 3
    lab = vo.random_labels(n, m, nmat, seed=7)
    for dims in ((n, m), (n + 2, m + 5), (2, m - 4)):
        geom_p, lines_p = vo.project(lab, nmat, angle, dims, 1.0, 3.7e-6)
        geom_c, lines_c = co.project(lab, nmat, angle, dims, 1.0, 3.7e-6, 2.0 ** 70)
        assert np.array_equal(_bits(lines_c), _bits(lines_p)) and np.array_equal(geom_c, geom_p)
        assert lines_p.any()


def test_line_through_a_slab_is_the_path_length():
    """A slab one voxel thick across the beam (slice row c0 of every slice, angle 0: the step r = c0 lands on it with
    dr = 0): the line of every ray that meets it inside the slice is L = sqrt(1 + (t0^2 + z0^2)/dso^2), the length of a
    unit step in depth along the ray -- not 1."""
    n, m, dso = 9, 17, 17.0
    lab = np.zeros((n, m, m), dtype=np.uint8)
    lab[:, m // 2, :] = 1
    dims = (7, 11)
    _, lines = co.project(lab, 1, 0.0, dims, 1.0, 1.0, dso)
    L = co.path_length(dims, 1.0, dso)
    assert np.allclose(lines[0], L, rtol=1e-14, atol=0) and L.max() > 1.02 and L[dims[0] // 2, dims[1] // 2] == 1.0


def test_centred_ball_projects_symmetrically():
    n, m, dso = 15, 33, 50.0
    z, i, j = np.mgrid[0:n, 0:m, 0:m]
    lab = ((z - n // 2) ** 2 + (i - m // 2) ** 2 + (j - m // 2) ** 2 <= 36).astype(np.uint8)
    for angle in (0.0, 90.0):
        _, lines = co.project(lab, 1, angle, (15, 33), 1.0, 1.0, dso)
        assert lines[0].max() > 10 and np.allclose(lines[0], lines[0][:, ::-1], rtol=0, atol=1e-9)


@pytest.mark.parametrize("angle", [0.0, 90.0, 200.0, -17.0])
def test_off_axis_voxel_lands_where_the_geometry_says(angle):
    """One voxel off the axis and off the mid-plane: the centroid of its projection is within a pixel of (t U, z U)."""
    n, m, dso = 21, 33, 40.0
    zi, i, j = 15, 9, 22
    lab = np.zeros((n, m, m), dtype=np.uint8)
    lab[zi, i, j] = 1
    dims = (41, 65)
    _, lines = co.project(lab, 1, angle, dims, 1.0, 1.0, dso)
    tU, zU, w = co.seen_at(i, j, zi - n // 2, m, angle, dso)
    x, y = np.mgrid[0:dims[0], 0:dims[1]]
    wsum = lines[0].sum()
    assert wsum > 0
    gx, gy = (lines[0] * x).sum() / wsum - dims[0] // 2, (lines[0] * y).sum() / wsum - dims[1] // 2
    print("angle %g: depth %.2f, expected (%.3f, %.3f), centroid (%.3f, %.3f); parallel would be (%d, %.3f)"
          % (angle, w, zU, tU, gx, gy, zi - n // 2, tU * (dso + w) / dso))
    assert abs(gx - zU) <= 1.0 and abs(gy - tU) <= 1.0


def test_the_nearer_of_two_equal_blobs_is_larger():
    """Two 5 x 5 x 5 blobs at depths w = -10 (towards the source) and w = +10, side by side: the nearer one covers more of
    the detector, in both axes."""
    n, m, dso = 11, 33, 33.0
    h = m // 2
    lab = np.zeros((n, m, m), dtype=np.uint8)
    lab[3:8, h - 12:h - 7, h - 7:h - 2] = 1            # rows i - h in [-12, -8]: w < 0 at angle 0
    lab[3:8, h + 8:h + 13, h + 3:h + 8] = 2
    _, lines = co.project(lab, 2, 0.0, (31, 65), 1.0, 1.0, dso)
    near, far = lines[0] > 0, lines[1] > 0
    # magnifications 33/(33 - 12) ... 33/(33 - 8) against 33/(33 + 8) ... 33/(33 + 12): 5 voxels cover 7 to 9 pixels, and 4 to 5
    assert near.any(axis=0).sum() >= far.any(axis=0).sum() + 2 and near.any(axis=1).sum() >= far.any(axis=1).sum() + 2


# ------------------------------------------------------------------------------------------------- FDK's oracle
# |mean over the ball's interior - 1| of fk.fdk on the ball's cone-beam chords (m = 64, dso = 3m = 192, 120 angles on the
# full turn), measured with numpy on the CPU
BALL_ERROR = 2.163e-4


def test_fdk_reconstructs_the_analytic_ball():
    """The closed-form chords of a ball off the axis and off the mid-plane come back as density 1: the pi/(2A) scale, the
    pre-weight and U^2 are right.  Measured: FDK 2.163e-4 (asserted at twice that), the parallel oracle on the ball's
    parallel chords (60 angles on the half turn) 4.598e-4 -- FDK has to stay within twice that --, and 5.853e-3 with the
    source on the wrong side of the axis, which has to be at least three times worse (dso = 3m = 192 shows the factor: 27)."""
    sino, theta = fk.ball_cone_sino(), fk.full_turn(fk.BALL_ANGLES)
    err = fk.ball_error(fk.fdk(sino, theta, fk.BALL_DSO))
    par, par_theta = fk.ball_parallel_sino()
    err_parallel = fk.ball_error(fo.fbp(par, par_theta))
    err_wrong = fk.ball_error(fk.fdk(sino, theta, fk.BALL_DSO, side=-1))
    print("ball: FDK %.3e (bound %.3e), parallel %.3e, source on the wrong side %.3e" % (err, 2 * BALL_ERROR, err_parallel, err_wrong))
    assert err <= 2 * BALL_ERROR
    assert err <= 2 * err_parallel
    assert err_wrong >= 3 * err
    assert fk.ball_interior().sum() > 200


def test_fdk_loses_density_with_height_as_the_cone_angle_squared():
    """FDK is exact in the mid-plane only.  A taller ball (radius 11 about height 4.5, the same axis offset, dso = 192): the
    mean over a slice's interior falls short of 1 by about (z/dso)^2 at height z -- measured 1.97e-3 at z = 9 and 4.32e-3
    at z = 12, against 2.20e-3 and 3.91e-3 -- while the mid-plane slice is off by 1.2e-4, and the parallel oracle on the
    ball's parallel chords by at most 6.6e-4 in any of these slices.  Asserted: the deficit within a factor two of
    (z/dso)^2 (the discretisation moves it by 0.3 of it at most), the mid-plane within the parallel figure, and the row
    pre-weight and the interpolation across rows at work: without the magnification of the heights (v = Z) the slice at
    z = 12 is far worse."""
    ball, n, A, dso = dict(fk.BALL, cz=4.5, R=11.0), 41, fk.BALL_ANGLES, fk.BALL_DSO
    sino, theta = fk.ball_cone_sino(A=A, n=n, dso=dso, ball=ball), fk.full_turn(A)
    vol = fk.fdk(sino, theta, dso)
    inside = fk.ball_interior(n=n, ball=ball)
    for z in (9, 12):
        Z = n // 2 + z
        deficit = 1.0 - vol[Z][inside[Z]].mean()
        print("height %d: deficit %.3e, (z/dso)^2 %.3e, ratio %.2f" % (z, deficit, (z / dso) ** 2, deficit / (z / dso) ** 2))
        assert inside[Z].sum() > 50 and 0.5 <= deficit / (z / dso) ** 2 <= 2.0
    mid = abs(vol[n // 2][inside[n // 2]].mean() - 1.0)
    print("mid-plane: %.3e" % mid)
    assert mid <= 6.6e-4
    flat = fo.fbp(sino * dso / fk.preweight(n, fk.BALL_M, fk.BALL_M // 2, (n - 1) / 2.0, dso), theta) * 0.5
    worse = abs(flat[n // 2 + 12][inside[n // 2 + 12]].mean() - 1.0)
    print("rows not magnified, no U^2, at height 12: %.3e" % worse)
    assert worse >= 5 * (12 / dso) ** 2


def test_fdk_oracle_at_a_far_source_is_the_fbp_oracle():
    A, n, m = 8, 3, 17
    sino, theta = fo.case_sino(A, n, m), fk.case_angles(A)
    ref = fo.fbp(sino, theta, 8.25, "ramp", True)
    far = fk.fdk(sino, theta, 1e12 * m, 8.25, 0.3, "ramp", True)
    assert np.abs(far - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("factor", fk.DSO_FACTORS)
@pytest.mark.parametrize("shape", fk.SHAPES)
def test_float32_yardstick(shape, factor):
    """F32_ERROR[shape, dso / m] is what the contract's float32 restatement costs against the float64 oracle, measured here."""
    worst = fk.f32_error(shape, factor)
    print("float32 restatement at %s, dso = %g m: %.3e (table %.3e)" % (shape, factor, worst, fk.F32_ERROR[shape, factor]))
    assert 0 < worst <= 1.25 * fk.F32_ERROR[shape, factor]


def test_fdk_is_continuous_at_the_detector_edges():
    """A sample just inside -1 or the size, on either axis, is close to 0: q[-1] = q[size] = 0 on rows as on columns."""
    q = np.ones((3, 4))
    u = np.array([[-1.0 + 1e-9, 4.0 - 1e-9], [1.5, 1.5]])
    v = np.broadcast_to(np.array([[1.0, 1.0], [-1.0 + 1e-9, 3.0 - 1e-9]]), (1, 2, 2))
    out = fk.sample2(q, v, u)
    assert np.all(np.abs(out) < 1e-8)
    assert fk.sample2(q, np.full((1, 1, 1), 1.0), np.full((1, 1), 1.5))[0, 0, 0] == 1.0
    assert fk.sample2(q, np.full((1, 1, 1), 3.0), np.full((1, 1), 1.5))[0, 0, 0] == 0.0


# ---------------------------------------------------------------------------------------------------- host rules
def _experiment(dimX=32, dimY=64, ov=2):
    ed = {'overSampling': ov, 'studyDimensions': [dimX, dimY], 'distSourceToMembrane': 0.08, 'distMembraneToObject': 0.016,
          'distObjectToDetector': 0.0036, 'magnification': (0.096 + 0.0036) / 0.096}
    return types.SimpleNamespace(exp_dict=ed, myDetector=types.SimpleNamespace(det_param={'myPixelSize': 1037.5}))


def test_source_distance_and_optical_row():
    from paresis_amd import tomography
    exp = _experiment()
    assert tomography.source_distance(exp) == 0.08 + 0.016
    assert tomography.optical_row(exp) == 7.75 and tomography.rotation_center(exp) == 15.75
    assert tomography.optical_row(_experiment(dimX=33, ov=1)) == 16.0
    assert tomography.BEAMS == ("parallel", "cone") and tomography.MODALITIES == ("attenuation", "phase")
    assert tuple(tomography.RECONSTRUCTIONS) == ("fbp", "sirt", "cgls", "tv")


def test_cone_beam_value_errors():
    from paresis_amd import tomography
    from paresis_amd.Sample import AnalyticalSample
    with pytest.raises(ValueError, match="beam must be one of parallel, cone"):
        tomography.check_beam("fan", False, "fbp")
    with pytest.raises(ValueError, match="no differential form"):
        tomography.check_beam("cone", True, "fbp")
    with pytest.raises(ValueError, match="method 'sirt' has no cone-beam form"):
        tomography.check_beam("cone", False, "sirt")
    tomography.check_beam("cone", False, "fbp")
    tomography.check_beam("parallel", True, "sirt")                   # the parallel beam's rules are elsewhere
    # reconstruct: a scan without the key is parallel; a cone scan takes 'fbp' only
    assert tomography.reconstruct({"sinograms": {}}, method="sirt", iterations=2) == {}
    assert tomography.reconstruct({"sinograms": {}, "beam": "cone"}) == {}
    for method, opts in (("sirt", {"iterations": 2}), ("cgls", {"iterations": 2}), ("tv", {"iterations": 2, "weight": 0.1})):
        with pytest.raises(ValueError, match="method %r has no cone-beam form" % method):
            tomography.reconstruct({"sinograms": {}, "beam": "cone"}, method=method, **opts)
    # main.run's options
    tomography.check_run_options(8, "attenuation", "fbp", 0, None)
    tomography.check_run_options(8, "attenuation", "fbp", 0, None, beam="cone")
    tomography.check_run_options(8, "attenuation", "fbp", 0, None, False, beam="cone")
    with pytest.raises(ValueError, match="tomography_beam must be one of"):
        tomography.check_run_options(8, "attenuation", "fbp", 0, None, beam="fan")
    with pytest.raises(ValueError, match="tomography_beam is an option of tomography"):
        tomography.check_run_options(0, "attenuation", "fbp", 0, None, beam="cone")
    with pytest.raises(ValueError, match="no cone-beam form"):
        tomography.check_run_options(8, "attenuation", "cgls", 3, None, beam="cone")
    with pytest.raises(ValueError, match="no differential form"):
        tomography.check_run_options(8, "phase", "fbp", 0, None, True, beam="cone")
    # scan refuses before it touches the experiment
    with pytest.raises(ValueError, match="no differential form"):
        tomography.scan(None, [0.0], modality="phase", differential=True, beam="cone")
    with pytest.raises(ValueError, match="beam must be one of"):
        tomography.scan(None, [0.0], beam="fan")
    # the contrast phantom does not diverge
    s = AnalyticalSample()
    assert s.mySourceDistance is None and s.source_distance_voxels() is None
    s.myType, s.myGeometryFunction, s.mySourceDistance = "sample_of_interest", "generateContrastPhantom", 0.5
    with pytest.raises(ValueError, match="mySourceDistance is an option of getVolumeFromFile"):
        s.getMyGeometry((8, 16), 500.0, 1)
    with pytest.raises(ValueError, match="a diverging beam needs a getVolumeFromFile sample"):
        tomography.project(s, 52.0, [0.0], (8, 16), 500.0, source_distance_m=0.5)
    assert s.mySourceDistance == 0.5
    s.myGeometryFunction, s.myVoxelSize = "getVolumeFromFile", 250.0
    assert s.source_distance_voxels() == 2000.0
    with tomography._diverging(s, 1.0):
        assert s.mySourceDistance == 1.0
    assert s.mySourceDistance == 0.5


def test_command_line_beam():
    from paresis_amd import tomography

    class Refused(Exception):
        pass

    def parser():
        ap = argparse.ArgumentParser()
        tomography.add_tomography_options(ap)
        ap.error = lambda msg: (_ for _ in ()).throw(Refused(msg))
        return ap

    ap = parser()
    a = ap.parse_args(["--tomography", "48", "--tomography-beam", "cone"])
    assert a.tomography_beam == "cone"
    tomography.check_tomography_options(ap, a)
    assert ap.parse_args(["--tomography", "48"]).tomography_beam == "parallel"
    with pytest.raises(Refused, match="invalid choice"):
        ap.parse_args(["--tomography", "48", "--tomography-beam", "fan"])
    for argv, msg in ((["--tomography-beam", "cone"], "--tomography-beam is an option of --tomography"),
                      (["--tomography", "8", "--tomography-beam", "cone", "--tomography-method", "sirt", "--tomography-iterations", "3"],
                       "--tomography-beam cone goes with --tomography-method fbp"),
                      (["--tomography", "8", "--tomography-beam", "cone", "--tomography-modality", "phase", "--tomography-differential"],
                       "--tomography-beam cone goes with")):
        with pytest.raises(Refused, match=msg):
            tomography.check_tomography_options(ap, ap.parse_args(argv))


NEW_SYMBOLS = ("psx_volume_project_cone_u8", "psx_fdk_plan_create", "psx_fdk_plan_destroy", "psx_fdk_plan_bytes", "psx_fdk_f32")
C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}


def test_binding_table_matches_the_header():
    """Each new symbol's row of _lib.PROTOTYPES against its declaration: the return type, and per argument a pointer or the
    scalar's ctypes type."""
    from paresis_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "paresis_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        decl = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, name
        res, args = _lib.PROTOTYPES[name]
        assert res is C_TYPES[decl.group(1)], name
        params = [p.strip() for p in decl.group(2).split(",")]
        assert len(params) == len(args), (name, params)
        for p, t in zip(params, args):
            if "*" in p:
                assert t in (ctypes.c_void_p, _lib._dp, _lib._vpp), (name, p, t)
            else:
                assert t is C_TYPES[p.split()[0]], (name, p, t)
    assert re.search(r"#define\s+PSX_FDK_MAX_SAMPLES\s+\(\(int64_t\)1 << 31\)", text) and _lib.PSX_FDK_MAX_SAMPLES == 1 << 31
    assert _lib.ABI_VERSION >= 24 and _lib.lib().psx_abi_version() == _lib.ABI_VERSION


def test_library_refuses_before_the_device():
    """psx_fdk_plan_create's and psx_volume_project_cone_u8's argument checks come before any allocation or launch."""
    from paresis_amd import _lib, ops
    lib = _lib.lib()
    th = (ctypes.c_double * 3)(0.0, 120.0, 240.0)

    def create(*args):
        h = ctypes.c_void_p(None)
        rc = lib.psx_fdk_plan_create(*args, ctypes.byref(h))
        assert not h.value
        return rc, lib.psx_last_error().decode()

    nan, inf = float("nan"), float("inf")
    for args, msg in (((3, 4, 8, th, 4.0, 1.5, 7.9, 0, 1), "dso=7.9"), ((3, 4, 8, th, 4.0, 1.5, nan, 0, 1), "dso="),
                      ((3, 4, 8, th, 4.0, 1.5, inf, 0, 1), "dso="), ((3, 4, 8, th, 4.0, 1.5, 2e30, 0, 1), "dso="),
                      ((3, 4, 8, th, 4.0, 1.5, 24.0, 16, 1), "no differential form"), ((3, 4, 8, th, 4.0, 1.5, 24.0, 17, 1), "filter 17"),
                      ((3, 4, 8, th, 4.0, nan, 24.0, 0, 1), "vcenter"), ((3, 4, 8, th, 4.0, 2.0 ** 21, 24.0, 0, 1), "vcenter"),
                      ((3, 0, 8, th, 4.0, 1.5, 24.0, 0, 1), "n=0"), ((3, 65536, 8, th, 4.0, 1.5, 24.0, 0, 1), "n=65536"),
                      ((4096, 65535, 8192, th, 4.0, 1.5, 1e4, 0, 1), "2^31"), ((3, 4, 1, th, 0.0, 1.5, 24.0, 0, 1), "m=1"),
                      ((3, 4, 8, None, 4.0, 1.5, 24.0, 0, 1), "null theta"), ((3, 4, 8, th, 4.0, 1.5, 24.0, 0, 2), "circle")):
        rc, text = create(*args)
        assert rc == -1 and msg in text, (args, rc, text)
    assert lib.psx_fdk_plan_create(3, 4, 8, th, 4.0, 1.5, 24.0, 0, 1, None) == -1
    assert lib.psx_fdk_f32(None, None, None, None) == -1 and "null plan" in lib.psx_last_error().decode()
    assert lib.psx_fdk_plan_bytes(None) == 0 and lib.psx_fdk_plan_destroy(None) == 0

    d = ops.volume_desc(2, 8, 1, 30.0, (2, 8), 1.0, 1e-6)
    somewhere = ctypes.c_void_p(64)                     # never dereferenced: every call below is refused first
    for dso, msg in ((7.9, "dso=7.9"), (nan, "dso="), (inf, "dso="), (-8.0, "dso=")):
        rc = lib.psx_volume_project_cone_u8(ctypes.byref(d), ctypes.c_double(dso), somewhere, None, somewhere, None)
        assert rc == -1 and msg in lib.psx_last_error().decode(), (dso, lib.psx_last_error())
    assert lib.psx_volume_project_cone_u8(None, ctypes.c_double(8.0), somewhere, None, somewhere, None) == -1
    assert "psx_volume_project_cone_u8: null descriptor" in lib.psx_last_error().decode()
    d.nmat = 17
    assert lib.psx_volume_project_cone_u8(ctypes.byref(d), ctypes.c_double(8.0), somewhere, None, somewhere, None) == -1
    assert "psx_volume_project_cone_u8: nmat=17" in lib.psx_last_error().decode()
    d.nmat = 1
    assert lib.psx_volume_project_u8(ctypes.byref(d), None, None, somewhere, None) == -1
    assert "psx_volume_project_u8: null labels" in lib.psx_last_error().decode()


def test_binding_checks_come_before_the_device():
    import torch
    from paresis_amd import ops, tomography
    with pytest.raises(ops.PsxError, match="filter"):
        ops.FdkPlan([0.0, 90.0], 2, 8, 24.0, filter="hilbert")
    with pytest.raises(ops.PsxError, match="theta_deg"):
        ops.FdkPlan(["x"], 2, 8, 24.0)
    with pytest.raises(ops.PsxError, match="FdkPlan"):
        ops.fdk(torch.zeros((2, 1, 8)), None)
    with pytest.raises(ops.PsxError, match="no CPU path|HBM"):
        tomography.fdk(torch.zeros((2, 1, 8)), [0.0, 90.0], 24.0)
