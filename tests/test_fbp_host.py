"""Filtered back-projection without a GPU: the float64 oracle of tests/_fbp_oracle.py against known answers (so that the GPU
tests compare against something that is itself right), the float32 yardstick of the GPU parity bound, the C entry points'
argument errors, and the host functions of paresis_amd.tomography against hand values."""
import ctypes
import types

import numpy as np
import pytest

from tests import _fbp_oracle as fo
from tests._fbp_oracle import F32_ERROR, PHANTOM_DELTA


@pytest.mark.parametrize("m", [2, 5, 64, 301])
def test_ramp_filter_is_the_direct_convolution(m):
    """P >= 2m, so the circular convolution behind q = Re IFFT(FFT(line) * H) never wraps: q[i] = sum_j 2 f[|i - j|] line[j].
    The factor 2 is H's own (H = 2 Re FFT f, scikit-image's ramp): with pi/(2A) it is what makes a disc reconstruct to 1
    (next test)."""
    rng = np.random.default_rng(m)
    line = rng.normal(size=m)
    f = fo.ramp_kernel(fo.pad_length(m))
    j = np.arange(m)
    direct = (2.0 * f[np.abs(j[:, None] - j[None, :])] * line[None, :]).sum(axis=1)
    q = fo.filter_lines(line[None, None, :], "ramp")[0, 0]
    assert np.abs(q - direct).max() <= 1e-13 * np.abs(direct).max()
    assert np.abs(fo.filter_lines(line[None, None, :], "none")[0, 0] - line).max() <= 1e-14 * np.abs(line).max()


def test_sampling_is_continuous_at_the_ends():
    """q(u) with q[-1] = q[m] = 0: linear to zero over the pixel beyond either end sample, zero from there on."""
    q = np.array([[2.0, 4.0, 8.0]])
    u = np.array([-1.5, -1.0, -0.5, 0.0, 0.25, 2.0, 2.5, 3.0, 3.5, 2.0 - 1e-16, 2.0 + 1e-12])
    want = np.array([0.0, 0.0, 1.0, 2.0, 2.5, 8.0, 4.0, 0.0, 0.0, 8.0, 8.0])
    assert np.allclose(fo.sample(q, u)[0], want, rtol=0, atol=1e-10)


def test_centred_disc_reconstructs_to_one():
    """A disc of radius rho about the axis has the sinogram 2 sqrt(rho^2 - t^2) at every angle: value 1 inside, 0 outside.
    Pins the filter's normalisation, pi/(2A) and the line-integral-in-pixels unit."""
    m, A, rho = 65, 90, 20.0
    t = np.arange(m) - m // 2
    line = 2 * np.sqrt(np.maximum(rho ** 2 - t ** 2, 0))
    theta = np.arange(A) * 180.0 / A
    vol = fo.fbp(np.broadcast_to(line, (A, 1, m)), theta)[0]
    i, j = np.mgrid[0:m, 0:m]
    rr = np.hypot(i - m // 2, j - m // 2)
    inside, outside = vol[rr < rho - 3], vol[(rr > rho + 3) & (rr < m // 2)]
    print("disc: interior %.4f .. %.4f, outside max |v| %.4f" % (inside.min(), inside.max(), np.abs(outside).max()))
    # the profile is point-sampled at unit steps and has a square-root edge: a discretisation error of the order of
    # 1/(2 rho) = 2.5 % of the value, so 3 % three pixels away from the edge; a wrong factor (2, pi/2, 1/A) misses by far more
    assert np.abs(inside - 1).max() <= 0.03 and np.abs(outside).max() <= 0.03


@pytest.fixture(scope="module")
def restated_phantom():
    """The 13 slices at 64 x 64, 500 um, and their sinograms [A][13][m] at 90 angles through k_phantom_lines' map."""
    slices = fo.phantom_slices(64, 500.0)
    theta = np.arange(90) * 2.0
    sino = np.stack([np.stack([fo.radon_line(s.astype(np.float64), a) for s in slices]) for a in theta])
    return slices, theta, sino


def test_restated_phantom_slices_come_back(restated_phantom):
    """radon's convention and the contract's are one: every one of the 13 indicator slices, pixel for pixel."""
    slices, theta, sino = restated_phantom
    assert [int(s.sum()) for s in slices[:3]] == [45, 49, 45] and slices[12].sum() > 2000
    vol = fo.fbp(sino, theta)
    wrong = [int(((vol[k] > 0.5) != slices[k]).sum()) for k in range(13)]
    print("misclassified pixels per material:", wrong)
    assert wrong == [0] * 13


def test_restated_phantom_delta_comes_back(restated_phantom):
    """The 13-material delta slice: the mean over each material's interior pixels within 1 % of the largest delta."""
    slices, theta, sino = restated_phantom
    delta = np.array(PHANTOM_DELTA)
    vol = fo.fbp(np.einsum("akm,k->am", sino, delta)[:, None, :], theta)[0]
    err = [abs(vol[fo.interior(slices[k])].mean() - delta[k]) / delta.max() for k in range(13)]
    print("worst interior mean error / max delta: %.4f" % max(err))
    assert max(err) <= 0.01


@pytest.mark.parametrize("shape", fo.SHAPES[:5])
def test_float32_yardstick(shape):
    """The float32 / complex64 restatement of the contract reproduces the figure the GPU bound is 8 times of, at the parity
    shapes (the 512-pixel one takes 40 s here and was measured once: 9.4e-7).  A quarter of slack: the float32 transform's
    rounding depends on the SIMD width numpy's pocketfft was built for."""
    A, n, m = shape
    theta, sino = fo.case_angles(A), fo.case_sino(A, n, m)
    worst = 0.0
    for flt in fo.FILTERS:
        for c in fo.case_centers(m):
            ref = fo.fbp(sino, theta, c, flt, False)
            worst = max(worst, float(np.abs(fo.fbp_f32(sino, theta, c, flt, False) - ref).max() / np.abs(ref).max()))
    print("float32 restatement at %s: %.3e (table %.3e)" % (shape, worst, F32_ERROR[shape]))
    assert 0 < worst <= 1.25 * F32_ERROR[shape]


@pytest.mark.parametrize("shape", fo.EDGE_FBP_SHAPES)
def test_edge_float32_yardstick(shape):
    """The same at the edge shapes (m about the pad-length step and the 64-sample run) on edge_angles, at the three
    truncating centres of dense_centers: the figures of EDGE_F32_ERROR."""
    A, n, m = shape
    theta, sino = fo.edge_angles(A), fo.case_sino(A, n, m)
    worst = 0.0
    for flt in fo.FILTERS:
        for c in fo.dense_centers(m):
            ref = fo.fbp(sino, theta, c, flt, False)
            worst = max(worst, float(np.abs(fo.fbp_f32(sino, theta, c, flt, False) - ref).max() / np.abs(ref).max()))
    print("float32 restatement at %s: %.3e (table %.3e)" % (shape, worst, fo.EDGE_F32_ERROR[shape]))
    assert 0 < worst <= 1.25 * fo.EDGE_F32_ERROR[shape]
    assert [fo.pad_length(k) for k in (31, 32, 33, 64, 65)] == [64, 64, 128, 128, 256]


def test_far_centers_reach_nothing():
    """From the last three centres of edge_centers no voxel has a sample on the detector, at any angle of EDGE_ANGLES: the
    oracle's back-projection is exactly zero; from an axis on the detector it is not."""
    for m in (2, 5, 17, 64):
        sino = fo.case_sino(len(fo.EDGE_ANGLES), 1, m)
        centers = fo.edge_centers(m)
        for c in centers:
            vol = fo.fbp(sino, fo.EDGE_ANGLES, c, "none", False)
            if c in centers[-fo.FAR_CENTERS:]:
                assert not vol.any(), (m, c)
            elif m >= 17 or c in fo.case_centers(m):            # a short detector is also out of reach of m / 2 + 7.3
                assert vol.any(), (m, c)


def test_case_angles_hold_the_special_ones():
    th = fo.case_angles(90)
    assert list(th[:4]) == [0.0, 90.0, -30.0, 270.0] and len(th) == 90
    assert list(fo.case_angles(3)) == [0.0, 90.0, -30.0] and list(fo.case_angles(1)) == [0.0]
    assert all(np.all(fo.case_sino(*s) != 0) for s in fo.SHAPES[:4])


def test_argument_errors_without_gpu():
    from paresis_amd import _lib
    lib = _lib.lib()
    th = (ctypes.c_double * 3)(0.0, 60.0, 120.0)
    bad = (ctypes.c_double * 3)(0.0, float("nan"), 120.0)

    def create(*args):
        h = ctypes.c_void_p(None)
        rc = lib.psx_fbp_plan_create(*args, ctypes.byref(h))
        assert not h.value
        return rc, lib.psx_last_error().decode()

    for args, msg in (((0, 8, th, 4.0, 0, 1, 0), "A=0"), ((4097, 8, th, 4.0, 0, 1, 0), "A=4097"),
                      ((3, 1, th, 0.0, 0, 1, 0), "m=1"), ((3, 8193, th, 0.0, 0, 1, 0), "m=8193"),
                      ((3, 8, None, 4.0, 0, 1, 0), "null theta"), ((3, 8, bad, 4.0, 0, 1, 0), "theta[1]"),
                      ((3, 8, th, float("inf"), 0, 1, 0), "center"), ((3, 8, th, 4.0, 3, 1, 0), "filter"),
                      ((3, 8, th, 4.0, 0, 2, 0), "circle"), ((3, 8, th, 4.0, 0, 1, -1), "max_rows")):
        rc, text = create(*args)
        assert rc == -1 and msg in text, (args, rc, text)
    assert lib.psx_fbp_plan_create(3, 8, th, 4.0, 0, 1, 0, None) == -1 and "null plan pointer" in lib.psx_last_error().decode()
    assert lib.psx_fbp_f32(None, None, 1, None, None) == -1 and "null plan" in lib.psx_last_error().decode()
    assert lib.psx_fbp_plan_bytes(None) == 0 and lib.psx_fbp_plan_destroy(None) == 0
    with pytest.raises(_lib.PsxError):
        _lib.check(-1, "psx_fbp_plan_create")
    assert _lib.FBP_FILTERS == {"ramp": 0, "hann": 1, "none": 2} and _lib.ABI_VERSION >= 17


def test_binding_checks_come_before_the_device():
    import torch
    from paresis_amd import ops, tomography
    with pytest.raises(ops.PsxError, match="filter"):
        ops.FbpPlan([0.0, 90.0], 8, filter="shepp")
    with pytest.raises(ops.PsxError, match="theta_deg"):
        ops.FbpPlan(["x"], 8)
    with pytest.raises(ops.PsxError, match="FbpPlan"):
        ops.fbp(torch.zeros((2, 1, 8)), None)
    with pytest.raises(ops.PsxError, match="no CPU path|HBM"):
        tomography.fbp(torch.zeros((2, 1, 8)), [0.0, 90.0])


def _experiment(dimY, ov, pixel_um=6.0, M=1.0254):
    return types.SimpleNamespace(exp_dict={"overSampling": ov, "studyDimensions": [ov * 5, dimY], "magnification": M},
                                 myDetector=types.SimpleNamespace(det_param={"myPixelSize": pixel_um}))


def test_rotation_center_and_units():
    from paresis_amd import tomography
    from paresis_amd.getk import getk
    # study pixel dimY // 2 through ov x ov binning (pad and crop cancel): (x - (ov - 1)/2)/ov
    assert tomography.rotation_center(_experiment(64, 1)) == 32.0
    assert tomography.rotation_center(_experiment(64, 2)) == 15.75            # m = 32: m/2 - 0.25
    assert tomography.rotation_center(_experiment(63, 2)) == 15.25            # odd study grid: 31 -> (31 - 0.5)/2
    assert tomography.rotation_center(_experiment(96, 3)) == (48 - 1.0) / 3
    assert tomography.rotation_center(_experiment(100, 4)) == (50 - 1.5) / 4
    assert tomography.voxel_size(_experiment(64, 2, pixel_um=6.0, M=1.5)) == pytest.approx(4e-6, rel=1e-15)
    # phi = -k delta L: a voxel of 5 um that the back-projection says shifted the phase by -0.02 rad at 52 keV
    k = 2 * np.pi * 52e3 * 1.6e-19 / (6.626e-34 * 2.998e8)
    assert getk(52e3) == pytest.approx(k, rel=1e-15)
    vol = np.array([[[-0.02, 0.0], [0.01, -0.04]]])
    d = tomography.delta_volume(vol, 52.0, 5e-6)
    assert np.allclose(d, -vol / (k * 5e-6), rtol=1e-15) and d[0, 0, 0] > 0
    assert d[0, 0, 0] == pytest.approx(0.02 / (2.6329e11 * 5e-6), rel=1e-3)    # k(52 keV) = 2.633e11 1/m
    assert np.allclose(tomography.mu_volume(vol, 5e-6), vol / 5e-6, rtol=1e-15)
    assert tomography.volume_name("attenuation") == "mu" and tomography.volume_name("phase") == "delta"


def test_scan_refuses_what_it_cannot_turn():
    from paresis_amd import tomography
    exp = _experiment(64, 2)
    exp.exp_dict["nbExpPoints"] = 1
    exp.mySampleofInterest = types.SimpleNamespace(myGeometryFunction="CreateSampleSphere")
    with pytest.raises(ValueError, match="generateContrastPhantom"):
        tomography.scan(exp, [0.0, 90.0])
    with pytest.raises(ValueError, match="generateContrastPhantom"):
        tomography.project(exp.mySampleofInterest, 52.0, [0.0], (24, 64), 500.0)
    exp.mySampleofInterest.myGeometryFunction = "generateContrastPhantom"
    with pytest.raises(ValueError, match="modality"):
        tomography.scan(exp, [0.0], modality="dark-field")
    with pytest.raises(ValueError, match="at least 3 positions"):
        tomography.scan(exp, [0.0], modality="phase")
    with pytest.raises(ValueError, match="options of modality='phase'"):
        tomography.scan(exp, [0.0], modality="attenuation", method="umpa")


def test_sample_angle_defaults_to_the_reference_constant():
    from paresis_amd.Sample import AnalyticalSample
    assert AnalyticalSample().myAngle == 30


def test_save_volume(tmp_path):
    from paresis_amd import tomography
    from paresis_amd.InputOutput.pagailleIO import openImage
    vol = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3) / 7
    (p,) = tomography.save_volume(vol, str(tmp_path / "tomography" / "mu_x"), ".npy")
    assert p.endswith("mu_x.npy") and np.array_equal(np.load(p), vol)
    paths = tomography.save_volume(vol, str(tmp_path / "tomography" / "mu_y"), ".tif")
    assert [q.split("/")[-1] for q in paths] == ["slice_0000.tif", "slice_0001.tif"]
    assert all(np.array_equal(openImage(q), vol[r]) for r, q in enumerate(paths))
    with pytest.raises(ValueError, match="volume"):
        tomography.save_volume(vol[0], str(tmp_path / "bad"), ".npy")
