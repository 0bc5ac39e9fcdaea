"""CPU: the detector's host side on the smallest grids it takes.  tests/_detector_oracle.detection is Detector.detection with
the margin as a parameter (at 15 it IS orc.detection, bit for bit); the dense composite of ops.detector_operator_host, applied
in float64, reproduces it within 2e-7 of the image maximum (the tolerance of test_detector_operator_matches_oracle in
tests/test_host_cpu.py; the float32 rounding of the weights is 6e-8 of each) at margins 0, 3 and 15, ov 1 ... 4, detectors of
1 x 2 to 40 x 65 pixels -- reflect pads that fold several times, bands wider than their axis -- and every blur of the list.
tests/test_gpu_detector.py holds the device to that dense composite."""
import ctypes

import numpy as np
import pytest

from oracle import paresis_oracle as orc
from tests import _detector_oracle as do
from tests._golden import relmax

TOL = 2e-7
MARGINS = (0, 3, 15)
OVS = (1, 2, 3, 4)
SIZES = ((1, 2), (2, 2), (3, 5), (7, 4), (16, 15), (17, 33), (40, 65))     # detector pixels
FWHMS = (0.0, 0.4, 1.3, 3.0, 9.0)
PSFS = (0.0, 0.5, 1.2, 1.7, 2.5, 6.0)


def grids(ov):
    """(nx, ny, Nx, Ny) of the list that the library takes: a study axis has at least 2 pixels."""
    return [(nx, ny, nx * ov, ny * ov) for nx, ny in SIZES if nx * ov >= 2 and ny * ov >= 2]


def image(Nx, Ny, seed):
    return np.random.default_rng(seed).uniform(0.2, 2.0, (Nx, Ny))


def test_oracle_at_margin_15_is_the_reference_chain():
    n = 0
    for ov in OVS:
        for nx, ny, Nx, Ny in grids(ov):
            img = image(Nx, Ny, 100 * Nx + Ny)
            for fwhm in FWHMS:
                for psf in PSFS:
                    assert np.array_equal(do.detection(img, fwhm, ov, (nx, ny), psf, 15), orc.detection(img, fwhm, ov, (nx, ny), psf))
                    n += 1
    assert n == (6 + 3 * 7) * len(FWHMS) * len(PSFS)        # ov = 1 leaves out the 1 x 2 detector


@pytest.mark.parametrize("ov", OVS)
@pytest.mark.parametrize("margin", MARGINS)
def test_host_operator_matches_oracle(margin, ov):
    from paresis_amd import ops
    worst, n = 0.0, 0
    for nx, ny, Nx, Ny in grids(ov):
        img = image(Nx, Ny, 100 * Nx + Ny + margin)
        for fwhm in FWHMS:
            for psf in PSFS:
                sig = fwhm / 2.355
                Cx = do.composite(ops, Nx, ov, nx, sig, psf, margin)
                Cy = do.composite(ops, Ny, ov, ny, sig, psf, margin)
                assert Cx.shape == (nx, Nx) and Cy.shape == (ny, Ny)
                assert Cx.min() >= 0.0 and Cy.min() >= 0.0       # the per-pixel bound of the device tests rests on this
                e = relmax(Cx @ img @ Cy.T, do.detection(img, fwhm, ov, (nx, ny), psf, margin))
                assert e < TOL, (margin, ov, nx, ny, fwhm, psf, e)
                worst, n = max(worst, e), n + 1
    assert n == (6 if ov == 1 else 7) * len(FWHMS) * len(PSFS)
    print("margin %d ov %d: %d cases, worst %.2e of the image maximum" % (margin, ov, n, worst))


def test_dense_drops_the_taps_beyond_the_axis():
    """A band wider than its axis: the operator's rows start at 0 and their taps at and beyond N carry no weight."""
    from paresis_amd import ops
    start, w = ops.detector_operator_host(2, 1, 2, 0.0, 5.4)       # 33 PSF taps folded onto 2 study pixels
    assert w.shape[1] == 2 and np.array_equal(start, [0, 0])
    start, w = ops.detector_operator_host(4, 2, 2, 9.0 / 2.355, 0.0, margin=0)
    assert w.shape[1] == 4 and np.array_equal(start, [0, 0])
    C = do.dense(np.array([0, 1]), np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]), 3)
    assert np.array_equal(C, [[1.0, 2.0, 3.0], [0.0, 4.0, 5.0]])


def test_abi_has_the_plan_accessor():
    from paresis_amd import _lib, ops
    lib = _lib.lib()
    assert _lib.ABI_VERSION >= 23 and lib.psx_abi_version() == _lib.ABI_VERSION
    assert "psx_detector_plan_info" in _lib.PROTOTYPES and hasattr(lib, "psx_detector_plan_info")
    assert _lib.PSX_DETECTOR_PLAN_INFO == len(ops.DetectorPlan.INFO_FIELDS) == 12
    buf = (ctypes.c_int * 12)(*([-7] * 12))
    assert lib.psx_detector_plan_info(None, buf, 12) == 0 and list(buf) == [-7] * 12      # no plan: nothing written
