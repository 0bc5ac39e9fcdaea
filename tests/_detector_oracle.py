"""Detector.detection (Detector.py:79-119) with the margin as a parameter, and the dense form of the host-composed operator.

`detection` is the chain of oracle.paresis_oracle.detection step for step -- reflect pad, source blur, bin SUM, PSF, crop --
with the reference's fixed margin of 15 detector pixels made an argument (the C ABI takes it as one): at margin 15 the two are
the same numbers bit for bit (tests/test_detector_host.py holds them to that)."""
import numpy as np
from scipy.signal import fftconvolve

from oracle import paresis_oracle as orc


def detection(img, fwhm, ov, dims, psf, margin):
    """The float64 expectation image of a `dims` detector behind the study-grid image `img`: source blur of `fwhm` study
    pixels (0: none), ov x ov bin sums, PSF of sigma `psf` detector pixels (0: none), over a reflect pad of `margin` detector
    pixels that is cropped again."""
    x = np.pad(img, margin * ov, mode="reflect")                                # DET:93
    if fwhm != 0:                                                               # DET:96-99
        x = fftconvolve(x, orc.create_gaussian_shape(fwhm / 2.355), mode="same")
    x = orc.resize(x, dims[0] + margin * 2, dims[1] + margin * 2)               # DET:103
    if psf != 0:                                                                # DET:106-110
        x = fftconvolve(x, orc.create_gaussian_shape(psf), mode="same")
    return x[margin:dims[0] + margin, margin:dims[1] + margin]                  # DET:118


def dense(start, w, N):
    """A banded operator (start[n], weights[n][W]) as a dense float64 [n x N] matrix; taps beyond the axis (a band wider than
    the axis) carry zero weights and are dropped."""
    C = np.zeros((len(start), N))
    for r in range(len(start)):
        k = min(w.shape[1], N - start[r])
        C[r, start[r]:start[r] + k] = w[r, :k]
    return C


def composite(ops, N, ov, n, sigma_src, sigma_psf, margin):
    """One axis of the host-composed detector operator (ops.detector_operator_host) as a dense float64 matrix."""
    start, w = ops.detector_operator_host(N, ov, n, sigma_src, sigma_psf, margin=margin)
    return dense(start, w, N)
