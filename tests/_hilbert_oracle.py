"""Float64 numpy oracle of the differential filters of the filtered back-projection contract (include/paresis_hip.h:
PSX_FBP_HILBERT, PSX_FBP_HILBERT_HANN), their float32 / complex64 restatement (the yardstick of the GPU parity bound), and
the analytic Gaussian-blob sinograms on which Hilbert(dp/du) and ramp(p) must agree.  Geometry, sampling and the parity
cases are tests/_fbp_oracle.py's; nothing here imports the package's kernels."""
import numpy as np

from tests import _fbp_oracle as fo

FILTERS = ("hilbert", "hilbert-hann")


def hilbert_kernel(P, sign=1.0):
    """g[j] = 2/(pi^2 s) for odd signed lag s (s = j for j < P/2, s = j - P for j > P/2), 0 for even s and at j = P/2.
    sign = -1: the other convention, which the tests show to be wrong."""
    j = np.arange(P)
    s = np.where(j < P // 2, j, j - P)
    g = np.zeros(P)
    odd = (s % 2 != 0) & (j != P // 2)
    g[odd] = sign * 2.0 / (np.pi ** 2 * s[odd])
    return g


def hilbert_transform(P):
    """G = FFT_P(g), complex: the tests look at its real part before it is dropped."""
    return np.fft.fft(hilbert_kernel(P))


def hilbert_response(P, name, sign=1.0):
    """Ho = Im FFT_P(g) with Ho[0] = Ho[P/2] = 0 exactly, times the shifted Hann window for 'hilbert-hann'."""
    Ho = np.imag(np.fft.fft(hilbert_kernel(P, sign)))
    Ho[0] = Ho[P // 2] = 0.0
    if name == "hilbert-hann":
        Ho = Ho * np.fft.fftshift(np.hanning(P))
    elif name != "hilbert":
        raise ValueError(name)
    return Ho


def filter_lines(sino, name, sign=1.0):
    """q = Re IFFT_P(FFT_P(line zero-padded to P) * i*Ho)[:m] along the last axis, float64."""
    sino = np.asarray(sino, dtype=np.float64)
    m = sino.shape[-1]
    P = fo.pad_length(m)
    Ho = hilbert_response(P, name, sign)
    return np.real(np.fft.ifft(np.fft.fft(sino, n=P, axis=-1) * (1j * Ho), axis=-1))[..., :m]


def _backproject(q, theta_deg, center, circle, dtype):
    A, n, m = q.shape
    vol = np.zeros((n, m, m), dtype=dtype)
    for a in range(A):
        vol += fo.sample(q[a], fo.grid_u(m, theta_deg[a], center)).astype(dtype)
    vol *= dtype(np.pi / (2 * A))
    if circle:
        vol *= fo.circle_mask(m)
    return vol


def fbp(sino, theta_deg, center=None, filter="hilbert", circle=True, sign=1.0):
    """sino [A][n][m], d(line integral)/d(column) per pixel -> vol [n][m][m], all float64: fo.fbp with the Hilbert filter."""
    sino = np.asarray(sino, dtype=np.float64)
    m = sino.shape[2]
    center = float(m // 2 if center is None else center)
    return _backproject(filter_lines(sino, filter, sign), theta_deg, center, circle, np.float64)


def fbp_f32(sino, theta_deg, center=None, filter="hilbert", circle=True):
    """The contract in the GPU's number formats, on the CPU, as fo.fbp_f32: complex64 transforms of two rows at a time, the
    table -- the odd part of Ho over P -- in float64, (x, y) -> (-w*y, w*x) rounded to float32, float32 weights, samples
    and accumulation in ascending angle."""
    sino = np.asarray(sino, dtype=np.float32)
    A, n, m = sino.shape
    center = float(m // 2 if center is None else center)
    P = fo.pad_length(m)
    Ho = hilbert_response(P, filter)
    w = 0.5 * (Ho - np.roll(Ho[::-1], 1)) / P
    npair = (n + 1) // 2
    z = np.zeros((A, npair, P), dtype=np.complex64)
    z.real[:, :, :m] = sino[:, 0::2]
    z.imag[:, :n // 2, :m] = sino[:, 1::2]
    Z = np.fft.fft(z, axis=-1)
    assert Z.dtype == np.complex64
    Z = (-Z.imag.astype(np.float64) * w).astype(np.float32) + 1j * (Z.real.astype(np.float64) * w).astype(np.float32)
    y = np.fft.ifft(Z.astype(np.complex64), axis=-1) * np.float32(P)                # numpy's inverse divides by P itself
    assert y.dtype == np.complex64
    q = np.empty((A, n, m), dtype=np.float32)
    q[:, 0::2] = y.real[:, :, :m]
    q[:, 1::2] = y.imag[:, :n // 2, :m]
    return _backproject(q, theta_deg, center, circle, np.float32)


# ---- the parity cases: fo.SHAPES and two more about the pad length, P = 64 = 2m exactly and the step to 128 ----------
EXTRA_SHAPES = [(5, 3, 32), (5, 3, 33)]
SHAPES = fo.SHAPES + EXTRA_SHAPES

# max|fbp_f32 - fbp| / max|fbp| per parity shape (A, n, m): the worst over the two filters and the two centres of
# fo.case_centers, circle off, on fo.case_sino / fo.case_angles -- measured with numpy's float32 pocketfft on the CPU, as
# fo.F32_ERROR was (tests/test_hilbert_host.py reproduces them).  The GPU parity bound of tests/test_gpu_hilbert.py is 8
# times these.
F32_ERROR_HILBERT = {(1, 1, 2): 6.6e-8, (3, 2, 5): 1.06e-7, (7, 1, 64): 2.8e-7, (90, 3, 64): 4.9e-7, (33, 5, 301): 4.1e-7,
                     (180, 2, 512): 1.02e-6, (5, 3, 32): 2.0e-7, (5, 3, 33): 2.5e-7}


# ---- Gaussian blobs: analytic p and dp/du ------------------------------------------------------------------------------
# (amplitude, slice row offset / m, slice column offset / m, sigma in pixels) about voxel (h, h), h = m // 2.  sigma >= 2:
# the spectrum exp(-2 pi^2 sigma^2 f^2) is 3e-9 of its peak at Nyquist, so the samples of p and of dp/du are band-limited
# to that, which is where the two discrete filters stand for the same operator.  The offsets stay within 0.13 m of the axis,
# so that at the smallest case (m = 33, 16 pixels to the detector's end) every blob's projection has fallen by 4.7 sigma
# or more where the detector cuts it.
BLOBS = ((1.0, 0.10, 0.05, 2.0), (-0.6, -0.08, 0.10, 2.5), (0.8, 0.0, -0.12, 2.0))
# (m, A, center or None for m // 2, the gap max|fbp_hilbert(dp/du) - fbp_ramp(p)| / max|fbp_ramp(p)| the float64 oracles
# were first seen to have on three such blobs): the identity's bound is twice the last.
BLOB_CASES = ((64, 90, None, 1.1e-6), (65, 60, 31.75, 2.1e-7), (128, 180, None, 1.3e-6), (33, 45, 16.25, 3.2e-5))


def blob_sinograms(m, A, center=None):
    """-> (theta [A], p [A][1][m], dp/du [A][1][m]) of BLOBS, float64: a blob a*exp(-r^2/(2 s^2)) at voxel (i0, j0) projects
    to a*s*sqrt(2 pi)*exp(-(u - u0)^2/(2 s^2)) with u0 = (j0 - h) cos - (i0 - h) sin + center, the contract's u."""
    center = float(m // 2 if center is None else center)
    theta = np.arange(A) * (180.0 / A)
    th = np.deg2rad(theta)[:, None]
    u = np.arange(m, dtype=np.float64)[None, :]
    p, dp = np.zeros((A, m)), np.zeros((A, m))
    for amp, di, dj, sigma in BLOBS:
        u0 = dj * m * np.cos(th) - di * m * np.sin(th) + center
        one = amp * sigma * np.sqrt(2 * np.pi) * np.exp(-(u - u0) ** 2 / (2 * sigma ** 2))
        p += one
        dp += -(u - u0) / sigma ** 2 * one
    return theta, p[:, None, :], dp[:, None, :]


def central_differences(sino):
    """(sino[..., k + 1] - sino[..., k - 1])/2 along the last axis with zeros beyond either end, numpy."""
    pad = np.zeros(sino.shape[:-1] + (1,), dtype=sino.dtype)
    s = np.concatenate([pad, sino, pad], axis=-1)
    return 0.5 * (s[..., 2:] - s[..., :-2])
