"""Float64 numpy oracle of the phase retrieval contract (paresis_amd/retrieval.py, csrc/retrieve.hip).

lcs():       per pixel, np.linalg.solve of the stacked 3x3 normal equations of R_k ~ x0*S_k + x1*g0_k + x2*g1_k, with
             (g0, g1) = np.gradient(R_k) on the float32 images (unit spacing, edge_order=1); fallback to (1, 0, 0) when
             det M <= 1e-12*M00*M11*M22 or x0 <= 0; transmission = 1/x0, dx = x1, dy = x2 as float32; optional clamp.
integrate(): Frankot-Chellappa with mirror extension, float64 FFTs.
"""
import numpy as np


def gradients(R):
    """np.gradient, unit spacing, edge_order=1, in the image's own precision (float32 images: float32 differences, as the
    kernel forms them)."""
    return np.gradient(np.asarray(R))


def normal_equations(S, R):
    """M [n, m, 3, 3] and v [n, m, 3] in float64 from K image pairs (float32 as the kernel sees them; float64 for the exact
    model on the host)."""
    K = len(S)
    n, m = np.asarray(S[0]).shape
    M = np.zeros((n, m, 3, 3))
    v = np.zeros((n, m, 3))
    for k in range(K):
        g0, g1 = gradients(R[k])
        a = np.stack([np.asarray(S[k]).astype(np.float64), g0.astype(np.float64), g1.astype(np.float64)], -1)
        b = np.asarray(R[k]).astype(np.float64)
        M += a[..., :, None] * a[..., None, :]
        v += a * b[..., None]
    return M, v


def det3(M):
    """det of symmetric 3x3 systems by the first row's cofactors (the kernel's own expression)."""
    m00, m01, m02 = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    m11, m12, m22 = M[..., 1, 1], M[..., 1, 2], M[..., 2, 2]
    return m00 * (m11 * m22 - m12 * m12) + m01 * (m02 * m12 - m01 * m22) + m02 * (m01 * m12 - m02 * m11)


def lcs(S, R, max_shift=None, return_mask=False, dtype=np.float32):
    """{'transmission', 'dx', 'dy'} as float32 like the kernel (dtype=np.float64: unrounded), and the fallback mask with
    return_mask."""
    M, v = normal_equations(S, R)
    det = det3(M)
    fb = ~(det > 1e-12 * M[..., 0, 0] * M[..., 1, 1] * M[..., 2, 2])
    x = np.zeros(v.shape)
    x[..., 0] = 1.0
    ok = ~fb
    if ok.any():
        x[ok] = np.linalg.solve(M[ok], v[ok][..., None])[..., 0]
    neg = ok & ~(x[..., 0] > 0)
    x[neg] = (1.0, 0.0, 0.0)
    fb = fb | neg
    t = np.where(fb, 1.0, 1.0 / np.where(fb, 1.0, x[..., 0])).astype(dtype)
    dx = x[..., 1].astype(dtype)
    dy = x[..., 2].astype(dtype)
    if max_shift is not None:
        ms = dtype(max_shift)
        dx = np.clip(dx, -ms, ms)
        dy = np.clip(dy, -ms, ms)
    out = {'transmission': t, 'dx': dx, 'dy': dy}
    if return_mask:
        out['fallback'] = fb
    return out


def integrate(gx, gy):
    """The contract's float64 Frankot-Chellappa with mirror extension -> phi [n, m], zero mean over the extension."""
    gx = np.asarray(gx, dtype=np.float64)
    gy = np.asarray(gy, dtype=np.float64)
    n, m = gx.shape
    Gx = np.concatenate([gx, -gx[::-1, :]], 0)
    Gx = np.concatenate([Gx, Gx[:, ::-1]], 1)
    Gy = np.concatenate([gy, gy[::-1, :]], 0)
    Gy = np.concatenate([Gy, -Gy[:, ::-1]], 1)
    kx = 2 * np.pi * np.fft.fftfreq(2 * n)[:, None]
    ky = 2 * np.pi * np.fft.fftfreq(2 * m)[None, :]
    den = kx ** 2 + ky ** 2
    den[0, 0] = 1.0
    P = (-1j * kx * np.fft.fft2(Gx) - 1j * ky * np.fft.fft2(Gy)) / den
    P[0, 0] = 0.0
    return np.fft.ifft2(P).real[:n, :m]


def speckle(n, m, rng, grain=3.0, mean=1e4, contrast=0.3):
    """A smooth, seeded speckle-like reference image (float64): Gaussian-filtered noise of `grain` pixels, positive."""
    f = rng.standard_normal((n, m))
    kx = np.fft.fftfreq(n)[:, None]
    ky = np.fft.fftfreq(m)[None, :]
    F = np.exp(-2 * (np.pi * grain) ** 2 * (kx ** 2 + ky ** 2) / 4)
    s = np.fft.ifft2(np.fft.fft2(f) * F).real
    s /= s.std()
    return mean * (1.0 + contrast * s)


def smooth_field(n, m, rng, amp):
    """A smooth seeded field of amplitude ~amp (a few sinusoids over the grid)."""
    i = np.arange(n)[:, None] / n
    j = np.arange(m)[None, :] / m
    f = np.zeros((n, m))
    for _ in range(3):
        a, b, c, d = rng.uniform(0.5, 2.0, 4)
        f += np.sin(2 * np.pi * (a * i + c)) * np.cos(2 * np.pi * (b * j + d))
    return amp * f / 3.0


def exact_model(n, m, K, seed=0, dmax=0.5, tmin=0.6):
    """float64 fields T, Dx, Dy and K reference images R_k with S_k = T*(R_k - Dx*g0_k - Dy*g1_k) (the model exactly).
    The gradients are those of the float32-rounded R_k, so a float32 copy of the inputs is still an exact instance up to
    the rounding of S_k."""
    rng = np.random.default_rng(seed)
    T = tmin + (1 - tmin) * 0.5 * (1 + smooth_field(n, m, rng, 1.0))
    Dx = smooth_field(n, m, rng, dmax)
    Dy = smooth_field(n, m, rng, dmax)
    R, S = [], []
    for _ in range(K):
        r = speckle(n, m, rng).astype(np.float32)
        g0, g1 = gradients(r)
        S.append(T * (r.astype(np.float64) - Dx * g0 - Dy * g1))
        R.append(r)
    return T, Dx, Dy, S, R
