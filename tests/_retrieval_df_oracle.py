"""Float64 numpy oracle of the LCS-DF contract (paresis_amd.retrieval.lcs(dark_field=True), csrc/retrieve.hip k_lcs_df).

laplacian():        the 5-point Laplacian with edge-replicated neighbours, in float64 from the image's own samples
normal_equations(): M [n, m, 4, 4] and v [n, m, 4] with a = (S, g0, g1, L)
ldl_pivots():       the pivots d_0..d_3 of M = L D L^T without pivoting, in the kernel's order
lcs_df():           per pixel, np.linalg.solve of the 4x4 system; fallback x = (1, 0, 0, 0) when a pivot <= 0,
                    prod d_i <= 1e-12*M00*M11*M22*M33 or x0 <= 0; transmission = 1/x0, dx = x1, dy = x2 (optional clamp),
                    df = -x3 (not clamped)
exact_model():      S_k = T*(R_k - Dx*g0_k - Dy*g1_k + Df*L_k), whose exact solution is (1/T, Dx, Dy, -Df)
"""
import numpy as np

from tests import _retrieval_oracle as orl


def laplacian(R):
    """R[i+1,j] + R[i-1,j] + R[i,j+1] + R[i,j-1] - 4 R[i,j] with edge-replicated neighbours, float64 (exact for float32
    image data)."""
    P = np.pad(np.asarray(R).astype(np.float64), 1, mode="edge")
    return P[2:, 1:-1] + P[:-2, 1:-1] + P[1:-1, 2:] + P[1:-1, :-2] - 4.0 * P[1:-1, 1:-1]


def normal_equations(S, R):
    """M [n, m, 4, 4] and v [n, m, 4] in float64 from K image pairs; gradients as tests/_retrieval_oracle.gradients."""
    n, m = np.asarray(S[0]).shape
    M = np.zeros((n, m, 4, 4))
    v = np.zeros((n, m, 4))
    for s, r in zip(S, R):
        g0, g1 = orl.gradients(r)
        a = np.stack([np.asarray(s).astype(np.float64), g0.astype(np.float64), g1.astype(np.float64), laplacian(r)], -1)
        b = np.asarray(r).astype(np.float64)
        M += a[..., :, None] * a[..., None, :]
        v += a * b[..., None]
    return M, v


def ldl_pivots(M):
    """d [..., 4]: the pivots of M = L D L^T without pivoting, column by column as the kernel forms them (NaN past a pivot
    <= 0 is harmless: the mask stops at the first)."""
    m = lambda i, j: M[..., i, j]
    with np.errstate(divide="ignore", invalid="ignore"):
        d0 = m(0, 0)
        l10, l20, l30 = m(0, 1) / d0, m(0, 2) / d0, m(0, 3) / d0
        d1 = m(1, 1) - l10 * m(0, 1)
        e21, e31 = m(1, 2) - l20 * m(0, 1), m(1, 3) - l30 * m(0, 1)
        l21, l31 = e21 / d1, e31 / d1
        d2 = m(2, 2) - l20 * m(0, 2) - l21 * e21
        e32 = m(2, 3) - l30 * m(0, 2) - l31 * e21
        l32 = e32 / d2
        d3 = m(3, 3) - l30 * m(0, 3) - l31 * e31 - l32 * e32
    return np.stack([d0, d1, d2, d3], -1)


def singular(M):
    """The contract's first two fallback rules: any pivot <= 0 (or NaN), or prod d_i <= 1e-12*M00*M11*M22*M33."""
    d = ldl_pivots(M)
    bad = ~(d > 0).all(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        bad |= ~(np.prod(d, -1) > 1e-12 * M[..., 0, 0] * M[..., 1, 1] * M[..., 2, 2] * M[..., 3, 3])
    return bad


def lcs_df(S, R, max_shift=None, return_mask=False, dtype=np.float32):
    """{'transmission', 'dx', 'dy', 'df'} as float32 like the kernel (dtype=np.float64: unrounded), and the fallback mask
    with return_mask."""
    M, v = normal_equations(S, R)
    fb = singular(M)
    x = np.zeros(v.shape)
    x[..., 0] = 1.0
    ok = ~fb
    if ok.any():
        x[ok] = np.linalg.solve(M[ok], v[ok][..., None])[..., 0]
    neg = ok & ~(x[..., 0] > 0)
    x[neg] = (1.0, 0.0, 0.0, 0.0)
    fb = fb | neg
    t = np.where(fb, 1.0, 1.0 / np.where(fb, 1.0, x[..., 0])).astype(dtype)
    dx = x[..., 1].astype(dtype)
    dy = x[..., 2].astype(dtype)
    df = np.where(fb, 0.0, -x[..., 3]).astype(dtype)
    if max_shift is not None:
        ms = dtype(max_shift)
        dx = np.clip(dx, -ms, ms)
        dy = np.clip(dy, -ms, ms)
    out = {'transmission': t, 'dx': dx, 'dy': dy, 'df': df}
    if return_mask:
        out['fallback'] = fb
    return out


def exact_model(n, m, K, seed=0, dmax=0.5, dfmax=0.3, tmin=0.6):
    """float64 fields T, Dx, Dy, Df (Df > 0, up to dfmax px^2) and K reference images R_k with
    S_k = T*(R_k - Dx*g0_k - Dy*g1_k + Df*L_k).  The gradients and Laplacians are those of the float32-rounded R_k, so a
    float32 copy of the inputs is still an exact instance up to the rounding of S_k."""
    rng = np.random.default_rng(seed)
    T = tmin + (1 - tmin) * 0.5 * (1 + orl.smooth_field(n, m, rng, 1.0))
    Dx = orl.smooth_field(n, m, rng, dmax)
    Dy = orl.smooth_field(n, m, rng, dmax)
    Df = dfmax * 0.5 * (1 + orl.smooth_field(n, m, rng, 1.0))
    R, S = [], []
    for _ in range(K):
        r = orl.speckle(n, m, rng).astype(np.float32)
        g0, g1 = orl.gradients(r)
        S.append(T * (r.astype(np.float64) - Dx * g0 - Dy * g1 + Df * laplacian(r)))
        R.append(r)
    return T, Dx, Dy, Df, S, R
