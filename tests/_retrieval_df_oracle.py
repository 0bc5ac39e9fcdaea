"""Float64 numpy oracle of the LCS-DF contract (paresis_amd.retrieval.lcs(dark_field=True), csrc/retrieve.hip k_lcs_df).

laplacian():        the 5-point Laplacian with edge-replicated neighbours, in float64 from the image's own samples
normal_equations(): M [n, m, 4, 4] and v [n, m, 4] with a = (S, g0, g1, L)
ldl_pivots():       the pivots d_0..d_3 of M = L D L^T without pivoting, in the kernel's order
lcs_df():           per pixel, np.linalg.solve of the 4x4 system; fallback x = (1, 0, 0, 0) when a pivot <= 0,
                    prod d_i <= 1e-12*M00*M11*M22*M33 or x0 <= 0; transmission = 1/x0, dx = x1, dy = x2 (optional clamp),
                    df = -x3 (not clamped)
exact_model():      S_k = T*(R_k - Dx*g0_k - Dy*g1_k + Df*L_k), whose exact solution is (1/T, Dx, Dy, -Df)
lcs_df_exact():     the contract in exact rational arithmetic; lcs_df_f64(): k_lcs_df's own expressions in float64 and
                    its wrong variants; lcs_df_parity(): both on one case of LCS_DF_CASES, and the yardstick between them
"""
import functools

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
    with np.errstate(invalid="ignore", over="ignore"):
        M, v = normal_equations(S, R)
    fb = singular(M) | ~(np.isfinite(M).all((-1, -2)) & np.isfinite(v).all(-1))   # non-finite sample read: never solved
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


# ------------------------------------------------------------------------------------------- exact and restated references
MAPS = ('transmission', 'dx', 'dy', 'df')
VARIANTS = orl.VARIANTS + ('zeropad',)                       # wrong kernels the bound must reject (droplast: odd K only)


def corners(n, m):
    """[n, m] bool: the four corners, structural fallbacks of LCS-DF (one-sided differences and replicated neighbours make
    L = g0 + g1 there up to the float32 rounding of the two differences, so det M is 0 or far below the threshold whatever
    the images hold)."""
    c = np.zeros((n, m), bool)
    c[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    return c


def lcs_df_exact(S, R):
    """The LCS-DF contract per pixel in exact rational arithmetic (tests/_retrieval_oracle.lcs_exact with the Laplacian,
    formed exactly, as fourth column).  The pivots of the unpivoted LDL^T are d_i = D_i/D_(i-1) of the leading principal
    minors, so `a pivot <= 0` is `a minor <= 0` and prod d_i is det M.  -> float64 {'transmission', 'dx', 'dy', 'df'},
    the bool 'fallback', and 'det_ratio' = det M/(1e-12 M00 M11 M22 M33), 'pivot_ratio' = min_i d_i/M_ii (0 where a minor is
    <= 0), 'x0' for the distance from the rules."""
    bad = orl.nonfinite_pixels(S, R)
    S, R = orl.finite_copy(S, R)
    g = [orl.gradients(r) for r in R]
    Rx = orl.exact(np.stack(R))
    P = np.pad(Rx, ((0, 0), (1, 1), (1, 1)), mode="edge")
    L = P[:, 2:, 1:-1] + P[:, :-2, 1:-1] + P[:, 1:-1, 2:] + P[:, 1:-1, :-2] - 4 * Rx
    cols = [orl.exact(np.stack(S)), orl.exact(np.stack([a for a, _ in g])), orl.exact(np.stack([b for _, b in g])), L]
    M, minors, num = orl.solve_exact(cols, Rx)
    det = minors[-1]
    thr = orl.Fraction(1e-12) * M[0][0] * M[1][1] * M[2][2] * M[3][3]
    pos = np.ones(bad.shape, bool)
    for D in minors:
        pos &= (D > 0).astype(bool)
    one = orl.Fraction(1)
    prev = [one + 0 * minors[0]] + minors[:-1]
    ratio = np.min([orl.to_float(np.where(pos, minors[i] / np.where(pos, prev[i] * M[i][i], one), 0 * one)) for i in range(4)], 0)
    fb = bad | ~pos | (det <= thr).astype(bool)
    return orl.finish_exact(fb, det, num, thr, {'pivot_ratio': ratio})


def lcs_df_f64(S, R, variant=None):
    """k_lcs_df restated in numpy float64: its sums and its unpivoted LDL^T with the kernel's reciprocals, products and
    tests in the kernel's order (NaN and infinity go where the kernel sends them) -> unrounded float64 maps and
    'fallback'.  variant: one of VARIANTS, a wrong kernel."""
    M, (v0, v1, v2, v3) = orl.kernel_sums(S, R, 4, variant)
    m00, m01, m02, m03 = M[0, 0], M[0, 1], M[0, 2], M[0, 3]
    m11, m12, m13, m22, m23, m33 = M[1, 1], M[1, 2], M[1, 3], M[2, 2], M[2, 3], M[3, 3]
    with np.errstate(all="ignore"):
        d0 = m00
        r0 = 1.0 / d0
        l10, l20, l30 = m01 * r0, m02 * r0, m03 * r0
        d1 = m11 - l10 * m01
        r1 = 1.0 / d1
        e21, e31 = m12 - l20 * m01, m13 - l30 * m01
        l21, l31 = e21 * r1, e31 * r1
        d2 = m22 - l20 * m02 - l21 * e21
        r2 = 1.0 / d2
        e32 = m23 - l30 * m02 - l31 * e21
        l32 = e32 * r2
        d3 = m33 - l30 * m03 - l31 * e31 - l32 * e32
        go = (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0) & (d3 > 0.0) & ~(d0 * d1 * d2 * d3 <= 1e-12 * m00 * m11 * m22 * m33)
        y1 = v1 - l10 * v0
        y2 = v2 - l20 * v0 - l21 * y1
        y3 = v3 - l30 * v0 - l31 * y1 - l32 * y2
        x3 = y3 / d3
        x2 = y2 * r2 - l32 * x3
        x1 = y1 * r1 - l21 * x2 - l31 * x3
        x0 = v0 * r0 - l10 * x1 - l20 * x2 - l30 * x3
        ok = go & (x0 > 0.0)
        out = {'transmission': np.where(ok, 1.0 / x0, 1.0), 'dx': np.where(ok, x1, 0.0), 'dy': np.where(ok, x2, 0.0),
               'df': np.where(ok, -x3, 0.0), 'fallback': ~ok}
    return out


# (n, m, K, seed, max_shift): tests/_retrieval_oracle.LCS_CASES with K raised to 4 at least.  Seeds 1 to 6 in turn, but for the second shape
# (Y = 2.4e-8 at seed 2 misses the host tests' condition 8 Y <= 2^-24); max_shift as there.
LCS_DF_CASES = [(3, 3, 4, 1, None), (5, 65, 4, 1, None), (4, 64, 5, 3, None), (5, 65, 5, 4, None), (9, 66, 8, 5, None),
                (3, 3, 64, 6, None), (5, 65, 5, 4, 0.2)]


@functools.lru_cache(maxsize=None)
def lcs_df_parity(n, m, K, seed, steep=False):
    """One case's inputs and CPU references, computed once per process: (S, R, exact, f64, Y).  steep: on
    tests/_retrieval_oracle.steep_model's images."""
    model = functools.partial(orl.steep_model, laplacian=laplacian) if steep else exact_model
    S, R = orl.case_inputs(model, n, m, K, seed)
    ref, f64 = lcs_df_exact(S, R), lcs_df_f64(S, R)
    return S, R, ref, f64, orl.yardstick(f64, ref, MAPS)
