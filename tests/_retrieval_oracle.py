"""Float64 numpy oracle of the phase retrieval contract (paresis_amd/retrieval.py, csrc/retrieve.hip).

lcs():       per pixel, np.linalg.solve of the stacked 3x3 normal equations of R_k ~ x0*S_k + x1*g0_k + x2*g1_k, with
             (g0, g1) = np.gradient(R_k) on the float32 images (unit spacing, edge_order=1); fallback to (1, 0, 0) when
             det M <= 1e-12*M00*M11*M22 or x0 <= 0; transmission = 1/x0, dx = x1, dy = x2 as float32; optional clamp.
integrate(): Frankot-Chellappa with mirror extension, float64 FFTs.
Further down: the exact rational reference lcs_exact(), the kernels' own expressions restated on the CPU (lcs_f64(),
integrate_f32()) and the parity bound built from the two.
"""
import functools
from fractions import Fraction

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
    with np.errstate(invalid="ignore", over="ignore"):
        M, v = normal_equations(S, R)
        det = det3(M)
        fb = ~(det > 1e-12 * M[..., 0, 0] * M[..., 1, 1] * M[..., 2, 2])
    fb |= ~(np.isfinite(M).all((-1, -2)) & np.isfinite(v).all(-1))   # a non-finite sample read: fallback, never solved
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


# ------------------------------------------------------------------------------------------- exact and restated references
# lcs_exact():     the contract in exact rational arithmetic (fractions.Fraction): float32 inputs and the float32 gradients
#                  converted exactly, normal equations, Cramer's rule and the fallback rule without a rounding
# lcs_f64():       k_lcs's own expressions in numpy float64 (cofactors, first-row determinant, the kernel's tests in the
#                  kernel's order), and its wrong variants for the host tests of the parity bound
# lcs_parity():    both on one case of LCS_CASES and the yardstick Y between them; parity_bound() / check_parity(): the bound
#                  the GPU is held to, 2^-24 |x*| + 8 Y scale
# integrate_f32(): k_integ_pack / k_integ_filter / k_integ_crop in their number formats around torch's complex64 transforms;
#                  integrate_yardstick(): its distance from integrate(), the yardstick of the GPU integrator's bound
_fraction = np.frompyfunc(Fraction, 1, 1)
_float = np.frompyfunc(float, 1, 1)
VARIANTS = ('acc32', 'spacing', 'wrap', 'droplast')          # wrong kernels the bound must reject (droplast: odd K only)


def exact(a):
    """An object array of Fractions holding the finite floats of `a` exactly."""
    return _fraction(np.asarray(a, dtype=np.float64))


def to_float(a):
    """The correctly rounded float64 of every Fraction of `a`."""
    return _float(a).astype(np.float64)


def det_exact(A):
    """The determinant of a square matrix given as a list of rows of (arrays of) Fractions, by Laplace expansion."""
    if len(A) == 1:
        return A[0][0]
    total = 0
    for j in range(len(A)):
        term = A[0][j] * det_exact([row[:j] + row[j + 1:] for row in A[1:]])
        total = total + term if j % 2 == 0 else total - term
    return total


def nonfinite_pixels(S, R):
    """[n, m] bool: the pixels whose own S_k, own R_k or one of the four clamped neighbours of R_k is not finite for some k.
    These return the fallback (include/paresis_hip.h); all others never read a non-finite sample."""
    bad_s = ~np.isfinite(np.stack(S)).all(0)
    bad_r = ~np.isfinite(np.stack(R)).all(0)
    P = np.pad(bad_r, 1, mode="edge")
    return bad_s | bad_r | P[2:, 1:-1] | P[:-2, 1:-1] | P[1:-1, 2:] | P[1:-1, :-2]


def finite_copy(S, R):
    """The images with every non-finite sample set to 0, for the references' arithmetic; nonfinite_pixels() decides there."""
    return ([np.where(np.isfinite(s), s, np.float32(0)) for s in S], [np.where(np.isfinite(r), r, np.float32(0)) for r in R])


def solve_exact(cols, b):
    """M = sum_k a a^T and v = sum_k a b from the columns a_i [K, n, m] (Fractions) -> (M as rows of [n, m] arrays, the
    leading principal minors D_1..D_p, the Cramer numerators N_i with x_i = N_i/D_p)."""
    p = len(cols)
    M = [[(cols[i] * cols[j]).sum(0) for j in range(p)] for i in range(p)]
    v = [(cols[i] * b).sum(0) for i in range(p)]
    minors = [det_exact([row[:q] for row in M[:q]]) for q in range(1, p + 1)]
    num = [det_exact([row[:i] + [v[r]] + row[i + 1:] for r, row in enumerate(M)]) for i in range(p)]
    return M, minors, num


def finish_exact(fb, det, num, thr, extra):
    """The maps of an exact solve: 1/x0, x1, x2 (, -x3) as float64, (1, 0, 0 (, 0)) at the fallback pixels; `det_ratio` =
    det/threshold and `x0` (float64) say how far every pixel is from the rules' thresholds."""
    one = Fraction(1)
    safe = np.where(fb, one, det)
    x = [np.where(fb, one if i == 0 else 0 * one, num[i] / safe) for i in range(len(num))]
    neg = ~fb & (x[0] <= 0).astype(bool)
    fb = fb | neg
    x = [np.where(neg, one if i == 0 else 0 * one, xi) for i, xi in enumerate(x)]
    out = {'transmission': to_float(one / x[0]), 'dx': to_float(x[1]), 'dy': to_float(x[2]), 'fallback': fb,
           'x0': to_float(x[0])}
    if len(x) == 4:
        out['df'] = to_float(-x[3])
    pos = (thr > 0).astype(bool)
    out['det_ratio'] = np.where(pos, to_float(det / np.where(pos, thr, one)), np.inf)
    out.update(extra)
    return out


def lcs_exact(S, R):
    """The LCS contract per pixel in exact rational arithmetic -> float64 {'transmission', 'dx', 'dy'} (each the correctly
    rounded exact value), the bool 'fallback', and 'det_ratio' = det M/(1e-12 M00 M11 M22), 'x0' for the distance from the
    rules.  Non-finite input: nonfinite_pixels() are fallbacks."""
    bad = nonfinite_pixels(S, R)
    S, R = finite_copy(S, R)
    g = [gradients(r) for r in R]
    cols = [exact(np.stack(S)), exact(np.stack([a for a, _ in g])), exact(np.stack([b for _, b in g]))]
    M, minors, num = solve_exact(cols, exact(np.stack(R)))
    det = minors[-1]
    thr = Fraction(1e-12) * M[0][0] * M[1][1] * M[2][2]
    fb = bad | (det <= thr).astype(bool)
    return finish_exact(fb, det, num, thr, {})


def clamped_neighbours(n, wrap=False):
    """(i+1, i-1) clamped to the image as the kernels index them (wrap: the wrong variant that wraps around)."""
    i = np.arange(n)
    return ((i + 1) % n, (i - 1) % n) if wrap else (np.minimum(i + 1, n - 1), np.maximum(i - 1, 0))


def kernel_columns(s, r, variant=None):
    """One position's a = (S, g0, g1, L) and b = R as k_lcs / k_lcs_df form them: float32 differences times 0.5f or 1.0f,
    the Laplacian in float64 from the same six loads.  Variants: 'spacing' (0.5 on the border too), 'wrap', 'zeropad' (the
    Laplacian's missing neighbours are 0), 'acc32' (the Laplacian in float32 as well)."""
    n, m = r.shape
    ip, im = clamped_neighbours(n, variant == 'wrap')
    jp, jm = clamped_neighbours(m, variant == 'wrap')
    border = np.float32(0.5 if variant == 'spacing' else 1.0)
    h0 = np.where(ip - im == 2, np.float32(0.5), border).astype(np.float32)[:, None]
    h1 = np.where(jp - jm == 2, np.float32(0.5), border).astype(np.float32)[None, :]
    ru, rd, rr, rl = r[ip], r[im], r[:, jp], r[:, jm]
    with np.errstate(invalid="ignore"):
        if variant == 'diff64':
            a1, a2 = (ru.astype(np.float64) - rd) * h0, (rr.astype(np.float64) - rl) * h1
        else:
            a1, a2 = (ru - rd) * h0, (rr - rl) * h1
            assert a1.dtype == np.float32 and a2.dtype == np.float32
        wide = np.float32 if variant == 'acc32' else np.float64
        lu, ld, lr, ll = (x.astype(wide) for x in (ru, rd, rr, rl))
        if variant == 'zeropad':
            lu[-1], ld[0], lr[:, -1], ll[:, 0] = 0, 0, 0, 0
        a3 = ((lu + ld) + (lr + ll)) - wide(4) * r.astype(wide)
    return [s, a1, a2, a3], r


def kernel_sums(S, R, p, variant=None):
    """m[i][j] (i <= j) and v[i] of the first p columns, accumulated over k in order in float64 ('acc32': products and sums
    in float32; 'droplast': an odd K loses its last position) -> float64."""
    K = len(S) - 1 if variant == 'droplast' and len(S) % 2 else len(S)
    dt = np.float32 if variant == 'acc32' else np.float64
    shape = np.asarray(R[0]).shape
    M = {(i, j): np.zeros(shape, dt) for i in range(p) for j in range(i, p)}
    v = [np.zeros(shape, dt) for _ in range(p)]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            a, b = kernel_columns(np.asarray(S[k]), np.asarray(R[k]), variant)
            a, b = [x.astype(dt) for x in a[:p]], b.astype(dt)
            for i in range(p):
                for j in range(i, p):
                    M[i, j] = M[i, j] + a[i] * a[j]
                v[i] = v[i] + a[i] * b
    return {key: x.astype(np.float64) for key, x in M.items()}, [x.astype(np.float64) for x in v]


def lcs_f64(S, R, variant=None):
    """k_lcs restated in numpy float64: its sums, cofactors, first-row determinant, `!(det <= threshold)` and `x0 > 0 &&
    x0 < INFINITY` as the kernel writes them (so NaN and infinity go where the kernel sends them) -> unrounded float64 maps and 'fallback'.
    variant: one of VARIANTS, a wrong kernel."""
    M, (v0, v1, v2) = kernel_sums(S, R, 3, variant)
    m00, m01, m02, m11, m12, m22 = M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]
    with np.errstate(all="ignore"):
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        det = m00 * c00 + m01 * c01 + m02 * c02
        go = ~(det <= 1e-12 * m00 * m11 * m22)
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        inv = 1.0 / det
        x0 = (c00 * v0 + c01 * v1 + c02 * v2) * inv
        ok = go & (x0 > 0.0) & (x0 < np.inf)
        t = np.where(ok, 1.0 / x0, 1.0)
        x = np.where(ok, (c01 * v0 + c11 * v1 + c12 * v2) * inv, 0.0)
        y = np.where(ok, (c02 * v0 + c12 * v1 + c22 * v2) * inv, 0.0)
    return {'transmission': t, 'dx': x, 'dy': y, 'fallback': ~ok}


MAPS = ('transmission', 'dx', 'dy')
EPS32 = 2.0 ** -24                                            # the relative rounding of a float32 output


def map_scales(ref, maps):
    """max|x*| per map; dx and dy share one."""
    s = {k: np.abs(ref[k]).max() for k in maps}
    s['dx'] = s['dy'] = max(s['dx'], s['dy'])
    return s


def yardstick(f64, ref, maps):
    """Y = max over the maps and pixels of |float64 restatement - x*| / scale: what float64 costs on this input."""
    s = map_scales(ref, maps)
    return max(np.abs(f64[k] - ref[k]).max() / s[k] for k in maps)


def clipped(ref, maps, max_shift):
    """The reference maps with dx, dy clamped to +-float32(max_shift), as float64 (None: unchanged)."""
    out = {k: ref[k] for k in maps}
    if max_shift is not None:
        ms = float(np.float32(max_shift))
        out['dx'], out['dy'] = np.clip(ref['dx'], -ms, ms), np.clip(ref['dy'], -ms, ms)
    return out


def parity_bound(ref, Y, maps):
    """Per map and pixel: 2^-24 |x*| (the float32 output's rounding) + 8 * Y * scale (the project's parity margin times what
    float64 costs on the input)."""
    s = map_scales(ref, maps)
    return {k: EPS32 * np.abs(ref[k]) + 8.0 * Y * s[k] for k in maps}


def worst_ratio(got, ref, bound, maps):
    """max over the maps and all pixels of |got - x*| / bound."""
    return max(float((np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]) / bound[k]).max()) for k in maps)


def check_parity(name, got, ref, Y, maps, max_shift=None):
    """Every map and pixel of the GPU's `got` within 2^-24 |x*| + 8 Y scale of the exact reference (dx, dy clamped as the
    kernel clamps them), the fallback pixels exactly (1, 0, ...) and the same set; prints Y and the worst error / bound."""
    want = clipped(ref, maps, max_shift)
    bound = parity_bound(want, Y, maps)
    worst = worst_ratio(got, want, bound, maps)
    print("%s: Y = %.2e, worst error / bound = %.3f" % (name, Y, worst))
    fb = np.ones(ref['fallback'].shape, bool)
    for k in maps:
        assert got[k].dtype == np.float32
        fb &= got[k] == (1.0 if k == 'transmission' else 0.0)
    assert np.array_equal(fb, ref['fallback'])
    assert worst <= 1.0
    if max_shift is not None:
        ms, count = np.float32(max_shift), 0
        for k in ('dx', 'dy'):
            over = np.abs(ref[k]) - float(ms) > bound[k]                   # clamped whatever the rounding
            count += int(over.sum())
            assert np.array_equal(got[k][over], np.where(ref[k][over] > 0, ms, -ms))
            assert np.all(np.abs(got[k]) <= ms)
        assert count > 0.1 * over.size
    return worst


def check_isolation(run, S, R, k, i, j):
    """Changing pixel (i, j) of R_k changes at most that pixel and its four neighbours; all other output bits stay."""
    before = run(S, R)
    R2 = [r.copy() for r in R]
    R2[k][i, j] *= np.float32(1.25)
    after = run(S, R2)
    near = np.zeros(R[0].shape, bool)
    near[max(i - 1, 0):i + 2, j] = True
    near[i, max(j - 1, 0):j + 2] = True
    changed = np.zeros(R[0].shape, bool)
    for key in before:
        changed |= before[key].view(np.uint32) != after[key].view(np.uint32)
    assert changed.any() and not (changed & ~near).any(), np.argwhere(changed & ~near)


# (n, m, K, seed, max_shift): a grid of border pixels only, the 64 x 4 block edges (m = 64 | 65 | 66, n = 3 | 4 | 5 | 9), both
# parities of `#pragma unroll 2`, the smallest K and PSX_MAX_LCS.  Seeds: 1 to 6 in turn, but for the second shape, where
# Y is 5.8e-9 at seed 2, next to the limit 2^-27 = 7.5e-9 of the host tests' condition 8 Y <= 2^-24 (seeds 3 and 5 miss
# it).  max_shift of the clamp case: |D| reaches dmax = 0.5, so 0.2 clamps a good part of the pixels.
LCS_CASES = [(3, 3, 3, 1, None), (5, 65, 3, 6, None), (4, 64, 4, 3, None), (5, 65, 5, 4, None), (9, 66, 8, 5, None),
             (3, 3, 64, 6, None), (5, 65, 5, 4, 0.2)]


def case_inputs(model, n, m, K, seed):
    """float32 S_k, R_k of `model` (an exact_model): S rounded to float32."""
    *_, S, R = model(n, m, K, seed=seed)
    return [s.astype(np.float32) for s in S], R


def steep_model(n, m, K, seed=0, laplacian=None):
    """exact_model (with `laplacian`: tests/_retrieval_df_oracle.exact_model) on log-normal white-noise references
    1e4*exp(1.2 z): neighbouring samples differ by more than a factor of two at most pixels, so the float32 difference
    ru - rd is NOT exact (on the smooth speckle it almost always is) and a kernel that forms it in float64 shows."""
    rng = np.random.default_rng(seed)
    T = 0.6 + 0.2 * (1 + smooth_field(n, m, rng, 1.0))
    Dx, Dy = smooth_field(n, m, rng, 0.5), smooth_field(n, m, rng, 0.5)
    Df = 0.15 * (1 + smooth_field(n, m, rng, 1.0))
    R, S = [], []
    for _ in range(K):
        r = (1e4 * np.exp(1.2 * rng.standard_normal((n, m)))).astype(np.float32)
        g0, g1 = gradients(r)
        S.append(T * (r.astype(np.float64) - Dx * g0 - Dy * g1 + (Df * laplacian(r) if laplacian else 0.0)))
        R.append(r)
    return (T, Dx, Dy, Df, S, R) if laplacian else (T, Dx, Dy, S, R)


def steep_fraction(R):
    """The fraction of horizontal neighbour pairs of the images R_k that differ by more than a factor of two."""
    r = np.stack(R).astype(np.float64)
    a, b = r[:, :, 1:], r[:, :, :-1]
    return float((np.maximum(a / b, b / a) > 2.0).mean())


LCS_STEEP_CASE = (5, 65, 6, 1)                               # (n, m, K, seed) of steep_model, for both kernels


@functools.lru_cache(maxsize=None)
def lcs_parity(n, m, K, seed, steep=False):
    """One case's inputs and CPU references, computed once per process: (S, R, exact, f64, Y)."""
    S, R = case_inputs(steep_model if steep else exact_model, n, m, K, seed)
    ref, f64 = lcs_exact(S, R), lcs_f64(S, R)
    return S, R, ref, f64, yardstick(f64, ref, MAPS)


def nonfinite_inputs(S, R):
    """Copies of S, R (n >= 8, m >= 60, K >= 5) with a NaN, a +inf and a -inf each in one S_k and one R_k, at interior, edge
    and corner pixels; three more +-inf in interior R_k so that every sign pattern of the kernel's sums is likely met."""
    S, R = [s.copy() for s in S], [r.copy() for r in R]
    n, m = S[0].shape
    S[0][4, 20] = np.nan
    S[1][0, 33] = np.inf
    S[2][n - 1, m - 1] = -np.inf
    R[3][5, 40] = np.inf
    R[4][n - 1, 0] = np.nan
    R[0][3, m - 1] = -np.inf
    R[1][2, 7] = np.inf
    R[2][6, 50] = np.inf
    R[4][2, 57] = -np.inf
    return S, R


def integrate_f32(gx, gy, scale=1.0):
    """psx_integrate_f32 restated on the CPU in its number formats: the pack (float)(scale * (double)g) with the mirror
    signs, complex64 transforms (torch's: single precision wherever torch runs), fc_filter's float32 products with
    (float)(k/den) from float64 k, P(0) = 0, the float32 norm 1/(4nm) -> phi [n, m] float32."""
    import torch
    gx, gy = np.asarray(gx, dtype=np.float32), np.asarray(gy, dtype=np.float32)
    n, m = gx.shape
    H, W = 2 * n, 2 * m
    x = (float(scale) * gx.astype(np.float64))
    y = (float(scale) * gy.astype(np.float64))
    X = np.concatenate([x, -x[::-1, :]], 0)
    X = np.concatenate([X, X[:, ::-1]], 1).astype(np.float32)
    Yy = np.concatenate([y, y[::-1, :]], 0)
    Yy = np.concatenate([Yy, -Yy[:, ::-1]], 1).astype(np.float32)
    Z = torch.complex(torch.from_numpy(X), torch.from_numpy(Yy))
    assert Z.dtype == torch.complex64
    Z = torch.fft.fft2(Z).numpy()
    a, b = np.arange(H)[:, None], np.arange(W)[None, :]
    zm = Z[(H - a) % H, (W - b) % W]
    zkx, zky, zmx, zmy = Z.real, Z.imag, zm.real, zm.imag
    half = np.float32(0.5)
    gxr, gxi = half * (zkx + zmx), half * (zky - zmy)
    gyr, gyi = half * (zky + zmy), -half * (zkx - zmx)
    kx = (2 * np.pi / H) * np.where(a < n, a, a - H).astype(np.float64)
    ky = (2 * np.pi / W) * np.where(b < m, b, b - W).astype(np.float64)
    den = kx * kx + ky * ky
    den[0, 0] = 1.0
    fx, fy = (kx / den).astype(np.float32), (ky / den).astype(np.float32)
    sr, si = fx * gxr + fy * gyr, fx * gxi + fy * gyi
    assert sr.dtype == np.float32 and si.dtype == np.float32
    P = (si + 1j * (-sr)).astype(np.complex64)
    P[0, 0] = 0
    out = torch.fft.ifft2(torch.from_numpy(P), norm="forward").numpy()
    assert out.dtype == np.complex64
    return (out.real[:n, :m] * np.float32(1.0 / (4.0 * n * m))).astype(np.float32)


INTEGRATE_SHAPES = [(2, 2), (2, 3), (3, 2), (5, 4), (17, 16), (64, 48), (33, 130), (130, 33)]


def integrate_inputs(n, m):
    """[(name, gx, gy)] float32 for one shape: white noise (independent gx, gy: not integrable), and a single non-zero pixel
    of gx, and separately of gy, at a corner and at (n//2, m//2) -- a wrong mirror sign moves its response at order one."""
    rng = np.random.default_rng(1000 * n + m)
    out = [("noise", rng.standard_normal((n, m)).astype(np.float32), rng.standard_normal((n, m)).astype(np.float32))]
    for where, (i, j) in (("corner", (n - 1, 0)), ("inside", (n // 2, m // 2))):
        for axis in (0, 1):
            g = [np.zeros((n, m), np.float32), np.zeros((n, m), np.float32)]
            g[axis][i, j] = 1.0
            out.append(("impulse g%s %s" % ("xy"[axis], where), g[0], g[1]))
    return out


def integrate_yardstick(gx, gy, scale=1.0):
    """(ref, yardstick, peak): the float64 contract on the pack's own float32 input float32(scale*g) (product in float64),
    max|integrate_f32 - ref|, max|ref|."""
    sx = (float(scale) * np.asarray(gx, dtype=np.float64)).astype(np.float32)
    sy = (float(scale) * np.asarray(gy, dtype=np.float64)).astype(np.float32)
    ref = integrate(sx, sy)
    return ref, float(np.abs(integrate_f32(gx, gy, scale).astype(np.float64) - ref).max()), float(np.abs(ref).max())
