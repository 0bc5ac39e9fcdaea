"""Float64 numpy oracle of the UMPA contract (include/paresis_hip.h: psx_umpa_f32; csrc/umpa.hip).

umpa():         the maps, the fallback mask, gap = (second-smallest - smallest valid cost)/E and u* = (a, b) per pixel.
umpa_brute():   the same contract as plain loops over pixels, candidates and window pixels (tiny images only).
warped_model(): sample images warped by smooth displacement fields of several pixels.
compare():      the comparison rule of the GPU tests (border band exact, fallback masks equal, near-ties excluded).

On images of small integers every sum E, B, C is an exact integer in float64 in any order, and what follows is a fixed
sequence of single IEEE operations, so a correct kernel gives umpa()'s four maps bit for bit:
integer_model(): such images, with a block without reference, a block of negative sample, or an exactly periodic reference.
classes():       which pixels of an instance are all-skipped, partly skipped, fallback through T <= 0, ordinary.
compare_exact(): np.array_equal on the four whole maps, no exclusion.
"""
import numpy as np

from tests import _retrieval_oracle as orl

GAP_MIN = 1e-10     # interior pixels whose two best costs are closer than this (relative to E) are ties: unspecified


def _box(A, w):
    """Sums over the (2w+1)^2 windows that lie inside A: [n, m] -> [n-2w, m-2w], by shifted slices (no running sums)."""
    n, m = A.shape[-2:]
    H = sum(A[..., :, d:m - 2 * w + d] for d in range(2 * w + 1))
    return sum(H[..., d:n - 2 * w + d, :] for d in range(2 * w + 1))


def cost_volume(S, R, window, search):
    """E [ni, mi], B, C [(2s+1)^2, ni, mi] on the interior (pixels at least w+s from every border), candidates in scan order
    (a outer, b inner, ascending)."""
    w, s = int(window), int(search)
    S = np.stack([np.asarray(x) for x in S]).astype(np.float64)
    R = np.stack([np.asarray(x) for x in R]).astype(np.float64)
    K, n, m = S.shape
    assert n >= 2 * (w + s) + 1 and m >= 2 * (w + s) + 1
    E = _box((S[:, s:n - s, s:m - s] ** 2).sum(0), w)
    boxC = _box((R ** 2).sum(0), w)                                  # centred on pixels [w, n-w) x [w, m-w)
    ni, mi = n - 2 * (w + s), m - 2 * (w + s)
    B, C = [], []
    for a in range(-s, s + 1):
        for b in range(-s, s + 1):
            prod = (S[:, s:n - s, s:m - s] * R[:, s - a:n - s - a, s - b:m - s - b]).sum(0)
            B.append(_box(prod, w))
            C.append(boxC[s - a:s - a + ni, s - b:s - b + mi])       # box_w[sum R^2](r - u), r = (w+s+i, w+s+j)
    return E, np.stack(B), np.stack(C)


def umpa(S, R, window=2, search=3):
    """{'transmission', 'dx', 'dy', 'residual'} float32 n x m, 'fallback' (bool, False in the border band), 'gap' (float64,
    inf in the border band and where fewer than two candidates are valid), 'interior' (bool)."""
    w, s = int(window), int(search)
    n, m = np.asarray(S[0]).shape
    E, B, C = cost_volume(S, R, w, s)
    nc = 2 * s + 1
    skipped = C == 0
    Cs = np.where(skipped, 1.0, C)
    L = np.where(skipped, np.inf, E[None] - B * B / Cs)
    T = B / Cs
    idx = np.argmin(L, axis=0)                                       # the first minimum in scan order
    L0 = np.take_along_axis(L, idx[None], 0)[0]
    T0 = np.take_along_axis(T, idx[None], 0)[0]
    none = ~np.isfinite(L0)
    fb = none | ~(T0 > 0)
    a0, b0 = idx // nc - s, idx % nc - s

    def refine(step, pos):
        ok = np.abs(pos) < s
        im = np.clip(idx - step, 0, nc * nc - 1)
        ip = np.clip(idx + step, 0, nc * nc - 1)
        Lm = np.take_along_axis(L, im[None], 0)[0]
        Lp = np.take_along_axis(L, ip[None], 0)[0]
        ok &= np.isfinite(Lm) & np.isfinite(Lp)
        with np.errstate(invalid='ignore', divide='ignore'):
            den = Lm - 2 * L0 + Lp
            ok &= den > 0
            d = np.clip(0.5 * (Lm - Lp) / np.where(ok, den, 1.0), -0.5, 0.5)
        return np.where(ok, d, 0.0)

    with np.errstate(invalid='ignore', divide='ignore'):
        da, db = refine(nc, a0), refine(1, b0)
        res = np.maximum(L0, 0) / E
        two = np.partition(L, 1, axis=0)[:2] if L.shape[0] > 1 else np.stack([L[0], np.full_like(L[0], np.inf)])
        gap = (two[1] - two[0]) / E
    gap = np.where(np.isfinite(two[1]) & np.isfinite(two[0]), gap, np.inf)
    out = {}
    band = w + s
    inner = (slice(band, n - band), slice(band, m - band))
    for key, val, fill in (('transmission', np.where(fb, 1.0, T0), 1.0), ('dx', np.where(fb, 0.0, a0 + da), 0.0),
                           ('dy', np.where(fb, 0.0, b0 + db), 0.0), ('residual', np.where(fb, 0.0, res), 0.0)):
        full = np.full((n, m), fill, np.float32)
        full[inner] = val.astype(np.float32)
        out[key] = full
    out['fallback'] = np.zeros((n, m), bool)
    out['fallback'][inner] = fb
    out['gap'] = np.full((n, m), np.inf)
    out['gap'][inner] = gap
    out['interior'] = np.zeros((n, m), bool)
    out['interior'][inner] = True
    for key, val in (('a', a0), ('b', b0)):                          # u*, 0 in the border band; meaningless where all skipped
        out[key] = np.zeros((n, m), np.int64)
        out[key][inner] = val
    return out


def umpa_brute(S, R, window, search):
    """The contract read literally: loops over pixels, candidates and the window.  -> (transmission, dx, dy, residual) float64."""
    w, s = int(window), int(search)
    S = [np.asarray(x).astype(np.float64) for x in S]
    R = [np.asarray(x).astype(np.float64) for x in R]
    n, m = S[0].shape
    t, dx, dy, res = np.ones((n, m)), np.zeros((n, m)), np.zeros((n, m)), np.zeros((n, m))
    for i in range(w + s, n - w - s):
        for j in range(w + s, m - w - s):
            win = lambda A, a, b: A[i - w - a:i + w + 1 - a, j - w - b:j + w + 1 - b]
            E = sum((win(x, 0, 0) ** 2).sum() for x in S)
            L, T = {}, {}
            for a in range(-s, s + 1):
                for b in range(-s, s + 1):
                    Bv = sum((win(x, 0, 0) * win(r, a, b)).sum() for x, r in zip(S, R))
                    Cv = sum((win(r, a, b) ** 2).sum() for r in R)
                    if Cv != 0:
                        L[a, b], T[a, b] = E - Bv * Bv / Cv, Bv / Cv
            best = None
            for u in sorted(L):                                      # (a, b) ascending, a outer
                if best is None or L[u] < L[best]:
                    best = u
            if best is None or not T[best] > 0:
                continue
            d = [0.0, 0.0]
            for ax in (0, 1):
                um = (best[0] - (ax == 0), best[1] - (ax == 1))
                up = (best[0] + (ax == 0), best[1] + (ax == 1))
                if abs(best[ax]) < s and um in L and up in L:
                    den = L[um] - 2 * L[best] + L[up]
                    if den > 0:
                        d[ax] = min(max(0.5 * (L[um] - L[up]) / den, -0.5), 0.5)
            t[i, j], dx[i, j], dy[i, j], res[i, j] = T[best], best[0] + d[0], best[1] + d[1], max(L[best], 0) / E
    return t, dx, dy, res


def warped_model(n, m, K, seed, dmax, grain=3.0):
    """T, Dx, Dy (float64) and K float32 pairs S_k(r) = T(r) * R_k(r - D(r)) (cubic-spline interpolation)."""
    import scipy.ndimage
    rng = np.random.default_rng(seed)
    T = 0.6 + 0.4 * 0.5 * (1 + orl.smooth_field(n, m, rng, 1.0))
    Dx = orl.smooth_field(n, m, rng, dmax)
    Dy = orl.smooth_field(n, m, rng, dmax)
    ii, jj = np.indices((n, m)).astype(np.float64)
    S, R = [], []
    for _ in range(K):
        r = orl.speckle(n, m, rng, grain=grain).astype(np.float32)
        S.append((T * scipy.ndimage.map_coordinates(r.astype(np.float64), [ii - Dx, jj - Dy], order=3,
                                                    mode='nearest')).astype(np.float32))
        R.append(r)
    return T, Dx, Dy, S, R


def compare(got, o, window, search, cap=1e-4, label=""):
    """The parity rule: `got` = {'transmission', 'dx', 'dy', 'residual'} numpy maps against the oracle's dict `o`.
    Border band bit-exact; fallback masks equal; interior pixels with gap < GAP_MIN excluded, their share <= cap (None: no
    cap); on the rest |ddx|, |ddy| <= 1e-5 px, relative dT <= 1e-5, |dresidual| <= 1e-7 + 1e-5*residual.  Prints the figures
    first; returns them."""
    inner = o['interior']
    for key, v in (('transmission', 1.0), ('dx', 0.0), ('dy', 0.0), ('residual', 0.0)):
        assert got[key].dtype == np.float32 and got[key].shape == inner.shape, key
        assert np.array_equal(got[key][~inner], np.full((~inner).sum(), v, np.float32)), "border band of " + key
    tie = inner & (o['gap'] < GAP_MIN)
    share = tie.sum() / max(inner.sum(), 1)
    ok = inner & ~tie
    gfb = (got['transmission'] == 1) & (got['dx'] == 0) & (got['dy'] == 0) & (got['residual'] == 0)
    ofb = o['fallback']
    live = ok & ~ofb
    f = {'ties': int(tie.sum()), 'share': float(share), 'fallback': int(ofb[ok].sum()), 'compared': int(live.sum())}
    if live.any():
        f['ddx'] = float(np.abs(got['dx'].astype(np.float64) - o['dx'])[live].max())
        f['ddy'] = float(np.abs(got['dy'].astype(np.float64) - o['dy'])[live].max())
        f['dT'] = float((np.abs(got['transmission'].astype(np.float64) - o['transmission']) / np.abs(o['transmission']))[live].max())
        f['dres'] = float((np.abs(got['residual'].astype(np.float64) - o['residual']) - 1e-5 * o['residual'])[live].max())
    print("umpa %s w=%d s=%d: %s" % (label, window, search, f))
    assert cap is None or share <= cap, f
    assert np.array_equal(gfb[ok & ofb], np.ones((ok & ofb).sum(), bool)), "oracle fallback pixels"
    assert not (gfb & live).any(), "fallback where the oracle has none"
    if live.any():
        assert f['ddx'] <= 1e-5 and f['ddy'] <= 1e-5 and f['dT'] <= 1e-5 and f['dres'] <= 1e-7, f
    return f


# ------------------------------------------------------------------------------------------------ exact comparison
KEYS = ('transmission', 'dx', 'dy', 'residual')
TILE_H = 16                                                          # the kernel's output tile: 16 x tile_width(w)


def tile_width(w):
    return 32 if w <= 4 else 16


def integer_shape(w, s):
    """The smallest convenient image whose interior has pixels in two tile rows and two tile columns at every (w, s), both
    last tiles ragged (n and m are odd), with room for the two planted blocks of side 2(w+s)+3 in opposite corners."""
    return 4 * (w + s) + 13, 4 * (w + s) + tile_width(w) + 5


def integer_model(w, s, K, seed, period=None, shape=None, vmax=4095, block=4):
    """S, R: K float32 image pairs holding integers only.  R_k is random in [0, vmax], or with period = (p, q) an exact
    tiling of a random p x q cell with entries in [1, vmax]; S_k(r) = 2 R_k(r - D(r)) + noise, D an integer field that is
    constant on block x block pixels with |a|, |b| <= s (indices wrap), noise integer in [0, 7].  |S| <= 2 vmax + 7, so every
    window sum is below K (2w+1)^2 (2 vmax + 7)^2 = 1.3e12 at K = 64, w = 8, vmax = 4095: 2^53 = 9.0e15 is far.
    With neither period nor shape (the image is then integer_shape(w, s)) two blocks of side 2(w+s)+3 are planted: R_k = 0
    in the first corner (before S is formed), so that 3 x 3 interior pixels have every candidate skipped and those around
    them some; S_k negated in the last corner, so that T(u) < 0 at every candidate of the pixels well inside.  D = 0 on the
    rows [Z-2w, Z] over the zero block, Z its side: the pixels of row Z-w then match at u = (0, 0) through the one row of
    their window that lies outside the block, while their candidate (1, 0) lies inside it and is skipped."""
    rng = np.random.default_rng(seed)
    planted = period is None and shape is None
    n, m = shape if shape is not None else integer_shape(w, s)
    Z = 2 * (w + s) + 3
    tiles = (-(-n // block), -(-m // block))
    A = np.kron(rng.integers(-s, s + 1, tiles), np.ones((block, block), np.int64))[:n, :m]
    Bf = np.kron(rng.integers(-s, s + 1, tiles), np.ones((block, block), np.int64))[:n, :m]
    if planted:                                                      # see below: D = 0 on the rows across the block's last edge
        A[Z - 2 * w:Z + 1, :Z] = 0
        Bf[Z - 2 * w:Z + 1, :Z] = 0
    ii, jj = np.indices((n, m))
    si, sj = (ii - A) % n, (jj - Bf) % m
    S, R = [], []
    for _ in range(K):
        if period is None:
            r = rng.integers(0, vmax + 1, (n, m))
        else:
            cell = rng.integers(1, vmax + 1, period)
            r = np.tile(cell, (n // period[0] + 1, m // period[1] + 1))[:n, :m]
        if planted:
            r[:Z, :Z] = 0
        x = 2 * r[si, sj] + rng.integers(0, 8, (n, m))
        if planted:
            x[n - Z:, m - Z:] *= -1
        S.append(x.astype(np.float32))
        R.append(r.astype(np.float32))
    assert all(np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 2 * vmax + 7 for x in S + R)
    return S, R


def classes(S, R, window, search):
    """Boolean n x m masks from the oracle's own cost volume (False in the border band): 'all_skipped'; 'some_skipped';
    'lacks_neighbour' (some skipped, not a fallback pixel, and u* has |a*| < s with L(a*-1, b*) or L(a*+1, b*) skipped, or
    the same along b); 'nonpositive' (a valid u* with T(u*) <= 0); 'ordinary' (no candidate skipped, T(u*) > 0).  And the
    integer maps 'tile_row', 'tile_col' of the kernel's 16 x tile_width(w) output tiles."""
    w, s = int(window), int(search)
    n, m = np.asarray(S[0]).shape
    E, B, C = cost_volume(S, R, w, s)
    nc = 2 * s + 1
    skipped = C == 0
    Cs = np.where(skipped, 1.0, C)
    L = np.where(skipped, np.inf, E[None] - B * B / Cs)
    idx = np.argmin(L, axis=0)
    T0 = np.take_along_axis(B / Cs, idx[None], 0)[0]
    allsk = skipped.all(0)
    a0, b0 = idx // nc - s, idx % nc - s
    at = lambda k: np.take_along_axis(skipped, np.clip(k, 0, nc * nc - 1)[None], 0)[0]
    lacks = ((np.abs(a0) < s) & (at(idx - nc) | at(idx + nc))) | ((np.abs(b0) < s) & (at(idx - 1) | at(idx + 1)))
    vals = {'all_skipped': allsk, 'some_skipped': skipped.any(0) & ~allsk,
            'lacks_neighbour': skipped.any(0) & ~allsk & (T0 > 0) & lacks, 'nonpositive': ~allsk & ~(T0 > 0),
            'ordinary': ~skipped.any(0) & (T0 > 0)}
    band = w + s
    out = {}
    for key, val in vals.items():
        out[key] = np.zeros((n, m), bool)
        out[key][band:n - band, band:m - band] = val
    ii, jj = np.indices((n, m))
    out['tile_row'], out['tile_col'] = ii // TILE_H, jj // tile_width(w)
    return out


def compare_exact(got, o, ties=False, label=""):
    """np.array_equal of `got`'s four maps with the oracle's over the whole image: no exclusion, no cap, no tolerance.
    Valid only where the inputs make the contract's float64 sums exact (integer_model).  An interior pixel whose two best
    costs are equal (gap == 0) is an error of the test's inputs unless ties=True: then the first minimum is what is asked.
    Prints and returns the counts; on a difference prints the first differing pixel of the first differing map."""
    inner = o['interior']
    tie = inner & (o['gap'] == 0)
    f = {'pixels': int(inner.size), 'interior': int(inner.sum()), 'ties': int(tie.sum())}
    print("umpa exact %s: %s" % (label, f))
    assert ties or not tie.any(), "exact ties in inputs that were to have none: %s" % f
    for key in KEYS:
        assert np.isfinite(o[key]).all(), "the oracle's %s is not finite" % key
        assert got[key].dtype == np.float32 and got[key].shape == inner.shape, key
        if not np.array_equal(got[key], o[key]):
            i, j = (int(x[0]) for x in np.nonzero(got[key] != o[key]))
            text = ("umpa exact %s: %s differs at %d pixels, first (%d, %d): got %r, oracle %r, u* = (%d, %d), fallback %s, "
                    "gap %.3g; there got %s, oracle %s"
                    % (label, key, int((got[key] != o[key]).sum()), i, j, got[key][i, j], o[key][i, j], o['a'][i, j],
                       o['b'][i, j], o['fallback'][i, j], o['gap'][i, j], [float(got[k][i, j]) for k in KEYS],
                       [float(o[k][i, j]) for k in KEYS]))
            print(text)
            raise AssertionError(text)
    return f


# The instances that tests/test_gpu_umpa.py runs and tests/test_umpa_host.py qualifies: every (w, s), K cycling through 1..4
# (both parities of the kernel's double buffer), and periodic references at both tile widths and every chunk count.
PAIRS = [(w, s) for w in range(1, 9) for s in range(1, 9)]
TIE_CASES = [(2, 3, (2, 3)), (1, 8, (3, 2)), (8, 5, (4, 5)), (5, 7, (2, 2)), (6, 2, (2, 3)), (3, 4, (3, 3))]    # w, s, period


def sweep_K(w, s):
    return 1 + (w + s) % 4


def sweep_instance(w, s, rep=0):
    return integer_model(w, s, sweep_K(w, s), seed=2000 + 100 * w + s + 10000 * rep)


def tie_instance(w, s, period):
    return integer_model(w, s, 2 + (w + s) % 2, seed=3000 + 100 * w + s, period=period)


def warped_instance(w, s, rep=0):
    """The float images of the warped sweep: displacements up to about s - 1/2 on (2(w+s)+21) x (2(w+s)+TW+9) pixels."""
    q = w + s
    return warped_model(2 * q + 21, 2 * q + tile_width(w) + 9, sweep_K(w, s), seed=1000 + 10 * w + s + 10000 * rep,
                        dmax=max(0.5, s - 0.5))[3:]
