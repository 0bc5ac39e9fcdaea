"""Float64 numpy oracle of the UMPA dark-field contract (include/paresis_hip.h: psx_umpa_df_f32; csrc/umpa.hip), built on
tests/_umpa_oracle.py.

umpa_df():          the five maps, the fallback mask, gap, interior and u* per pixel, as _umpa_oracle.umpa() plus 'visibility'.
umpa_df_brute():    the same contract as plain loops over pixels, candidates and window pixels (tiny images only).
integer_df_model(): images of small integers S_k = a R_k(q - D) + b mu_k + noise with planted blocks.  Every sum E, B, C, F,
                    G, H is then an exact integer in float64 in any order, and what follows is a fixed sequence of single IEEE
                    operations, so a correct kernel gives umpa_df()'s five maps bit for bit.
classes_df():       which pixels of an instance are ordinary, skipped through C == 0, skipped through a flat reference, T <= 0.
compare_df():       _umpa_oracle.compare()'s rule on T, dx, dy, residual plus |dV| <= 1e-5.
compare_exact_df(): np.array_equal on the five whole maps.
"""
import numpy as np

from tests import _umpa_oracle as ou

KEYS = ('transmission', 'dx', 'dy', 'visibility', 'residual')
FILL = dict(zip(KEYS, (1.0, 0.0, 0.0, 1.0, 0.0)))
PAIRS_AB = ((2, 0), (1, 3), (3, 1), (1, 1), (3, -1))                 # (a, b) of S = a R + b mu: T = a + b, V = a/T
REL_DET = 1e-12


def big_h(mean, window):
    """H = (2w+1)^2 sum_k mu_k^2, the squares summed in the order of k."""
    sq = 0.0
    for v in np.asarray(mean, np.float64):
        sq += float(v) * float(v)
    side = float(2 * int(window) + 1)
    return side * side * sq


def cost_volume_df(S, R, mean, window, search):
    """E, F [ni, mi], B, C, G [(2s+1)^2, ni, mi] on the interior, candidates in scan order, and the scalar H."""
    w, s = int(window), int(search)
    E, B, C = ou.cost_volume(S, R, w, s)
    S = np.stack([np.asarray(x) for x in S]).astype(np.float64)
    R = np.stack([np.asarray(x) for x in R]).astype(np.float64)
    mu = np.asarray(mean, np.float64)
    assert mu.shape == (S.shape[0],)
    K, n, m = S.shape
    F = ou._box((mu[:, None, None] * S[:, s:n - s, s:m - s]).sum(0), w)
    boxG = ou._box((mu[:, None, None] * R).sum(0), w)
    ni, mi = n - 2 * (w + s), m - 2 * (w + s)
    G = [boxG[s - a:s - a + ni, s - b:s - b + mi] for a in range(-s, s + 1) for b in range(-s, s + 1)]
    return E, F, B, C, np.stack(G), big_h(mu, w)


def solve(E, F, B, C, G, H):
    """The contract's sequence, one rounded operation each (numpy contracts nothing): -> ok, alpha, beta, L (inf where
    skipped), T."""
    p = C * H
    q = G * G
    det = p - q
    ok = det > REL_DET * p
    d = np.where(ok, det, 1.0)
    bh, fg, cf, gb = B * H, F * G, C * F, G * B
    al = (bh - fg) / d
    be = (cf - gb) / d
    ab, bf = al * B, be * F
    L = np.where(ok, E - (ab + bf), np.inf)
    return ok, al, be, L, al + be


def finish(L, T, A, E, shape, window, search):
    """From the cost volume L (inf where skipped), T and alpha per candidate: the first minimum, the parabola, the fallback
    rule and the maps, as _umpa_oracle.umpa()."""
    w, s = int(window), int(search)
    n, m = shape
    nc = 2 * s + 1
    idx = np.argmin(L, axis=0)                                       # the first minimum in scan order
    take = lambda X, i: np.take_along_axis(X, i[None], 0)[0]
    L0, T0, A0 = take(L, idx), take(T, idx), take(A, idx)
    fb = ~np.isfinite(L0) | ~(T0 > 0)
    a0, b0 = idx // nc - s, idx % nc - s

    def refine(step, pos):
        ok = np.abs(pos) < s
        Lm = take(L, np.clip(idx - step, 0, nc * nc - 1))
        Lp = take(L, np.clip(idx + step, 0, nc * nc - 1))
        ok &= np.isfinite(Lm) & np.isfinite(Lp)
        with np.errstate(invalid='ignore', divide='ignore'):
            den = Lm - 2 * L0 + Lp
            ok &= den > 0
            d = np.clip(0.5 * (Lm - Lp) / np.where(ok, den, 1.0), -0.5, 0.5)
        return np.where(ok, d, 0.0)

    with np.errstate(invalid='ignore', divide='ignore'):
        da, db = refine(nc, a0), refine(1, b0)
        res = np.maximum(L0, 0) / E
        V = A0 / np.where(fb, 1.0, T0)
        two = np.partition(L, 1, axis=0)[:2]
        gap = (two[1] - two[0]) / E
    gap = np.where(np.isfinite(two[1]) & np.isfinite(two[0]), gap, np.inf)
    band = w + s
    inner = (slice(band, n - band), slice(band, m - band))
    vals = {'transmission': T0, 'dx': a0 + da, 'dy': b0 + db, 'visibility': V, 'residual': res}
    out = {}
    for key in KEYS:
        full = np.full((n, m), FILL[key], np.float32)
        full[inner] = np.where(fb, FILL[key], vals[key]).astype(np.float32)
        out[key] = full
    for key, val, fill, dt in (('fallback', fb, False, bool), ('gap', gap, np.inf, np.float64), ('interior', True, False, bool),
                               ('a', a0, 0, np.int64), ('b', b0, 0, np.int64)):
        out[key] = np.full((n, m), fill, dt)
        out[key][inner] = val
    return out


def umpa_df(S, R, mean, window=2, search=3, vol=None):
    """{'transmission', 'dx', 'dy', 'visibility', 'residual'} float32 n x m, and 'fallback', 'gap', 'interior', 'a', 'b' as
    _umpa_oracle.umpa().  vol: cost_volume_df()'s result for these arguments, if the caller has it."""
    E, F, B, C, G, H = vol if vol is not None else cost_volume_df(S, R, mean, window, search)
    ok, al, be, L, T = solve(E[None], F[None], B, C, G, H)
    return finish(L, T, al, E, np.asarray(S[0]).shape, window, search)


def umpa_df_brute(S, R, mean, window, search):
    """The contract read literally.  -> (transmission, dx, dy, visibility, residual) float64."""
    w, s = int(window), int(search)
    S = [np.asarray(x).astype(np.float64) for x in S]
    R = [np.asarray(x).astype(np.float64) for x in R]
    mu = [float(v) for v in mean]
    n, m = S[0].shape
    H = float(2 * w + 1) ** 2 * sum(v * v for v in mu)
    t, dx, dy, vis, res = np.ones((n, m)), np.zeros((n, m)), np.zeros((n, m)), np.ones((n, m)), np.zeros((n, m))
    for i in range(w + s, n - w - s):
        for j in range(w + s, m - w - s):
            win = lambda A, a, b: A[i - w - a:i + w + 1 - a, j - w - b:j + w + 1 - b]
            E = sum((win(x, 0, 0) ** 2).sum() for x in S)
            F = sum(v * win(x, 0, 0).sum() for v, x in zip(mu, S))
            L, T, A = {}, {}, {}
            for a in range(-s, s + 1):
                for b in range(-s, s + 1):
                    Bv = sum((win(x, 0, 0) * win(r, a, b)).sum() for x, r in zip(S, R))
                    Cv = sum((win(r, a, b) ** 2).sum() for r in R)
                    Gv = sum(v * win(r, a, b).sum() for v, r in zip(mu, R))
                    p = Cv * H
                    q = Gv * Gv
                    det = p - q
                    if det > REL_DET * p:
                        bh, fg, cf, gb = Bv * H, F * Gv, Cv * F, Gv * Bv
                        al = (bh - fg) / det
                        be = (cf - gb) / det
                        ab, bf = al * Bv, be * F
                        L[a, b], T[a, b], A[a, b] = E - (ab + bf), al + be, al
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
            t[i, j], dx[i, j], dy[i, j] = T[best], best[0] + d[0], best[1] + d[1]
            vis[i, j], res[i, j] = A[best] / T[best], max(L[best], 0) / E
    return t, dx, dy, vis, res


def integer_df_model(w, s, K, seed, period=None, shape=None, vmax=4095, block=4, near_flat=False):
    """S, R (K float32 image pairs holding integers only) and mu (K integers in [1, vmax], float64).  R_k is random in
    [0, vmax], or with period = (p, q) an exact tiling of a random p x q cell with entries in [1, vmax];
    S_k(r) = a R_k(r - D(r)) + b mu_k + noise, D an integer field and (a, b) a pair of PAIRS_AB, both constant on
    block x block pixels (|D| <= s per axis, indices wrap), noise integer in [0, 7].  |S| <= 4 vmax + 7, so every window sum
    is below K (2w+1)^2 (4 vmax + 7)^2 = 5.0e12 at K = 64, w = 8: 2^53 = 9.0e15 is far.
    With neither period nor shape the image is _umpa_oracle.integer_shape(w, s) and blocks of side Z = 2(w+s)+3 are planted:
    R_k = 0 in the first corner (before S is formed): 3 x 3 interior pixels have C == 0 at every candidate; R_k = mu_k in the
    corner of the first rows and last columns: there C != 0 and C H == G G exactly, det == 0, 3 x 3 pixels have every
    candidate skipped; S_k negated in the last corner: T(u) < 0.  D = 0 on the rows [Z-2w, Z] over the zero block, as
    _umpa_oracle.integer_model.
    near_flat (K >= 2): mu_k = vmax - k, and R_k = mu_k - 1 in the corner of the last rows and first columns.  That window
    is almost, not exactly, proportional to mu: 0 < det/p = sum_{j<k}(mu_j - mu_k)^2/(sum mu^2)^2 < 5e-15, below the 1e-12 of
    the skip rule, while det itself (N^2 sum_{j<k}(mu_j - mu_k)^2, N = (2w+1)^2) is several units in the last place of p:
    only the relative test skips these candidates."""
    rng = np.random.default_rng(seed)
    planted = period is None and shape is None
    n, m = shape if shape is not None else ou.integer_shape(w, s)
    Z = 2 * (w + s) + 3
    tiles = (-(-n // block), -(-m // block))
    grow = lambda t: np.kron(t, np.ones((block, block), np.int64))[:n, :m]
    A, Bf = grow(rng.integers(-s, s + 1, tiles)), grow(rng.integers(-s, s + 1, tiles))
    pair = grow(rng.integers(0, len(PAIRS_AB), tiles))
    ca, cb = np.array(PAIRS_AB)[pair, 0], np.array(PAIRS_AB)[pair, 1]
    if planted:
        A[Z - 2 * w:Z + 1, :Z] = 0
        Bf[Z - 2 * w:Z + 1, :Z] = 0
    mu = vmax - np.arange(K) if near_flat else rng.integers(1, vmax + 1, K)
    assert not near_flat or (planted and K >= 2)
    ii, jj = np.indices((n, m))
    si, sj = (ii - A) % n, (jj - Bf) % m
    S, R = [], []
    for k in range(K):
        if period is None:
            r = rng.integers(0, vmax + 1, (n, m))
        else:
            cell = rng.integers(1, vmax + 1, period)
            r = np.tile(cell, (n // period[0] + 1, m // period[1] + 1))[:n, :m]
        if planted:
            r[:Z, :Z] = 0
            r[:Z, m - Z:] = mu[k]
            if near_flat:
                r[n - Z:, :Z] = mu[k] - 1
        x = ca * r[si, sj] + cb * mu[k] + rng.integers(0, 8, (n, m))
        if planted:
            x[n - Z:, m - Z:] *= -1
        S.append(x.astype(np.float32))
        R.append(r.astype(np.float32))
    assert all(np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 4 * vmax + 7 for x in S + R)
    return S, R, mu.astype(np.float64)


def classes_df(S, R, mean, window, search, vol=None):
    """Boolean n x m masks from the oracle's own cost volume (False in the border band): 'zero_skipped' (every candidate has
    C == 0), 'flat_skipped' (every candidate is skipped and has C != 0), 'some_skipped', 'nonpositive' (a valid u* with
    T(u*) <= 0), 'ordinary' (no candidate skipped, T(u*) > 0), and the maps 'tile_row', 'tile_col' of the kernel's tiles."""
    w, s = int(window), int(search)
    n, m = np.asarray(S[0]).shape
    E, F, B, C, G, H = vol if vol is not None else cost_volume_df(S, R, mean, w, s)
    ok, al, be, L, T = solve(E[None], F[None], B, C, G, H)
    idx = np.argmin(L, axis=0)
    T0 = np.take_along_axis(T, idx[None], 0)[0]
    allsk = (~ok).all(0)
    vals = {'zero_skipped': (C == 0).all(0), 'flat_skipped': allsk & (C != 0).all(0), 'some_skipped': (~ok).any(0) & ~allsk,
            'nonpositive': ~allsk & ~(T0 > 0), 'ordinary': ok.all(0) & (T0 > 0), 'all_skipped': allsk}
    band = w + s
    out = {}
    for key, val in vals.items():
        out[key] = np.zeros((n, m), bool)
        out[key][band:n - band, band:m - band] = val
    ii, jj = np.indices((n, m))
    out['tile_row'], out['tile_col'] = ii // ou.TILE_H, jj // ou.tile_width(w)
    return out


def compare_df(got, o, window, search, cap=1e-4, label=""):
    """_umpa_oracle.compare() on transmission, dx, dy and residual, then the visibility: exactly 1 in the border band and at
    the oracle's fallback pixels, |dV| <= 1e-5 on the pixels compare() compares.  Prints the figures first; returns them."""
    f = ou.compare({k: got[k] for k in ou.KEYS}, o, window, search, cap=cap, label=label)
    inner = o['interior']
    v = got['visibility']
    assert v.dtype == np.float32 and v.shape == inner.shape
    assert np.array_equal(v[~inner], np.ones((~inner).sum(), np.float32)), "border band of visibility"
    ok = inner & ~(o['gap'] < ou.GAP_MIN)
    assert np.array_equal(v[ok & o['fallback']], np.ones((ok & o['fallback']).sum(), np.float32)), "visibility at fallback pixels"
    live = ok & ~o['fallback']
    f['dV'] = float(np.abs(v.astype(np.float64) - o['visibility'])[live].max()) if live.any() else 0.0
    print("umpa-df %s w=%d s=%d: dV %.3g" % (label, window, search, f['dV']))
    assert f['dV'] <= 1e-5, f
    return f


def compare_exact_df(got, o, ties=False, label=""):
    """np.array_equal of `got`'s five maps with the oracle's over the whole image, as _umpa_oracle.compare_exact()."""
    inner = o['interior']
    tie = inner & (o['gap'] == 0)
    f = {'pixels': int(inner.size), 'interior': int(inner.sum()), 'ties': int(tie.sum())}
    print("umpa-df exact %s: %s" % (label, f))
    assert ties or not tie.any(), "exact ties in inputs that were to have none: %s" % f
    for key in KEYS:
        assert np.isfinite(o[key]).all(), "the oracle's %s is not finite" % key
        assert got[key].dtype == np.float32 and got[key].shape == inner.shape, key
        if not np.array_equal(got[key], o[key]):
            i, j = (int(x[0]) for x in np.nonzero(got[key] != o[key]))
            text = ("umpa-df exact %s: %s differs at %d pixels, first (%d, %d): u* = (%d, %d), fallback %s, gap %.3g; there got "
                    "%s, oracle %s" % (label, key, int((got[key] != o[key]).sum()), i, j, o['a'][i, j], o['b'][i, j],
                                       o['fallback'][i, j], o['gap'][i, j], [float(got[k][i, j]) for k in KEYS],
                                       [float(o[k][i, j]) for k in KEYS]))
            print(text)
            raise AssertionError(text)
    return f


# The instances that tests/test_gpu_umpa_df.py runs and tests/test_umpa_df_host.py qualifies.
NEAR_FLAT_CASES = [(1, 1, 2), (2, 3, 2), (4, 5, 3), (6, 2, 4), (8, 8, 3)]       # w, s, K


def sweep_instance(w, s, rep=0):
    return integer_df_model(w, s, ou.sweep_K(w, s), seed=6000 + 100 * w + s + 10000 * rep)


def tie_instance(w, s, period):
    return integer_df_model(w, s, 2 + (w + s) % 2, seed=7000 + 100 * w + s, period=period)


def near_flat_instance(w, s, K):
    return integer_df_model(w, s, K, seed=8000 + 100 * w + s, near_flat=True)


def warped_instance(w, s, rep=0, vis=0.6):
    """The images of _umpa_oracle.warped_instance (same shapes, seeds and fields) with the visibility set to `vis` in the
    second half of the columns: S_k <- T (mu_k + vis (R_k(q - D) - mu_k)) = vis S_k + (1 - vis) T mu_k there, mu_k the mean of
    R_k in float64 (returned, to be passed explicitly)."""
    q = w + s
    T, Dx, Dy, S, R = ou.warped_model(2 * q + 21, 2 * q + ou.tile_width(w) + 9, ou.sweep_K(w, s),
                                      seed=1000 + 10 * w + s + 10000 * rep, dmax=max(0.5, s - 0.5))
    mu = np.array([r.astype(np.float64).mean() for r in R])
    h = S[0].shape[1] // 2
    for k, x in enumerate(S):
        x[:, h:] = (vis * x[:, h:].astype(np.float64) + (1 - vis) * T[:, h:] * mu[k]).astype(np.float32)
    return S, R, mu
