"""Plain numpy references of the dark-field re-splat (refractionFileNumba2.py:168-186; paresis_amd/csrc/darkfield.hip), the
cases that reach every form the kernels are built in, and the error yardsticks the GPU bounds come from.  numpy only: nothing
here imports the package's kernels.

resplat()      float64, the reference's literal rule: a source with weight (I2DF != 0) and half > 0 deposits the normalised
               patch exp(-(di^2 + dj^2) / (2 sigma^2)), sigma = DF32 / 2, over |di|, |dj| <= half, clipped at the border;
               half == 0 deposits on itself; I2 is added at the end.  S[p] = |I2[p]| + sum of |terms| reaching p.
resplat_f32()  the LDS kernels' arithmetic in numpy float32: w = I2DF * inv, c = -log2(e) / (2 sigma^2), term
               w * exp2((di^2 + dj^2) * c) selected by half >= max(|di|, |dj|), summed rows first, then columns.
selection()    k_df_gather_tiled's choice of body per 32 x 32 tile; bands(): launch_banded's band heights.

Widths come from a target half-size h: d = (2/3)(h + u), |u| <= 0.4 (d = 0 for h = 0), so that k_df_split's
rint((d / 2) * 3) in float64 and k_df_prepare's rintf(3 * (0.5f * (float)d)) are both h: asserted for every pixel.  The two
entry points therefore draw the same patches, and their 1 / normalisation is the float32 of a float64 sum either way: one
restatement serves both.

BOUNDS.  YARDSTICK[reach] = max over the dense cases of that reach (widest patch among the weighted sources) of
|resplat_f32 - resplat| / S, measured on the CPU by measure_yardsticks(); tests/test_darkfield_host.py reproduces the table.
The GPU bound is 4 x the yardstick: 2 because the hardware 2^x and numpy's exp2f may each be 1 ulp off per term, 2 of headroom
for the maximum over a few thousand pixels and for multiply-add contraction, which only removes roundings.  The global-memory
gather (R > 2032) forms expf(-d2 / (2 sigma^2)): two roundings fewer in the exponent than d2 * c, so the same bound holds.

A single source is different: S at a pixel of its patch is that one term, and the term's own relative error grows with the
exponent.  single_bound() is derived, not measured: inv and w = I2DF * inv round once each (2), c = const / (2 sigma sigma)
carries the constant's, the square's and the quotient's rounding (3) and d2 * c one more (4 on the exponent x = d2 * c), the
2^x is 1 ulp = 2 half-ulps (2), the product w * 2^x one (1): relative error <= (5 + 4 ln2 |x|) u, u = 2^-24, and
4 ln2 |x| = 2 d2 / sigma^2.  Summed over an unclipped patch, sum t (5 + 2 d2 / sigma^2) u <= (5 + 2 * 2) u sum t since the
mean of d2 under the (truncated) Gaussian is at most 2 sigma^2: within the (2h + 1)^2 u the tests assert, for every h >= 1.
"""
import collections
import functools

import numpy as np

DT = 32                      # tile side of both LDS kernels
LOG2E_F32 = np.float32(1.4426950408889634)
U = 2.0 ** -24

Case = collections.namedtuple("Case", "name I2DF DF64 DF32 half I2 reach")


# ---- the references ----------------------------------------------------------------------------------------------------

def _norm(sigma, half):
    """(sum_{|d| <= half} exp(-d^2 / 2 sigma^2))^2 per source, float64 (the patch normalisation is separable)."""
    s = np.ones_like(sigma)
    for d in range(1, int(half.max()) + 1):
        s += np.where(half >= d, 2.0 * np.exp(-(d * d) / 2.0 / np.where(sigma != 0, sigma, 1.0) ** 2), 0.0)
    return s * s


def _gather(w, c, half, fexp, want_abs):
    """sum over (di, dj), rows first, of the per-source term w * fexp((di^2 + dj^2) * c) where half >= max(|di|, |dj|), moved
    to the pixel it lands on; in w's dtype.  Also the sum of |terms| if asked."""
    Nx, Ny = w.shape
    acc = np.zeros_like(w)
    sab = np.zeros_like(w) if want_abs else None
    H = int(half.max())
    for di in range(-H, H + 1):                      # output (i, j) takes source (i + di, j + dj)
        i0, i1 = max(0, -di), min(Nx, Nx - di)
        if i0 >= i1:
            continue
        for dj in range(-H, H + 1):
            j0, j1 = max(0, -dj), min(Ny, Ny - dj)
            if j0 >= j1:
                continue
            src = (slice(i0 + di, i1 + di), slice(j0 + dj, j1 + dj))
            sel = half[src] >= max(abs(di), abs(dj))
            if not sel.any():
                continue
            d2 = w.dtype.type(di * di + dj * dj)
            t = np.where(sel, w[src] * fexp(d2 * c[src]), w.dtype.type(0))
            acc[i0:i1, j0:j1] += t
            if want_abs:
                sab[i0:i1, j0:j1] += np.abs(t)
    return acc, sab


def _half_of(I2DF, half):
    return np.where(np.asarray(I2DF) != 0, np.asarray(half, dtype=np.int64), -1)      # no weight: deposits nothing


def resplat(I2DF, DF32, half, I2):
    """(out, S) in float64 by the reference's literal rule; half: the patch half-size per source."""
    v = np.asarray(I2DF, dtype=np.float64)
    sigma = np.asarray(DF32, dtype=np.float64) / 2
    h = _half_of(I2DF, half)
    hp = np.maximum(h, 0)
    ok = hp > 0
    w = v / _norm(np.where(ok, sigma, 0.0), hp)
    c = np.where(ok, -1.0 / (2.0 * np.where(ok, sigma, 1.0) ** 2), 0.0)
    acc, sab = _gather(w, c, h, np.exp, True)
    i2 = np.zeros_like(v) if I2 is None else np.asarray(I2, dtype=np.float64)
    return acc + i2, sab + np.abs(i2)


def resplat_f32(I2DF, DF32, half, I2):
    """The LDS kernels' float32 arithmetic, term by term and in their order, on the CPU."""
    f = np.float32
    v = np.asarray(I2DF, dtype=f)
    sg = f(0.5) * np.asarray(DF32, dtype=f)
    h = _half_of(I2DF, half)
    hp = np.maximum(h, 0)
    ok = hp > 0
    inv = (1.0 / _norm(np.where(ok, sg.astype(np.float64), 0.0), hp)).astype(f)
    w = v * inv
    with np.errstate(divide="ignore"):
        c = np.where(ok, -LOG2E_F32 / (f(2) * sg * sg), f(0)).astype(f)
    acc, _ = _gather(w, c, h, np.exp2, False)
    assert acc.dtype == f
    return acc + (f(0) if I2 is None else np.asarray(I2, dtype=f))


def patch(DF32_src, half_src):
    """The normalised (2 half + 1)^2 patch of one source, float64 (gaussian_shape(DF / 2), RF2:14-23)."""
    sigma = float(DF32_src) / 2
    q = np.arange(-half_src, half_src + 1, dtype=np.float64) ** 2
    g = np.exp(-(q[:, None] + q[None, :]) / 2.0 / sigma ** 2)
    return g / g.sum()


def single_bound(DF32_src, half_src):
    """(2 half + 1)^2 table of the derived relative bound of one source's terms (module docstring)."""
    sigma = float(DF32_src) / 2
    q = np.arange(-half_src, half_src + 1, dtype=np.float64) ** 2
    return (5.0 + 2.0 * (q[:, None] + q[None, :]) / sigma ** 2) * U


# ---- the kernels' selection rules ----------------------------------------------------------------------------------------

def selection(I2DF, half, R):
    """The (Re, uniform) pairs k_df_gather_tiled takes over the 32 x 32 tiles of the image.  half: the patch table's
    half-sizes (k_df_split fills them for every pixel; k_df_prepare writes -1 where I2DF == 0).  Re == 0 is `case 0`, the one
    body without a uniform form: reported as (0, True)."""
    I2DF, half = np.asarray(I2DF), np.asarray(half)
    Nx, Ny = I2DF.shape
    got = set()
    for t0 in range(0, Nx, DT):
        for c0 in range(0, Ny, DT):
            win = (slice(max(0, t0 - R), min(Nx, t0 + DT + R)), slice(max(0, c0 - R), min(Ny, c0 + DT + R)))
            hw, ww = half[win], (I2DF[win] != 0) & (half[win] >= 0)
            hmax = max(0, int(hw.max()))
            hlow = int(hw[ww].min()) if ww.any() else 1 << 20
            Re = min(R, hmax)
            got.add((Re, True if Re == 0 else hlow >= Re))
    return got


def bands(R):
    """Row counts of the bands k_df_gather_banded stages for a tile at reach R; [] where launch_banded takes the
    global-memory gather instead (a window row does not fit 64 KiB)."""
    W = DT + 2 * R
    band = min(W, (64 * 1024) // (16 * W))
    if band < 1:
        return []
    return [min(band, W - b) for b in range(0, W, band)]


# ---- the cases -------------------------------------------------------------------------------------------------------------

def build(name, hmap, seed, weightless=0.2):
    """A case from a map of target half-sizes: widths d = (2/3)(h + u), weights in [1, 9) with a fraction at zero, I2 in [0, 3)."""
    rng = np.random.default_rng(seed)
    h = np.asarray(hmap, dtype=np.int64)
    u = rng.uniform(-0.4, 0.4, h.shape)
    d = np.where(h > 0, (2.0 / 3.0) * (h + u), 0.0)
    d32 = d.astype(np.float32)
    assert np.array_equal(np.rint((d / 2) * 3), h), name                                   # k_df_split
    assert np.array_equal(np.rint(np.float32(3) * (np.float32(0.5) * d32)), h), name       # k_df_prepare
    I2DF = np.where(rng.uniform(size=h.shape) < weightless, 0.0, rng.uniform(1.0, 9.0, h.shape)).astype(np.float32)
    I2 = rng.uniform(0.0, 3.0, h.shape).astype(np.float32)
    wh = h[I2DF != 0]
    return Case(name, I2DF, d, d32, h, I2, int(wh.max()) if wh.size else 0)


def uniform(name, k, shape, seed):
    """Every source has half-size k."""
    return build(name, np.full(shape, k), seed)


def mixed(name, k, shape, seed):
    """Half-sizes drawn from 0 ... k."""
    return build(name, np.random.default_rng(seed + 7919).integers(0, k + 1, shape), seed)


GRID = (70, 45)              # six tiles, ragged on both axes
SHAPES = ((1, 1), (1, 100), (100, 1), (32, 32), (33, 31), (31, 33), (65, 33))
DENSE_R = (15, 16, 17, 31, 48)
NARROW_R = (17, 40)
SINGLE_POS = ((31, 31), (32, 32), (31, 32), (0, 0), (63, 40))
SINGLE_GRID = (64, 64)


def _corner(name, seed, weight):
    """96 x 64, patches of h <= 2 and one h = 20 source in a corner tile (with weight, or without)."""
    h = np.random.default_rng(seed + 7919).integers(0, 3, (96, 64))
    h[5, 58] = 20
    c = build(name, h, seed)
    I2DF = c.I2DF.copy()
    I2DF[5, 58] = 6.5 if weight else 0.0
    wh = h[I2DF != 0]
    return c._replace(I2DF=I2DF, reach=int(wh.max()))


def _all_cases():
    cs = []
    for k in range(15):
        cs.append(uniform("uniform %d" % k, k, GRID, 100 + k))
    for k in range(1, 15):
        cs.append(mixed("mixed %d" % k, k, GRID, 200 + k))
    for R in DENSE_R:
        cs.append(mixed("dense %d" % R, R, (75, 58), 300 + R))
    for m in range(6):
        cs.append(mixed("narrow %d" % m, m, GRID, 400 + m))
    cs.append(_corner("corner 20", 500, True))
    cs.append(_corner("weightless 20", 501, False))
    for n, shape in enumerate(SHAPES):
        tag = "%dx%d" % shape
        cs.append(mixed("mixed 3 %s" % tag, 3, shape, 600 + n))
        cs.append(uniform("uniform 14 %s" % tag, 14, shape, 620 + n))
        cs.append(mixed("dense 17 %s" % tag, 17, shape, 640 + n))
    cs.append(mixed("far 3", 3, (40, 33), 700))          # the global-memory gather's case (R = 2033)
    return collections.OrderedDict((c.name, c) for c in cs)


ALL = _all_cases()
CASES = collections.OrderedDict((n, c) for n, c in ALL.items()                      # the 29 bodies of the tiled kernel
                                if n.split()[0] in ("uniform", "mixed") and len(n.split()) == 2)


def single(pos, h, second=False):
    """One weighted source of half-size h at pos on 64 x 64, everything else zero; second: a weighted h = 0 source h + 1 rows
    away (outside the patch, inside the window of the tiles the patch touches), None where the grid has no room for it."""
    Nx, Ny = SINGLE_GRID
    I2DF = np.zeros(SINGLE_GRID, dtype=np.float32)
    d = np.zeros(SINGLE_GRID)
    hm = np.zeros(SINGLE_GRID, dtype=np.int64)
    I2DF[pos] = 5.3
    d[pos] = (2.0 / 3.0) * (h + 0.25)
    hm[pos] = h
    assert np.rint((d[pos] / 2) * 3) == h and np.rint(np.float32(3) * (np.float32(0.5) * np.float32(d[pos]))) == h
    other = None
    if second:
        for i2 in (pos[0] + h + 1, pos[0] - h - 1):
            if 0 <= i2 < Nx:
                other = (i2, pos[1])
                break
        if other is None:
            return None, None
        I2DF[other] = 2.1
    return Case("single %d at %s" % (h, pos), I2DF, d, d.astype(np.float32), hm, None, h), other


@functools.lru_cache(maxsize=None)
def reference(name):
    """(out, S) of resplat() for a named case: computed once, shared, never written to."""
    c = ALL[name]
    out, S = resplat(c.I2DF, c.DF32, c.half, c.I2)
    out.setflags(write=False)
    S.setflags(write=False)
    return out, S


def measure(c, ref=None):
    """max |resplat_f32 - resplat| / S of one case."""
    out, S = ref if ref is not None else resplat(c.I2DF, c.DF32, c.half, c.I2)
    f32 = resplat_f32(c.I2DF, c.DF32, c.half, c.I2).astype(np.float64)
    return float(np.max(np.abs(f32 - out) / np.where(S > 0, S, 1.0)))


def measure_yardsticks():
    """reach -> max over the dense cases of that reach of measure()."""
    tab = {}
    for name, c in ALL.items():
        tab[c.reach] = max(tab.get(c.reach, 0.0), measure(c, reference(name)))
    return tab


# measured by measure_yardsticks() on the CPU (numpy float32 against float64); reproduced by tests/test_darkfield_host.py
YARDSTICK = {
    0: 5.958e-08, 1: 2.306e-07, 2: 2.733e-07, 3: 3.281e-07, 4: 4.774e-07, 5: 5.226e-07, 6: 7.422e-07, 7: 6.732e-07,
    8: 7.814e-07, 9: 9.328e-07, 10: 8.343e-07, 11: 9.832e-07, 12: 9.955e-07, 13: 1.481e-06, 14: 1.328e-06,      # tiled
    15: 8.826e-07, 16: 9.600e-07, 17: 1.402e-06, 20: 2.215e-07, 31: 1.688e-06, 48: 1.949e-06,                      # banded
}


def bound(reach):
    """The GPU bound on |out - ref| / S for a dense case of that reach: 4 x the yardstick (module docstring)."""
    return 4.0 * YARDSTICK[reach]
