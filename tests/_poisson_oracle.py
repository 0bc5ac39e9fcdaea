"""Host-side oracle for the shot-noise kernel k_poisson (paresis_amd/csrc/detect.hip).  numpy / scipy only.

  * Philox4x32-10 with the kernel's counter layout and its uint32 -> float32 uniform mapping, vectorised;
  * `first_candidate`: the (U, V) both kernel paths give pixel p for its first PTRS candidate;
  * `sample`: a float64 restatement of the sampler (product of uniforms below a mean of 10, Hormann's PTRS with the kernel's
    constants above, the acceptance test against the exact log-pmf through gammaln) over any source of uniforms, with
    switchable planted defects for the power check of tests/test_poisson_host.py;
  * the statistics of tests/test_gpu_poisson.py, each a chi-square with its degrees of freedom or a z-score, and `Level`,
    which holds every one of them to alpha = 1e-9 / (number of statistical assertions of the GPU file).
"""
import numpy as np
from scipy import special, stats

MASK = np.uint64(0xFFFFFFFF)
TAG_FIRST, TAG_OWN = 0x5058, 0x5059
F32 = np.float32


# ------------------------------------------------------------------------------------------------ generator
def philox_words(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011): counter words c0..c3, key words k0, k1 (arrays or ints) -> uint32 [4, ...]."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        n0, n2 = (p1 >> s32) ^ c1 ^ k0, (p0 >> s32) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & MASK, p0 & MASK, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def philox4x32_10(ctr, sub, tag, key):
    """The kernel's block: counter words (ctr low, ctr high, sub, tag), key words (key low, key high)."""
    ctr, key = np.asarray(ctr, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    s32 = np.uint64(32)
    return philox_words(ctr & MASK, ctr >> s32, sub, tag, key & MASK, key >> s32)


def uniform_f32(words):
    """The kernel's mapping ((float)(c >> 8) + 0.5f) * 2^-24, in float32 with round-to-nearest-even like the device: in
    (0, 1]; 1.0 is reached because the + 0.5f is rounded away for c >> 8 >= 2^23."""
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(F32) + F32(0.5)) * F32(2.0 ** -24)


def first_candidate_words(p, seed):
    """The two Philox words (for U, for V) of pixel p's first candidate: block p >> 1, sub 0, tag 0x5058; words 0, 1 for even p
    and 2, 3 for odd p."""
    p = np.asarray(p, dtype=np.uint64)
    w = philox4x32_10(p >> np.uint64(1), 0, TAG_FIRST, seed)
    odd = (p & np.uint64(1)).astype(bool)
    return np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])


def first_candidate(p, seed):
    """(U, V) of pixel p exactly as both kernel paths assign them (float32; U = u - 0.5f)."""
    wu, wv = first_candidate_words(p, seed)
    return uniform_f32(wu) - F32(0.5), uniform_f32(wv)


class PhiloxSource:
    """The kernel's own streams: pixel p (0-based in the image) under key `seed`."""

    def __init__(self, seed):
        self.seed = int(seed) & (2 ** 64 - 1)

    def first(self, n):
        return first_candidate(np.arange(n, dtype=np.uint64), self.seed)

    def block(self, idx, sub):
        return uniform_f32(philox4x32_10(idx, sub, TAG_OWN, self.seed))


class NumpySource:
    """Independent uniforms from a numpy generator, through the same 32-bit word -> float32 mapping."""

    def __init__(self, rng):
        self.rng = rng

    def _u(self, shape):
        return uniform_f32(self.rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32))

    def first(self, n):
        return self._u(n) - F32(0.5), self._u(n)

    def block(self, idx, sub):
        return self._u((4, len(idx)))


# ------------------------------------------------------------------------------------------------ the sampler, restated
DEFECTS = ("direct_f32", "stirling_logL", "no_guard", "lam_scale", "shared_candidate", "ptrs_small")


def ptrs_constants(L):
    slam = np.sqrt(L)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    return a, b, 1.1239 + 1.1328 / (b - 3.4), 0.9277 - 3.6224 / (b - 2.0)


def _log_pmf(k, L, defects):
    if "direct_f32" in defects:        # the three terms rounded to float32 and summed there: what the Stirling branch avoids
        k32, L32 = k.astype(F32), L.astype(F32)
        return ((-L32 + k32 * np.log(L32)) - special.gammaln(k32 + F32(1)).astype(F32)).astype(np.float64)
    if "stirling_logL" in defects:     # the kernel's series form in float64, with log(2 pi L) for log(2 pi k)
        x = (k - L) / L
        g = (1 + x) * np.log1p(x) - x
        return -L * g - 0.5 * np.log(2 * np.pi * L) - 1 / (12 * k) + 1 / (360 * k ** 3)
    return -L + k * np.log(L) - special.gammaln(k + 1)


def sample(lam, source, defects=(), info=None):
    """One draw per entry of lam (float64 restatement of poisson_finish and of the squeeze in k_poisson).  `info`, a dict,
    receives per pixel: 'ncand' candidates examined by PTRS, 'margin' the smallest |log V' - log pmf| of its exact tests (inf
    when none ran), 'edge' the smallest distance of a candidate's value before the floor to an integer, in units of the
    DELTA of first_candidate_check, 'vgap' the smallest |V - vr| of its squeeze tests, 'near' the smallest
    |prod / exp(-lam) - 1| met by the product of uniforms (float32 products).  `safe_draws` turns them into one mask."""
    for d in defects:
        assert d in DEFECTS, d
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.size
    out = np.zeros(n)
    U0, V0 = source.first(n)
    U0, V0 = U0.astype(np.float64), V0.astype(np.float64)
    if "shared_candidate" in defects:
        m = n // 2
        U0[1:2 * m:2], V0[1:2 * m:2] = U0[0:2 * m:2], V0[0:2 * m:2]
    L_all = lam * (1 + 2e-4) if "lam_scale" in defects else lam
    ptrs = (lam >= 10.0) | (("ptrs_small" in defects) & (lam > 0.0))
    ncand = np.zeros(n, dtype=np.int32)
    margin = np.full(n, np.inf)
    near = np.full(n, np.inf)
    edge = np.full(n, np.inf)
    vgap = np.full(n, np.inf)
    # ---- PTRS
    idx = np.flatnonzero(ptrs)
    L = L_all[idx]
    a, b, invalpha, vr = ptrs_constants(L)
    out[idx] = np.floor(L)                       # the kernel's value when 128 candidates all fail
    U, V = U0[idx], V0[idx]
    delta = 4.0 * np.spacing((L + b / 2).astype(F32)).astype(np.float64)
    spare = None
    sub = 1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for it in range(128):
            if idx.size == 0:
                break
            ncand[idx] += 1
            us = 0.5 - np.abs(U)
            v = (2 * a / us + b) * U + L + 0.43
            k = np.floor(v)
            if info is not None:
                fin = np.isfinite(v)
                edge[idx[fin]] = np.minimum(edge[idx[fin]], (np.minimum(v - k, k + 1 - v) / delta)[fin])
                vgap[idx] = np.minimum(vgap[idx], np.abs(V - vr))
            acc = ((us >= 0.07) | ("no_guard" in defects)) & (V <= vr)
            test = ~acc & ~((k < 0) | ((us < 0.013) & (V > us)))
            if test.any():
                t = np.flatnonzero(test)
                lhs = np.log(V[t] * invalpha[t] / (a[t] / (us[t] * us[t]) + b[t]))
                d = lhs - _log_pmf(k[t], L[t], defects)
                margin[idx[t]] = np.minimum(margin[idx[t]], np.abs(d))
                acc[t] = d <= 0
            out[idx[acc]] = k[acc]
            keep = ~acc
            idx, L, a, b, invalpha, vr, delta = idx[keep], L[keep], a[keep], b[keep], invalpha[keep], vr[keep], delta[keep]
            if spare is not None:
                U, V, spare = spare[0][keep], spare[1][keep], None
            else:
                u = source.block(idx, sub)
                sub += 1
                u = [(u[0] - F32(0.5)).astype(np.float64), u[1].astype(np.float64), (u[2] - F32(0.5)).astype(np.float64),
                     u[3].astype(np.float64)]
                U, V, spare = u[0], u[1], (u[2], u[3])
    # ---- product of uniforms (float32 products, as the kernel forms them; the limit in float64)
    idx = np.flatnonzero((lam > 0.0) & ~ptrs)
    lim = np.exp(-L_all[idx])
    prod = np.ones(idx.size, dtype=F32)
    k = np.zeros(idx.size)
    for sub in range(1, 64):
        if idx.size == 0:
            break
        u = source.block(idx, sub)
        done = np.zeros(idx.size, dtype=bool)
        for i in range(4):
            prod = np.where(done, prod, prod * u[i])
            near[idx] = np.where(done, near[idx], np.minimum(near[idx], np.abs(prod / lim - 1.0)))
            hit = ~done & (prod <= lim)
            k += ~done & ~hit
            done |= hit
        out[idx[done]] = k[done]
        keep = ~done
        out[idx[keep]] = k[keep]                # the kernel's value when 252 uniforms do not get there
        idx, lim, prod, k = idx[keep], lim[keep], prod[keep], k[keep]
    if info is not None:
        info.update(ncand=ncand, margin=margin, near=near, edge=edge, vgap=vgap)
    return out


def safe_draws(info):
    """Pixels whose restated draw the float32 kernel must reproduce exactly: no exact test closer than 1e-3 (the kernel
    claims 1e-4 for its log-pmf), no candidate within DELTA of an integer before the floor, no squeeze within 1e-6 of vr,
    no running product within PRODUCT_NEAR of exp(-lam)."""
    return (info["margin"] > 1e-3) & (info["edge"] > 1.0) & (info["vgap"] > 1e-6) & (info["near"] > PRODUCT_NEAR)


def sample_hist(lam, N, source, defects=(), chunk=1 << 22):
    """Histogram (index = count) of N draws at the constant mean lam."""
    h = np.zeros(1, dtype=np.int64)
    for n0 in range(0, N, chunk):
        x = sample(np.full(min(chunk, N - n0), float(lam)), source, defects)
        x = np.clip(np.nan_to_num(x), 0, 4 * lam + 1000).astype(np.int64)      # a planted defect may leave the range of counts
        c = np.bincount(x)
        if c.size > h.size:
            c, h = h, c
        h[:c.size] += c
    return h


def first_candidate_check(lam, p, seed):
    """The first candidate of pixels p at means lam (>= 10), restated in float64 from the float32 (U, V).
    Returns (k, squeeze, checked): floor of the candidate, whether the squeeze accepts it with margin, and whether the value
    before the floor also stays DELTA away from an integer -- where `checked` holds the kernel's count must equal k exactly.

    DELTA.  The kernel forms v = (2 a rcp(us) + b) U + L + 0.43 in float32 (eps = 2^-24 per rounding, 2 eps for the hardware
    sqrt and rcp, which are good to 1 ulp): us = 0.5 - |U| is exact; b = 0.931 + 2.53 sqrt(L) carries 4 eps relative, a =
    -0.059 + 0.02483 b about 8 eps, 2 a rcp(us) 11 eps on a term <= 2 a / 0.07 = 0.71 b; the bracket t <= 1.71 b is off by at
    most 13.5 eps b, t U (|U| <= 0.43) by 6.6 eps b, and the two additions add eps (L + 0.74 b) each:
    |v32 - v64| <= 2 eps L + 9 eps b.  DELTA = four float32 spacings of L + b/2 is no less than that bound for every L
    >= 12.5 (at 12.5: 114 eps against 128 eps; at 100: 436 against 512; at 30000: 1.95 spacings against 4).
    The squeeze margin: vr = 0.9277 - 3.6224 rcp(b - 2) is off by at most 5.1 eps = 3e-7 in float32; V <= vr - 1e-6."""
    lam = np.asarray(lam, dtype=np.float64)
    U, V = first_candidate(p, seed)
    us = (F32(0.5) - np.abs(U)).astype(np.float64)
    U, V = U.astype(np.float64), V.astype(np.float64)
    a, b, _, vr = ptrs_constants(lam)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (2 * a / us + b) * U + lam + 0.43
    squeeze = (lam >= 10.0) & (us >= 0.07) & (V <= vr - 1e-6)
    delta = 4.0 * np.spacing((lam + b / 2).astype(F32)).astype(np.float64)
    k = np.floor(v)
    checked = squeeze & (v - k > delta) & (k + 1 - v > delta)
    return k, squeeze, checked


# a running product this close (relative) to exp(-lam) may fall either side of the device's expf (a few ulp of float32)
PRODUCT_NEAR = 8 * 2.0 ** -24


def find_unit_uniform(which, nseeds=64, npix=1 << 20):
    """The first (seed, pixel < npix) whose first-candidate U word (which = 0) or V word (which = 1) is 0xFFFFFFxx: u = 1.0."""
    p = np.arange(npix, dtype=np.uint64)
    for seed in range(nseeds):
        w = first_candidate_words(p, seed)[which]
        hit = np.flatnonzero(w >= np.uint32(0xFFFFFF00))
        if hit.size:
            return seed, int(hit[0])
    raise AssertionError("no u = 1.0 among %d seeds" % nseeds)


# ------------------------------------------------------------------------------------------------ statistics
def _cells(lam, N, min_expected=20.0):
    """Cells of counts for the chi-square at mean lam: (lo, hi, p) with p[j] the probability of count lo + j, the tails
    (<= lo, >= hi) pooled into the end cells so that every expected count N p is >= min_expected."""
    sd = np.sqrt(lam)
    lo, hi = int(max(0, np.floor(lam - 12 * sd - 30))), int(np.ceil(lam + 12 * sd + 30))
    ks = np.arange(lo, hi + 1)
    p = stats.poisson.pmf(ks, lam)
    p[0] = stats.poisson.cdf(lo, lam)
    p[-1] = stats.poisson.sf(hi - 1, lam)
    ok = np.flatnonzero(N * p >= min_expected)
    i, j = ok[0], ok[-1]
    q = p[i:j + 1].copy()
    q[0] += p[:i].sum()
    q[-1] += p[j + 1:].sum()
    return lo + i, lo + j, q


def _observed(h, lo, hi):
    idx = np.clip(np.arange(h.size), lo, hi) - lo
    return np.bincount(idx, weights=h.astype(np.float64), minlength=hi - lo + 1)


def chi2_fine(h, lam):
    """(a) per-count chi-square of the histogram h against Poisson(lam): (statistic, degrees of freedom)."""
    N = int(h.sum())
    lo, hi, p = _cells(lam, N)
    o, e = _observed(h, lo, hi), N * p
    return float(((o - e) ** 2 / e).sum()), p.size - 1


def chi2_coarse(h, lam, ncell=64):
    """(b) the same counts in at most ncell near-equiprobable cells of consecutive counts."""
    N = int(h.sum())
    lo, hi, p = _cells(lam, N)
    g = np.minimum(np.floor((np.cumsum(p) - p / 2) * ncell), ncell - 1).astype(np.int64)
    g = np.unique(g, return_inverse=True)[1]
    o, e = np.bincount(g, weights=_observed(h, lo, hi)), N * np.bincount(g, weights=p)
    return float(((o - e) ** 2 / e).sum()), e.size - 1


def moment_z(h, lam):
    """(c) z of the mean, of the variance and of the third central moment, all taken about the known mean lam:
    var(mean) = lam / N; var(s2 / lam) = 2/N + 1/(lam N) (mu4 = 3 lam^2 + lam); var(m3) = (mu6 - lam^2) / N with
    mu6 = 15 lam^3 + 25 lam^2 + lam."""
    N = float(h.sum())
    d = np.arange(h.size, dtype=np.float64) - lam
    w = h.astype(np.float64)
    m1, m2, m3 = (w * d).sum() / N, (w * d * d).sum() / N, (w * d * d * d).sum() / N
    return (m1 / np.sqrt(lam / N), (m2 / lam - 1) / np.sqrt(2 / N + 1 / (lam * N)),
            (m3 - lam) / np.sqrt((15 * lam ** 3 + 24 * lam ** 2 + lam) / N))


def binom_p(nonzero, N, lam):
    """Two-sided exact p-value of the number of nonzero pixels against Binomial(N, 1 - exp(-lam))."""
    return float(stats.binomtest(int(nonzero), int(N), -np.expm1(-lam)).pvalue)


def pit(x, lam, rng):
    """(d) the randomised probability-integral transform u = F(x - 1; lam_p) + w pmf(x; lam_p), w uniform: exactly uniform
    when x_p ~ Poisson(lam_p) independently.  A pixel of mean 0 (x must be 0 there) gets u = w."""
    x, lam = np.asarray(x, dtype=np.float64).ravel(), np.asarray(lam, dtype=np.float64).ravel()
    w = rng.random(x.size)
    pos = lam > 0
    xs, ls = x[pos], lam[pos]
    u = w.copy()
    cdf = np.where(xs > 0, special.pdtr(np.maximum(xs - 1, 0), ls), 0.0)
    u[pos] = cdf + w[pos] * np.exp(special.xlogy(xs, ls) - ls - special.gammaln(xs + 1))
    return np.clip(u, 0.0, 1.0)


def chi2_uniform(u, ncell=256):
    o = np.bincount(np.minimum((u * ncell).astype(np.int64), ncell - 1), minlength=ncell)
    e = u.size / ncell
    return float(((o - e) ** 2 / e).sum()), ncell - 1


def normal_scores(u):
    return special.ndtri(np.clip(u, 1e-300, 1 - 1e-16))


def corr_z(a, b):
    """(e) z = r sqrt(n) of the sample correlation of two equally long sets."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()) * np.sqrt(a.size))


# ------------------------------------------------------------------------------------------------ levels
# Statistical assertions of tests/test_gpu_poisson.py at PSX_FUZZ=1, per test (each test checks its own figure when it ends)
GPU_ASSERTIONS = {"fit": 87, "varying": 35, "independence": 36}
T_GPU = sum(GPU_ASSERTIONS.values())


class Level:
    """Every statistical assertion at alpha = 1e-9 / (T mult): together a correct sampler fails with probability <= 1e-9."""

    def __init__(self, T=None, mult=1):
        self.alpha = 1e-9 / ((T_GPU if T is None else T) * mult)
        self.zmax = float(stats.norm.isf(self.alpha / 2))
        self.made = 0
        self.log = []        # (label, kind, statistic, threshold)
        self.failed = []     # messages of the assertions that did not hold: a test reads them when it ends (`settle`)

    def chi2_limit(self, dof):
        return float(stats.chi2.isf(self.alpha, dof))

    def chi2(self, sd, label):
        stat, dof = sd
        lim = self.chi2_limit(dof)
        self.made += 1
        self.log.append((label, "chi2", stat, lim))
        if not stat <= lim:
            self.failed.append("%s: chi2 %.1f > %.1f (dof %d, alpha %.2e)" % (label, stat, lim, dof, self.alpha))

    def z(self, z, label):
        self.made += 1
        self.log.append((label, "z", abs(z), self.zmax))
        if not abs(z) <= self.zmax:
            self.failed.append("%s: |z| %.2f > %.2f (alpha %.2e)" % (label, abs(z), self.zmax, self.alpha))

    def p(self, p, label):
        self.made += 1
        self.log.append((label, "p", p, self.alpha))
        if not p >= self.alpha:
            self.failed.append("%s: p %.3e < alpha %.2e" % (label, p, self.alpha))

    def settle(self, made_before, expected=None):
        """End of a test: every statistic was inside its limit, and the test made the number of assertions alpha counts on."""
        failed, self.failed = self.failed, []
        assert not failed, "\n".join(failed)
        assert expected is None or self.made - made_before == expected, (self.made - made_before, expected)

    def rejects_chi2(self, sd):
        return sd[0] > self.chi2_limit(sd[1])

    def rejects_z(self, z):
        return abs(z) > self.zmax


# ------------------------------------------------------------------------------------------------ the GPU file's cases
def f32(x):
    return float(F32(x))


LAM_GRID = [f32(v) for v in (1e-6, 1e-3, 0.1, 0.5, 3.0, np.nextafter(F32(10), F32(0)), 10.0, np.nextafter(F32(10), F32(np.inf)),
                             12.5, 30.0, 63.5, 64.0, 64.5, 100.0, 1000.0, 7500.0, 30000.0, 2e5, 1e6)]


def fit_size(lam):
    return 1 << 24 if lam >= 1000 else 1 << 22


def smooth_field(n, lo=2.0, hi=20000.0):
    """A detector-like mean image of n pixels (rows of 1024): a smooth positive field spanning lo..hi, float32."""
    i = np.arange(n, dtype=np.float64)
    r, c = i // 1024, i % 1024
    s = 0.5 + 0.25 * np.cos(r / 97.0 + 0.3) * np.cos(c / 61.0 + 1.1) + 0.25 * np.cos(r / 23.0 - 0.7 + c / 151.0)
    return (lo * (hi / lo) ** np.clip(s, 0.0, 1.0)).astype(F32)


CYCLE = (0.0, 0.7, 11.0, 40.0, 90.0, 7500.0)


def cycle_field(n, rot):
    return np.asarray(CYCLE, dtype=F32)[(np.arange(n) + rot) % len(CYCLE)]


def lone_pending_field(n):
    """7500 everywhere but one pixel per wave of the 16-byte path (256 pixels) at 12: after the squeeze most waves hold that
    pixel's exact test beside a few dozen pending pixels of the other branch."""
    f = np.full(n, 7500.0, dtype=F32)
    f[37::256] = 12.0
    return f


# keys of the GPU file, fixed before its first run on a GPU; repetition `rep` of PSX_FUZZ shifts them
SEED = {"fit": 0x0F17 << 20, "varying": 0x7A21 << 20, "first": 0xF125 << 20, "product": 0x9D0D << 20, "indep": 0x1DE9 << 20,
        "edges": 0xED6E << 20}
FIRST_LAMS = (12.5, 100.0, 7500.0, 30000.0)
PRODUCT_LAMS = (0.5, 3.0, LAM_GRID[5])
EXACT_N = 1 << 20        # pixels of the bit-for-bit comparisons and of the independence fields


def key(test, rep, j=0):
    return SEED[test] + (rep << 12) + j


UNIT_U, UNIT_V = (21, 543356), (6, 621649)      # find_unit_uniform(0), (1): (seed, pixel) whose first-candidate u is 1.0
PIT_MIN = 256 * 20                              # pixels a chi-square on 256 cells of u needs (expected count 20)
SIZES = (4 * 64 * 3 + 4 * 17, 300007, 2048 * 2048)    # the last round of the 16-byte path runs with inactive lanes
COMPARE_MAX = 300007                            # fields up to this size are also compared with the restatement, draw by draw


def varying_fields():
    """(name, mean image) of the varying-mean tests."""
    out = [("smooth-%d" % n, smooth_field(n)) for n in SIZES]
    out += [("cycle-rot%d" % r, cycle_field(SIZES[1], r)) for r in range(len(CYCLE))]
    out += [("lone-%d" % n, lone_pending_field(n)) for n in (SIZES[0], SIZES[2])]
    return out


def strata(lam):
    """(name, mask) of the PIT chi-squares of one field: all pixels, and each branch of the sampler that holds enough."""
    lam = np.asarray(lam).ravel()
    out = [("all", np.ones(lam.size, dtype=bool))]
    for name, m in (("<10", (lam > 0) & (lam < 10)), ("10-64", (lam >= 10) & (lam < 64)), (">=64", lam >= 64)):
        if m.sum() >= PIT_MIN:
            out.append((name, m))
    return out
