"""The spectral material decomposition of psx_decompose_f32 (include/paresis_hip.h) in numpy, vectorised over the pixels:
float64 by default, np.longdouble as the rounding yardstick.  Also the test materials and spectra the spectral tests share."""
import numpy as np


def effective(bin_size, w, a):
    """Abar [B, M]: Abar_bm = sum_e w_be a_mbe."""
    a = np.asarray(a)
    out = np.zeros((len(bin_size), a.shape[0]), dtype=a.dtype)
    e0 = 0
    for b, ne in enumerate(bin_size):
        out[b] = a[:, e0:e0 + ne] @ np.asarray(w)[e0:e0 + ne]
        e0 += ne
    return out


def linear_start(bin_size, w, a, v):
    """G [M, B] = (Abar^T V Abar)^-1 Abar^T V in float64: what the host hands the kernel."""
    A = effective(bin_size, np.asarray(w, np.float64), np.asarray(a, np.float64))
    V = np.diag(np.asarray(v, np.float64))
    return np.linalg.solve(A.T @ V @ A, A.T @ V)


def transmission(bin_size, w, a, x, dtype=np.float64):
    """T [B, n] of thicknesses x [M, n]."""
    w, a, x = np.asarray(w, dtype), np.asarray(a, dtype), np.asarray(x, dtype)
    out, e0 = [], 0
    for ne in bin_size:
        out.append((w[e0:e0 + ne, None] * np.exp(-(a[:, e0:e0 + ne].T @ x))).sum(axis=0))
        e0 += ne
    return np.stack(out)


def _ldl_solve(N, rhs):
    """N d = rhs per pixel by LDL^T without pivoting.  N [n, M, M], rhs [n, M] -> (d [n, M], ok [n]): ok is false where a
    pivot is <= 0 or not finite."""
    n, M = rhs.shape
    Lf = np.zeros_like(N)
    D = np.zeros_like(rhs)
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(M):
            dj = N[:, j, j] - sum(Lf[:, j, k] ** 2 * D[:, k] for k in range(j))
            ok &= (dj > 0) & np.isfinite(dj)
            dj = np.where(ok, dj, 1)
            D[:, j] = dj
            for i in range(j + 1, M):
                Lf[:, i, j] = (N[:, i, j] - sum(Lf[:, i, k] * Lf[:, j, k] * D[:, k] for k in range(j))) / dj
        y = np.zeros_like(rhs)
        for i in range(M):
            y[:, i] = rhs[:, i] - sum(Lf[:, i, k] * y[:, k] for k in range(i))
        y /= D
        d = np.zeros_like(rhs)
        for i in range(M - 1, -1, -1):
            d[:, i] = y[:, i] - sum(Lf[:, k, i] * d[:, k] for k in range(i + 1, M))
    return d, ok


def _residuals(bin_size, w, a, x, L):
    """Per bin: r [B, n], g [B, n, M] at x [n, M]."""
    r, g, e0 = [], [], 0
    with np.errstate(all="ignore"):
        for b, ne in enumerate(bin_size):
            ab = a[:, e0:e0 + ne]                                   # [M, ne]
            s = w[None, e0:e0 + ne] * np.exp(-(x @ ab))             # [n, ne]
            T = s.sum(axis=1)
            g.append((s @ ab.T) / T[:, None])
            r.append(L[b] + np.log(T))
            e0 += ne
    return np.stack(r), np.stack(g)


def decompose(L, bin_size, w, a, v, G, iterations=12, tol=1e-13, dtype=np.float64):
    """L [B, n] (the float32 data, widened) -> (x [M, n], residual [n], steps [n]) in `dtype`, the algorithm of the header."""
    L = np.asarray(L).astype(dtype)
    w, a, v, G = (np.asarray(t).astype(dtype) for t in (w, a, v, G))
    B, n = L.shape
    M = a.shape[0]
    abar = effective(bin_size, w, a).max(axis=0)
    bad = ~np.isfinite(L).all(axis=0)
    Lc = np.where(bad[None], 0, L)
    x = (G @ Lc).T.copy()                                            # [n, M]
    steps = np.zeros(n, dtype=np.int64)
    active = ~bad
    for k in range(1, iterations + 1):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        r, g = _residuals(bin_size, w, a, x[idx], Lc[:, idx])
        N = np.einsum("b,bni,bnj->nij", v, g, g)
        rhs = np.einsum("b,bni,bn->ni", v, g, r)
        d, ok = _ldl_solve(N, rhs)
        ok &= np.isfinite(d).all(axis=1)
        steps[idx[~ok]] = -2
        good = idx[ok]
        x[good] += d[ok]
        steps[good] = k
        done = np.zeros(idx.size, dtype=bool)
        done[~ok] = True
        with np.errstate(invalid="ignore"):
            done[ok] = (np.abs(d[ok]) * abar[None]).max(axis=1) <= tol
        active[idx[done]] = False
    r, _ = _residuals(bin_size, w, a, x, Lc)
    with np.errstate(all="ignore"):
        res = np.sqrt((v[:, None] * r * r).sum(axis=0))
    x[bad] = 0
    res[bad] = np.inf
    steps[bad] = -1
    return x.T.copy(), res, steps


# ---- the test materials: linear attenuation coefficients in 1/m at E in keV, of the size of real ones ---------------------
def mu_soft(E):
    """Water-like: photoelectric E^-4 (as tabulated between 20 and 80 keV) plus a Compton-like E^-1 term."""
    E = np.asarray(E, np.float64)
    return 54.0 * (20.0 / E) ** 4 + 18.0 * (60.0 / E)


def mu_bone(E):
    E = np.asarray(E, np.float64)
    return 700.0 * (20.0 / E) ** 3.2 + 38.0 * (60.0 / E) ** 0.8


def _kedge(edge, below, jump):
    def mu(E):
        E = np.asarray(E, np.float64)
        return below * (edge / E) ** 2.8 * np.where(E >= edge, jump, 1.0) + 6.0 * (60.0 / E)
    return mu


mu_iodine = _kedge(33.2, 40.0, 5.5)        # a dilute contrast agent: K-edge step at 33.2 keV
mu_gadolinium = _kedge(50.2, 30.0, 4.8)    # K-edge step at 50.2 keV
MU = {"SpecSoft": mu_soft, "SpecBone": mu_bone, "SpecIodine": mu_iodine, "SpecGd": mu_gadolinium}
ORDER = ("SpecSoft", "SpecBone", "SpecIodine", "SpecGd")


def register_materials():
    """The four as paresis_amd materials: beta = mu/(2k), k = getk(E) (Sample.stack_rt's catt = -2 k beta = -mu); delta ~ E^-2."""
    from paresis_amd import materials
    from paresis_amd.getk import k_sample
    for name, mu in MU.items():
        materials.register_material(name, lambda e, mu=mu: (1e-6 * (30.0 / e) ** 2, float(mu(e)) / (2.0 * k_sample(e))), "test")


def flux_of(E):
    """A tungsten-like hump on 20-80 keV."""
    t = (np.asarray(E, np.float64) - 18.0) / 62.0
    return t * (1.2 - t) ** 2 + 0.02


def spectrum(lo=20.0, hi=80.0, step=2.0):
    """(E, flux) on [lo, hi] keV, sampled every `step`."""
    E = np.arange(lo, hi + step / 2, step)
    return E, flux_of(E)


def model_arrays(sizes, M, exact_weights=False):
    """(E, w, a) of bins of `sizes` energies spread evenly over 20-80 keV (bin centres for single-energy bins) and the first M
    test materials.  exact_weights: every weight a multiple of 2^-20, each bin's summing to 1 exactly in any order."""
    n = int(sum(sizes))
    E = np.linspace(20.0, 80.0, n) if n > len(sizes) else 20.0 + 60.0 * (np.arange(n) + 0.5) / n
    w, e0 = [], 0
    for ne in sizes:
        f = flux_of(E[e0:e0 + ne])
        f = f / f.sum()
        if exact_weights:
            f = np.round(f * 2.0 ** 20) / 2.0 ** 20
            f[-1] = 1.0 - f[:-1].sum()
        w.append(f)
        e0 += ne
    return E, np.concatenate(w), coefficients(E, M)


def split(E, flux, thresholds):
    """Bins closing at the first energy >= each threshold, the last bin taking the rest -> (bin_size, w) with w normalised
    per bin, and the energies in order."""
    edges = [int(np.searchsorted(E, t, side="left")) + 1 for t in thresholds] + [len(E)]
    sizes, w, e0 = [], [], 0
    for e1 in edges:
        sizes.append(e1 - e0)
        w.append(flux[e0:e1] / flux[e0:e1].sum())
        e0 = e1
    return sizes, np.concatenate(w)


def coefficients(E, M):
    return np.stack([MU[ORDER[m]](E) for m in range(M)])
