"""float64 numpy oracle of the Paganin contract (include/paresis_hip.h, psx_paganin_f32), the inputs the CPU and GPU tests
share, and the blob experiment that pins the filter's units."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)


def ratio(I, I0=None):
    """r = I/I0 in float64 (I where I0 is None); 1 where I is not finite or I0 is not finite or not > 0."""
    I = np.asarray(I, dtype=np.float32).astype(np.float64)
    if I0 is None:
        return np.where(np.isfinite(I), I, 1.0)
    I0 = np.asarray(I0, dtype=np.float32).astype(np.float64)
    ok = np.isfinite(I) & np.isfinite(I0) & (I0 > 0)
    with np.errstate(all="ignore"):
        return np.where(ok, I / np.where(ok, I0, 1.0), 1.0)


def extend(x):
    """The even mirror extension to 2n x 2m: ext[a][b] = x[a < n ? a : 2n-1-a][b < m ? b : 2m-1-b]."""
    e = np.concatenate([x, x[::-1, :]], 0)
    return np.concatenate([e, e[:, ::-1]], 1)


def k2(n, m):
    kx = 2 * np.pi * np.fft.fftfreq(2 * n)[:, None]
    ky = 2 * np.pi * np.fft.fftfreq(2 * m)[None, :]
    return kx * kx + ky * ky


def paganin(I, I0, alpha, mu):
    """-> {'contact', 'thickness'} float32, 'r' (float64, after the guards), 'y' (float64, the filtered contrast)."""
    r = ratio(I, I0)
    x = (r - 1.0).astype(np.float32).astype(np.float64)
    n, m = x.shape
    # the extension is real and the filter even in k: the half-spectrum transforms compute the same y at half the cost
    y = np.fft.irfft2(np.fft.rfft2(extend(x)) / (1.0 + float(alpha) * k2(n, m)[:, :m + 1]), s=(2 * n, 2 * m))[:n, :m]
    c = 1.0 + y
    with np.errstate(all="ignore"):
        t = np.where(c > 0, -np.log1p(np.where(c > 0, y, 0.0)), -np.log(FLT_MIN)) / float(mu)
    return {'contact': c.astype(np.float32), 'thickness': t.astype(np.float32), 'r': r, 'y': y}


def bounds(o, mu):
    """The parity bound of the issue: (contact, thickness) = (5e-6*max|r - 1| + 1.2e-7*max|c|, the same / (mu*c_min))."""
    c = o['contact'].astype(np.float64)
    bc = 5e-6 * np.abs(o['r'] - 1.0).max() + 1.2e-7 * np.abs(c).max()
    return bc, bc / (float(mu) * c.min())


def cosine_series(n, m, rng, terms=6, fmax=8):
    """A sum of cos(pi a (i+1/2)/n) cos(pi b (j+1/2)/m): even about every border, so periodic on the extension."""
    i = np.arange(n)[:, None] + 0.5
    j = np.arange(m)[None, :] + 0.5
    t = np.zeros((n, m))
    for _ in range(terms):
        a, b = rng.integers(0, fmax, 2)
        t += rng.standard_normal() * np.cos(np.pi * a * i / n) * np.cos(np.pi * b * j / m)
    return t


def known_answer(n, m, alpha, mu, seed=4, tmax=1e-2):
    """t >= 0 a cosine series (max tmax metres), c0 = exp(-mu t), r = ifft2((1 + alpha k^2) fft2(ext c0)) on the corner:
    the image whose exact Paganin retrieval is t.  -> (t, r) float64."""
    t = cosine_series(n, m, np.random.default_rng(seed))
    t = (t - t.min()) * (tmax / (t.max() - t.min()))
    c0 = np.exp(-mu * t)
    r = np.fft.ifft2((1.0 + alpha * k2(n, m)) * np.fft.fft2(extend(c0))).real[:n, :m]
    return t, r


def image_pair(n, m, seed, contrast=0.3):
    """A propagation image with structure at every scale and its flat field (float32): I = I0*(1 + contrast*u), |u| <= 1."""
    rng = np.random.default_rng(seed)
    u = 0.6 * cosine_series(n, m, rng, terms=5, fmax=max(2, min(n, m, 12))) + 0.4 * rng.standard_normal((n, m))
    u /= np.abs(u).max()
    I0 = 1000.0 * (1.0 + 0.1 * rng.random((n, m)))
    return (I0 * (1.0 + contrast * u)).astype(np.float32), I0.astype(np.float32)


# ---- the blob experiment: Fil_Nylon_ID17's configuration at magnification 2, no membrane, a Gaussian blob of nylon -------------
BLOB_HEIGHT_M, BLOB_SIGMA_PX = 1e-3, 80.0


def bin2(a):
    n, m = a.shape
    return a.reshape(n // 2, 2, m // 2, 2).mean(axis=(1, 3))


def blob_cfg():
    """(cfg, T): the oracle configuration of Fil_Nylon_ID17 (tests/_build.cfg_from_experiment) with the membrane zero,
    dSM = 1.0, dMO = 0.2, dOD = 1.2 (M = 2), study pixel 6/(2*M) um, and a centred Gaussian blob, 1 mm high, sigma 80 study
    pixels, on the 400^2 grid as the sample; T the blob in metres.  Needs no GPU."""
    from oracle import paresis_oracle as orc
    from paresis_amd.Experiment import Experiment
    from tests._build import cfg_from_experiment
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": "/tmp/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": "RayT", "noise": False}
    exp = Experiment(ed)
    exp.myMembrane.myGeometry = np.zeros((2, 400, 400), dtype=np.float32)
    cfg = cfg_from_experiment(exp, orc.Obj)
    M = 2.0
    cfg.update(dSM=1.0, dMO=0.2, dOD=1.2, M=M, pix_um=6.0 / (2 * M))
    i = np.arange(400)[:, None] - 199.5
    j = np.arange(400)[None, :] - 199.5
    T = BLOB_HEIGHT_M * np.exp(-(i * i + j * j) / (2 * BLOB_SIGMA_PX ** 2))
    cfg["sample"] = orc.Obj(T[None], cfg["sample"].delta, cfg["sample"].beta)
    return cfg, T


def blob_params(cfg):
    """retrieval.paganin's keyword arguments for the blob experiment."""
    return dict(delta=float(cfg["sample"].delta[0][0]), beta=float(cfg["sample"].beta[0][0]),
                energy_keV=float(cfg["spectrum"][0][0]), pixel_um=float(cfg["det_pix_um"]), distance_m=float(cfg["dOD"]),
                magnification=float(cfg["M"]))


def blob_error(thickness, T):
    """max|thickness - bin2(T)| / max T"""
    return float(np.abs(np.asarray(thickness, dtype=np.float64) - bin2(T)).max() / T.max())
