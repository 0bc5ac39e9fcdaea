"""End-to-end accuracy of the phase retrieval on Fil_Nylon_ID17: the truths of one run and the figures the GPU test and
its CPU calibration both compute (tests/test_gpu_retrieval.py)."""
import numpy as np

from tests import _retrieval_oracle as orl


def bin2(a):
    n, m = a.shape
    return a.reshape(n // 2, 2, m // 2, 2).mean(axis=(1, 3))


def truths(Dxreal, Dyreal, T_sample, delta, E_keV):
    """Position 0's padded Dxreal / Dyreal (study pixels) cropped by 15, 2x2-binned and halved -> detector pixels; the true
    phase -k*delta*T of the sample, 2x2-binned."""
    from paresis_amd.getk import k_sample
    c = lambda a: np.asarray(a, dtype=np.float64)[15:-15, 15:-15]
    dx, dy = bin2(c(Dxreal)) / 2, bin2(c(Dyreal)) / 2
    phi = bin2(-k_sample(E_keV) * float(delta) * np.asarray(T_sample, dtype=np.float64))
    return dx, dy, phi


def mask(dx_t, dy_t, margin=3, border=8):
    """Pixels with |D_true| < 1 px that lie more than `margin` pixels from any pixel with |D_true| >= 1 (the wire's edges),
    and `border` pixels inside the frame."""
    bad = (np.abs(dx_t) >= 1) | (np.abs(dy_t) >= 1)
    grown = bad.copy()
    for di in range(-margin, margin + 1):
        for dj in range(-margin, margin + 1):
            grown |= np.roll(np.roll(bad, di, 0), dj, 1)
    ok = ~grown
    ok[:border, :] = False
    ok[-border:, :] = False
    ok[:, :border] = False
    ok[:, -border:] = False
    return ok


def figures(ret, true, ok):
    """Pearson correlation and least-squares slope of retrieved against true inside the mask (both mean-removed)."""
    r = np.asarray(ret, dtype=np.float64)[ok]
    t = np.asarray(true, dtype=np.float64)[ok]
    r = r - r.mean()
    t = t - t.mean()
    return float(np.dot(r, t) / np.sqrt(np.dot(r, r) * np.dot(t, t))), float(np.dot(r, t) / np.dot(t, t))


def evaluate(S, R, Dxreal, Dyreal, T_sample, delta, params):
    """numpy LCS + integration of one bin's stacks -> {'dx': (corr, slope), 'dy': ..., 'phi': ...}."""
    from paresis_amd.retrieval import gradient_scale
    r = orl.lcs(S, R)
    c = gradient_scale(params['energy_keV'], params['pixel_um'], params['distance_m'], params['magnification'])
    phi = orl.integrate(r['dx'].astype(np.float64) * c, r['dy'].astype(np.float64) * c)
    dx_t, dy_t, phi_t = truths(Dxreal, Dyreal, T_sample, delta, params['energy_keV'])
    ok = mask(dx_t, dy_t)
    return {'dx': figures(r['dx'], dx_t, ok), 'dy': figures(r['dy'], dy_t, ok), 'phi': figures(phi, phi_t, ok),
            'npix': int(ok.sum()), 'maxD': float(max(np.abs(dx_t).max(), np.abs(dy_t).max()))}
