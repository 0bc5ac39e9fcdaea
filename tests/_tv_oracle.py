"""Float64 numpy oracle of total-variation reconstruction on the matched projector pair (include/paresis_hip.h, "the voxel
step of total-variation reconstruction"; paresis_amd.tomography.tv): the masks and the difference operators, the voxel
step, the primal-dual solver on _project_oracle.project / adjoint, the objective, and the float32 restatement of each on
project_f32 / adjoint_f32, the yardstick of the GPU bounds.  Nothing here imports the package's kernels."""
import numpy as np

from tests import _fbp_oracle as fo
from tests import _project_oracle as po


# ---- masks and differences -----------------------------------------------------------------------------------------------
def masks(m, circle):
    """-> (lit, ax, ay, deg): the circle mask, the active differences along i and along j (bool [m][m]) and the number of
    active differences every voxel takes part in (int, 0 to 4)."""
    lit = fo.circle_mask(m) if circle else np.ones((m, m), dtype=bool)
    ax, ay = np.zeros((m, m), dtype=bool), np.zeros((m, m), dtype=bool)
    ax[:-1, :] = lit[:-1, :] & lit[1:, :]
    ay[:, :-1] = lit[:, :-1] & lit[:, 1:]
    deg = ax.astype(int) + ay.astype(int)
    deg[1:, :] += ax[:-1, :]
    deg[:, 1:] += ay[:, :-1]
    return lit, ax, ay, deg


def grad(x, ax, ay):
    """The forward differences of [..., m, m] along i and j, 0 where the difference is not active."""
    gx, gy = np.zeros_like(x), np.zeros_like(x)
    gx[..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
    gy[..., :, :-1] = x[..., :, 1:] - x[..., :, :-1]
    return gx * ax, gy * ay


def grad_t(px, py, ax, ay):
    """grad's transpose: ((px[i-1][j] - px[i][j]) + py[i][j-1]) - py[i][j], the inactive differences' terms 0, in this order."""
    a, b = px * ax, py * ay
    up, left = np.zeros_like(a), np.zeros_like(b)
    up[..., 1:, :] = a[..., :-1, :]
    left[..., :, 1:] = b[..., :, :-1]
    return ((up - a) + left) - b


# ---- the voxel step -------------------------------------------------------------------------------------------------------
def step(dtype, lam, nonneg, circle, u, c, x, xbar, px, py):
    """One voxel step in `dtype` (np.float64: the oracle; np.float32: the contract's formats and order, each product rounded
    where the device fuses it) -> (x', xbar', px', py', info); info holds the fraction of the active differences whose voxel
    was projected ('saturated') and the fraction of the lit voxels whose step went below 0 ('clamped', counted with or
    without nonneg)."""
    u, c, x, xbar, px, py = (np.asarray(v, dtype=dtype) for v in (u, c, x, xbar, px, py))
    m = x.shape[-1]
    lit, ax, ay, deg = masks(m, circle)
    lam, half = dtype(lam), dtype(0.5)
    gx, gy = grad(xbar, ax, ay)
    tx, ty = px + half * gx, py + half * gy
    nr = np.sqrt(tx * tx + ty * ty)
    sat = nr > lam
    s = np.where(sat, lam / np.where(sat, nr, 1), 1).astype(dtype)
    pxn, pyn = np.where(sat, tx * s, tx), np.where(sat, ty * s, ty)
    cd = c + deg.astype(dtype)
    tau = np.where(cd > dtype(1e-6), dtype(1) / np.where(cd > dtype(1e-6), cd, 1), 0).astype(dtype)
    xn = x - tau * (u + grad_t(pxn, pyn, ax, ay))
    active = int(ax.sum() + ay.sum()) * int(np.prod(x.shape[:-2], dtype=int))
    info = {"saturated": float((sat & ax).sum() + (sat & ay).sum()) / max(active, 1),
            "clamped": float((xn < 0)[..., lit].mean())}
    if nonneg:
        xn = np.maximum(xn, 0)
    out = (xn, dtype(2) * xn - x, pxn, pyn)
    assert all(v.dtype == dtype for v in out)
    return out + (info,)


def step_f64(*args):
    return step(np.float64, *args)


def step_f32(*args):
    return step(np.float32, *args)


# the step's cases on the GPU: tests/test_gpu_tv.py
STEP_TILE = (8, 32)                                     # the kernel's tile (rows i, columns j)
STEP_M = (2, 5, 7, 8, 9, 31, 32, 33, 64, 301)           # the issue's sizes, and one below, at and above either tile edge
STEP_N = (1, 2, 5)
LAMBDA_KINDS = ("zero", "middle", "large")


def step_case(n, m, circle, kind):
    """Random state for one call, float32 -> (lambda, u, c, x, xbar, px, py).  It holds a flat patch of xbar (the voxels
    with i, j <= m // 2: gx = gy = 0 exactly inside it), voxels of that patch whose p is exactly on the bound ((lambda, 0)
    and (0, -lambda): nr == lambda, not projected), voxels with c = 0 inside and outside the circle, and x and u of both
    signs.  kind 'zero': lambda = 0; 'middle': the median of nr over the voxels with an active difference, so about half
    saturate; 'large': four times the largest nr, so nothing does."""
    rng = np.random.default_rng(100000 * n + 100 * m + 10 * int(circle) + LAMBDA_KINDS.index(kind))
    shape = (n, m, m)
    u = rng.uniform(-1, 1, shape).astype(np.float32)
    c = rng.uniform(0.2, 3.0, shape).astype(np.float32)
    i, j = np.mgrid[0:m, 0:m]
    c[:, (i + 2 * j) % 5 == 0] = 0
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    xbar = (x + rng.uniform(-0.5, 0.5, shape)).astype(np.float32)
    patch = (i <= m // 2) & (j <= m // 2)
    xbar[:, patch] = np.float32(0.75)
    px, py = rng.uniform(-1, 1, shape).astype(np.float32), rng.uniform(-1, 1, shape).astype(np.float32)
    _, ax, ay, _ = masks(m, circle)
    gx, gy = grad(xbar, ax, ay)
    tx, ty = px + np.float32(0.5) * gx, py + np.float32(0.5) * gy
    nr = np.sqrt(tx.astype(np.float64) ** 2 + ty.astype(np.float64) ** 2)
    lam = {"zero": 0.0, "middle": float(np.float32(np.median(nr[:, ax | ay]))), "large": float(np.float32(4 * nr.max()))}[kind]
    inner = (i < m // 2) & (j < m // 2)                 # both differences of these voxels stay inside the patch
    on_x, on_y = inner & ((i + j) % 2 == 0), inner & ((i + j) % 2 == 1)
    px[:, on_x], py[:, on_x] = np.float32(lam), 0
    px[:, on_y], py[:, on_y] = 0, np.float32(-lam)
    return lam, u, c, x, xbar, px, py


# ---- the solver -----------------------------------------------------------------------------------------------------------
def _tv(P, Bk, dtype, sino, iterations, lam, circle, nonneg, x0, info=None):
    b = np.asarray(sino, dtype=dtype)
    A, n, m = b.shape
    x = np.zeros((n, m, m), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    xbar, y = x.copy(), np.zeros_like(b)
    px, py = np.zeros_like(x), np.zeros_like(x)
    s1, c = po._reciprocal(P(np.ones_like(x))), Bk(np.ones_like(b))
    den = dtype(1) + s1
    for _ in range(iterations):
        y = (y + s1 * (P(xbar) - b)) / den
        x, xbar, px, py, last = step(dtype, lam, nonneg, circle, Bk(y), c, x, xbar, px, py)
        if info is not None:
            info.append(last)
    assert x.dtype == dtype
    return x


def tv(sino, theta_deg, iterations, lam, center=None, circle=True, nonneg=False, x0=None, info=None):
    """The primal-dual hybrid gradient method with Pock and Chambolle's diagonal preconditioners (alpha = 1) on
    min 0.5 |B^T x - b|^2 + lam TV(x): s1 = 1/R, R = B^T 1; 1/2 for the TV dual; tau = 1/(C + deg), C = B 1; float64.
    info: a list that receives every step's info."""
    return _tv(lambda v: po.project(v, theta_deg, center, circle), lambda q: po.adjoint(q, theta_deg, center, circle),
               np.float64, sino, iterations, lam, circle, nonneg, x0, info)


def tv_f32(sino, theta_deg, iterations, lam, center=None, circle=True, nonneg=False, x0=None, info=None):
    return _tv(lambda v: po.project_f32(v, theta_deg, center, circle), lambda q: po.adjoint_f32(q, theta_deg, center, circle),
               np.float32, sino, iterations, lam, circle, nonneg, x0, info)


def objective(vol, sino, theta_deg, lam, center=None, circle=True):
    """0.5 |B^T vol - b|^2 + lam TV(vol) per detector row, float64 [n]."""
    vol = np.asarray(vol, dtype=np.float64)
    _, ax, ay, _ = masks(vol.shape[-1], circle)
    gx, gy = grad(vol, ax, ay)
    r = po.project(vol, theta_deg, center, circle) - np.asarray(sino, dtype=np.float64)
    return 0.5 * (r ** 2).sum(axis=(0, 2)) + lam * np.sqrt(gx ** 2 + gy ** 2).sum(axis=(1, 2))


# ---- the solver's cases and the measured yardsticks (tests/test_tv_host.py reproduces them; the GPU bounds are 8 times these)
SOLVER_ITERATIONS = (4, 10, 30)
SOLVER_SETTINGS = ((0.3, True), (0.0, False))           # (lambda, nonneg)


def solver_case(A, n, m, which):
    """po.solver_case's angles and centre with the sinogram of case_vol - 1.5, which has both signs, so that the clamp
    acts: project(case_vol - 1.5) in float64, rounded to float32, row 1 set to zero."""
    theta = np.arange(A) * (180.0 / A)
    center = fo.case_centers(m)[which]
    sino = po.project(po.case_vol(A, n, m).astype(np.float64) - 1.5, theta, center, True).astype(np.float32)
    sino[:, 1, :] = 0
    return theta, center, sino


# max|tv_f32 - tv| / max|tv| per (case, iterations, (lambda, nonneg)), measured on the CPU.  The iteration is a contraction
# towards the minimiser, not a stationary recurrence of the data alone: the error grows slowly with the count and stays at
# a few units of float32's last place.  With (0.3, True) nothing is saturated after 4 iterations (that count exercises the
# clamp alone); after 10 and 30, 0.07 to 0.16 of the differences of the whole stack are, and 0.29 to 0.49 of its lit voxels
# are clamped (the zero row included, which has neither).
_A, _B = (12, 2, 64, 0), (5, 3, 33, 1)
TV_F32_ERROR = {(_A, 4, (0.3, True)): 9.8e-8, (_A, 10, (0.3, True)): 2.5e-7, (_A, 30, (0.3, True)): 1.4e-6,
                (_A, 4, (0.0, False)): 1.4e-7, (_A, 10, (0.0, False)): 2.4e-7, (_A, 30, (0.0, False)): 3.6e-7,
                (_B, 4, (0.3, True)): 1.1e-7, (_B, 10, (0.3, True)): 2.5e-7, (_B, 30, (0.3, True)): 6.9e-7,
                (_B, 4, (0.0, False)): 1.4e-7, (_B, 10, (0.0, False)): 1.5e-7, (_B, 30, (0.0, False)): 3.9e-7}


# ---- few angles -----------------------------------------------------------------------------------------------------------
def phantom_truth(m=64, pixel_um=500.0):
    """The delta-weighted phantom slice of the few-angle tests, in units of the support's delta."""
    return np.einsum("kij,k->ij", fo.phantom_slices(m, pixel_um).astype(np.float64), np.array(fo.PHANTOM_DELTA) / 1.62e-7)


FEW_ANGLES = np.arange(12) * 15.0
