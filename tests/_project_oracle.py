"""Float64 numpy oracle of the matched projector pair (include/paresis_hip.h, "the matched projector pair of a plan"): the
forward projector B^T in two independent forms, the back-projector B, SIRT and CGLS on them, and the float32 restatement of
each, the yardstick of the GPU bounds.  Nothing here imports the package's kernels."""
import numpy as np

from tests import _fbp_oracle as fo

SHAPES = fo.SHAPES


def case_angles(A):
    """fo.case_angles with exactly 45 and 135 degrees (the major-axis tie, from either side) after the special ones, where
    A has room for them."""
    th = fo.case_angles(A)
    k = len(fo.SPECIAL_ANGLES)
    if A >= k + 2:
        th[k], th[k + 1] = 45.0, 135.0
    return th


def case_vol(A, n, m, seed=0):
    """A random volume without zeros, float32: smooth structure plus noise."""
    rng = np.random.default_rng(7000 * A + 70 * n + m + seed)
    x = np.linspace(-1, 1, m)
    v = 1.0 + 0.5 * np.cos(3 * x)[None, :, None] * np.sin(2 * x + 0.3)[None, None, :] + rng.uniform(0.1, 1.0, (n, m, m))
    return v.astype(np.float32)


def _center(m, center):
    return float(m // 2 if center is None else center)


def _lit(m, circle):
    return fo.circle_mask(m) if circle else np.ones((m, m), dtype=bool)


# ---- float64 -------------------------------------------------------------------------------------------------------------
def project(vol, theta_deg, center=None, circle=True):
    """B^T vol by scattering: every lit voxel adds w0*v to sample fl and w1*v to fl + 1.  vol [n][m][m] -> [A][n][m]."""
    vol = np.asarray(vol, dtype=np.float64)
    n, m = vol.shape[0], vol.shape[1]
    lit = _lit(m, circle)
    v = vol[:, lit]                                               # [n][V]
    out = np.zeros((len(theta_deg), n, m))
    row = np.arange(n)[:, None] * (m + 2)
    for a, th in enumerate(theta_deg):
        u = fo.grid_u(m, th, _center(m, center))[lit]
        fl = np.floor(u)
        w1 = u - fl
        k = fl.astype(np.int64) + 1                               # into a line padded by one sample on either side
        ok = (k >= 0) & (k <= m)
        k = np.clip(k, 0, m)
        line = np.zeros(n * (m + 2))                              # the n padded lines, flat: add.at's fast path
        np.add.at(line, (row + k).ravel(), np.where(ok, (1 - w1) * v, 0).ravel())
        np.add.at(line, (row + k + 1).ravel(), np.where(ok, w1 * v, 0).ravel())
        out[a] = line.reshape(n, m + 2)[:, 1:-1]
    return out


def project_tent(vol, theta_deg, center=None, circle=True):
    """B^T vol by gathering: sample s is the sum of max(0, 1 - |u - s|) * v over the lit voxels."""
    vol = np.asarray(vol, dtype=np.float64)
    n, m = vol.shape[0], vol.shape[1]
    lit = _lit(m, circle)
    v = vol[:, lit]
    s = np.arange(m, dtype=np.float64)
    out = np.zeros((len(theta_deg), n, m))
    for a, th in enumerate(theta_deg):
        u = fo.grid_u(m, th, _center(m, center))[lit]
        out[a] = v @ np.maximum(0.0, 1.0 - np.abs(u[:, None] - s[None, :]))
    return out


def adjoint(sino, theta_deg, center=None, circle=True):
    """B sino: fo.fbp's back-projection without filter and scale.  sino [A][n][m] -> [n][m][m]."""
    sino = np.asarray(sino, dtype=np.float64)
    A, n, m = sino.shape
    vol = np.zeros((n, m, m))
    for a in range(A):
        vol += fo.sample(sino[a], fo.grid_u(m, theta_deg[a], _center(m, center)))
    return vol * _lit(m, circle)


def matrix(m, theta_deg, center=None, circle=True):
    """The contract's matrix written down directly, in the layout of ops.fbp_project of an identity: [A][m*m][m] float32,
    entry [a][i*m + j][k] the weight of voxel (i, j) on sample k of angle a.  A lit voxel gives float32(1) - w1 to sample
    floor(u) and w1 = float32(u - floor(u)) to sample floor(u) + 1; samples outside [0, m) are dropped."""
    lit = _lit(m, circle).ravel()
    row = np.arange(m * m)
    out = np.zeros((len(theta_deg), m * m, m), dtype=np.float32)
    for a, th in enumerate(theta_deg):
        u = fo.grid_u(m, th, _center(m, center)).ravel()
        fl = np.floor(u)
        w1 = (u - fl).astype(np.float32)
        k = fl.astype(np.int64)
        ok = lit & (k >= 0) & (k < m)
        out[a, row[ok], k[ok]] = np.float32(1) - w1[ok]
        ok = lit & (k + 1 >= 0) & (k + 1 < m)
        out[a, row[ok], k[ok] + 1] = w1[ok]
    return out


def impulses(A, m):
    """[A][A*m][m] float32 with [a][a*m + k][k] = 1: one unit impulse per detector row, so that adjoint's [A*m][m][m]
    holds the back-projector's whole matrix, row a*m + k the column (a, k)."""
    s = np.zeros((A, A * m, m), dtype=np.float32)
    a, k = np.divmod(np.arange(A * m), m)
    s[a, np.arange(A * m), k] = 1
    return s


def as_matrix(vol, A, m):
    """adjoint(impulses) [A*m][m][m] in matrix()'s layout [A][m*m][m]."""
    return np.ascontiguousarray(np.asarray(vol).reshape(A, m, m * m).transpose(0, 2, 1))


def _reciprocal(t):
    return np.where(t > 1e-6, 1.0 / np.where(t > 1e-6, t, 1), 0).astype(t.dtype)


def _sirt(P, Bk, dtype, sino, iterations, nonneg, x0):
    b = np.asarray(sino, dtype=dtype)
    A, n, m = b.shape
    x = np.zeros((n, m, m), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    Rinv, Cinv = _reciprocal(P(np.ones_like(x))), _reciprocal(Bk(np.ones_like(b)))
    for _ in range(iterations):
        x = x + Cinv * Bk(Rinv * (b - P(x)))
        if nonneg:
            x = np.maximum(x, 0)
    return x


def _cgls(P, Bk, dtype, sino, iterations, x0):
    """gamma and |q|^2 per detector row in float64; alpha = beta = 0 for a row where either is 0."""
    b = np.asarray(sino, dtype=dtype)
    A, n, m = b.shape
    x = np.zeros((n, m, m), dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)

    def ratio(num, den):
        ok = (num != 0) & (den != 0)
        return np.where(ok, num / np.where(ok, den, 1), 0).astype(dtype)

    r = b.copy() if x0 is None else b - P(x)
    s = Bk(r)
    p = s.copy()
    gamma = (s.astype(np.float64) ** 2).sum(axis=(1, 2))
    for _ in range(iterations):
        q = P(p)
        alpha = ratio(gamma, (q.astype(np.float64) ** 2).sum(axis=(0, 2)))
        x = x + alpha[:, None, None] * p
        r = r - alpha[None, :, None] * q
        s = Bk(r)
        gamma_new = (s.astype(np.float64) ** 2).sum(axis=(1, 2))
        p = s + ratio(gamma_new, gamma)[:, None, None] * p
        gamma = gamma_new
    return x


def sirt(sino, theta_deg, iterations, center=None, circle=True, nonneg=False, x0=None):
    """x <- x + Cinv * B(Rinv * (b - B^T x)), R = B^T 1, C = B 1, reciprocals where > 1e-6 and 0 elsewhere; float64."""
    return _sirt(lambda v: project(v, theta_deg, center, circle), lambda q: adjoint(q, theta_deg, center, circle),
                 np.float64, sino, iterations, nonneg, x0)


def cgls(sino, theta_deg, iterations, center=None, circle=True, x0=None):
    """Standard CGLS on min |B^T x - b|, every detector row its own problem; float64."""
    return _cgls(lambda v: project(v, theta_deg, center, circle), lambda q: adjoint(q, theta_deg, center, circle),
                 np.float64, sino, iterations, x0)


# ---- the contract in the GPU's number formats ---------------------------------------------------------------------------
def project_f32(vol, theta_deg, center=None, circle=True):
    """u, floor and u - fl in float64, the weights, the products and the sums in float32, in the contract's order: lines of
    the major axis (constant i when |cos| >= |sin|, constant j otherwise), line L into partial sum L & 3, the voxels of a
    line in ascending minor index, the sample (p0 + p1) + (p2 + p3).  (The device fuses each multiply-add; numpy rounds
    the product first: the same error to its order.)"""
    vol = np.asarray(vol, dtype=np.float32)
    n, m = vol.shape[0], vol.shape[1]
    lit = _lit(m, circle)
    out = np.zeros((len(theta_deg), n, m), dtype=np.float32)
    for a, th in enumerate(theta_deg):
        t = np.deg2rad(np.float64(th))
        u = fo.grid_u(m, th, _center(m, center))
        v, ok = vol, lit
        if not abs(np.cos(t)) >= abs(np.sin(t)):                  # lines of constant j: the minor index is i
            u, v, ok = u.T, vol.transpose(0, 2, 1), lit.T
        fl = np.floor(u)
        w1 = (u - fl).astype(np.float32)
        w0 = np.float32(1) - w1
        k = fl.astype(np.int64) + 1
        ok = ok & (k >= 0) & (k <= m)
        k = np.clip(k, 0, m)
        part = np.zeros((4, n, m + 2), dtype=np.float32)
        idx = np.empty(2 * m, dtype=np.int64)
        val = np.empty((n, 2 * m), dtype=np.float32)
        for L in range(m):
            idx[0::2], idx[1::2] = k[L], k[L] + 1                 # voxel q adds to fl, then to fl + 1, before voxel q + 1
            val[:, 0::2] = np.where(ok[L], w0[L] * v[:, L, :], np.float32(0))
            val[:, 1::2] = np.where(ok[L], w1[L] * v[:, L, :], np.float32(0))
            np.add.at(part[L & 3], (slice(None), idx), val)
        out[a] = ((part[0] + part[1]) + (part[2] + part[3]))[:, 1:-1]
    assert out.dtype == np.float32
    return out


def adjoint_f32(sino, theta_deg, center=None, circle=True):
    """float64 u, float32 weights, samples and accumulation in ascending angle: fo.fbp_f32 without filter and scale."""
    sino = np.asarray(sino, dtype=np.float32)
    A, n, m = sino.shape
    vol = np.zeros((n, m, m), dtype=np.float32)
    for a in range(A):
        vol += fo.sample(sino[a], fo.grid_u(m, theta_deg[a], _center(m, center))).astype(np.float32)
    return vol * _lit(m, circle).astype(np.float32)


def sirt_f32(sino, theta_deg, iterations, center=None, circle=True, nonneg=False, x0=None):
    return _sirt(lambda v: project_f32(v, theta_deg, center, circle), lambda q: adjoint_f32(q, theta_deg, center, circle),
                 np.float32, sino, iterations, nonneg, x0)


def cgls_f32(sino, theta_deg, iterations, center=None, circle=True, x0=None):
    return _cgls(lambda v: project_f32(v, theta_deg, center, circle), lambda q: adjoint_f32(q, theta_deg, center, circle),
                 np.float32, sino, iterations, x0)


def dot_mismatch(Px, y, x, By):
    """|<B^T x, y> - <x, B y>| / <B^T x, y>, the sums in float64."""
    lhs = float(np.sum(np.asarray(Px, dtype=np.float64) * np.asarray(y, dtype=np.float64)))
    rhs = float(np.sum(np.asarray(x, dtype=np.float64) * np.asarray(By, dtype=np.float64)))
    return abs(lhs - rhs) / abs(lhs)


def rms_in_circle(vol, truth):
    """rms error inside the inscribed circle over the largest value of the truth."""
    mask = fo.circle_mask(truth.shape[-1])
    d = (np.asarray(vol, dtype=np.float64) - truth)[..., mask]
    return float(np.sqrt(np.mean(d ** 2)) / np.abs(truth).max())


# ---- the measured yardsticks (tests/test_project_host.py reproduces them; the GPU bounds are 8 times these) --------------
# max|project_f32 - project| / max|project| per shape (A, n, m) on case_vol / case_angles: the worst over the two centres
# of fo.case_centers and circle on and off, measured on the CPU
F32_ERROR = {(1, 1, 2): 6.4e-8, (3, 2, 5): 7.3e-8, (7, 1, 64): 1.3e-7, (90, 3, 64): 2.1e-7, (33, 5, 301): 3.8e-7,
             (180, 2, 512): 4.5e-7}

# |<P32 x, y> - <x, B32 y>| / <P32 x, y> of the float32 restatements (P32 = project_f32, B32 = adjoint_f32) with
# x = case_vol, y = fo.case_sino: the worst over the two centres, circle on and off and the seeds 0 and 1
DOT_SHAPES = [(7, 1, 64), (90, 3, 64), (33, 5, 301)]
DOT_F32_ERROR = {(7, 1, 64): 6.3e-9, (90, 3, 64): 2.2e-9, (33, 5, 301): 7.4e-10}

# the solver cases: (A, n, m, which centre of fo.case_centers); the sinogram is project(case_vol) in float64, rounded to
# float32, with row 1 set to zero; 10 iterations
SOLVER_CASES = [(12, 2, 64, 0), (5, 3, 33, 1)]
# max|solver_f32 - solver| / max|solver| per (case, iterations), measured on the CPU.  SIRT is a stationary iteration and
# stays at the projectors' own error.  CGLS is not: the dominant singular value of B^T (the constant mode) is far from the
# rest, its Ritz value converges within a few steps, and from there a float32 Lanczos recurrence loses orthogonality and
# leaves the float64 trajectory by a factor of about 5 per step (6e-7 after 4 steps, 7e-6 after 7, 9e-3 after 10) while
# still converging.  The 10-step figure therefore bounds little; the 4-step one is the check with teeth.
SOLVER_ITERATIONS = (4, 10)
SIRT_F32_ERROR = {((12, 2, 64, 0), 4): 2.2e-7, ((12, 2, 64, 0), 10): 2.7e-7, ((5, 3, 33, 1), 4): 1.8e-7, ((5, 3, 33, 1), 10): 2.3e-7}
CGLS_F32_ERROR = {((12, 2, 64, 0), 4): 6.4e-7, ((12, 2, 64, 0), 10): 8.9e-3, ((5, 3, 33, 1), 4): 7.2e-7, ((5, 3, 33, 1), 10): 1.3e-2}
# the cases of EDGE_SOLVER_CASES (below): SIRT the worse of the clamp on and off, CGLS at the 4-step count only, the one the
# GPU is held to there (its 10-step figures are 2.5e-2 and 1.6e-2)
SIRT_F32_ERROR.update({((12, 2, 64, -3.5), 4): 2.8e-7, ((12, 2, 64, -3.5), 10): 2.6e-7, ((5, 3, 33, -3.5), 4): 1.5e-7,
                       ((5, 3, 33, -3.5), 10): 2.3e-7})
CGLS_F32_ERROR.update({((12, 2, 64, -3.5), 4): 1.1e-6, ((5, 3, 33, -3.5), 4): 1.9e-6})


# ---- the edge cases (tests/test_gpu_tomo_edges.py; the host tests reproduce every figure) -------------------------------
# the matrix cases: every angle of fo.EDGE_ANGLES and every centre of fo.edge_centers at the small sizes (about the 16-voxel
# tile, across the pad-length step); ten angles and four centres at the large ones (about the 64-sample run, three runs)
MATRIX_M = (2, 5, 15, 16, 17, 33)
MATRIX_LARGE_M = (63, 64, 65, 129)
MATRIX_LARGE_ANGLES = fo.EDGE_ANGLES[:8] + (17.3, 44.999999)


def matrix_large_centers(m):
    return (float(m // 2), -3.5, m + 2.75, m / 2 + 7.3)


# the dense cases (A, n, m): m about the tile, the pad-length step and the run, A about the 32-angle chunk, n not a multiple
# of the four-row block; on case_vol / fo.case_sino / fo.edge_angles at the three centres of fo.dense_centers
EDGE_SHAPES = [(31, 4, 15), (32, 7, 16), (33, 8, 17), (64, 9, 31), (65, 1, 32), (63, 3, 33), (5, 6, 63), (6, 2, 65), (4, 5, 127),
               (3, 3, 129)]
# max|project_f32 - project| / max|project| per edge shape: the worst over the three centres and circle on and off
EDGE_F32_ERROR = {(31, 4, 15): 1.3e-7, (32, 7, 16): 1.4e-7, (33, 8, 17): 1.3e-7, (64, 9, 31): 1.7e-7, (65, 1, 32): 1.4e-7,
                  (63, 3, 33): 1.5e-7, (5, 6, 63): 1.7e-7, (6, 2, 65): 2.3e-7, (4, 5, 127): 2.3e-7, (3, 3, 129): 1.9e-7}
# max|adjoint_f32 - adjoint| / max|adjoint|, likewise
EDGE_ADJ_F32_ERROR = {(31, 4, 15): 1.9e-7, (32, 7, 16): 2.3e-7, (33, 8, 17): 2.3e-7, (64, 9, 31): 3.5e-7, (65, 1, 32): 3.7e-7,
                      (63, 3, 33): 4.3e-7, (5, 6, 63): 1.5e-7, (6, 2, 65): 1.4e-7, (4, 5, 127): 1.4e-7, (3, 3, 129): 1.3e-7}
# dot_mismatch of the restatements, likewise and over the seeds 0 and 1
EDGE_DOT_F32_ERROR = {(31, 4, 15): 7.3e-9, (32, 7, 16): 4.7e-9, (33, 8, 17): 5.1e-9, (64, 9, 31): 1.8e-9, (65, 1, 32): 1.1e-8,
                      (63, 3, 33): 6.5e-9, (5, 6, 63): 8.0e-9, (6, 2, 65): 8.0e-9, (4, 5, 127): 1.0e-8, (3, 3, 129): 8.9e-9}

# the solver cases where the guards act: the axis 3.5 samples below the detector, the circle on.  Most rays meet no lit
# voxel (R = 0) and a crescent of lit voxels meets no sample (C = 0); the fourth entry is the centre itself
EDGE_SOLVER_CASES = [(12, 2, 64, -3.5), (5, 3, 33, -3.5)]


def solver_case(A, n, m, which):
    """-> (angles, centre, the float32 sinogram [A][n][m] whose row 1 is zero).  which: an index into fo.case_centers, or
    (a float) the centre itself."""
    theta = np.arange(A) * (180.0 / A)
    center = fo.case_centers(m)[which] if isinstance(which, int) else float(which)
    sino = project(case_vol(A, n, m), theta, center, True).astype(np.float32)
    sino[:, 1, :] = 0
    return theta, center, sino
