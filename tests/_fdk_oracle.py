"""Float64 numpy oracle of the FDK contract (include/paresis_hip.h, "FDK"), its float32 / complex64 restatement (the
yardstick of the GPU parity bound, as tests/_fbp_oracle.py's fbp_f32 is), the analytic ball both test files reconstruct and
the shared parity cases.  Nothing here imports the package's kernels."""
import numpy as np

from tests import _fbp_oracle as fo

FILTERS = fo.FILTERS


def preweight(n, m, center, vcenter, dso):
    """den[r][k] = sqrt((dso^2 + (k - center)^2) + (r - vcenter)^2): p' = p * dso / den."""
    dk = np.arange(m, dtype=np.float64) - center
    dr = np.arange(n, dtype=np.float64) - vcenter
    return np.sqrt((dso * dso + dk * dk)[None, :] + (dr * dr)[:, None])


def geometry(m, theta_deg, dso, side=1):
    """(t, U) [m][m] of one angle: t = dj c - di s, w = dj s + di c, U = dso/(dso + w).  side=-1: the source on the wrong
    side (w -> -w)."""
    h = m // 2
    th = np.deg2rad(np.float64(theta_deg))
    c, s = np.cos(th), np.sin(th)
    i, j = np.mgrid[0:m, 0:m]
    di, dj = (i - h).astype(np.float64), (j - h).astype(np.float64)
    t, w = dj * c - di * s, dj * s + di * c
    return t, dso / (dso + side * w)


def sample2(q, v, u):
    """q [n][m] at (v [n][m][m], u [m][m]): bilinear with the weights fl = floor, w1 = (coord - fl) in q's dtype, w0 = 1 - w1,
    q zero outside the detector, and 0 unless -1 < coord < size on both axes -> [n][m][m] in q's dtype."""
    n, m = q.shape
    qp = np.zeros((n + 2, m + 2), dtype=q.dtype)
    qp[1:-1, 1:-1] = q
    fu, fv = np.floor(u), np.floor(v)
    wu, wv = (u - fu).astype(q.dtype), (v - fv).astype(q.dtype)
    ok = (u > -1) & (u < m) & (v > -1) & (v < n)
    ku = np.clip(fu, -1, m - 1).astype(np.int64) + 1
    kv = np.clip(fv, -1, n - 1).astype(np.int64) + 1
    one = q.dtype.type(1)
    lo = (one - wu) * qp[kv, ku] + wu * qp[kv, ku + 1]
    hi = (one - wu) * qp[kv + 1, ku] + wu * qp[kv + 1, ku + 1]
    return np.where(ok, (one - wv) * lo + wv * hi, q.dtype.type(0))


def _heights(n, vcenter):
    return (np.arange(n, dtype=np.float64) - vcenter)[:, None, None]


def fdk(sino, theta_deg, dso, center=None, vcenter=None, filter="ramp", circle=True, side=1):
    """sino [A][n][m] -> vol [n][m][m], all float64."""
    sino = np.asarray(sino, dtype=np.float64)
    A, n, m = sino.shape
    dso = float(dso)
    center = float(m // 2 if center is None else center)
    vcenter = float((n - 1) / 2.0 if vcenter is None else vcenter)
    q = fo.filter_lines(sino * dso / preweight(n, m, center, vcenter, dso), filter)
    vol = np.zeros((n, m, m))
    for a in range(A):
        t, U = geometry(m, theta_deg[a], dso, side)
        vol += (U * U) * sample2(q[a], _heights(n, vcenter) * U + vcenter, t * U + center)
    vol *= np.pi / (2 * A)
    if circle:
        vol *= fo.circle_mask(m)
    return vol


def filter_lines_f32(sino, filter):
    """The filter in the GPU's number formats (fo.fbp_f32's, restated): complex64 transforms of two rows at a time, the table
    in float64."""
    A, n, m = sino.shape
    if filter == "none":
        return sino
    P = fo.pad_length(m)
    H = fo.filter_response(P, filter)
    He = 0.5 * (H + np.roll(H[::-1], 1)) / P
    npair = (n + 1) // 2
    z = np.zeros((A, npair, P), dtype=np.complex64)
    z.real[:, :, :m] = sino[:, 0::2]
    z.imag[:, :n // 2, :m] = sino[:, 1::2]
    Z = np.fft.fft(z, axis=-1)
    assert Z.dtype == np.complex64
    Z = (Z.real.astype(np.float64) * He).astype(np.float32) + 1j * (Z.imag.astype(np.float64) * He).astype(np.float32)
    y = np.fft.ifft(Z.astype(np.complex64), axis=-1) * np.float32(P)
    assert y.dtype == np.complex64
    q = np.empty((A, n, m), dtype=np.float32)
    q[:, 0::2] = y.real[:, :, :m]
    q[:, 1::2] = y.imag[:, :n // 2, :m]
    return q


def fdk_f32(sino, theta_deg, dso, center=None, vcenter=None, filter="ramp", circle=True):
    """The contract in the GPU's number formats, on the CPU: the pre-weight in float64 rounded to float32, complex64
    transforms, the geometry in float64, float32 weights, samples and accumulation in ascending angle.  Its distance from
    fdk() is what float32 costs at a shape; the GPU parity bound is 8 times that."""
    sino = np.asarray(sino, dtype=np.float32)
    A, n, m = sino.shape
    dso = float(dso)
    center = float(m // 2 if center is None else center)
    vcenter = float((n - 1) / 2.0 if vcenter is None else vcenter)
    q = filter_lines_f32((sino.astype(np.float64) * dso / preweight(n, m, center, vcenter, dso)).astype(np.float32), filter)
    vol = np.zeros((n, m, m), dtype=np.float32)
    for a in range(A):
        t, U = geometry(m, theta_deg[a], dso)
        vol += (U * U).astype(np.float32) * sample2(q[a], _heights(n, vcenter) * U + vcenter, t * U + center)
    vol *= np.float32(np.pi / (2 * A))
    if circle:
        vol *= fo.circle_mask(m)
    assert vol.dtype == np.float32
    return vol


# ---- the analytic ball: a sphere of density 1 off the axis and off the mid-plane ------------------------------------------
# FDK is exact in the mid-plane only: at height z the reconstructed density falls short by about (z/dso)^2 (measured on this
# oracle: -1.0e-3 at z = 6, -4.3e-3 at z = 12, dso = 192, against (z/dso)^2 = 9.8e-4, 3.9e-3).  The parallel reconstruction the
# ball is compared with is off by a few 1e-4 in a slice's mean at m = 64, so the ball is kept low: its interior (radius
# R - 2 = 4 about height 1.5) has a mean z^2 of cz^2 + (R - 2)^2/5 = 5.45, a mean deficit of about 5.45/192^2 = 1.5e-4.
BALL_M, BALL_N, BALL_ANGLES = 64, 24, 120
BALL_DSO = 3.0 * BALL_M
BALL = dict(ci=27.0, cj=41.5, cz=1.5, R=6.0)          # centre (slice row, slice column, height above the optical axis), radius


def full_turn(A):
    return np.arange(A, dtype=np.float64) * (360.0 / A)


def ball_center(m, theta_deg, ball=BALL):
    """(t, w, z) of the ball's centre at an angle."""
    h = m // 2
    th = np.deg2rad(np.float64(theta_deg))
    c, s = np.cos(th), np.sin(th)
    di, dj = ball['ci'] - h, ball['cj'] - h
    return dj * c - di * s, dj * s + di * c, ball['cz']


def ball_cone_sino(A=BALL_ANGLES, n=BALL_N, m=BALL_M, dso=BALL_DSO, ball=BALL):
    """The chord of every ray of a full turn through the ball, in closed form: the ray from the source (0, -dso, 0) through
    the virtual detector's point (t0, 0, z0), t0 = k - m // 2, z0 = r - (n - 1)/2; chord = 2 sqrt(R^2 - d^2), d the distance
    of the ball's centre from the ray.  float64 [A][n][m]."""
    t0 = (np.arange(m, dtype=np.float64) - m // 2)[None, :]
    z0 = (np.arange(n, dtype=np.float64) - (n - 1) / 2.0)[:, None]
    norm = np.sqrt(t0 * t0 + z0 * z0 + dso * dso)
    out = np.empty((A, n, m))
    for a, th in enumerate(full_turn(A)):
        tc, wc, zc = ball_center(m, th, ball)
        along = (tc * t0 + (wc + dso) * dso + zc * z0) / norm            # the centre's coordinate along the ray
        d2 = tc * tc + (wc + dso) ** 2 + zc * zc - along * along
        out[a] = 2.0 * np.sqrt(np.clip(ball['R'] ** 2 - d2, 0.0, None))
    return out


def ball_parallel_sino(A=60, n=BALL_N, m=BALL_M, ball=BALL):
    """The same ball's parallel chords at A angles on a half turn -> (sino [A][n][m], the angles)."""
    theta = np.arange(A, dtype=np.float64) * (180.0 / A)
    t0 = (np.arange(m, dtype=np.float64) - m // 2)[None, :]
    z0 = (np.arange(n, dtype=np.float64) - (n - 1) / 2.0)[:, None]
    out = np.empty((A, n, m))
    for a, th in enumerate(theta):
        tc, _, zc = ball_center(m, th, ball)
        out[a] = 2.0 * np.sqrt(np.clip(ball['R'] ** 2 - (t0 - tc) ** 2 - (z0 - zc) ** 2, 0.0, None))
    return out, theta


def ball_interior(n=BALL_N, m=BALL_M, ball=BALL, inset=2.0):
    """The voxels at least `inset` inside the ball, [n][m][m] bool; slice Z lies at height Z - (n - 1)/2."""
    z, i, j = np.mgrid[0:n, 0:m, 0:m].astype(np.float64)
    d2 = (i - ball['ci']) ** 2 + (j - ball['cj']) ** 2 + (z - (n - 1) / 2.0 - ball['cz']) ** 2
    return d2 <= (ball['R'] - inset) ** 2


def ball_error(vol):
    """|mean over the ball's interior - 1|."""
    return abs(float(np.asarray(vol, dtype=np.float64)[ball_interior()].mean()) - 1.0)


# ---- the parity cases of tests/test_gpu_fdk.py (shared with the host test that measures the float32 yardstick) ------------
# (A, n, m): the smallest, odd sizes, several tiles; (5, 9, 17) is one slice past the back-projector's block of 8 slices and
# one column past its 16 x 16 tile
SHAPES = [(1, 1, 2), (3, 2, 5), (8, 3, 17), (36, 5, 33), (60, 9, 64), (5, 9, 17)]
DSO_FACTORS = (1.0, 2.5, 1e6)                       # dso = factor * m


def case_angles(A):
    """A angles over the full turn whose first entries are exactly 0, 90, -30 and 270 degrees (as many as fit)."""
    th = np.arange(A, dtype=np.float64) * (360.0 / A) + 0.37
    k = min(A, len(fo.SPECIAL_ANGLES))
    th[:k] = fo.SPECIAL_ANGLES[:k]
    return th


def smooth_sino(A, n, m):
    """A smooth sinogram that vanishes towards the detector's ends: a Gaussian bump that wanders with the angle, float32.
    On it the geometry's own difference between dso = 1e6 m and the parallel beam (u moves by up to m/2 * 0.7e-6 m samples)
    stays at a third of the parity bound (measured on the oracles: 8e-7 and 1.2e-6 of the peak at (36, 5, 33) and
    (60, 9, 64)); on fo.case_sino, whose filtered lines jump from sample to sample, it does not (up to 1.5e-5; tests/test_gpu_fdk.py takes it to 1e8 m)."""
    k = np.arange(m)[None, None, :]
    r = np.arange(n)[None, :, None]
    a = np.arange(A)[:, None, None]
    return ((1.0 + 0.1 * r + 0.2 * np.cos(0.7 * a)) * np.exp(-((k - 0.45 * m - 0.1 * m * np.sin(0.5 * a)) / (0.12 * m)) ** 2)).astype(np.float32)


def case_vcenters(n):
    return ((n - 1) / 2.0, 0.3, -4.0)


# max|fdk_f32 - fdk| / max|fdk| per (shape, dso factor): the worst over the three filters, the three optical rows of
# case_vcenters and the two centres of fo.case_centers, circle off, on fo.case_sino / case_angles -- measured with numpy's
# float32 pocketfft on the CPU (tests/test_cone_host.py reproduces them).  The GPU parity bound is 8 times these.
F32_ERROR = {
    ((1, 1, 2), 1.0): 1.1e-7, ((1, 1, 2), 2.5): 1.2e-7, ((1, 1, 2), 1e6): 2.2e-7,
    ((3, 2, 5), 1.0): 1.4e-7, ((3, 2, 5), 2.5): 1.3e-7, ((3, 2, 5), 1e6): 1.5e-7,
    ((8, 3, 17), 1.0): 2.1e-7, ((8, 3, 17), 2.5): 2.0e-7, ((8, 3, 17), 1e6): 1.9e-7,
    ((36, 5, 33), 1.0): 3.7e-7, ((36, 5, 33), 2.5): 3.4e-7, ((36, 5, 33), 1e6): 3.4e-7,
    ((60, 9, 64), 1.0): 4.4e-7, ((60, 9, 64), 2.5): 4.5e-7, ((60, 9, 64), 1e6): 4.1e-7,
    ((5, 9, 17), 1.0): 2.2e-7, ((5, 9, 17), 2.5): 2.0e-7, ((5, 9, 17), 1e6): 1.8e-7,
}


def f32_error(shape, factor):
    """max|fdk_f32 - fdk| / max|fdk| over the cases F32_ERROR is the worst of."""
    A, n, m = shape
    sino, angles = fo.case_sino(A, n, m), case_angles(A)
    worst = 0.0
    for filt in FILTERS:
        for vc in case_vcenters(n):
            for c in fo.case_centers(m):
                ref = fdk(sino, angles, factor * m, c, vc, filt, False)
                worst = max(worst, float(np.abs(fdk_f32(sino, angles, factor * m, c, vc, filt, False) - ref).max() / np.abs(ref).max()))
    return worst
