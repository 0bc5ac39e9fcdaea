"""Float64 numpy oracle of the filtered back-projection contract (include/paresis_hip.h, "filtered back-projection"), its
float32 / complex64 restatement (the yardstick of the GPU parity bound), and the restated contrast phantom the host tests
reconstruct.  Nothing here imports the package's kernels."""
import numpy as np

FILTERS = ("ramp", "hann", "none")


def pad_length(m):
    return max(64, 1 << int(np.ceil(np.log2(2 * m))))


def ramp_kernel(P):
    """f[0] = 1/4, f[j] = -1/(pi*jj)^2 for odd jj = min(j, P - j), 0 otherwise."""
    j = np.arange(P)
    jj = np.minimum(j, P - j)
    f = np.zeros(P)
    f[0] = 0.25
    odd = jj % 2 == 1
    f[odd] = -1.0 / (np.pi * jj[odd]) ** 2
    return f


def filter_response(P, name):
    if name == "none":
        return np.ones(P)
    H = 2.0 * np.real(np.fft.fft(ramp_kernel(P)))
    if name == "hann":
        H = H * np.fft.fftshift(np.hanning(P))
    elif name != "ramp":
        raise ValueError(name)
    return H


def filter_lines(sino, name):
    """q = Re IFFT_P(FFT_P(line zero-padded to P) * H)[:m] along the last axis, float64."""
    sino = np.asarray(sino, dtype=np.float64)
    m = sino.shape[-1]
    P = pad_length(m)
    H = filter_response(P, name)
    return np.real(np.fft.ifft(np.fft.fft(sino, n=P, axis=-1) * H, axis=-1))[..., :m]


def sample(q, u):
    """q (..., m) at the positions u (any shape) by linear interpolation with q[-1] = q[m] = 0, 0 beyond: -> (..., *u.shape)."""
    m = q.shape[-1]
    qp = np.concatenate([np.zeros(q.shape[:-1] + (1,), q.dtype), q, np.zeros(q.shape[:-1] + (1,), q.dtype)], axis=-1)
    fl = np.floor(u)
    w = u - fl
    k = fl.astype(np.int64) + 1                       # index into qp of sample floor(u)
    ok = (k >= 0) & (k <= m)                          # floor(u) in [-1, m - 1]
    k = np.clip(k, 0, m)
    w = w.astype(q.dtype)
    return np.where(ok, (1 - w) * qp[..., k] + w * qp[..., k + 1], 0)


def grid_u(m, theta_deg, center):
    """u[i][j] of one angle, float64."""
    h = m // 2
    th = np.deg2rad(np.float64(theta_deg))
    i, j = np.mgrid[0:m, 0:m]
    return (j - h) * np.cos(th) - (i - h) * np.sin(th) + center


def circle_mask(m):
    h = m // 2
    i, j = np.mgrid[0:m, 0:m]
    return (i - h) ** 2 + (j - h) ** 2 <= h * h


def fbp(sino, theta_deg, center=None, filter="ramp", circle=True):
    """sino [A][n][m] -> vol [n][m][m], all float64."""
    sino = np.asarray(sino, dtype=np.float64)
    A, n, m = sino.shape
    center = float(m // 2 if center is None else center)
    q = filter_lines(sino, filter)
    vol = np.zeros((n, m, m))
    for a in range(A):
        vol += sample(q[a], grid_u(m, theta_deg[a], center))
    vol *= np.pi / (2 * A)
    if circle:
        vol *= circle_mask(m)
    return vol


def fbp_f32(sino, theta_deg, center=None, filter="ramp", circle=True):
    """The contract in the GPU's number formats, on the CPU: complex64 transforms of two lines at a time, the filter and u
    in float64, float32 weights, samples and accumulation in ascending angle.  Its distance from fbp() is what float32
    costs at a shape; the GPU parity bound is 8 times that."""
    sino = np.asarray(sino, dtype=np.float32)
    A, n, m = sino.shape
    center = float(m // 2 if center is None else center)
    if filter == "none":
        q = sino
    else:
        P = pad_length(m)
        H = filter_response(P, filter)
        He = 0.5 * (H + np.roll(H[::-1], 1)) / P
        npair = (n + 1) // 2
        z = np.zeros((A, npair, P), dtype=np.complex64)
        z.real[:, :, :m] = sino[:, 0::2]
        z.imag[:, :n // 2, :m] = sino[:, 1::2]
        Z = np.fft.fft(z, axis=-1)
        assert Z.dtype == np.complex64
        Z = (Z.real.astype(np.float64) * He).astype(np.float32) + 1j * (Z.imag.astype(np.float64) * He).astype(np.float32)
        y = np.fft.ifft(Z.astype(np.complex64), axis=-1) * np.float32(P)            # numpy's inverse divides by P itself
        assert y.dtype == np.complex64
        q = np.empty((A, n, m), dtype=np.float32)
        q[:, 0::2] = y.real[:, :, :m]
        q[:, 1::2] = y.imag[:, :n // 2, :m]
    vol = np.zeros((n, m, m), dtype=np.float32)
    for a in range(A):
        vol += sample(q[a], grid_u(m, theta_deg[a], center)).astype(np.float32)
    vol *= np.float32(np.pi / (2 * A))
    if circle:
        vol *= circle_mask(m)
    return vol


# delta at 52 keV of the contrast phantom's 13 materials in the order of the ID17 phantom's myMaterials: the stand-ins of
# tests/test_gpu_phantom.py (ID17_DELTA_BETA_52KEV), copied
PHANTOM_DELTA = (1.62e-7, 1.45e-7, 1.55e-7, 8.7e-8, 8.1e-8, 9.6e-8, 8.5e-8, 9.2e-8, 1.40e-7, 8.9e-8, 1.0e-10, 1.0e-10, 8.7e-8)

# max|fbp_f32 - fbp| / max|fbp| per parity shape (A, n, m): the worst over the three filters and the two centres of
# fo.case_centers, circle off, on fo.case_sino / fo.case_angles -- measured with numpy's float32 pocketfft on the CPU.
# The GPU parity bound of tests/test_gpu_fbp.py is 8 times these.
F32_ERROR = {(1, 1, 2): 5.5e-8, (3, 2, 5): 9.8e-8, (7, 1, 64): 1.6e-7, (90, 3, 64): 5.2e-7, (33, 5, 301): 3.9e-7,
             (180, 2, 512): 9.5e-7}


# ---- the parity cases of tests/test_gpu_fbp.py (shared with the host test that measures the float32 yardstick) ----------
SHAPES = [(1, 1, 2), (3, 2, 5), (7, 1, 64), (90, 3, 64), (33, 5, 301), (180, 2, 512)]
SPECIAL_ANGLES = (0.0, 90.0, -30.0, 270.0)


def case_angles(A):
    """A angles over [0, 180) whose first entries are exactly 0, 90, -30 and 270 degrees (as many as fit)."""
    th = np.arange(A, dtype=np.float64) * (180.0 / A) + 0.37
    k = min(A, len(SPECIAL_ANGLES))
    th[:k] = SPECIAL_ANGLES[:k]
    return th


def case_sino(A, n, m, seed=0):
    """A random sinogram without zeros: smooth structure plus noise, float32."""
    rng = np.random.default_rng(1000 * A + 10 * n + m + seed)
    x = np.linspace(-1, 1, m)
    s = 1.0 + 0.5 * np.cos(3 * x)[None, None, :] + rng.uniform(0.1, 1.0, (A, n, m))
    return s.astype(np.float32)


def case_centers(m):
    return (float(m // 2), m / 2 - 0.25)


# ---- the edge cases: off-centre axes, sizes about the tiles, every quadrant (tests/test_gpu_tomo_edges.py) --------------
# the axes and the ties of all four quadrants, negative angles, a hair either side of a tie and of an axis, more than a turn
# (3645 = 10 * 360 + 45), then three ordinary ones
EDGE_ANGLES = (0.0, 45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0, 360.0, -45.0, -90.0, -180.0, 44.999999, 45.000001, 1e-9,
               89.999999999, 3645.0, -30.0, 17.3, 101.9)


def edge_angles(A):
    """The first A of EDGE_ANGLES; a larger A continues over the whole turn, [0, 360)."""
    th = np.arange(A, dtype=np.float64) * (360.0 / A) + 0.37
    k = min(A, len(EDGE_ANGLES))
    th[:k] = EDGE_ANGLES[:k]
    return th


FAR_CENTERS = 3          # the last three of edge_centers: nothing reaches the detector


def edge_centers(m):
    """The two of case_centers, an axis on the first sample, off the detector on either side, on the last sample and well
    off the middle; then three (FAR_CENTERS) from which no voxel reaches the detector: |u - center| <= sqrt(2) * (m // 2)
    < m, so every u is beyond m at 3m and far beyond either end at +-2^20, the largest the contract admits."""
    return (float(m // 2), m / 2 - 0.25, 0.0, -3.5, m - 1.0, m + 2.75, m / 2 + 7.3, 3.0 * m, 2.0 ** 20, -2.0 ** 20)


def dense_centers(m):
    """The three truncating centres of the dense edge cases: off the detector's low end, on its last sample, off the middle."""
    return (-3.5, m - 1.0, m / 2 + 7.3)


# the filtered edge cases: m one below, at and above the pad-length step (P = 64, 64, 128) and the 64-sample run, A one above
# the 32-angle chunk
EDGE_FBP_SHAPES = [(33, 7, 31), (33, 7, 32), (33, 7, 33), (9, 7, 64), (9, 7, 65)]
# max|fbp_f32 - fbp| / max|fbp| per edge shape on case_sino / edge_angles: the worst over the three filters and the three
# centres of dense_centers, circle off, measured on the CPU as F32_ERROR was (tests/test_fbp_host.py reproduces them)
EDGE_F32_ERROR = {(33, 7, 31): 2.9e-7, (33, 7, 32): 3.0e-7, (33, 7, 33): 2.9e-7, (9, 7, 64): 1.9e-7, (9, 7, 65): 2.0e-7}


# ---- the contrast phantom restated (Samples/generateContrastPhantom.py, csrc/phantom.hip) ----------------------------
TUBES_CENTERS0 = [[22, 7], [16.4, 4.7], [10, 7], [6, 12.5], [6, 19.5], [10, 25], [16.4, 27], [22, 25], [21, 16], [11, 16],
                  [16, 11], [16, 21]]


def phantom_slices(dimY, pixsize_um):
    """The 13 indicator slices [13][dimY][dimY] (12 tubes, then the support minus the tubes), phantom_scalars' centres and
    windows, in_disc's strict inequality."""
    pix = pixsize_um / 1000
    r, R = 2 / pix, 15 / pix
    rint, Rint = int(np.floor(r) + 2), int(np.floor(R) + 2)
    origin = dimY / 2 - 16 / pix
    centres = np.asarray(TUBES_CENTERS0, dtype=np.float64) / pix + origin
    i, j = np.mgrid[0:dimY, 0:dimY]
    out = np.zeros((13, dimY, dimY), dtype=bool)
    for t in range(12):
        ci, cj = centres[t]
        ii, ij = int(np.round(ci)), int(np.round(cj))
        win = (i >= ii - rint) & (i < ii + rint) & (j >= ij - rint) & (j < ij + rint)
        out[t] = win & ((i - ci) ** 2 + (j - cj) ** 2 < r ** 2)
    c = dimY / 2
    ic = int(np.round(c))
    end = int(np.round(27 / pix + origin))
    win = (i >= ic - Rint) & (i < max(end, ic - Rint)) & (j >= ic - Rint) & (j < ic + Rint)
    out[12] = win & ((i - c) ** 2 + (j - c) ** 2 < R ** 2) & ~out[:12].any(axis=0)
    return out


def radon_line(img, theta_deg):
    """k_phantom_lines' map: line[c] = sum_r bilinear(img) at column cos*c + sin*r + off_x, row -sin*c + cos*r + off_y, zero
    outside (skimage radon(img, [theta], circle=True))."""
    m = img.shape[0]
    th = np.deg2rad(np.float64(theta_deg))
    co, si = np.cos(th), np.sin(th)
    ctr = m // 2
    offx, offy = -ctr * (co + si - 1), -ctr * (co - si - 1)
    r, c = np.mgrid[0:m, 0:m]
    x = co * c + si * r + offx
    y = -si * c + co * r + offy
    pad = np.zeros((m + 2, m + 2))
    pad[1:-1, 1:-1] = img
    fx, fy = np.floor(x), np.floor(y)
    dx, dy = x - fx, y - fy
    ix, iy = fx.astype(np.int64) + 1, fy.astype(np.int64) + 1
    ok = (ix >= 0) & (ix <= m) & (iy >= 0) & (iy <= m)
    ix, iy = np.clip(ix, 0, m), np.clip(iy, 0, m)
    v = (1 - dy) * ((1 - dx) * pad[iy, ix] + dx * pad[iy, ix + 1]) + dy * ((1 - dx) * pad[iy + 1, ix] + dx * pad[iy + 1, ix + 1])
    return np.where(ok, v, 0.0).sum(axis=0)


def interior(mask):
    """The pixels of a boolean slice whose four neighbours are in it too."""
    m = mask.copy()
    m[1:] &= mask[:-1]
    m[:-1] &= mask[1:]
    m[:, 1:] &= mask[:, :-1]
    m[:, :-1] &= mask[:, 1:]
    return m
