"""Float64 numpy oracle of the labelled-voxel-volume contract (include/paresis_hip.h, "labelled voxel volume"), and the
shared cases of tests/test_volume_host.py and tests/test_gpu_volume.py.  Nothing here imports the package's kernels.

numpy evaluates a * b + c as two rounded operations, which is the contract's "every product and sum rounded on its own";
the sum over r is an explicit ascending loop."""
import numpy as np


def scalars(m, angle_deg):
    """(cos, sin, c, off_x, off_y) by phantom_scalars' expressions."""
    th = np.deg2rad(np.asarray([angle_deg], dtype=np.float64))[0]
    co, si = np.cos(th), np.sin(th)
    c = m // 2
    return float(co), float(si), c, float(-c * (co + si - 1)), float(-c * (co - si - 1))


def rows(n, dimX, s):
    """z of every study row x: n // 2 + floor((x - dimX // 2) * s + 0.5), as int64 (may lie outside [0, n))."""
    x = np.arange(dimX, dtype=np.int64)
    return n // 2 + np.floor((x - dimX // 2).astype(np.float64) * s + 0.5).astype(np.int64)


def slice_lines(sl, nmat, angle_deg, dimY, s):
    """lines[k][y] of one m x m label slice: the contract's line integral, float64 [nmat][dimY]."""
    m = sl.shape[0]
    co, si, c, offx, offy = scalars(m, angle_deg)
    y = np.arange(dimY, dtype=np.int64)
    cpos = (y - dimY // 2).astype(np.float64) * s + float(c)
    pad = np.zeros((m + 2, m + 2), dtype=np.int64)                 # label 0 around the slice
    pad[1:-1, 1:-1] = sl
    acc = np.zeros((nmat, dimY))
    for r in range(m):
        X = co * cpos + si * float(r) + offx
        Y = (-si * cpos) + co * float(r) + offy
        minr, minc = np.floor(Y).astype(np.int64), np.floor(X).astype(np.int64)
        maxr, maxc = np.ceil(Y).astype(np.int64), np.ceil(X).astype(np.int64)
        dr, dc = Y - minr, X - minc

        def at(i, j):
            ok = (i >= 0) & (i < m) & (j >= 0) & (j < m)
            return np.where(ok, pad[np.clip(i, -1, m) + 1, np.clip(j, -1, m) + 1], 0)

        l00, l01, l10, l11 = at(minr, minc), at(minr, maxc), at(maxr, minc), at(maxr, maxc)
        for k in range(nmat):
            tl, tr, bl, br = (l00 == k + 1) * 1.0, (l01 == k + 1) * 1.0, (l10 == k + 1) * 1.0, (l11 == k + 1) * 1.0
            acc[k] += (1 - dr) * ((1 - dc) * tl + dc * tr) + dr * ((1 - dc) * bl + dc * br)
    return acc


def project(labels, nmat, angle_deg, dims, s, voxel_m):
    """labels [n][m][m] -> (geom [nmat][dimX][dimY] float32, lines [nmat][dimX][dimY] float64)."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    dimX, dimY = int(dims[0]), int(dims[1])
    lines = np.zeros((nmat, dimX, dimY))
    done = {}
    for x, z in enumerate(rows(n, dimX, float(s))):
        if 0 <= z < n:
            if z not in done:
                done[z] = slice_lines(labels[z], nmat, angle_deg, dimY, float(s))
            lines[:, x, :] = done[z]
    return (lines * float(voxel_m)).astype(np.float32), lines


# ---- shared cases ----------------------------------------------------------------------------------------------------
def circle(m):
    c = m // 2
    i, j = np.mgrid[0:m, 0:m]
    return (i - c) ** 2 + (j - c) ** 2 <= c * c


def random_labels(n, m, nmat, seed, in_circle=True):
    """Random labels 0 .. nmat (a third empty), inside the circle; with n >= 3, slice 0 is left empty and slice n - 1 is
    one material (the last) over the whole circle."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, nmat + 1, size=(n, m, m)).astype(np.uint8)
    lab[rng.random((n, m, m)) < 0.33] = 0
    if in_circle:
        lab *= circle(m).astype(np.uint8)
    if n >= 3:
        lab[0] = 0
        lab[n - 1] = nmat * circle(m).astype(np.uint8)
    return lab


def chiral_slice(m=64):
    """A two-material slice that differs from its mirror image and its transpose: an off-centre square of material 0
    (value 1.0), an L of material 1 (value 2.5) -- inside the circle at m = 64 and m = 33 (scaled)."""
    f = m / 64.0
    lab = np.zeros((m, m), dtype=np.uint8)
    q = lambda v: int(round(v * f))
    lab[q(14):q(26), q(30):q(44)] = 1                              # the square: up and to the right of the centre
    lab[q(34):q(50), q(18):q(24)] = 2                              # the L's stem
    lab[q(44):q(50), q(18):q(40)] = 2                              # the L's foot
    assert not np.any(lab[~circle(m)])
    return lab


CHIRAL_VALUES = (1.0, 2.5)


def classify(img, values=CHIRAL_VALUES):
    """Labels by thresholds halfway between 0 and the ascending `values`."""
    edges = [0.5 * (a + b) for a, b in zip((0.0,) + tuple(values[:-1]), values)]
    return np.digitize(img, edges).astype(np.uint8)
