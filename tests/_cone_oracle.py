"""Float64 numpy oracle of the divergent projection of a labelled voxel volume (include/paresis_hip.h, "the same volume
under a point source"), the way tests/_volume_oracle.py restates the parallel one.  Nothing here imports the package's
kernels.

numpy evaluates a * b + c as two rounded operations and a / b, np.sqrt as correctly rounded ones: the contract's "every
product, quotient, sum and square root rounded on its own"; the sum over r is an explicit ascending loop."""
import numpy as np

from tests import _volume_oracle as vo


def magnification(dso, r, c0, side=1):
    """g of step r: (dso + (r - c0))/dso.  side=-1 puts the source on the far side (w -> -w): the wrong geometry, for the tests
    that must tell the two apart."""
    return (float(dso) + side * float(r - c0)) / float(dso)


def path_length(dims, s, dso):
    """L[x][y] = sqrt(1 + (t0^2 + z0^2)/dso^2)."""
    dimX, dimY = int(dims[0]), int(dims[1])
    t0 = (np.arange(dimY, dtype=np.int64) - dimY // 2).astype(np.float64) * float(s)
    z0 = (np.arange(dimX, dtype=np.int64) - dimX // 2).astype(np.float64) * float(s)
    return np.sqrt(1.0 + ((t0 * t0)[None, :] + (z0 * z0)[:, None]) / (float(dso) * float(dso)))


def project(labels, nmat, angle_deg, dims, s, voxel_m, dso, side=1):
    """labels [n][m][m] -> (geom [nmat][dimX][dimY] float32, lines [nmat][dimX][dimY] float64)."""
    labels = np.asarray(labels)
    n, m = labels.shape[0], labels.shape[1]
    dimX, dimY = int(dims[0]), int(dims[1])
    s, dso = float(s), float(dso)
    co, si, c0, offx, offy = vo.scalars(m, angle_deg)
    t0 = (np.arange(dimY, dtype=np.int64) - dimY // 2).astype(np.float64) * s
    z0 = (np.arange(dimX, dtype=np.int64) - dimX // 2).astype(np.float64) * s
    pad = np.zeros((n + 1, m + 2, m + 2), dtype=np.int64)         # label 0 around every slice; slice n is empty
    pad[:n, 1:-1, 1:-1] = labels
    acc = np.zeros((nmat, dimX, dimY))
    for r in range(m):
        g = magnification(dso, r, c0, side)
        cpos = t0 * g + float(c0)
        z = n // 2 + np.floor(z0 * g + 0.5).astype(np.int64)
        z = np.where((z >= 0) & (z < n), z, n)[:, None]           # a step outside [0, n) reads the empty slice
        X = co * cpos + si * float(r) + offx
        Y = (-si * cpos) + co * float(r) + offy
        minr, minc = np.floor(Y).astype(np.int64), np.floor(X).astype(np.int64)
        maxr, maxc = np.ceil(Y).astype(np.int64), np.ceil(X).astype(np.int64)
        dr, dc = Y - minr, X - minc

        def at(i, j):
            ok = (i >= 0) & (i < m) & (j >= 0) & (j < m)
            return np.where(ok[None, :], pad[z, (np.clip(i, -1, m) + 1)[None, :], (np.clip(j, -1, m) + 1)[None, :]], 0)

        l00, l01, l10, l11 = at(minr, minc), at(minr, maxc), at(maxr, minc), at(maxr, maxc)
        for k in range(nmat):
            tl, tr, bl, br = (l00 == k + 1) * 1.0, (l01 == k + 1) * 1.0, (l10 == k + 1) * 1.0, (l11 == k + 1) * 1.0
            acc[k] += (1 - dr) * ((1 - dc) * tl + dc * tr) + dr * ((1 - dc) * bl + dc * br)
    lines = acc * path_length(dims, s, dso)
    return (lines * float(voxel_m)).astype(np.float32), lines


def seen_at(i, j, z, m, angle_deg, dso):
    """Where the voxel (slice row i, slice column j, height z above the optical axis) of an m x m slice is seen on the virtual
    detector: (t U, z U) with t = (j - h) c - (i - h) s, w = (j - h) s + (i - h) c, U = dso/(dso + w) -- and w."""
    h = m // 2
    th = np.deg2rad(np.float64(angle_deg))
    c, s = np.cos(th), np.sin(th)
    t, w = (j - h) * c - (i - h) * s, (j - h) * s + (i - h) * c
    U = dso / (dso + w)
    return t * U, z * U, w
