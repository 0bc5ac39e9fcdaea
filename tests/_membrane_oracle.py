"""Per-pixel reference of the membrane sphere splat (Samples/getMembraneFromFile.py:143-159) and the sphere lists built for it.

`splat` is the rule as both kernels of csrc/membrane.hip implement it, in plain numpy float64, gathered per sphere over
window ∩ cropped grid -- it never indexes outside an array, whatever the window (oracle_membrane_splat of oracle/oracle_loops.c
scatters over the whole window on the margin-extended grid and writes outside it when a window leaves that grid):

  * xi = rint(xf), yi = rint(yf): half to even;  radInt = floor(r) + 1;
  * a sphere is admitted iff r > 0, xf, yf and r are finite and margin2 < xi < dimX + margin + margin2 (the same for yi, dimY);
  * its window is [xi - radInt, xi + radInt) x [yi - radInt, yi + radInt) on the margin-extended grid;
  * it adds 2 sqrt(r^2 - d^2) where d^2 = (px - xf)^2 + (py - yf)^2 < r^2 -- in the reference program's own arithmetic: dist =
    sqrt(d^2), the test dist < r, the chord 2 sqrt(r r - dist dist).  The kernels compare and subtract the squares themselves,
    which spares dist dist its two roundings: a relative 3 * 2^-53 d^2 / (2 (r^2 - d^2)) of the chord, below 1e-9 of it wherever
    r^2 - d^2 is more than 1e-6 of d^2 -- and in a built list r^2 - d^2 is at least 1/64;
  * the map is cropped to [margin, margin + dim) and multiplied by scale.

It returns the float64 map, the number of chords n(p) of every pixel and the pixels that are rim-ambiguous: those with a
(pixel, sphere) pair where |d^2 - r^2| <= 8 ulp(r^2).  The reference program tests sqrt(d^2) < r and the kernels d^2 < r^2, and
a kernel may form d^2 with one rounding fewer (fma), so there -- and only there -- two correct implementations may differ by a
whole chord.  tests/test_membrane_host.py caps how many pixels the flag may take out of the device tests.

`cases()` are the lists tests/test_gpu_membrane.py renders with all three entry points: every built list has centres and radii
on the 1/8-pixel lattice (d^2 and r^2 are then exact in float64: no rounding decides a rim) except where a case says otherwise.
"""
import collections
import functools

import numpy as np

AMBIGUOUS_ULPS = 8.0


def admitted(xf, yf, r, dimX, dimY, margin, margin2):
    """(xi, yi, radInt) as Python ints, or None when the sphere is not drawn."""
    if not (np.isfinite(xf) and np.isfinite(yf) and np.isfinite(r) and r > 0.0):
        return None
    xr, yr = float(np.rint(xf)), float(np.rint(yf))
    if not (margin2 < xr < dimX + margin + margin2 and margin2 < yr < dimY + margin + margin2):
        return None
    return int(xr), int(yr), int(np.floor(r)) + 1


def splat(xf, yf, r, dimX, dimY, margin, margin2, scale=1.0):
    """One layer.  xf, yf, r: pixels of the margin-extended grid.  Returns (map float64, n int64, ambiguous bool), each
    [dimX][dimY]."""
    out = np.zeros((dimX, dimY))
    cnt = np.zeros((dimX, dimY), dtype=np.int64)
    amb = np.zeros((dimX, dimY), dtype=bool)
    for x, y, rad in zip(np.asarray(xf, dtype=np.float64), np.asarray(yf, dtype=np.float64), np.asarray(r, dtype=np.float64)):
        a = admitted(x, y, rad, dimX, dimY, margin, margin2)
        if a is None:
            continue
        xi, yi, radInt = a
        i0, i1 = max(xi - radInt, margin), min(xi + radInt, margin + dimX)
        j0, j1 = max(yi - radInt, margin), min(yi + radInt, margin + dimY)
        if i0 >= i1 or j0 >= j1:
            continue
        dx = np.arange(i0, i1, dtype=np.float64) - x
        dy = np.arange(j0, j1, dtype=np.float64) - y
        d2 = (dx * dx)[:, None] + (dy * dy)[None, :]
        r2 = rad * rad
        dist = np.sqrt(d2)                                   # getMembraneFromFile.py:157-159, operation by operation
        hit = dist < rad
        sl = (slice(i0 - margin, i1 - margin), slice(j0 - margin, j1 - margin))
        out[sl] += np.where(hit, 2.0 * np.sqrt(np.where(hit, r2 - dist * dist, 0.0)), 0.0)
        cnt[sl] += hit
        amb[sl] |= np.abs(d2 - r2) <= AMBIGUOUS_ULPS * np.spacing(r2)
    return out * scale, cnt, amb


# ---- the lists of tests/test_gpu_membrane.py ---------------------------------------------------------------------------------
# x, y, r: the list frame of a plan; layer l is drawn at xf = x - offs[l][0], yf = y - offs[l][1].  kind: "built" (no pixel may
# be ambiguous) or "random" (at most 1e-4 of the hit pixels).
Case = collections.namedtuple("Case", "name kind x y r offs dimX dimY margin margin2 scale")

PIX_SCALE = 1.45e-6             # a pixel size, metres: the `scale` the library is called with
GRIDS = ((1, 1), (31, 63), (32, 64), (33, 65), (64, 128), (70, 130))
# No pixel of a built list may sit exactly ON a rim (d^2 = r^2: flagged ambiguous although the lattice is exact).  In eighths of a
# pixel d^2 = a^2 + b^2 and r^2 = c^2, so a radius of an odd number of eighths goes with centres on the quarter-pixel lattice (a, b
# even: a^2 + b^2 is even, c^2 odd) and a radius of an even number of eighths -- an integer radius -- with centres whose two
# fractions are both odd eighths (a^2 + b^2 = 2 mod 4, c^2 = 0 mod 4).  RADII and FRACS are cycled over a list.
RADII = (2.625, 3.375, 4.125, 7.125, 0.875, 6.125, 1.125, 9.625)
FRACS = (0.0, 0.25, 0.5, -0.25, -0.5, 0.75, 0.5, -0.75)


def _case(name, kind, xf, yf, r, dimX, dimY, margin, offs=((0, 0),), scale=1.0, margin2=None):
    """A case from coordinates on the margin-extended grid of its FIRST layer: the list frame is that grid moved by offs[0]."""
    xf, yf, r = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (xf, yf, r))
    offs = tuple((int(a), int(b)) for a, b in offs)
    x, y = xf + float(offs[0][0]), yf + float(offs[0][1])
    return Case(name, kind, x, y, r, offs, dimX, dimY, margin, margin // 2 if margin2 is None else margin2, scale)


def _anchors(dim, margin, steps):
    """Coordinates of one axis where a tiling can go wrong: first and last pixel, both sides of every tile border (steps:
    the tile sides in use along this axis), three pixels into either margin."""
    a = {margin, margin + dim - 1, margin - 3, margin + dim + 2}
    for s in steps:
        for k in range(s, dim, s):
            a |= {margin + k - 1, margin + k}
    return sorted(a)


def _grid_case(dimX, dimY, scale):
    margin = 12
    pts = [(a, b) for a in _anchors(dimX, margin, (32,)) for b in _anchors(dimY, margin, (32, 64))]
    xf = [a + FRACS[k % 8] * (k % 3 != 0) for k, (a, b) in enumerate(pts)]
    yf = [b + FRACS[(3 * k + 1) % 8] * (k % 2 != 0) for k, (a, b) in enumerate(pts)]
    r = [RADII[(k + k // 8) % 8] for k in range(len(pts))]
    return _case("grid-%dx%d" % (dimX, dimY), "built", xf, yf, r, dimX, dimY, margin, offs=((5, -3),), scale=scale)


def _window_cases():
    out = []
    # ties on either axis, even and odd k: k + 0.5 goes to the even neighbour, and the window goes with it
    ties = [(24.5, 30.0), (25.5, 41.25), (30.0, 50.5), (33.25, 51.5), (40.5, 60.5), (41.5, 61.5), (44.5, 33.5), (47.5, 70.5)]
    rad = [1.875, 1.875, 2.125, 2.875, 1.125, 3.125, 0.875, 4.125]
    out.append(_case("window-ties", "built", [t[0] for t in ties], [t[1] for t in ties], rad, 33, 65, 20))
    # integer radii (radInt = r + 1), just below an integer, below one pixel
    rr = [1.0, 2.0, 3.0, 5.0, 8.0, 1.875, 2.875, 4.875, 0.125, 0.5, 0.875, 0.625]
    even = [(v * 8) % 2 == 0 for v in rr]                # these take centres on odd eighths, the others on quarters
    xs = [22.0 + 2.25 * k + 0.125 * e for k, e in enumerate(even)]
    ys = [24.0 + 5.25 * k + 0.375 * e for k, e in enumerate(even)]
    out.append(_case("window-radii", "built", xs, ys, rr, 33, 65, 20))
    # 2 radInt = 16, 18 (> 16), 32, 34 (> 32, > 33): the 16 lanes of a sphere take one, two and three turns over its columns
    out.append(_case("window-reach", "built", [30.125, 41.375, 25.625, 47.125, 36.875], [31.375, 75.625, 52.125, 40.875, 84.375],
                     [7.5, 8.5, 15.5, 16.25, 16.0], 33, 65, 20))
    return out


def _admission_case(margin, name):
    dimX, dimY = 33, 65
    m2 = margin // 2
    xs = [m2, m2 + 1, dimX + margin + m2 - 1, dimX + margin + m2]
    ys = [m2, m2 + 1, dimY + margin + m2 - 1, dimY + margin + m2]
    xf, yf, r = [], [], []
    for a in xs:                       # each bound of one axis with the other axis well inside, then both at once
        xf += [a, a + 0.25, a - 0.5]; yf += [margin + 20.25] * 3; r += [6.625] * 3
    for b in ys:
        yf += [b, b - 0.25, b + 0.5]; xf += [margin + 11.5] * 3; r += [6.625] * 3
    for a in xs:
        for b in ys:
            xf.append(a); yf.append(b); r.append(7.125)
    # entries that are never drawn, between the valid ones
    bad = [(20.0, 30.0, 0.0), (20.0, 30.0, -3.0), (np.nan, 30.0, 3.0), (20.0, np.nan, 3.0), (20.0, 30.0, np.nan),
           (np.inf, 30.0, 3.0), (20.0, -np.inf, 3.0), (20.0, 30.0, np.inf), (20.0, 30.0, -np.inf), (-np.inf, np.inf, 3.0)]
    for k, (a, b, c) in enumerate(bad):
        xf.insert(3 * k + 1, a); yf.insert(3 * k + 1, b); r.insert(3 * k + 1, c)
    return _case(name, "built", xf, yf, r, dimX, dimY, margin)


def _row_case(count):
    """`count` small spheres in ONE cell row of the list frame (axis-0 coordinates within 32 pixels of the smallest), all of
    them reaching the single 32 x 64 tile: one job of the layers kernel holds them all."""
    k = np.arange(count)
    xf = 10.0 + (k * 7 % 28) + 0.25 * (k % 4)           # [10, 37.75]: the smallest is 10, so one 32-pixel cell row has all
    yf = 12.0 + (k * 13 % 58) + 0.25 * (k % 4)
    r = 1.125 + 0.25 * (k % 6)
    return _case("row-%d" % count, "built", xf, yf, r, 32, 64, 8, offs=((64, 32),))


def _few(n, seed, lo, hi, rmax=6.0):
    """n spheres, centres on the quarter-pixel lattice in [lo, hi) on both axes (axis 1 stretched by two), radii odd eighths."""
    g = np.random.default_rng(seed)
    return (np.floor(g.uniform(lo, hi, n) * 4) / 4, np.floor(g.uniform(lo, 2 * hi, n) * 4) / 4,
            np.floor(g.uniform(0.5, rmax, n) * 4) / 4 + 0.125)


def _job_cases():
    out = []
    # (layers, largest radius): the cell rows a tile's window can meet grow with the radius; jobs = layers x rows
    for tag, nl, big in (("7", 1, 70.625), ("8", 2, 20.125), ("9", 3, 6.125), ("18", 6, 6.125), ("rows9", 1, 100.375)):
        x, y, r = _few(24, 5, 14.0, 80.0)
        r[0] = big
        x[0], y[0] = 40.0, 70.5
        offs = [(3 + 5 * l, -2 + 7 * l) for l in range(nl)]
        out.append(_case("jobs-" + tag, "built", x, y, r, 70, 130, 14, offs=offs))
    for nl in (1, 7, 8, 9, 16, 17):
        x, y, r = _few(20, 9, 12.0, 44.0)
        offs = [((l * 5) % 11 - 4, (l * 3) % 13 - 6) for l in range(nl)]
        out.append(_case("layers-%d" % nl, "built", x, y, r, 33, 65, 12, offs=offs))
    # offsets: negative; the tile's window left of / above cell 0 of the list frame and past its last cell; far off
    x, y, r = _few(40, 13, 20.0, 90.0)
    out.append(_case("offsets", "built", x, y, r, 70, 130, 10,
                     offs=[(-60, -60), (-75, -40), (-20, -100), (-120, -60), (40, 60), (1 << 30, 0), (0, -(1 << 30)),
                           (-(1 << 30), 1 << 30)]))
    return out


def _extreme_cases():
    out = []
    out.append(_case("radius-300", "built", [37.5, 30.0], [52.25, 80.0], [300.125, 4.125], 33, 65, 20))
    # the largest radius a plan takes on the 1/8 lattice: 2^14 - 1/8
    out.append(_case("radius-plan-max", "built", [28.0, 30.0], [60.5, 40.0], [16383.875, 3.125], 33, 65, 20))
    # radii whose chords are below the accumulator's unit, centred exactly on a pixel, alone and next to ordinary spheres
    out.append(_case("radius-tiny", "built", [25.0, 30.0, 41.0, 30.0], [33.0, 40.0, 70.0, 42.5], [1e-12, 1e-30, 1e-30, 2.625],
                     33, 65, 20))
    out.append(_case("radius-tiny-alone", "built", [25.0, 30.0], [33.0, 40.0], [1e-12, 1e-30], 33, 65, 20))
    return out


def _random_case(seed):
    """A dense uniform list, not on any lattice: about 12 spheres per 32 x 32 cell, so a job (one cell row of a tile's window,
    four to five cells) holds more than a batch."""
    g = np.random.default_rng(seed)
    n = 420
    x, y = g.uniform(0.0, 125.0, n), g.uniform(0.0, 185.0, n)
    r = g.uniform(0.3, 6.9, n)
    return Case("random-%d" % seed, "random", x, y, r, ((0, 0), (3, -2)), 70, 130, 25, 12, PIX_SCALE)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_grid_case(dx, dy, PIX_SCALE if k % 2 else 1.0) for k, (dx, dy) in enumerate(GRIDS)]
    out += _window_cases()
    out += [_admission_case(9, "admission"), _admission_case(0, "admission-margin0")]
    out.append(_case("none-valid", "built", [20.0, np.nan, 2.0], [30.0, 20.0, 30.0], [-1.0, 3.0, 5.0], 33, 65, 9))
    out.append(_case("empty", "built", [], [], [], 33, 65, 9))
    out += [_row_case(c) for c in (31, 32, 33, 64, 65, 200)]
    out += _job_cases()
    out += _extreme_cases()
    out += [_random_case(s) for s in (1, 2, 3)]
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


INFO_FIELDS = ("kept", "ncx", "ncy", "rmax_int", "MC", "MLX", "MLY", "ML_CAP", "ML_SEGS", "ML_MAX")   # psx_membrane_plan_info
ACC_UNIT = 2.0 ** -36           # the layers kernel's accumulator unit, pixels (the second term of the device tolerance)


def plan_keeps(case):
    """The entries a plan keeps: drawable somewhere, and the longest chord 2 r more than half an accumulator unit."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(case.x) & np.isfinite(case.y) & np.isfinite(case.r) & (2.0 * case.r > 0.5 * ACC_UNIT)


def staging(info, case):
    """How psx_membrane_layers_f32 stages a case, from what the plan reports (psx_membrane_plan_info as a dict over
    INFO_FIELDS) -- so that a case can show that it reaches the condition it is named for.  A job is (layer, cell row of the
    list frame); a tile stages the spheres of the cells of that row that its window (tile + rmax_int + 1 on every side) meets,
    ML_CAP per batch, ML_SEGS jobs per round, ML_MAX layers per launch.  Returns rows (cell rows per layer), launches, jobs and
    rounds (of the fullest launch), and over all tiles and jobs the largest number of spheres staged (`staged`), its batches,
    and the largest number of those whose window meets the tile (`hits`)."""
    MC, MLX, MLY = info["MC"], info["MLX"], info["MLY"]
    keep = plan_keeps(case)
    x, y, r = case.x[keep], case.y[keep], case.r[keep]
    nl = len(case.offs)
    rows = (MLX + 2 * (info["rmax_int"] + 1)) // MC + 2
    launches = max(1, -(-nl // info["ML_MAX"]))
    jobs = min(nl, info["ML_MAX"]) * rows
    res = dict(rows=rows, launches=launches, jobs=jobs, rounds=-(-jobs // info["ML_SEGS"]), staged=0, hits=0, kept=len(r))
    if len(r):
        x0, y0 = np.floor(x.min()), np.floor(y.min())
        cx, cy = ((x - x0) // MC).astype(int), ((y - y0) // MC).astype(int)
        R = info["rmax_int"]
        for ox, oy in case.offs:
            xi, yi, ri = np.rint(x - ox), np.rint(y - oy), np.floor(r) + 1
            ok = ((case.margin2 < xi) & (xi < case.dimX + case.margin + case.margin2) & (case.margin2 < yi) &
                  (yi < case.dimY + case.margin + case.margin2))
            for tx0 in range(case.margin, case.margin + case.dimX, MLX):
                for ty0 in range(case.margin, case.margin + case.dimY, MLY):
                    c0 = max(0, int(np.floor((ox + tx0 - R - 1 - x0) / MC)))
                    c1 = min(info["ncx"] - 1, int(np.floor((ox + tx0 + MLX + R + 1 - x0) / MC)))
                    d0 = max(0, int(np.floor((oy + ty0 - R - 1 - y0) / MC)))
                    d1 = min(info["ncy"] - 1, int(np.floor((oy + ty0 + MLY + R + 1 - y0) / MC)))
                    assert c1 - c0 + 1 <= rows          # the kernel walks `rows` cell rows from c0: none may be left over
                    hit = ok & (xi + ri > tx0) & (xi - ri < tx0 + MLX) & (yi + ri > ty0) & (yi - ri < ty0 + MLY)
                    for c in range(c0, c1 + 1):
                        job = (cx == c) & (cy >= d0) & (cy <= d1)
                        res["staged"] = max(res["staged"], int(job.sum()))
                        res["hits"] = max(res["hits"], int((job & hit).sum()))
    res["batches"] = -(-res["staged"] // info["ML_CAP"])
    return res


def layer_coords(case, l):
    ox, oy = case.offs[l]
    return case.x - float(ox), case.y - float(oy), case.r


@functools.lru_cache(maxsize=None)
def layer_reference(name, l):
    """(map, n, ambiguous) of layer l of a case; computed once, read-only."""
    c = cases()[name]
    xf, yf, r = layer_coords(c, l)
    res = splat(xf, yf, r, c.dimX, c.dimY, c.margin, c.margin2, c.scale)
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(name):
    """(map, n, ambiguous) of all layers of a case: what psx_membrane_layers_f32 renders in one call."""
    c = cases()[name]
    parts = [layer_reference(name, l) for l in range(len(c.offs))]
    res = (sum(p[0] for p in parts), sum(p[1] for p in parts), np.logical_or.reduce([p[2] for p in parts]))
    for a in res:
        a.setflags(write=False)
    return res
