"""The refraction step in plain numpy float64, a DERIVED per-pixel error bound for the tile kernels of
paresis_amd/csrc/refract.hip, a numpy restatement of the kernels' own arithmetic (with seeded wrong variants), and the frames,
phases and grids the host and GPU tests share.

scatter() restates orc.fast_refraction (gradient -> displacement -> clamp -> pad -> fastloop -> crop) share by share, so that
besides the image it can say, per pixel, how many shares landed there and how large they were.

The bound, term by term (u = 2^-24: one float32 rounding is relative u; line numbers are refract.hip's).  Nothing below is
fitted to a run.  os = |out_scale|, base = the image an add=True call adds onto.

displacement and weights                                                                  os * u * A[p]
    :424-425, :458-459   D = (float)(float64 difference * scale): |dD| <= u |D|.  The float64 differencing itself (:372-374,
                         :435-452; up to three products and two sums of phases) is within 2^-50 * scale * max|phi|, carried in A.
    :489, :512           w = D - floor(D) is exact for D >= 0 and for D <= -0.5; for D in (-0.5, 0) it is 1 + D rounded: u/2.
    :540-541             1 - w is exact for w >= 0.5, else rounded into (0.5, 1]: u/2.  (Never both for one axis.)  The far
                         replay's axis_split_ref (:127-141) forms the same two numbers.  The reference zeroes |D| < 1e-12
                         (RF2:59-60) and the kernel does not: 1e-12 < u/2 of a weight.
    A change dw of a weight moves I_s |dw| between the two pixels of that axis; with both weights in [0, 1],
    |d(wx wy)| <= |dwx| + |dwy| <= (|Dx| + |Dy| + 1) u.  Hence A[p] = sum over the rays with a share at p (a share of weight 0
    included: the float32 D may fall on the integer the float64 D just misses, never beyond it) of
    |I_s| (1 + |Dx_s| + |Dy_s| + 2^-26 scale max|phi|).
share products                                                                             os * 3 u * S[p]
    :542-543, :820-824   I * (wx-part * wy-part): two products, 2 u |share|; the replay's `out_scale * v` (:794) one more.
                         S[p] = sum |share|.  (:518, the scaling by the tile's power of two, is exact.)
tile fixed point                                                                           os * N_near[p] * unit(tile) / 2
    :322-324, :527-531   every share is rounded to the tile's unit (v_cvt_rpi: floor(v + 0.5)): half a unit each, summed exactly.
                         unit = 2^-sexp, sexp = clamp(30 - (ilogb(W) + 1), -120, 120), W the largest |source intensity| staged in
                         the WINDOW of p's tile: rows [r0 - H, r0 + T + H) x cols [c0 - H, c0 + T + H) inside the image, both
                         sides of a split call together (:319-320).  unit / 2 <= 2^-30 W unless the clamp at 120 holds (W < 2^-91).
                         N_near counts the shares with I_s != 0 whose source lies in that window.
write-out                                                                                  2 u os |near sum|  [+ u |result|]
    :609                 (float)((double)q * finv) and the product with out_scale: one rounding each of the tile's sum
                         (|near sum| <= S_near[p]); :610 with add=True one more of base + os * sum.
far shares, float replay                                                                   n_far[p] * u * (|base[p]| + os S[p])
    :796                 n_far float atomics onto the stored tile value, each rounding a partial sum that is at most
                         |base| + os * S[p] in magnitude.  A product below 2^-126 may be flushed: n_far * 2^-126 * 3 on top.
far shares, order-independent replay                           os * n_far[p] * unit_det / 2 + 2 u os S_far[p] + u (|base| + os S)
    :768, :802-813       xq = v * unit (exact), llrintf: half a unit per share, shares below it vanish.  unit_det = 2^-s,
                         s = det_unit_exp(bits) = clamp(30 - (ilogb(m) + 1), -120, 120), m the call's largest finite staged
                         intensity, or 64 x the caller's set_deterministic_scale (:907-913).
    :755-757             (float)(sum * inv), its product with out_scale, and ONE add onto the stored value.
source intensity
    Exact when I0 = 1 and I_in is given.  From thickness maps (:227-234): the coefficient (float)(catt log2 e) is one rounding,
    every fmaf rounds a partial sum <= |la| log2 e: the base-2 exponent is off by at most (nmat + 1) u |la| log2 e, the factor
    by (nmat + 1) u |la| relatively; v_exp_f32 is within 1 ulp (2 u) and `I0 * Iin`, `I *= exp2` are two products (2 u).
    tests/_materials_oracle.py bounds k_transmit_rt by (|la| + 4) u |I| (bound_intensity without its add term): there the
    exponent is a float64 sum rounded ONCE; the refraction staging sums it in float32, which is nmat more roundings of |la|.
    The allowance dI_s = ((nmat + 1) |la| + 4) u |I_s| is scattered with the reference's own weights (the scatter is linear
    in I).  The tile's W is read off the reference intensity times (1 + max dI / I).
reference                                                                                   2^-48 S[p]
    float64 sums of at most a few hundred shares.

Three terms are stated differently from the first sketch of this bound, each because the code says so:
  * W is the maximum over the window of p's OWN tile (the tiling starts at pixel 0, so the tile is known), not over a box that
    covers every tile that could hold p: tighter, and what lets a dim-only tile next to a bright one be held to its own unit.
  * A sums over the rays with a share at p itself, not also at p's neighbours: a float32 D never leaves the 2 x 2 pixels of the
    float64 D (see above), so nothing else can move onto p.
  * the float replay's adds round the RUNNING value of the pixel, which holds the tile's near sum (and the base image), not only
    the far shares: n_far u (|base| + os S), not (n_far + 1) u S_far -- one far share of 1e-6 added onto a near sum of 1.5 is
    off by up to u * 1.5.

Only the clamp is discontinuous inside the crop (a ray with |D| > clamp is zeroed, RF2:61-64): scatter() flags every pixel that
receives a share of a ray whose |D| lies within a relative 2^-20 of a clamp.  The tests' inputs are chosen so that no pixel is
flagged (tests/test_refraction_host.py asserts the count is 0 for every case)."""
import functools

import numpy as np

U = 2.0 ** -24
TILE = {4: 56, 6: 52, 8: 48, 12: 40, 16: 32}           # gather halo -> tile size (the Geo<> table of refract.hip)
HALOS = (4, 6, 8, 12, 16)
VARIANT = {"v2": (15, None), "v1": (10, (1e3, 1e3))}   # margin, clamp (None: the grid, RF2:61-64)


def grid(H):
    """The smallest grid with one interior tile, ragged last tiles and unequal axes."""
    T = TILE[H]
    return 2 * T + H + 4, 2 * T + H + 9


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ reference
def _axis_ref(d, p):
    """One axis of fastloopNumba's split (RF2:228-233 and the sign cases of RF2:237-262): base, neighbour, their weights."""
    big = np.abs(d) > 1.0
    f = np.floor(d)
    b = np.where(big, p + f, p).astype(np.int64)
    r = np.where(big, d - f, d)
    nb = np.where(r >= 0, b + 1, b - 1)
    wn = np.abs(r)
    return b, nb, 1.0 - wn, wn


def displacement(phi, dscale, clamp):
    """(Dx, Dy, killed): RF2:54-64 on the unpadded grid; killed = the sources whose intensity the clamp zeroes."""
    gx, gy = np.gradient(np.asarray(phi, dtype=np.float64), edge_order=2)
    Dx, Dy = gx * dscale, gy * dscale
    Dx[np.abs(Dx) < 1e-12] = 0
    Dy[np.abs(Dy) < 1e-12] = 0
    kx, ky = np.abs(Dx) > clamp[0], np.abs(Dy) > clamp[1]
    Dx[kx] = 0
    Dy[ky] = 0
    return Dx, Dy, kx | ky


class Scatter:
    """What scatter() returns: image, padded Dx / Dy, killed, and the per-pixel statistics N, A, S (+ _far / _near)."""


def _shares(Dx, Dy, margin):
    """The four shares of every source pixel in unpadded target coordinates: (ti, tj, weight, valid) each [4][Nx][Ny];
    valid applies the reference's border rules in padded coordinates (RF2:235-262)."""
    Nx, Ny = Dx.shape
    ii, jj = np.meshgrid(np.arange(Nx) + margin, np.arange(Ny) + margin, indexing="ij")
    bi, ni, wbi, wni = _axis_ref(Dx, ii)
    bj, nj, wbj, wnj = _axis_ref(Dy, jj)
    Px, Py = Nx + 2 * margin, Ny + 2 * margin
    base_ok = (bi >= 0) & (bi < Px) & (bj >= 0) & (bj < Py)
    nb_ok = base_ok & (ni >= 0) & (ni < Px) & (nj >= 0) & (nj < Py)
    ti = np.stack([bi, ni, ni, bi]) - margin
    tj = np.stack([bj, bj, nj, nj]) - margin
    w = np.stack([wbi * wbj, wni * wbj, wni * wnj, wbi * wnj])
    ok = np.stack([base_ok, nb_ok, nb_ok, nb_ok])
    ok &= (ti >= 0) & (ti < Nx) & (tj >= 0) & (tj < Ny)              # the crop (RF2:78)
    return ti, tj, w, ok


def _is_far(ti, tj, H, T):
    """Per share: the source lies outside the window of the target's tile (the test of k_refract_far, :790-791)."""
    Nx, Ny = ti.shape[1:]
    si, sj = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
    r0, c0 = (ti // T) * T, (tj // T) * T
    return ~((si >= r0 - H) & (si < r0 + T + H) & (sj >= c0 - H) & (sj < c0 + T + H))


def scatter(I_src, phi, dscale, clamp=None, margin=None, variant="v2", halo=None):
    """orc.fast_refraction's scatter on (I_src, phi) with displacement scale dscale = z / k / (h M) / h.  clamp / margin
    default to the variant's.  With `halo` the far statistics are those of that tile geometry."""
    I_src = np.asarray(I_src, dtype=np.float64)
    Nx, Ny = I_src.shape
    vm, vc = VARIANT[variant]
    margin = vm if margin is None else margin
    clamp = (vc or (Nx, Ny)) if clamp is None else clamp
    Dx, Dy, killed = displacement(phi, dscale, clamp)
    I = np.where(killed, 0.0, I_src)
    ti, tj, w, ok = _shares(Dx, Dy, margin)
    s = Scatter()
    s.shape, s.margin, s.clamp, s.killed, s.halo = (Nx, Ny), margin, clamp, killed, halo
    s.Dx, s.Dy = np.pad(Dx, margin), np.pad(Dy, margin)
    s.I_after = I
    lit = ok & (I != 0)[None]
    flat = (ti * Ny + tj)[lit]
    share = (I[None] * w)[lit]
    f64 = 2.0 ** -26 * abs(dscale) * np.max(np.abs(phi))
    a = np.broadcast_to((np.abs(I) * (1 + np.abs(Dx) + np.abs(Dy) + f64))[None], w.shape)[lit]

    def acc(v, sel=None):
        return np.bincount(flat if sel is None else flat[sel], None if v is None else (v if sel is None else v[sel]),
                           minlength=Nx * Ny).reshape(Nx, Ny)
    s.image = acc(share)
    s.N, s.A, s.S = acc(None), acc(a), acc(np.abs(share))
    # the clamp's neighbourhood: rays within a relative 2^-20 of a clamp, and every pixel one of their shares reaches
    gx, gy = np.gradient(np.asarray(phi, dtype=np.float64), edge_order=2)
    close = (np.abs(np.abs(gx * dscale) / clamp[0] - 1) < 2.0 ** -20) | (np.abs(np.abs(gy * dscale) / clamp[1] - 1) < 2.0 ** -20)
    s.flagged = np.zeros((Nx, Ny), dtype=bool)
    if close.any():
        for D0x, D0y in ((gx * dscale, gy * dscale), (Dx, Dy)):              # as if kept, as if zeroed
            fi, fj, _, fok = _shares(np.where(close, D0x, 0.0), np.where(close, D0y, 0.0), margin)
            sel = fok & close[None]
            s.flagged.reshape(-1)[(fi * Ny + fj)[sel]] = True
    if halo is not None:
        far = _is_far(ti, tj, halo, TILE[halo])[lit]
        s.N_far, s.A_far, s.S_far = acc(None, far), acc(a, far), acc(np.abs(share), far)
        s.N_near, s.S_near = s.N - s.N_far, acc(np.abs(share), ~far)
    return s


def tile_window_max(I_abs, H):
    """Per pixel: the largest |source intensity| in the window of the pixel's tile."""
    T = TILE[H]
    Nx, Ny = I_abs.shape
    W = np.zeros((Nx, Ny))
    for r0 in range(0, Nx, T):
        for c0 in range(0, Ny, T):
            W[r0:r0 + T, c0:c0 + T] = np.max(I_abs[max(r0 - H, 0):r0 + T + H, max(c0 - H, 0):c0 + T + H], initial=0.0)
    return W


def unit_of(m):
    """The fixed-point unit 2^-sexp of a tile (or of the order-independent replay) whose largest intensity is m > 0
    (:322, det_unit_exp): sexp = clamp(30 - (ilogb(m) + 1), -120, 120).  0 where m == 0."""
    m = np.asarray(m, dtype=np.float64)
    _, e = np.frexp(np.where(m > 0, m, 1.0))                # m = f 2^e, f in [0.5, 1): ilogb(m) + 1 = e
    return np.where(m > 0, np.ldexp(1.0, -np.clip(30 - e, -120, 120)), 0.0)


def det_unit(I_abs_max, det_scale=0.0):
    s = np.float32(det_scale) * np.float32(64.0)
    return float(unit_of(float(s) if 0 < det_scale < 1e30 else float(np.float32(I_abs_max))))


def bound(s, I_window, out_scale=1.0, base=None, det=False, det_scale=0.0, src_allow=None, src_rel=0.0):
    """The per-pixel allowance for |out - (out_scale * s.image + base)| (module docstring).  s: scatter(..., halo=H);
    I_window: |source intensity| as the tiles stage it (the whole frame, both sides of a split call); det: the
    order-independent replay, with the caller's det_scale if any; src_allow: the scattered allowance of the source intensity
    (None: exact), src_rel its largest relative size."""
    os_ = abs(f32(out_scale))
    b0 = 0.0 if base is None else np.abs(np.asarray(base, dtype=np.float64))
    W = tile_window_max(np.abs(I_window) * (1 + src_rel), s.halo)
    total = b0 + os_ * s.S
    out = os_ * U * s.A + os_ * 3 * U * s.S + os_ * s.N_near * unit_of(W) / 2 + 2 * U * os_ * s.S_near
    if base is not None:
        out = out + U * (b0 + os_ * s.S_near)
    if det:
        ud = det_unit(np.max(np.abs(I_window)) * (1 + src_rel), det_scale)
        out = out + os_ * s.N_far * ud / 2 + (s.N_far > 0) * (2 * U * os_ * s.S_far + U * total)
    else:
        out = out + s.N_far * (U * total + 3 * 2.0 ** -126)
    if src_allow is not None:
        out = out + os_ * src_allow
    return out + 2.0 ** -48 * os_ * s.S


def margin_of(err, bnd):
    """max err / bound (0 / 0 = 0: where the bound is zero the result must be exact)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(err == 0, 0.0, err / bnd)))


# ---------------------------------------------------------------------------- the kernels' arithmetic, restated
def _f(x):
    return np.asarray(x, dtype=np.float32)


def kernel_model(I32, phi, dscale, clamp, margin, halo, out_scale=1.0, base=None, order=0, wrong=None, dim=None,
                 side_mask=None, side=0, det_u=None):
    """refract.hip's arithmetic in numpy: float32 displacement from float64 differences, the near shares in the tile's
    unit with round-half-up, a float32 write-out, the far shares as float32 sums in index order (order=0) or reversed (1).
    I32: the staged float32 source intensity.  det_u: the order-independent replay with that unit (far shares rounded to it
    half-to-even, summed exactly, added once).  side_mask / side: a split call (sources of the other side deposit nothing; the
    unit comes from both).  wrong: one of the seeded faults below, applied only where `dim` is True:
        'drop_far'    one far ray (the largest far share into a dim pixel) is lost
        'swap'        the two x-weights of a ray with Dx in (-1, 0) are swapped
        'frame_unit'  the tile's unit comes from the frame's maximum
        'phase32'     the phase is rounded to float32 before it is differenced
        'empty_far'   the far shares into a tile whose window holds no intensity are lost
        'split_skip'  side 1 is skipped in a tile whose side-0 maximum is zero"""
    H, T = halo, TILE[halo]
    Nx, Ny = I32.shape
    I32 = _f(I32)
    dimm = np.zeros((Nx, Ny), dtype=bool) if dim is None else dim
    ph = np.asarray(phi, dtype=np.float64)
    gx, gy = np.gradient(ph, edge_order=2)
    if wrong == "phase32":
        g32x, g32y = np.gradient(ph.astype(np.float32).astype(np.float64), edge_order=2)
        gx, gy = np.where(dimm, g32x, gx), np.where(dimm, g32y, gy)
    dx, dy = _f(gx * dscale), _f(gy * dscale)
    clx, cly = np.abs(dx) > np.float32(clamp[0]), np.abs(dy) > np.float32(clamp[1])
    I = np.where(clx | cly, np.float32(0), I32)
    if side_mask is not None:
        I = np.where((side_mask != 0) == bool(side), I, np.float32(0))
    dx, dy = np.where(clx, np.float32(0), dx), np.where(cly, np.float32(0), dy)
    si, sj = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
    # ---- near: unified floor split (:489-547)
    fx, fy = np.floor(dx), np.floor(dy)
    wx, wy = dx - fx, dy - fy
    ax0, ax1 = np.float32(1) - wx, wx
    if wrong == "swap":
        sw = dimm & (dx > -1) & (dx < 0)
        ax0, ax1 = np.where(sw, ax1, ax0), np.where(sw, ax0, ax1)
    omy = np.float32(1) - wy
    Wt = tile_window_max(np.abs(I32).astype(np.float64), H)
    unit = unit_of(Wt)
    if wrong == "frame_unit":
        unit = np.where(dimm, unit_of(float(np.max(np.abs(I32)))), unit)
    bi, bj = si + fx.astype(np.int64), sj + fy.astype(np.int64)
    nti = np.stack([bi, bi + 1, bi, bi + 1])
    ntj = np.stack([bj, bj, bj + 1, bj + 1])
    inside = (nti >= 0) & (nti < Nx) & (ntj >= 0) & (ntj < Ny)
    ci, cj = np.clip(nti, 0, Nx - 1), np.clip(ntj, 0, Ny - 1)
    r0, c0 = (ci // T) * T, (cj // T) * T
    near = inside & (si >= r0 - H) & (si < r0 + T + H) & (sj >= c0 - H) & (sj < c0 + T + H)
    ut = unit[ci, cj]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale_t = np.where(ut > 0, 1.0 / ut, 0.0)
        w4 = np.stack([ax0 * omy, ax1 * omy, ax0 * wy, ax1 * wy])                      # float32 products
        Is = _f(I[None].astype(np.float64) * scale_t)                                  # exact: a power of two
        q = np.floor((w4 * Is).astype(np.float64) + 0.5)                               # v_cvt_rpi_i32_f32
    q = np.where(near, q, 0.0)
    if wrong == "split_skip" and side_mask is not None and side == 1:
        m0 = tile_window_max(np.where(side_mask == 0, np.abs(I32), 0).astype(np.float64), H)
        q = np.where((m0 == 0)[ci, cj], 0.0, q)
    acc = np.zeros(Nx * Ny)
    np.add.at(acc, (ci * Ny + cj)[near], q[near])                                      # integers below 2^53: exact
    acc = acc.reshape(Nx, Ny)
    osf = np.float32(out_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        out = osf * _f(acc * unit)
    if wrong == "split_skip" and side_mask is not None and side == 1:
        out = np.where(m0 == 0, np.float32(0), out)
    if base is not None:
        out = _f(out + _f(base))
    # ---- far: the replay with the reference's split (:777-825), float32 atomics
    bi, ni, wbi, wni = _axis_ref(dx, si + margin)
    bj, nj, wbj, wnj = _axis_ref(dy, sj + margin)
    Px, Py = Nx + 2 * margin, Ny + 2 * margin
    base_ok = (bi >= 0) & (bi < Px) & (bj >= 0) & (bj < Py)
    nb_ok = base_ok & (ni >= 0) & (ni < Px) & (nj >= 0) & (nj < Py)
    fti = np.stack([bi, ni, ni, bi]) - margin
    ftj = np.stack([bj, bj, nj, nj]) - margin
    v = np.stack([I * wbi * wbj, I * wni * wbj, I * wni * wnj, I * wbi * wnj])         # float32, left to right
    ok = np.stack([base_ok, nb_ok, nb_ok, nb_ok]) & (fti >= 0) & (fti < Nx) & (ftj >= 0) & (ftj < Ny) & (v != 0)
    ci, cj = np.clip(fti, 0, Nx - 1), np.clip(ftj, 0, Ny - 1)
    ok &= _is_far(ci, cj, H, T)
    if wrong == "empty_far":
        ok &= ~(dimm & (Wt == 0))[ci, cj]
    if wrong == "drop_far":
        cand = np.where(ok & dimm[ci, cj], np.abs(v), 0).max(axis=0)
        faint = np.abs(I32) <= 1e-4 * np.max(np.abs(I32))              # a ray that is itself dim, where there is one
        if (cand * faint).max() > 0:
            cand = cand * faint
        assert cand.max() > 0, "no far share reaches the dim part: nothing to drop"
        k = np.unravel_index(np.argmax(cand), cand.shape)
        ok[:, k[0], k[1]] = False
    if det_u is not None:
        far = np.zeros(Nx * Ny)
        np.add.at(far, (ci * Ny + cj)[ok], np.rint(v[ok].astype(np.float64) / det_u))
        hit = far != 0
        flat = out.reshape(-1).copy()
        flat[hit] = _f(flat[hit] + osf * _f(far[hit] * det_u))
        return flat.reshape(Nx, Ny)
    idx, add = (ci * Ny + cj)[ok], _f(osf * v)[ok]
    if order:
        idx, add = idx[::-1], add[::-1]
    flat = out.reshape(-1).copy()
    np.add.at(flat, idx, add)                                                          # sequential float32 adds
    return flat.reshape(Nx, Ny)


# ------------------------------------------------------------------------------------- frames, phases, cases
FRAMES = ("step", "hot", "dark_tile", "absorber1", "absorber5", "tiny", "huge")
PHASES = ("near", "far", "far_v1", "clamped")
DSCALE = 0.73


def _smooth(rng, shape, cells):
    x = np.arange(shape[0])[:, None] / cells
    y = np.arange(shape[1])[None, :] / cells
    f = np.zeros(shape)
    for _ in range(4):
        kx, ky = rng.uniform(0.3, 2.0, 2)
        px, py = rng.uniform(0, 2 * np.pi, 2)
        f += rng.uniform(0.3, 1.0) * np.cos(kx * x + px) * np.cos(ky * y + py)
    return f


class Frame:
    """I_in (float32 or None), the absorber's maps / coefficients, the float64 reference intensity, its allowance, and the
    region the wrong variants are confined to."""


@functools.lru_cache(maxsize=None)
def frame(name, H):
    T = TILE[H]
    Nx, Ny = grid(H)
    rng = np.random.default_rng(1000 * H + FRAMES.index(name))
    f = Frame()
    f.name, f.T, f.catt, f.I_in, f.nmat = name, None, None, None, 0
    f.rel = np.zeros((Nx, Ny))
    I = rng.uniform(1.0, 2.0, (Nx, Ny))
    edge = T + T // 2                                        # inside the interior tile's core
    if name == "step":
        I[edge:] *= 1e-6
        f.dim = np.zeros((Nx, Ny), dtype=bool)
        f.dim[2 * T:] = True                                 # the tiles whose window lies on the dim side
    elif name == "hot":
        I -= 0.5
        I[T + T // 3, T + T // 2] = 2.0 ** 20
        I[3, 5] = 2.0 ** 20
        f.dim = np.zeros((Nx, Ny), dtype=bool)
        f.dim[2 * T:, :T] = True                             # a tile that sees neither hot pixel
    elif name == "dark_tile":
        I[:T + H, :T + H] = 0.0                              # the whole window of tile (0, 0)
        f.dim = np.zeros((Nx, Ny), dtype=bool)
        f.dim[:T, :T] = True
    elif name in ("absorber1", "absorber5"):
        f.nmat = int(name[-1])
        ramp = np.linspace(0.0, 1.0, Nx)[:, None] * np.ones((1, Ny))
        part = rng.uniform(0.5, 1.5, f.nmat)
        part /= part.sum()
        f.T = np.stack([(ramp * rng.uniform(0.5, 2.0) * 1e-4) for _ in range(f.nmat)]).astype(np.float32)
        f.catt = [float(-80.0 * part[m] / f.T[m].astype(np.float64).max()) for m in range(f.nmat)]
        la = sum(c * t.astype(np.float64) for c, t in zip(f.catt, f.T))
        I = np.exp(la)
        f.rel = ((f.nmat + 1) * np.abs(la) + 4) * U
        f.dim = np.zeros((Nx, Ny), dtype=bool)
        f.dim[2 * T:] = True
    else:
        I = np.ldexp(I, -100 if name == "tiny" else 100)
        f.dim = np.zeros((Nx, Ny), dtype=bool)
        f.dim[2 * T:] = True
    if f.nmat == 0:
        f.I_in = I.astype(np.float32)
        I = f.I_in.astype(np.float64)
    f.I = I
    return f


@functools.lru_cache(maxsize=None)
def phase(name, H):
    """(phi float64, variant): a smooth field whose steepest slope moves a ray by `reach` pixels at DSCALE."""
    Nx, Ny = grid(H)
    rng = np.random.default_rng(77 * H + PHASES.index(name))
    phi = _smooth(rng, (Nx, Ny), 9.0)
    g = np.max(np.abs(np.gradient(phi, edge_order=2)))
    reach = H / 2.0 if name == "near" else 3.0 * H
    phi *= 0.97 * reach / (g * DSCALE)
    if name != "near":
        unit = 1.0 / DSCALE
        # single rays thrown beyond the margin at the borders, and long rays inside
        for (i, j, amp) in ((1, Ny // 2, 90.0), (Nx - 2, 7, -70.0), (Nx // 3, 1, 110.0), (Nx // 2, Ny - 2, -64.0),
                            (TILE[H] + 9, TILE[H] + 11, 47.0)):
            phi[i, j] += amp * unit
        # ... and two rays aimed, whatever the smooth field does there, from a pixel outside a tile's window into that tile:
        # into tile (2, 0), which every frame but dark_tile keeps dim, and into tile (0, 0), whose window dark_tile empties
        T = TILE[H]
        for (si, sj, ti, tj) in ((2 * T + 2, T + H + 6, 2 * T + 2.25, T - 5.5), (T + H + 10, T // 3, T - 5.5, T // 3 + 0.25)):
            phi[si + 1, sj] = phi[si - 1, sj] + 2.0 * (ti - si) / DSCALE
            phi[si, sj + 1] = phi[si, sj - 1] + 2.0 * (tj - sj) / DSCALE
        if name == "clamped":
            for (i, j, amp) in ((TILE[H] // 2, TILE[H] + 5, 1900.0), (2 * TILE[H] + 1, 2 * TILE[H] + 3, -2600.0), (6, 4, 3100.0)):
                phi[i, j] += amp * unit
    return phi, ("v1" if name == "far_v1" else "v2")


def clamp_margin(variant, shape):
    vm, vc = VARIANT[variant]
    return (vc or (float(shape[0]), float(shape[1]))), vm


@functools.lru_cache(maxsize=None)
def reference(fname, pname, H, dscale=DSCALE):
    """(frame, phi, scatter, scattered source allowance or None) of one case."""
    f = frame(fname, H)
    phi, variant = phase(pname, H)
    s = scatter(f.I, phi, dscale, variant=variant, halo=H)
    allow = None
    if f.nmat:
        allow = scatter(f.I * f.rel, phi, dscale, variant=variant).S
    return f, phi, s, allow


def case_bound(fname, pname, H, dscale=DSCALE, **kw):
    f, phi, s, allow = reference(fname, pname, H, dscale)
    return bound(s, f.I, src_allow=allow, src_rel=float(np.max(f.rel)), **kw)


# ------------------------------------------------------- split and batch calls: the phase comes from a thickness map
CPHASE = -3.7e5
MASKS = ("bright0", "bright1", "all0", "all1")


@functools.lru_cache(maxsize=None)
def phase_map(pname, H):
    """(T float32, phi float64 = CPHASE * T exactly as the staging's float64 fma forms it, variant)."""
    phi, variant = phase(pname, H)
    T = (phi / CPHASE).astype(np.float32)
    return T, CPHASE * T.astype(np.float64), variant


@functools.lru_cache(maxsize=None)
def split_mask(which, H):
    """float32 mask of a split call on the `step` frame: its bright rows on side 0 and its dim rows on side 1, the sides
    swapped, or everything on one side."""
    Nx, Ny = grid(H)
    T = TILE[H]
    m = np.zeros((Nx, Ny), dtype=np.float32)
    if which in ("bright0", "bright1"):
        m[T + T // 2:] = 1.0
        if which == "bright1":
            m = 1.0 - m
    elif which == "all1":
        m[:] = 1.0
    return m


@functools.lru_cache(maxsize=None)
def split_reference(fname, pname, H, which, side, dscale=DSCALE):
    """(frame, phi, mask, scatter of the sources of `side`)."""
    f = frame(fname, H)
    _, phi, variant = phase_map(pname, H)
    m = split_mask(which, H)
    return f, phi, m, scatter(np.where((m != 0) == bool(side), f.I, 0.0), phi, dscale, variant=variant, halo=H)


@functools.lru_cache(maxsize=None)
def map_reference(fname, pname, H, dscale=DSCALE):
    """reference() with the phase of phase_map() (refract_batch takes no phi_in)."""
    f = frame(fname, H)
    _, phi, variant = phase_map(pname, H)
    return f, phi, scatter(f.I, phi, dscale, variant=variant, halo=H)
