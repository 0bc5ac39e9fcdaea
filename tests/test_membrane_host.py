"""CPU: the per-pixel membrane reference (tests/_membrane_oracle.py) against the project oracle and against known answers, and
the caps on what its rim-ambiguous flag may take out of the device tests (tests/test_gpu_membrane.py) for every list they use."""
import numpy as np
import pytest

from oracle import paresis_oracle as orc
from tests import _membrane_oracle as mo


def c_splat(xf, yf, r, dimX, dimY, margin, margin2):
    """oracle_membrane_splat, cropped.  Only for lists whose windows stay on the margin-extended grid."""
    xf, yf, r = (np.ascontiguousarray(v, dtype=np.float64) for v in (xf, yf, r))
    assert np.all(np.floor(r) + 1 <= margin2), "a window would leave the array of oracle_membrane_splat"
    mem = np.zeros((dimX + 2 * margin, dimY + 2 * margin))
    orc._lib().oracle_membrane_splat(len(r), orc._dp(xf), orc._dp(yf), orc._dp(r), dimX, dimY, margin, margin2, orc._dp(mem))
    return mem[margin:margin + dimX, margin:margin + dimY]


@pytest.mark.parametrize("margin", (8, 25))
def test_agrees_with_the_project_oracle(margin):
    """Lists with radInt <= margin2, centres also in the margins and beyond the admission bounds: per pixel 1e-13 of the pixel's
    own value outside the rim-ambiguous flag, zero exactly."""
    margin2 = margin // 2
    worst, hit_px = 0.0, 0
    for seed, (dimX, dimY), n in ((1, (40, 70), 300), (2, (33, 65), 150), (3, (64, 31), 600), (4, (5, 90), 80)):
        g = np.random.default_rng(100 * margin + seed)
        xf = g.uniform(-3.0, dimX + 2 * margin + 3.0, n)
        yf = g.uniform(-3.0, dimY + 2 * margin + 3.0, n)
        r = g.uniform(0.05, margin2 - 1e-9, n)
        xf[::7] = np.floor(xf[::7]) + 0.5                       # ties
        r[::11] = np.floor(r[::11]) + (margin2 > np.floor(r[::11]) + 1)     # integer radii (0 is not drawn by either)
        ref, cnt, amb = mo.splat(xf, yf, r, dimX, dimY, margin, margin2)
        c = c_splat(xf, yf, r, dimX, dimY, margin, margin2)
        use = ~amb
        assert np.array_equal(c[use] == 0.0, cnt[use] == 0) and np.all(ref[cnt == 0] == 0.0)
        err = np.abs(ref - c)[use] / np.maximum(np.abs(c[use]), 1e-300)
        worst, hit_px = max(worst, float(err.max())), hit_px + int((cnt > 0).sum())
        assert err.max() <= 1e-13, (margin, seed, float(err.max()))
        assert amb.sum() <= 1e-4 * max(1, (cnt > 0).sum())
    print("margin %d: worst relative difference per pixel %.2e over %d hit pixels" % (margin, worst, hit_px))


def test_rim_flag_caps_for_every_device_case():
    """What the flag leaves out of the device tests: nothing in a built list, at most 1e-4 of the hit pixels in a random one."""
    kinds = set()
    for name, c in mo.cases().items():
        ref, cnt, amb = mo.reference(name)
        assert ref.shape == cnt.shape == amb.shape == (c.dimX, c.dimY) and ref.dtype == np.float64
        assert np.all(np.isfinite(ref)) and np.all((ref > 0) == (cnt > 0)), name
        if c.kind == "built":
            assert not amb.any(), name
        else:
            assert amb.sum() <= 1e-4 * (cnt > 0).sum(), (name, int(amb.sum()), int((cnt > 0).sum()))
        kinds.add(c.kind)
    assert kinds == {"built", "random"}


def test_built_lists_are_on_the_eighth_pixel_lattice():
    """...so that d^2 and r^2 are exact in float64 and no rounding decides a rim -- but for the two cases about radii far below
    the lattice, whose spheres sit exactly on a pixel."""
    for name, c in mo.cases().items():
        if c.kind != "built" or name.startswith("radius-tiny"):
            continue
        ok = np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.r)
        for v in (c.x[ok], c.y[ok], c.r[ok]):
            assert np.array_equal(v * 8, np.rint(v * 8)) and np.all(np.abs(v) < 2.0 ** 20), name
    for name in ("radius-tiny", "radius-tiny-alone"):
        c = mo.cases()[name]
        tiny = c.r < 1e-6
        assert tiny.sum() >= 2 and np.array_equal(c.x[tiny], np.rint(c.x[tiny])) and np.array_equal(c.y[tiny], np.rint(c.y[tiny]))
        assert (mo.reference(name)[1] > 0).sum() > 0          # the reference does add their 2 r


def test_cases_reach_what_they_are_named_for():
    """The properties of a case that need no GPU (those of the staging are asserted next to the device runs)."""
    cs = mo.cases()
    assert [(c.dimX, c.dimY) for n, c in cs.items() if n.startswith("grid-")] == list(mo.GRIDS)
    for name, c in cs.items():
        if name.startswith("grid-"):
            n = mo.reference(name)[1]
            assert n[0, 0] > 0 and n[-1, -1] > 0 and n[-1, 0] > 0 and n[0, -1] > 0, name      # corners, last row and column
            xi, yi = np.rint(c.x - c.offs[0][0]), np.rint(c.y - c.offs[0][1])
            assert np.any(xi < c.margin) and np.any(xi >= c.margin + c.dimX) and np.any(yi < c.margin) and np.any(yi >= c.margin + c.dimY)
    c = cs["window-ties"]
    fx, fy = c.x % 1.0 == 0.5, c.y % 1.0 == 0.5
    assert {int(v) % 2 for v in np.floor(c.x[fx])} == {0, 1} and {int(v) % 2 for v in np.floor(c.y[fy])} == {0, 1}
    c = cs["window-radii"]
    assert np.any(c.r == np.floor(c.r)) and np.any(c.r < 1.0) and np.any(np.ceil(c.r) - c.r == 0.125)
    assert sorted(set(2 * (np.floor(cs["window-reach"].r) + 1))) == [16, 18, 32, 34]
    for name in ("admission", "admission-margin0"):
        c = cs[name]
        assert c.margin2 == c.margin // 2 and (name == "admission") == (c.margin > 0)
        for v, dim in ((c.x, c.dimX), (c.y, c.dimY)):
            vi = np.rint(v[np.isfinite(v)])
            assert {c.margin2, c.margin2 + 1, dim + c.margin + c.margin2 - 1, dim + c.margin + c.margin2} <= set(vi)
        drawn = [mo.admitted(a, b, r, c.dimX, c.dimY, c.margin, c.margin2) is not None for a, b, r in zip(c.x, c.y, c.r)]
        assert 0 < sum(drawn) < len(drawn) - 10 and (~(np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.r))).sum() == 8
    assert not mo.reference("none-valid")[1].any() and len(cs["none-valid"].r) == 3 and len(cs["empty"].r) == 0
    c = cs["offsets"]
    per_layer = [int(mo.layer_reference("offsets", l)[1].sum()) for l in range(len(c.offs))]
    assert all(v > 0 for v in per_layer[:4]) and per_layer[5:] == [0, 0, 0] and min(o[0] for o in c.offs) < 0 and c.x.min() < 0
    assert mo.reference("radius-300")[1].min() >= 1 and mo.reference("radius-plan-max")[1].min() >= 1   # over the whole grid
    assert cs["radius-plan-max"].r.max() == 2.0 ** 14 - 0.125


def chord(r, d2):
    """The reference program's chord at squared distance d2 (getMembraneFromFile.py:157-159): within 3 * 2^-53 d2 / (2 (r^2 - d2))
    of 2 sqrt(r^2 - d2)."""
    dist = np.sqrt(d2)
    return 2.0 * np.sqrt(r * r - dist * dist)


def test_known_answers():
    # one sphere, dyadic centre and radius: the chord in closed form, the window half open
    ref, cnt, amb = mo.splat([10.25], [12.5], [3.5], 20, 24, 0, 0)
    for i in range(20):
        for j in range(24):
            d2 = (i - 10.25) ** 2 + (j - 12.5) ** 2
            inside = 6 <= i < 14 and 8 <= j < 16 and d2 < 12.25       # xi = 10, yi = rint(12.5) = 12, radInt = 4
            exact = 2.0 * np.sqrt(12.25 - d2) if inside else 0.0
            # sqrt(d2)^2 is d2 within 3 roundings: that much of d2 / (2 (r2 - d2)) of the chord, and the last root's own rounding
            assert abs(ref[i, j] - exact) <= (3 * d2 / (2 * (12.25 - d2)) + 1) * 2.0 ** -53 * exact if inside else ref[i, j] == 0.0
            assert cnt[i, j] == int(inside)
    assert not amb.any()
    # scale and crop: the same sphere seen through a margin
    ref2, cnt2, _ = mo.splat([15.25], [15.5], [3.5], 10, 18, 5, 2, scale=0.5)
    assert np.array_equal(ref2, 0.5 * ref[:10, 2:20]) and np.array_equal(cnt2, cnt[:10, 2:20])
    # 3-4-5: d^2 = r^2 exactly, and the strict < leaves the pixel out (flagged: it IS on the rim)
    ref, cnt, amb = mo.splat([10.0], [10.0], [5.0], 20, 20, 0, 0)
    for di, dj in ((3, 4), (4, 3), (-3, 4), (-4, -3), (0, 5), (-5, 0)):
        if -6 <= di < 6 and -6 <= dj < 6:
            assert ref[10 + di, 10 + dj] == 0.0 and cnt[10 + di, 10 + dj] == 0 and amb[10 + di, 10 + dj]
    assert ref[10, 10] == 10.0 and ref[13, 13] == chord(5.0, 18.0) and amb.sum() == 12
    # r = 1.9: radInt = 2.  xf = 2.5 rounds to 2 (even): window rows [0, 4) and pixel 4 (d = 1.5 < r) is clipped away;
    # xf = 3.5 rounds to 4: window rows [2, 6) holds every pixel within r of the centre
    ref, cnt, _ = mo.splat([2.5], [5.0], [1.9], 10, 10, 0, 0)
    assert ref[4, 5] == 0.0 and ref[3, 5] == chord(1.9, 0.25) and ref[1, 5] == chord(1.9, 2.25)
    assert cnt[:, 5].tolist() == [0, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    ref, cnt, _ = mo.splat([3.5], [5.0], [1.9], 10, 10, 0, 0)
    assert cnt[:, 5].tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0] and ref[5, 5] == ref[2, 5] == chord(1.9, 2.25)
    # admission: the bounds are strict on both sides, r = 0 and non-finite entries are not drawn
    assert mo.admitted(4.5, 10.0, 1.0, 8, 8, 9, 4) is None and mo.admitted(4.51, 10.0, 1.0, 8, 8, 9, 4) == (5, 10, 2)
    assert mo.admitted(20.5, 10.0, 1.0, 8, 8, 9, 4) == (20, 10, 2) and mo.admitted(20.51, 10.0, 1.0, 8, 8, 9, 4) is None
    for bad in ((np.nan, 10.0, 1.0), (10.0, np.inf, 1.0), (10.0, 10.0, np.inf), (10.0, 10.0, 0.0), (10.0, 10.0, -1.0), (10.0, 10.0, np.nan)):
        assert mo.admitted(*bad, 8, 8, 9, 4) is None


def test_staging_counts_a_row_of_spheres():
    """mo.staging on a stated build: 33 spheres of one cell row are one job of two batches."""
    info = dict(zip(mo.INFO_FIELDS, (33, 1, 3, 3, 32, 32, 64, 32, 8, 8)))
    st = mo.staging(info, mo.cases()["row-33"])
    assert (st["kept"], st["staged"], st["hits"], st["batches"], st["rows"], st["jobs"], st["rounds"], st["launches"]) == (33, 33, 33, 2, 3, 3, 1, 1)


def test_abi_has_the_membrane_plan_accessor():
    import ctypes
    from paresis_amd import _lib
    lib = _lib.lib()
    assert _lib.ABI_VERSION >= 25 and lib.psx_abi_version() == _lib.ABI_VERSION
    assert _lib.PSX_MEMBRANE_PLAN_INFO == len(mo.INFO_FIELDS) == 10
    buf = (ctypes.c_int * 10)(*([-7] * 10))
    assert lib.psx_membrane_plan_info(None, buf, 10) == 0 and list(buf) == [-7] * 10      # no plan: nothing written
