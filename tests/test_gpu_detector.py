"""GPU: every kernel form of the detector (csrc/detect.hip) on the smallest grids it takes.

Reference: the dense float64 product Cx @ img @ Cy.T of the host-composed operator (tests/test_detector_host.py holds that
operator to Detector.detection at these sizes and margins).

Bound, per pixel: weights and images are non-negative, so a float32 FMA chain of K terms errs by at most K 2^-24 of its sum;
the float32 weights of each of the four operators carry one rounding more, the float32 intermediates one each, the
reference's own float32 weights one per axis:
    |out - ref| <= (fx.W + fy.W + bx.W + by.W + 8) 2^-24 ref        at every pixel,
with the widths read from plan.info().  For a unit impulse the reference is the outer product of two operator columns, and
outside their support the output is exactly 0.

Which form ran is worked out from plan.info() and the kernel counts of the profile: `dispatch` restates the rules of
detect_impl, band_cols, band_rows, band_pair and psf_tile ON PURPOSE, and a case whose launches differ from what it predicts
fails -- so does test_cases_reach_every_form when the cases no longer reach every instantiation.  Who moves a threshold
in detect.hip has to look here and move the cases along.

Run with -s: each test prints the form it ran in and the worst err / bound it met (1.0 = at the bound)."""
import functools

import numpy as np
import pytest
import torch

from tests import _detector_oracle as do
from tests._profile import profile_counts

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
M = 15          # the product's margin (Detector.py:92)


@pytest.fixture(scope="module")
def ops():
    from paresis_amd import ops as _ops
    from paresis_amd._lib import lib
    assert lib().psx_device_ok() == 1, lib().psx_last_error()
    return _ops


def case(Nx, Ny, ov, fwhm, psf, margin=M, off=0):
    """(Nx, Ny, ov, FWHM, sigma_psf, margin, floats the input is viewed off 16-byte alignment)"""
    return (Nx, Ny, ov, float(fwhm), float(psf), margin, off)


# the form each case runs in (as replayed on the host; the tests assert it from the launches) is noted behind it
CASES = [
    # one form each, no PSF
    case(2, 2, 1, 0, 0),            # cols<8> + rows<4>
    case(4, 4, 2, 0, 0),            # front pair<4>
    case(8, 8, 4, 0.4, 0),          # front pair<8>
    case(16, 12, 1, 3.0, 0),        # front pair<12>
    case(18, 16, 2, 5.0, 0),        # front pair<16>
    case(5, 3, 1, 1.3, 0),          # cols<8> + rows<8>
    case(10, 6, 2, 3.0, 0),         # cols<8> + rows<16>
    case(15, 9, 3, 2.6, 0),         # cols<16> + rows<16>
    case(36, 33, 1, 9.0, 0),        # cols<32> + rows<0>
    case(36, 33, 1, 16.0, 0),       # cols<64> + rows<0>: both bands are the whole axis
    case(40, 66, 1, 26.0, 0),       # cols<128> + rows<0>: both bands are the whole axis
    case(17, 20, 1, 9.0, 0),        # cols_v4<32> + rows<0>
    case(33, 36, 1, 16.0, 0),       # cols_v4<64> + rows<0>
    # four-pass front and back
    case(16, 12, 1, 2.6, 0.4),      # cols_v4<8> + rows<8> | cols<8> + rows<4>
    case(16, 12, 1, 3.0, 0.4),      # cols_v4<16> + rows<16> | cols<8> + rows<4>
    case(5, 3, 1, 0, 0.4),          # cols<8> + rows<4> | cols<8> + rows<4>   (3 taps)
    case(5, 3, 1, 0, 0.8),          # ... | cols<8> + rows<8>                (5 taps)
    case(5, 3, 1, 0, 1.2),          # ... | cols<16> + rows<16>              (9 taps)
    case(2, 2, 1, 0, 5.4),          # ... | cols_v4<64> + rows<0>: 33 taps over the 32 samples of the padded axis
]
# the PSF as a stencil of 3, 11 and 15 taps and as two passes of 17 and 33, behind a four-pass front (the reflect pad of 15
# detector pixels makes the halos of a tiny grid expensive: the plan reports front_cheap = 0) and behind a fused front
# (grids whose axis 0 is long enough for cheap halos; 38 = 8 + 30 columns: the pair writes t2 at a pitch that is no multiple of 4)
for _psf in (0.4, 1.7, 2.4, 2.7, 5.4):
    CASES += [case(4, 4, 2, 0, _psf), case(6, 6, 3, 0.4, _psf), case(128, 8, 1, 0, _psf), case(240, 4, 2, 0.4, _psf)]
# the back pair in its four widths (3, 5, 9, 13 taps): PSF radius beyond the margin, bands cut at both ends of the axis
for _m in (0, 3):
    for _psf in (0.4, 0.8, 1.2, 2.0):
        CASES += [case(4, 4, 2, 0, _psf, _m), case(16, 12, 1, 3.0, _psf, _m)]
CASES += [
    # a one-pixel detector axis
    case(2, 4, 2, 0, 0),            # front pair<4>, one output row
    case(2, 4, 2, 1.3, 0.8),        # four-pass front | psf_tile<3> with one output row
    case(2, 4, 2, 0, 1.2, 0),       # front pair<4> | back pair<12>: 9 taps over one sample
    # 256-output blocks: fy.n_out = 257 and 513, the other axis 8 pixels
    case(8, 257, 1, 1.3, 0),        # cols<8> (two blocks) + rows<8>
    case(8, 227, 1, 0, 0.8),        # cols<8> (two blocks) + rows<4> (two blocks) | cols<8> + rows<8>
    case(8, 513, 1, 1.3, 0),        # cols<8> (three blocks) + rows<8>
    case(8, 483, 1, 0.4, 1.2),      # the same behind a PSF: fy.n_out = 513
    case(8, 1028, 4, 0.4, 0),       # front pair<8>, 257 output columns
    case(8, 516, 1, 1.3, 0),        # front pair<8>, 516 output columns
    # k_psf_tile's 16 x 128 tiles: 17 x 129 outputs (odd row length: scalar stores) and 17 x 130
    case(68, 516, 4, 0, 0.8, 2),    # front pair<4> | psf_tile<3>
    case(17, 130, 1, 0, 1.2),       # four-pass front | psf_tile<3>
    # k_band_pair's row tiles: 17 output rows at 16 a tile, front and back
    case(34, 8, 2, 0, 0),
    case(34, 8, 2, 0, 1.2, 0),
    case(17, 8, 1, 1.3, 2.0, 0),
    # a four-pass front (Ny % 4 != 0) whose rows the back pair / the stencil can read: 6 + 2 * 3 = 12 columns
    case(16, 6, 1, 3.0, 1.2, 3),    # cols<8> + rows<16> | back pair<12>
    case(16, 6, 1, 0, 0.8, 3),      # cols<8> + rows<4> | psf_tile<3>
    # bands wider than their axis in the scalar kernels: 9, 17 and 33 taps over 3 / 5 and 11 / 13 samples
    case(5, 3, 1, 0, 1.2, 0),       # cols<8> + rows<4> | cols<16> + rows<16>
    case(5, 3, 1, 0, 2.7, 0),       # cols<8> + rows<4> | cols<32> + rows<0>
    case(7, 5, 1, 1.3, 5.4, 3),     # cols<8> + rows<8> | cols<64> + rows<0>
    # inputs one float off 16-byte alignment: the scalar four-pass form whatever the plan found to fit
    case(4, 4, 2, 0, 0, M, 1),
    case(16, 12, 1, 3.0, 1.2, 0, 1),
    case(128, 8, 1, 0, 1.7, M, 1),
]
assert len(set(CASES)) == len(CASES)


def ident(c):
    return "%dx%d-ov%d-fwhm%g-psf%g-m%d%s" % (c[:6] + ("-off%d" % c[6] if c[6] else "",))


def shifted(a, off):
    """a on the device, starting `off` floats into its buffer: off = 1 ... 3 break the 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


@functools.lru_cache(maxsize=None)
def operators(ops, c):
    Nx, Ny, ov, fwhm, psf, margin, _ = c
    return (do.composite(ops, Nx, ov, Nx // ov, fwhm / 2.355, psf, margin),
            do.composite(ops, Ny, ov, Ny // ov, fwhm / 2.355, psf, margin))


def impulses(c):
    """Unit impulses at the four corners and, per axis, at min(N - 1, margin * ov) and its mirror image."""
    Nx, Ny, ov, _, _, margin, _ = c
    ax, ay = min(Nx - 1, margin * ov), min(Ny - 1, margin * ov)
    at = [(0, 0), (0, Ny - 1), (Nx - 1, 0), (Nx - 1, Ny - 1), (ax, ay), (Nx - 1 - ax, Ny - 1 - ay)]
    return list(dict.fromkeys(at))


@functools.lru_cache(maxsize=None)
def inputs(ops, c):
    """[(image, float64 reference)]: uniform(0.2, 2.0) with one hot pixel of 50, then the impulses."""
    Nx, Ny = c[:2]
    Cx, Cy = operators(ops, c)
    rng = np.random.default_rng(1000 * Nx + Ny)
    img = rng.uniform(0.2, 2.0, (Nx, Ny)).astype(np.float32)
    img[rng.integers(Nx), rng.integers(Ny)] = 50.0
    out = [(img, Cx @ img.astype(np.float64) @ Cy.T)]
    for i, j in impulses(c):
        e = np.zeros((Nx, Ny), np.float32)
        e[i, j] = 1.0
        out.append((e, np.outer(Cx[:, i], Cy[:, j])))
    return out


def cols_class(W, n_in, aligned):
    """band_cols: the 16-byte staging kernel for aligned rows of whole float4s and bands of at most 64 taps (its third rule,
    a staged span of at most 1280 floats, holds for every grid of this file: a span is at most max(W, n_in))."""
    assert max(W, n_in) + 6 <= 1280
    v4 = n_in % 4 == 0 and aligned and W <= 64
    for cap in (8, 16, 32, 64) if v4 else (8, 16, 32, 64, 128):
        if W <= cap:
            return ("cols_v4<%d>" if v4 else "cols<%d>") % cap
    raise AssertionError("no k_band_cols for %d taps" % W)


def rows_class(W):
    return "rows<%d>" % (4 if W <= 4 else 8 if W <= 8 else 16 if W <= 16 else 0)


def pair_class(W):
    assert W <= 16
    return "pair<%d>" % (4 if W <= 4 else 8 if W <= 8 else 12 if W <= 12 else 16)


def dispatch(info, c, forced):
    """detect_impl for ONE image, restated: ([kernel classes of the front stage], [of the back stage], {kernel: launches})."""
    Nx, Ny, ov, _, psf, margin, off = c
    aligned = off == 0
    has_psf = psf != 0
    assert (info["bx_W"] != 0) == has_psf and (info["by_W"] != 0) == has_psf
    assert info["fy_n_out"] == Ny // ov + (2 * margin if has_psf else 0) and info["pitch2"] == (info["fy_n_out"] + 3) // 4 * 4
    front_f = not forced and info["front_ok"] and info["front_cheap"] and Ny % 4 == 0 and aligned
    back_f = not forced and has_psf and info["back_ok"] and (front_f or info["pitch2"] == info["fy_n_out"])
    counts = {}

    def ran(*kernels):
        for k in kernels:
            counts[k] = counts.get(k, 0) + 1

    if front_f:
        front = ["front " + pair_class(info["fy_W"])]
        ran("k_band_pair")
    else:
        front = [cols_class(info["fy_W"], Ny, aligned), rows_class(info["fx_W"])]
        ran("k_band_cols", "k_band_rows")
    back = []
    if has_psf:
        if back_f and info["back_stencil"] and max(info["bx_W"], info["by_W"]) <= 17:
            W = max(info["bx_W"], info["by_W"])
            back = ["psf_tile<%d>" % (3 if W <= 9 else 4 if W <= 13 else 5)]
            ran("k_psf_tile")
        elif back_f:
            back = ["back " + pair_class(info["by_W"])]
            ran("k_band_pair")
        else:       # t2 comes from hipMalloc: aligned; its rows are fy.n_out floats
            back = [cols_class(info["by_W"], info["fy_n_out"], True), rows_class(info["bx_W"])]
            ran("k_band_cols", "k_band_rows")
    return front, back, counts


def combination(front, back):
    fused = front[0].startswith("front pair")
    if not back:
        return "no PSF, fused" if fused else "no PSF, four-pass"
    if not fused:
        return "four-pass front + PSF"
    return "fused front + four-pass back" if back[0].startswith("cols") else "fused front + stencil" if back[0].startswith("psf") \
        else "fused front + back pair"


def check(out, ref, K, what):
    """|out - ref| <= K 2^-24 ref at every pixel (exactly 0 where ref is); returns the worst err / bound."""
    assert out.shape == ref.shape and np.all(np.isfinite(out)), what
    err, bound = np.abs(out.astype(np.float64) - ref), K * U * ref
    assert np.array_equal(out[ref == 0], np.zeros(np.count_nonzero(ref == 0), np.float32)), (what, "not 0 outside the support")
    live = ref > 0
    ratio = float(np.max(err[live] / bound[live])) if live.any() else 0.0
    assert ratio <= 1.0, (what, "err / bound = %.3f" % ratio, "at", np.unravel_index(np.argmax(err - bound), ref.shape))
    return ratio


@functools.lru_cache(maxsize=None)
def run_case(ops, c):
    """The case in the form the dispatch picks and, where a fused form fits, again under the detect_4pass switch: the launches
    are the ones `dispatch` predicts, every image meets the bound.  Returns (front classes, back classes, worst err / bound)."""
    Nx, Ny, ov, fwhm, psf, margin, off = c
    nx, ny = Nx // ov, Ny // ov
    plan = ops.DetectorPlan(Nx, Ny, ov, nx, ny, fwhm / 2.355, psf, margin=margin)
    info = plan.info()
    K = info["fx_W"] + info["fy_W"] + info["bx_W"] + info["by_W"] + 8
    data = inputs(ops, c)
    imgs = [shifted(img, off) for img, _ in data]
    worst, forms = 0.0, None
    try:
        for forced in (False, True) if (info["front_ok"] or info["back_ok"]) else (False,):
            front, back, want = dispatch(info, c, forced)
            if forced:
                ops.debug_switch("detect_4pass", 1)
                assert set(want) == {"k_band_cols", "k_band_rows"}
            else:
                forms = (front, back)
            outs = []
            got = profile_counts(lambda: outs.append(plan.detect(imgs[0])))
            got = {k: v for k, v in got.items() if k in ("k_band_cols", "k_band_rows", "k_band_pair", "k_psf_tile")}
            assert got == want, (ident(c), "forced" if forced else "free", info, "launched", got, "expected", want)
            outs += [plan.detect(im) for im in imgs[1:]]
            ops.check_status(imgs[0].device, "detector")
            for k, (o, (_, ref)) in enumerate(zip(outs, data)):
                assert o.shape == (nx, ny)
                worst = max(worst, check(o.cpu().numpy(), ref, K, (ident(c), "forced" if forced else "free", "image %d" % k)))
    finally:
        ops.debug_switch("detect_4pass", 0)
        plan.close()
    return forms[0], forms[1], worst


@pytest.mark.parametrize("c", CASES, ids=ident)
def test_every_form_meets_the_bound(ops, c):
    front, back, worst = run_case(ops, c)
    print("\n%s: %s%s [%s], worst err / bound %.3f" % (ident(c), " + ".join(front), " | " + " + ".join(back) if back else "",
                                                      combination(front, back), worst))


def test_cases_reach_every_form(ops):
    """Every instantiation the host side of detect.hip can launch, and every combination of stages, is run by some case."""
    ran, combos, worst = set(), set(), (-1.0, "")
    for c in CASES:
        front, back, w = run_case(ops, c)
        ran.update(front + back)
        combos.add(combination(front, back))
        worst = max(worst, (w, ident(c)))
    want = (["cols<%d>" % w for w in (8, 16, 32, 64, 128)] + ["cols_v4<%d>" % w for w in (8, 16, 32, 64)]
            + ["rows<%d>" % w for w in (4, 8, 16, 0)] + ["front pair<%d>" % w for w in (4, 8, 12, 16)]
            + ["back pair<%d>" % w for w in (4, 8, 12, 16)] + ["psf_tile<%d>" % q for q in (3, 4, 5)])
    assert sorted(ran) == sorted(want), ("missing", sorted(set(want) - ran), "unknown", sorted(ran - set(want)))
    want_combos = {"no PSF, fused", "no PSF, four-pass", "fused front + stencil", "fused front + four-pass back",
                   "four-pass front + PSF", "fused front + back pair"}
    assert combos == want_combos, ("missing", sorted(want_combos - combos))
    print("\nworst err / bound of the file: %.3f (%s)" % worst)


# ten tiny cases over every combination of stages; the last two are never fused
MANY = [case(4, 4, 2, 0, 0), case(18, 16, 2, 5.0, 0), case(5, 3, 1, 1.3, 0), case(128, 8, 1, 0, 0.4), case(240, 4, 2, 0.4, 2.4),
        case(128, 8, 1, 0, 2.7), case(4, 4, 2, 0, 1.2, 0), case(16, 12, 1, 3.0, 2.0, 0), case(6, 6, 3, 0.4, 1.7),
        case(16, 6, 1, 3.0, 1.2, 3)]
assert set(MANY) <= set(CASES)


@pytest.mark.parametrize("c", MANY, ids=ident)
def test_images_of_a_call_are_each_the_single_detection(ops, c):
    """detect_many of 2, 4 and 5 images (5: two calls) is bit for bit detect of each alone -- in one launch per fused stage
    where both stages are fused, one by one elsewhere, and one by one when an image of the call is not 16-byte aligned (the
    launches of that call are the three images' own: `dispatch` for a misaligned image, times three)."""
    Nx, Ny, ov, fwhm, psf, margin, _ = c
    plan = ops.DetectorPlan(Nx, Ny, ov, Nx // ov, Ny // ov, fwhm / 2.355, psf, margin=margin)
    info = plan.info()
    front, back, _ = dispatch(info, c, False)
    g = torch.Generator(device="cuda").manual_seed(Nx * 7 + Ny)
    imgs = [torch.rand((Nx, Ny), generator=g, device="cuda") * (3.0 + k) + 0.1 for k in range(5)]
    single = [plan.detect(im).clone() for im in imgs]
    for n in (2, 4, 5):
        outs = []
        got = profile_counts(lambda: outs.extend(plan.detect_many(imgs[:n])))
        shared = front[0].startswith("front pair") and not (back and back[0].startswith("cols"))
        if shared:      # the images of a call share each launch (4 a call)
            calls = (n + 3) // 4
            assert got.get("k_band_pair", 0) + got.get("k_psf_tile", 0) == calls * (2 if back else 1), (ident(c), n, got)
            assert "k_band_cols" not in got and "k_band_rows" not in got, (ident(c), n, got)
        for k in range(n):
            assert torch.equal(outs[k], single[k]), (ident(c), n, k)
    mis = shifted(imgs[1].cpu().numpy(), 1)
    outs = [torch.full_like(single[0], -1.0) for _ in range(3)]
    # one misaligned image decides for the call: every image takes the two-pass front on its own (no k_band_pair for the
    # front stage), then its own back stage -- two passes, or one k_psf_tile / k_band_pair launch per image, never shared
    front_m, back_m, one = dispatch(info, c[:6] + (1,), False)
    assert front_m[0].startswith("cols") and one["k_band_cols"] == one["k_band_rows"] == (2 if back_m and back_m[0].startswith("cols") else 1)
    assert one.get("k_band_pair", 0) + one.get("k_psf_tile", 0) == (1 if back_m and not back_m[0].startswith("cols") else 0)
    res = []
    got = profile_counts(lambda: res.extend(plan.detect_many([imgs[0], mis, imgs[2]], outs)))
    got = {k: v for k, v in got.items() if k in ("k_band_cols", "k_band_rows", "k_band_pair", "k_psf_tile")}
    assert got == {k: 3 * v for k, v in one.items()}, (ident(c), "misaligned", info, "launched", got, "one image", one)
    for k in range(3):
        assert res[k] is outs[k] and torch.equal(outs[k], single[k]), (ident(c), "misaligned", k)
    plan.close()
    ops.check_status(imgs[0].device, "detector")
