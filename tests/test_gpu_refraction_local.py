"""The refraction kernels (k_refract_near*, k_refract_far*, the order-independent replay) held to a PER-PIXEL bound on frames
with a wide intensity range: |out - ref| <= bound at every pixel, reference and bound from tests/_refraction_oracle.py (numpy
float64 scatter; the bound is derived there term by term from refract.hip and proven able to fail by
tests/test_refraction_host.py).  The whole-frame norm max|out - ref| / max|ref| of the other refraction tests cannot see an
error confined to a region 1e-4 as bright as the frame's peak: a dropped far ray, a swapped weight pair, a tile with the wrong
fixed-point unit.

Grids: per tile geometry (halo H, tile T) the smallest with one interior tile, ragged last tiles and unequal axes,
(2T + H + 4) x (2T + H + 9) -- the interior tile is what reaches stage_interior, the hoisted phase differences and the
two-distances-per-pass path.  Frames, phases: _refraction_oracle.FRAMES / PHASES.  Every test prints its worst err / bound."""
import numpy as np
import pytest
import torch

from tests import _refraction_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from paresis_amd import ops as _ops
    from paresis_amd._lib import lib
    assert lib().psx_device_ok() == 1, lib().psx_last_error()
    yield _ops
    _ops.set_refract_halo(4)
    _ops.set_deterministic(False)
    _ops.set_deterministic_scale(0.0)


@pytest.fixture
def halo(ops, request):
    ops.set_refract_halo(request.param)
    yield request.param
    ops.set_refract_halo(4)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def host(t):
    return t.cpu().numpy().astype(np.float64)


def within(out, ref, bnd, what):
    """Every pixel inside its allowance; returns the worst err / bound."""
    o = host(out)
    assert np.all(np.isfinite(o)), what
    err = np.abs(o - ref)
    r = ro.margin_of(err, bnd)
    bad = np.argwhere(err > bnd)
    assert bad.size == 0, (what, "err / bound %.4g at %d pixels, first %s" % (r, len(bad), bad[0]))
    return r


def source(ops, f, phi):
    """The keyword arguments that state frame f with phase phi to refract / refract_multi, and its material stack."""
    kw = dict(I_in=None if f.I_in is None else dev(f.I_in), I0=1.0, phi_in=dev(phi, torch.float64))
    m = None
    if f.nmat:                                               # the absorber: attenuation only, the phase stays phi_in
        m = ops.MaterialStack(dev(f.T), cphase=[0.0] * f.nmat, catt=f.catt)
    return m, kw


def base_image(f, shape):
    return np.random.default_rng(5).uniform(0.0, 2.0, shape).astype(np.float32) * np.float32(np.max(f.I))


def case(fname, pname, H, dscale=ro.DSCALE):
    f, phi, s, allow = ro.reference(fname, pname, H, dscale)
    clamp, margin = ro.clamp_margin(ro.phase(pname, H)[1], s.shape)
    return f, phi, s, clamp, margin


HALO = pytest.mark.parametrize("halo", ro.HALOS, indirect=True)
FRAME = pytest.mark.parametrize("fname", ro.FRAMES)


@HALO
@FRAME
def test_refract_plain_maps_and_add(ops, halo, fname):
    """ops.refract on every phase: the plain call (the empty-window skip path on dark_tile), the call that also asks for the
    displacement maps and the zeroed input (which never skips), and add=True with out_scale=0.37 onto a random image."""
    worst = {}
    for pname in ro.PHASES:
        f, phi, s, clamp, margin = case(fname, pname, halo)
        m, kw = source(ops, f, phi)
        out = ops.refract(s.shape, m, ro.DSCALE, clamp, margin=margin, **kw)[0]
        worst[pname] = within(out, s.image, ro.case_bound(fname, pname, halo), (halo, fname, pname, "plain"))
        I_mut = kw["I_in"].clone() if f.I_in is not None else None
        kw2 = dict(kw, I_in=I_mut) if I_mut is not None else kw
        out2, Dx, Dy = ops.refract(s.shape, m, ro.DSCALE, clamp, margin=margin, want_D=True, I_mut=I_mut, **kw2)
        r = within(out2, s.image, ro.case_bound(fname, pname, halo), (halo, fname, pname, "with maps"))
        # D = (float)(float64 difference * scale): u |D|, the float64 differencing, and the 1e-12 cut on either side of it
        for got, ref in ((Dx, s.Dx), (Dy, s.Dy)):
            tol = ro.U * np.abs(ref) + 2.0 ** -50 * ro.DSCALE * np.max(np.abs(phi)) + 1.1e-12
            assert np.all(np.abs(host(got) - ref) <= tol), (halo, fname, pname, "D")
        if I_mut is not None:
            assert np.array_equal(I_mut.cpu().numpy(), np.where(s.killed, np.float32(0), f.I_in)), (halo, fname, pname, "I_mut")
        base = base_image(f, s.shape)
        out3 = ops.refract(s.shape, m, ro.DSCALE, clamp, margin=margin, out=dev(base), out_scale=0.37, add=True, **kw)[0]
        ref3 = ro.f32(0.37) * s.image + base.astype(np.float64)
        r3 = within(out3, ref3, ro.case_bound(fname, pname, halo, out_scale=0.37, base=base), (halo, fname, pname, "add"))
        worst[pname] = max(worst[pname], r, r3)
        ops.check_status(out.device)
    print("halo %2d %-9s err / bound: %s" % (halo, fname, "  ".join("%s %.4f" % kv for kv in worst.items())))


@HALO
@FRAME
def test_refract_multi(ops, halo, fname):
    """2 and 3 distances (halo >= 8: one pair, and a pair plus a single tail, in the interior tile).  With all rays near the
    images do not depend on the replay's order: each equals the one-distance call bit for bit."""
    scales = [ro.DSCALE, 0.6 * ro.DSCALE, 0.35 * ro.DSCALE]
    worst = 0.0
    for pname in ("near", "far"):
        f, phi, s, clamp, margin = case(fname, pname, halo)
        m, kw = source(ops, f, phi)
        for nd in (2, 3):
            outs = ops.refract_multi(s.shape, m, scales[:nd], clamp, margin=margin, **kw)
            for d in range(nd):
                sd = ro.reference(fname, pname, halo, scales[d])[2]
                worst = max(worst, within(outs[d], sd.image, ro.case_bound(fname, pname, halo, scales[d]),
                                          (halo, fname, pname, nd, d)))
                if pname == "near":
                    assert sd.N_far.sum() == 0
                    one = ops.refract(s.shape, m, scales[d], clamp, margin=margin, **kw)[0]
                    assert torch.equal(outs[d], one), (halo, fname, nd, d)
        ops.check_status(outs[0].device)
    print("halo %2d %-9s multi err / bound %.4f" % (halo, fname, worst))


@HALO
def test_refract_split(ops, halo):
    """The step frame split by a mask: bright rows on side 0 and dim rows on side 1 (a dim-only tile then has smax[0] == 0 and
    must still run side 1 in the unit of the window), the sides swapped, and everything on one side (the other image is zero
    to the bit: its bound is)."""
    worst = 0.0
    for pname in ("near", "far"):
        T, phi, variant = ro.phase_map(pname, halo)
        m = ops.MaterialStack(dev(T[None]), cphase=[ro.CPHASE], catt=[0.0])
        for which in ro.MASKS:
            f, _, mask, s0 = ro.split_reference("step", pname, halo, which, 0)
            s1 = ro.split_reference("step", pname, halo, which, 1)[3]
            clamp, margin = ro.clamp_margin(variant, s0.shape)
            o0, o1 = ops.refract_split(s0.shape, m, ro.DSCALE, clamp, dev(mask), margin=margin, I_in=dev(f.I_in))
            for o, s, side in ((o0, s0, 0), (o1, s1, 1)):
                worst = max(worst, within(o, s.image, ro.bound(s, f.I), (halo, pname, which, side)))
        ops.check_status(o0.device)
    print("halo %2d split err / bound %.4f" % (halo, worst))


@HALO
def test_refract_batch(ops, halo):
    """Two different frames (step, hot) over the same phase map in one launch, each at its own distance."""
    frames, scales = ("step", "hot"), (ro.DSCALE, 0.6 * ro.DSCALE)
    T, phi, variant = ro.phase_map("far", halo)
    m = ops.MaterialStack(dev(T[None]), cphase=[ro.CPHASE], catt=[0.0])
    refs = [ro.map_reference(fn, "far", halo, sc) for fn, sc in zip(frames, scales)]
    clamp, margin = ro.clamp_margin(variant, refs[0][2].shape)
    outs = ops.refract_batch(refs[0][2].shape, [m, m], scales, clamp, margin=margin, I_in=[dev(r[0].I_in) for r in refs])
    worst = [within(o, s.image, ro.bound(s, f.I), (halo, f.name)) for o, (f, _, s) in zip(outs, refs)]
    ops.check_status(outs[0].device)
    print("halo %2d batch err / bound %.4f %.4f" % (halo, worst[0], worst[1]))


@HALO
@FRAME
def test_refract_deterministic(ops, halo, fname):
    """The order-independent replay on the far phases: two runs equal bit for bit and both within the deterministic bound --
    with the unit from the call's own maximum, and (where the scale is one the library takes) from set_deterministic_scale."""
    worst = []
    try:
        ops.set_deterministic(True)
        for pname in ("far", "clamped"):
            f, phi, s, clamp, margin = case(fname, pname, halo)
            m, kw = source(ops, f, phi)
            scale = 3.0 * float(np.max(f.I))
            for sc in (0.0, scale) if scale < 1e30 and pname == "far" else (0.0,):
                ops.set_deterministic_scale(sc)
                a = ops.refract(s.shape, m, ro.DSCALE, clamp, margin=margin, **kw)[0]
                b = ops.refract(s.shape, m, ro.DSCALE, clamp, margin=margin, **kw)[0]
                assert torch.equal(a, b), (halo, fname, pname, sc)
                worst.append(within(a, s.image, ro.case_bound(fname, pname, halo, det=True, det_scale=sc),
                                    (halo, fname, pname, sc)))
            ops.check_status(a.device)
    finally:
        ops.set_deterministic(False)
        ops.set_deterministic_scale(0.0)
    print("halo %2d %-9s deterministic err / bound %s" % (halo, fname, " ".join("%.4f" % w for w in worst)))


def test_refraction_local_status_flag(ops):
    """A NaN inside the interior tile of the smallest grid raises the status flag, once; the tile whose window does not hold
    it (rows and columns from 2T on) is within its bound all the same."""
    T = ro.TILE[4]
    f, phi, s, clamp, margin = case("step", "near", 4)
    I = f.I_in.copy()
    I[T + 3, T + 5] = np.nan
    out = ops.refract(s.shape, None, ro.DSCALE, clamp, margin=margin, I_in=dev(I), phi_in=dev(phi, torch.float64))[0]
    with pytest.raises(Exception, match="nans or insane"):
        ops.check_status(out.device)
    ops.check_status(out.device)
    o = host(out)
    assert np.isnan(o[T + 3, T + 5])
    within(out[2 * T:, 2 * T:], s.image[2 * T:, 2 * T:], ro.case_bound("step", "near", 4)[2 * T:, 2 * T:], "clean tile")
