"""CPU-only proof that the per-pixel refraction bound of tests/_refraction_oracle.py is neither too tight nor too loose, on
every case tests/test_gpu_refraction_local.py runs (5 tile geometries x 7 frames x 4 phases, and the split calls):

(a) a numpy restatement of refract.hip's own arithmetic (float32 displacement from float64 differences, per-tile units with
    round-half-up, float32 write-out, far shares summed in float32 in two orders, or in the order-independent replay's unit)
    stays within the bound against the float64 scatter;
(b) each seeded wrong variant, applied only in the dim part of a frame, exceeds the bound at some pixel;
(c) the first three of them pass the old whole-frame norm max|out - ref| / max|ref| < 1e-5 on the frames with a wide
    intensity range (step, hot, absorber): the gap the per-pixel bound closes.  On the flat frames (tiny, huge) and on
    dark_tile a dropped far ray or a swapped weight pair is an O(1) error of an O(1) frame, which the old norm sees too;
    `frame_unit` changes nothing on a flat frame (every window holds the frame's maximum), so it is not seeded there.

Worst err / bound of the restatement per halo (max over frames, phases, both far orders; plain / add=True out_scale=0.37 /
order-independent / order-independent with a caller's scale / split), as printed by test_restatement_within_bound, which
also prints one line per (halo, frame) with the worst of each phase:
    halo  4: 0.9996 0.9948 0.9996 0.9998 0.9994     halo  6: 0.9999 0.9978 0.9999 0.9999 0.9987
    halo  8: 0.9995 0.9941 0.9993 0.9993 0.9968     halo 12: 0.9998 0.9933 0.9998 0.9998 0.9979
    halo 16: 0.9996 0.9826 0.9993 0.9999 0.9988
    ("plain" includes the further distances of the refract_multi cases and the refract_batch cases)
    (per frame, max over halos and phases: step 0.9999, hot 0.9999, absorber 0.9999, dark_tile 0.77, tiny 0.81, huge 0.77)
They sit just below 1 because the fixed-point term is sharp: a pixel that receives ONE dim share in a tile whose window holds a
bright source is off by up to exactly half that tile's unit, which is that pixel's whole allowance but for the float32 terms.
The wrong variants, smallest err / bound over the halos and the frames each is seeded on (test_wrong_variants_exceed_the_bound
prints every one, with the old norm beside it): drop_far 3.7e3, swap 2.1e2, frame_unit 3.4e3, phase32 2.1, empty_far 4.8e5,
split_skip 1.9e6; the largest old norm of the first three on step / hot / absorber is 6.2e-6 (swap), 2.2e-6 and 1.8e-6.
Excluded (clamp-flagged) pixels: 0 in every case."""
import numpy as np
import pytest

from oracle import paresis_oracle as orc
from tests import _refraction_oracle as ro
from tests._golden import load, relmax

WIDE = ("step", "hot", "absorber1", "absorber5")          # frames whose dim part is far below the frame maximum
OLD_TOL = 1e-5


def _model(fname, pname, H, **kw):
    f, phi, s, _ = ro.reference(fname, pname, H)
    clamp, margin = ro.clamp_margin(ro.phase(pname, H)[1], s.shape)
    return ro.kernel_model(f.I.astype(np.float32), phi, ro.DSCALE, clamp, margin, H, **kw)


def test_scatter_matches_fast_refraction_on_goldens():
    g = load("refraction.npz")
    for k in range(int(g["n"])):
        z, E, M, pix = (float(v) for v in g["%d/params" % k])
        h = pix * 1e-6
        for ver in ("v2", "v1"):
            out, Dx, Dy = orc.fast_refraction(g["%d/I" % k].copy(), g["%d/phi" % k].copy(), z, E, M, pix, ver)
            s = ro.scatter(g["%d/I" % k], g["%d/phi" % k], z / orc.k_refraction(E) / (h * M) / h, variant=ver)
            assert relmax(s.image, out) < 1e-10, (k, ver)
            assert relmax(s.image, g["%d/%s/out" % (k, ver)]) < 1e-9, (k, ver)
            assert np.max(np.abs(s.Dx - Dx)) <= 1e-10 * max(1.0, np.max(np.abs(Dx))), (k, ver)
            assert np.max(np.abs(s.Dy - Dy)) <= 1e-10 * max(1.0, np.max(np.abs(Dy))), (k, ver)
            assert np.array_equal(s.I_after, g["%d/%s/I_after" % (k, ver)]), (k, ver)
            assert np.all(s.S >= np.abs(s.image) * (1 - 1e-12)) and np.all((s.N > 0) | (s.image == 0))


def test_statistics_of_a_hand_made_scatter():
    """Three rays on a 20 x 20 grid (halo 4: one tile, nothing far): counts, sums and the far split by hand."""
    I = np.zeros((20, 20))
    phi = np.zeros((20, 20))
    I[5, 5], I[10, 10] = 2.0, 3.0
    s = ro.scatter(I, phi, 1.0, variant="v2", halo=4)
    assert s.N[5, 5] == 1 and s.N[6, 6] == 1 and s.N[10, 10] == 1 and s.S[5, 5] == 2.0 and s.A[10, 10] == 3.0 and s.N_far.sum() == 0
    phi = 0.25 * np.arange(20.0)[:, None] * np.ones((1, 20))             # Dx = 0.25 everywhere
    s = ro.scatter(I, phi, 1.0, variant="v2", halo=4)
    assert s.image[5, 5] == 1.5 and s.image[6, 5] == 0.5 and s.image[11, 10] == 0.75
    assert abs(s.A[6, 5] - 2.0 * 1.25) < 1e-6 and abs(s.A[5, 5] - 2.0 * 1.25) < 1e-6
    # a far share: grid of the halo-16 geometry, a ray thrown 40 pixels
    Nx, Ny = ro.grid(16)
    I = np.zeros((Nx, Ny))
    I[2, 3] = 1.0
    phi = np.zeros((Nx, Ny))
    phi[1, 3], phi[3, 3] = -40.5, 40.5                                   # Dx(2, 3) = 40.5
    s = ro.scatter(I, phi, 1.0, variant="v2", halo=16)
    assert s.image[42, 3] == 0.5 and s.image[43, 3] == 0.5
    assert s.N_far[42, 3] == 1 and s.N_near[42, 3] == 0 and s.N[42, 4] == 1 and s.S_far[42, 3] == 0.5 and s.S_far[43, 3] == 0.5 and s.S_near.sum() == 0


def test_unit_constants():
    """The tile unit and the replay's unit as refract.hip forms them (:322, det_unit_exp, det_scale_bits)."""
    assert ro.unit_of(1.0) == 2.0 ** -29 and ro.unit_of(1.999) == 2.0 ** -29 and ro.unit_of(2.0) == 2.0 ** -28
    assert ro.unit_of(2.0 ** -100) == 2.0 ** -120 and ro.unit_of(2.0 ** 100) == 2.0 ** 71 and ro.unit_of(0.0) == 0.0
    assert ro.det_unit(1.5) == 2.0 ** -29 and ro.det_unit(1.5, 3.0) == ro.unit_of(192.0) == 2.0 ** -22


@pytest.mark.parametrize("H", ro.HALOS)
def test_no_pixel_left_out(H):
    """The inputs are chosen so that no ray sits within a relative 2^-20 of a clamp: the GPU tests check EVERY pixel."""
    for fname in ro.FRAMES:
        for pname in ro.PHASES:
            s = ro.reference(fname, pname, H)[2]
            assert int(s.flagged.sum()) == 0, (H, fname, pname)
            if pname == "clamped":
                assert s.killed.sum() >= 8
            if pname in ("near", "far"):                                 # the further distances of refract_multi
                for dscale in (0.6 * ro.DSCALE, 0.35 * ro.DSCALE):
                    assert int(ro.reference(fname, pname, H, dscale)[2].flagged.sum()) == 0, (H, fname, pname, dscale)
    for which in ro.MASKS:
        for side in (0, 1):
            for pname in ("near", "far"):
                assert int(ro.split_reference("step", pname, H, which, side)[3].flagged.sum()) == 0
    for fname, dscale in (("step", ro.DSCALE), ("hot", 0.6 * ro.DSCALE)):
        assert int(ro.map_reference(fname, "far", H, dscale)[2].flagged.sum()) == 0
    # the flag itself: a ray put right at the clamp flags the pixels it reaches either way
    Nx, Ny = ro.grid(H)
    phi = np.zeros((Nx, Ny))
    phi[9, 7] = 2.0 * Nx * (1 + 2.0 ** -22)                              # Dx(8, 7) = Nx (1 + 2^-22), Dx(10, 7) = -that
    s = ro.scatter(np.ones((Nx, Ny)), phi, 1.0, variant="v2", halo=H)
    assert s.flagged[8, 7] and s.flagged[10, 7] and 2 <= s.flagged.sum() <= 16


@pytest.mark.parametrize("H", ro.HALOS)
def test_restatement_within_bound(H):
    worst = np.zeros(5)
    for fname in ro.FRAMES:
        per_phase = []
        for pname in ro.PHASES:
            per_phase.append(0.0)
            f, phi, s, _ = ro.reference(fname, pname, H)
            base = np.random.default_rng(5).uniform(0.0, 2.0, s.shape).astype(np.float32) * np.float32(np.max(f.I))
            calls = [({}, {}),
                     (dict(out_scale=0.37, base=base), dict(out_scale=0.37, base=base)),
                     (dict(det_u=ro.det_unit(np.max(f.I))), dict(det=True))]
            scale = 3.0 * np.max(f.I)
            if scale < 1e30:                                             # set_deterministic_scale takes nothing larger
                calls.append((dict(det_u=ro.det_unit(0, scale)), dict(det=True, det_scale=scale)))
            for c, (mk, bk) in enumerate(calls):
                bnd = ro.case_bound(fname, pname, H, **bk)
                ref = ro.f32(mk.get("out_scale", 1.0)) * s.image + (base.astype(np.float64) if "base" in mk else 0.0)
                for order in (0, 1):
                    r = ro.margin_of(np.abs(_model(fname, pname, H, order=order, **mk).astype(np.float64) - ref), bnd)
                    assert r < 1, (H, fname, pname, c, order, r)
                    worst[c] = max(worst[c], r)
                    per_phase[-1] = max(per_phase[-1], r)
        print("halo %2d %-9s restatement err / bound: %s" % (H, fname, "  ".join("%s %.4f" % kv for kv in zip(ro.PHASES, per_phase))))
    for which in ro.MASKS:
        for side, pname in ((0, "far"), (1, "far"), (0, "near"), (1, "near")):
            f, phi, m, s = ro.split_reference("step", pname, H, which, side)
            clamp, margin = ro.clamp_margin("v2", s.shape)
            out = ro.kernel_model(f.I_in, phi, ro.DSCALE, clamp, margin, H, side_mask=m, side=side)
            r = ro.margin_of(np.abs(out.astype(np.float64) - s.image), ro.bound(s, f.I))
            assert r < 1, (H, which, side, r)
            worst[4] = max(worst[4], r)
    # the other distances of the refract_multi cases, and the refract_batch cases (phase from a float32 map)
    for fname in ro.FRAMES:
        for pname in ("near", "far"):
            for dscale in (0.6 * ro.DSCALE, 0.35 * ro.DSCALE):
                f, phi, s, _ = ro.reference(fname, pname, H, dscale)
                clamp, margin = ro.clamp_margin(ro.phase(pname, H)[1], s.shape)
                out = ro.kernel_model(f.I.astype(np.float32), phi, dscale, clamp, margin, H)
                r = ro.margin_of(np.abs(out.astype(np.float64) - s.image), ro.case_bound(fname, pname, H, dscale))
                assert r < 1, (H, fname, pname, dscale, r)
                worst[0] = max(worst[0], r)
    for fname, dscale in (("step", ro.DSCALE), ("hot", 0.6 * ro.DSCALE)):
        f, phi, s = ro.map_reference(fname, "far", H, dscale)
        clamp, margin = ro.clamp_margin("v2", s.shape)
        r = ro.margin_of(np.abs(ro.kernel_model(f.I_in, phi, dscale, clamp, margin, H).astype(np.float64) - s.image), ro.bound(s, f.I))
        assert r < 1, (H, fname, "batch", r)
        worst[0] = max(worst[0], r)
    print("halo %2d restatement err / bound: plain %.4f add %.4f det %.4f det+scale %.4f split %.4f" % ((H,) + tuple(worst)))


# which frames each wrong variant is seeded on, and with which phase (it needs far rays, or an empty window, ...)
LIT = tuple(f for f in ro.FRAMES if f != "dark_tile")      # dark_tile's dim part holds no source: nothing to swap or round
# (phase32 moves a share by a few u |D|: the absorber's own allowance, ((nmat + 1) |la| + 4) u at |la| = 66 ... 80, is wider,
# and so is the unit of `tiny`, which the clamp of the tile exponent at 120 holds at 2^-20 of the intensity)
FLAT_SRC = ("step", "hot", "huge")
SEEDS = {"drop_far": (ro.FRAMES, "far"), "swap": (LIT, "near"), "frame_unit": (WIDE, "far"),
         "phase32": (FLAT_SRC, "near"), "empty_far": (("dark_tile",), "far")}


@pytest.mark.parametrize("H", ro.HALOS)
def test_wrong_variants_exceed_the_bound(H):
    for wrong, (frames, pname) in SEEDS.items():
        for fname in frames:
            f, phi, s, _ = ro.reference(fname, pname, H)
            bnd = ro.case_bound(fname, pname, H)
            out = _model(fname, pname, H, wrong=wrong, dim=f.dim).astype(np.float64)
            err = np.abs(out - s.image)
            r = ro.margin_of(err, bnd)
            if wrong in ("frame_unit", "empty_far"):                     # (the others' shares also land next to the dim part)
                assert np.all((err <= bnd) | f.dim), "confined to the dim tiles"
            print("halo %2d %-10s %-9s err / bound %.3g, old norm %.3g" % (H, wrong, fname, r, relmax(out, s.image)))
            assert r > 1, (H, wrong, fname, r)
            if wrong in ("drop_far", "swap", "frame_unit") and fname in WIDE:      # (c): the old norm does not see it
                assert relmax(out, s.image) < OLD_TOL, (H, wrong, fname)
    # the split call: side 1 skipped where side 0 holds nothing (the dim tiles of `step` with its bright rows on side 0)
    f, phi, m, s = ro.split_reference("step", "far", H, "bright0", 1)
    clamp, margin = ro.clamp_margin("v2", s.shape)
    out = ro.kernel_model(f.I_in, phi, ro.DSCALE, clamp, margin, H, side_mask=m, side=1, wrong="split_skip").astype(np.float64)
    r = ro.margin_of(np.abs(out - s.image), ro.bound(s, f.I))
    print("halo %2d split_skip err / bound %.3g" % (H, r))
    assert r > 1, (H, r)
