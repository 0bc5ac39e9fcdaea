"""GPU: the dark-field re-splat (paresis_amd/csrc/darkfield.hip) at every reach and in every form it is built in, per pixel
against the float64 oracle of tests/_darkfield_oracle.py: |out - ref| <= bound(reach) * S, S = |I2| + sum of |terms|.

Every bound is 4 x a yardstick measured on the CPU (the table in that module; tests/test_darkfield_host.py reproduces it and
proves that the cases reach all 29 bodies of k_df_gather_tiled and the band layouts of k_df_gather_banded), or the derived
single-source bound written beside it.  Exact statements (bit for bit) are derived from the kernels' code where they stand.

Run with -s: each test prints the worst error / bound it met (1.0 = at the bound)."""
import numpy as np
import pytest
import torch

from tests import _darkfield_oracle as do

pytestmark = pytest.mark.gpu

FAR = 2033                   # the smallest R whose window row does not fit the LDS budget: the global-memory gather


@pytest.fixture(scope="module")
def ops():
    from paresis_amd import ops as _ops
    from paresis_amd._lib import lib
    assert lib().psx_device_ok() == 1, lib().psx_last_error()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tables(ops, c):
    """(I2DF, DF32, prep) on the device through psx_darkfield_split_f32 (scale 1, no limit); the float32 widths and the
    table's half-sizes are the builder's."""
    I2DF = dev(c.I2DF)
    _, _, DF32, prep, _ = ops.darkfield_split(I2DF, dev(c.DF64), 1.0, 1.0, 1e9)
    assert np.array_equal(DF32.cpu().numpy(), c.DF32), c.name
    tab = prep.view(torch.float32).view(c.I2DF.shape + (2,)).cpu().numpy()
    assert np.array_equal(tab[..., 0], c.half), c.name
    return I2DF, DF32, prep


def prepared(ops, c, R, I2="case", **kw):
    """The case through darkfield_split + darkfield_blur_prepared, as a device tensor."""
    I2DF, DF32, prep = tables(ops, c)
    i2 = (None if c.I2 is None else dev(c.I2)) if isinstance(I2, str) else I2
    return ops.darkfield_blur_prepared(I2DF, DF32, prep, i2, R, **kw)


def blur(ops, c, R):
    """The case through darkfield_blur: k_df_prepare and patch sides from the float32 widths."""
    return ops.darkfield_blur(dev(c.I2DF), dev(c.DF32), None if c.I2 is None else dev(c.I2), R)


def ratio(ops, out, name):
    """max over the pixels of |out - ref| / (bound(reach) * S) for a named dense case; the status word must be clear."""
    ops.check_status(out.device)
    ref, S = do.reference(name)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    b = do.bound(do.ALL[name].reach)
    return float(np.max(np.where(S > 0, err / (b * np.where(S > 0, S, 1.0)), np.where(err == 0, 0.0, np.inf))))


def check(ops, worst, out, name, what):
    r = ratio(ops, out, name)
    worst[0] = max(worst[0], r)
    assert r <= 1.0, (name, what, r)


def test_parity_at_every_tiled_body(ops):
    """uniform k -> df_terms<k, true>, mixed k -> df_terms<k, false>, uniform 0 -> case 0: at the declared reach R = k and at
    R = 14, where Re = min(R, widest patch of the window) decides."""
    worst = [0.0]
    for name in do.CASES:
        k = int(name.split()[1])
        for R in sorted({k, 14}):
            check(ops, worst, prepared(ops, do.CASES[name], R), name, R)
    print("dark-field re-splat, 29 tiled bodies x R in (k, 14): worst error / bound %.3f" % worst[0])


def test_parity_banded(ops):
    """k_df_gather_banded: dense widths up to the reach (one, two, three and four bands), a wide declared R over narrow
    patches (only the tail of the column loop and the row-gap skip run), one wide source in a corner tile, a wide source
    without weight (must not widen a band's reach), and the tiled kernel's mixed cases through this kernel at R = 15."""
    worst = [0.0]
    for R in do.DENSE_R:
        check(ops, worst, prepared(ops, do.ALL["dense %d" % R], R), "dense %d" % R, R)
    print("dark-field re-splat, banded, dense R = %s: worst error / bound %.3f" % (do.DENSE_R, worst[0]))
    worst = [0.0]
    for R in do.NARROW_R:
        for m in range(6):
            check(ops, worst, prepared(ops, do.ALL["narrow %d" % m], R), "narrow %d" % m, R)
    print("dark-field re-splat, banded, widest patch 0 ... 5 under R = %s: worst error / bound %.3f" % (do.NARROW_R, worst[0]))
    worst = [0.0]
    for name in ("corner 20", "weightless 20"):
        check(ops, worst, prepared(ops, do.ALL[name], 20), name, 20)
    print("dark-field re-splat, banded, one h = 20 source with / without weight: worst error / bound %.3f" % worst[0])
    worst = [0.0]
    for k in range(1, 15):
        check(ops, worst, prepared(ops, do.ALL["mixed %d" % k], 15), "mixed %d" % k, 15)
    print("dark-field re-splat, banded, mixed 1 ... 14 at R = 15: worst error / bound %.3f" % worst[0])


@pytest.mark.parametrize("shape", do.SHAPES)
def test_parity_on_small_and_ragged_shapes(ops, shape):
    worst = [0.0]
    for kind, R in (("mixed 3", 3), ("uniform 14", 14), ("dense 17", 17)):
        name = "%s %dx%d" % ((kind,) + shape)
        check(ops, worst, prepared(ops, do.ALL[name], R), name, R)
    print("dark-field re-splat on %d x %d: worst error / bound %.3f" % (shape + (worst[0],)))


@pytest.mark.parametrize("R", [0, 3, 14, 17, FAR])
def test_zero_widths_are_a_plain_sum(ops, R):
    """All widths zero: every source deposits on itself, out == I2DF + I2 bit for bit in case 0, in the banded kernel's
    single-entry tail (exp2(0) = 1, w * 1 + 0) and in the global gather's h == 0 branch; through both entry points."""
    c = do.ALL["uniform 0"]
    want = c.I2DF + c.I2
    assert np.array_equal(prepared(ops, c, R).cpu().numpy(), want)
    assert np.array_equal(blur(ops, c, R).cpu().numpy(), want)
    ops.check_status(torch.device("cuda", torch.cuda.current_device()))


def _window(out, pos, h):
    """The (2h + 1)^2 neighbourhood of pos, NaN where it leaves the image; and the image with that neighbourhood zeroed."""
    Nx, Ny = out.shape
    P = np.full((2 * h + 1, 2 * h + 1), np.nan)
    i0, i1 = max(0, pos[0] - h), min(Nx, pos[0] + h + 1)
    j0, j1 = max(0, pos[1] - h), min(Ny, pos[1] + h + 1)
    P[i0 - pos[0] + h:i1 - pos[0] + h, j0 - pos[1] + h:j1 - pos[1] + h] = out[i0:i1, j0:j1]
    rest = out.copy()
    rest[i0:i1, j0:j1] = 0
    return P, rest


def _same_where_both(a, b):
    m = np.isfinite(a) & np.isfinite(b)
    return np.array_equal(a[m], b[m])


@pytest.mark.parametrize("pos", do.SINGLE_POS)
def test_one_source_draws_a_symmetric_normalised_patch(ops, pos):
    """One weighted source on 64 x 64, placed so that mirror pixels fall in different tiles and bands, or so that the border
    clips the patch.  A term depends on di^2 + dj^2 alone and every other term of an output is +0: the patch is bit for bit
    symmetric under both sign flips and the transpose; it is the oracle's patch within the derived single-source bound, sums
    to the weight within (2h + 1)^2 2^-24 where it is not clipped, and nothing lands outside it.  With a second, distant
    h = 0 source the tiles that see it take the non-uniform body and the banded kernel another band reach: the same bits."""
    worst = 0.0
    for h, R in [(k, k) for k in range(1, 15)] + [(17, 17), (40, 40)]:
        c, _ = do.single(pos, h)
        if R <= 14:
            assert do.selection(c.I2DF, c.half, R) <= {(h, True), (0, True)}
        out = prepared(ops, c, R).cpu().numpy()
        P, rest = _window(out, pos, h)
        assert not rest.any(), (h, pos)
        seen = np.isfinite(P)
        assert _same_where_both(P, P[::-1]) and _same_where_both(P, P[:, ::-1]) and _same_where_both(P, P.T), (h, pos)
        w = float(c.I2DF[pos])
        want = w * do.patch(c.DF32[pos], h)
        r = np.max(np.abs(P - want)[seen] / (do.single_bound(c.DF32[pos], h) * want)[seen])
        worst = max(worst, float(r))
        assert r <= 1.0, (h, pos, r)
        if seen.all():
            assert abs(P.sum() - w) <= (2 * h + 1) ** 2 * do.U * w, (h, pos)
        c2, other = do.single(pos, h, second=True)
        if c2 is None:
            continue
        if R <= 14:
            assert (h, False) in do.selection(c2.I2DF, c2.half, R)
        out2 = prepared(ops, c2, R).cpu().numpy()
        assert out2[other] == c2.I2DF[other] and out[other] == 0
        out2[other] = 0
        assert np.array_equal(out2, out), (h, pos)
    ops.check_status(torch.device("cuda", torch.cuda.current_device()))
    print("dark-field re-splat, one source at %s, h = 1 ... 14, 17, 40: worst error / derived bound %.3f" % (pos, worst))


@pytest.mark.parametrize("name,R", [("mixed 3", 3), ("uniform 14", 14), ("dense 17", 17)])
def test_options_bit_for_bit(ops, name, R):
    """add=True is `out[p] + v` on the store, I2=None adds +0, and neither kernel has an atomic on its result."""
    c = do.ALL[name]
    plain = prepared(ops, c, R)
    assert torch.equal(prepared(ops, c, R), plain)                                  # two runs, equal bits
    pre = dev(np.random.default_rng(R).uniform(-5.0, 5.0, c.I2DF.shape).astype(np.float32))
    acc = pre.clone()
    assert prepared(ops, c, R, out=acc, add=True) is acc
    assert torch.equal(acc, pre + plain)
    into = torch.full_like(pre, 7.0)
    prepared(ops, c, R, out=into)                                                   # out without add: overwritten
    assert torch.equal(into, plain)
    none = prepared(ops, c, R, I2=None)
    assert torch.equal(none, prepared(ops, c, R, I2=torch.zeros_like(pre)))
    assert not torch.equal(none, plain)
    ops.check_status(pre.device)


@pytest.mark.parametrize("R", [3, 17, FAR])
@pytest.mark.parametrize("what", ["nan in I2", "inf weight"])
def test_nonfinite_results_raise_the_status_word(ops, R, what):
    """A NaN in I2 or an inf weight at the last pixel of a ragged tile raises PSX_STATUS_NONFINITE on the store of the tiled
    and banded kernels and in the scan that follows the global gather; the word is then clear again; with scan=False nothing
    is raised and the value is stored as it is."""
    c = do.mixed("flag", 3, (45, 40), 800)
    last = (44, 39)
    if what == "nan in I2":
        I2 = c.I2.copy()
        I2[last] = np.nan
        c = c._replace(I2=I2)
    else:
        I2DF = c.I2DF.copy()
        I2DF[last] = np.inf
        c = c._replace(I2DF=I2DF)
    device = torch.device("cuda", torch.cuda.current_device())
    ops.check_status(device)
    out = prepared(ops, c, R)
    with pytest.raises(Exception, match="nans or insane"):
        ops.check_status(device)
    ops.check_status(device)                         # cleared
    assert not torch.isfinite(out[last])
    quiet = prepared(ops, c, R, scan=False)
    ops.check_status(device)                         # nothing raised
    assert not torch.isfinite(quiet[last])
    assert torch.equal(torch.nan_to_num(quiet, nan=-1.0, posinf=-2.0), torch.nan_to_num(out, nan=-1.0, posinf=-2.0))


def test_blur_entry_point_with_float32_patch_sides(ops):
    """ops.darkfield_blur: k_df_prepare takes the patch side from the float32 width and marks the sources without weight;
    then the same gathers."""
    worst = [0.0]
    for name, R in (("uniform 0", 0), ("mixed 3", 3), ("uniform 14", 14), ("dense 17", 17)):
        check(ops, worst, blur(ops, do.ALL[name], R), name, R)
    print("dark-field re-splat through darkfield_blur (k_df_prepare): worst error / bound %.3f" % worst[0])


def test_global_gather_beyond_the_lds_budget(ops):
    """R = 2033: k_df_gather from global memory through both entry points, and its refusal to accumulate in place."""
    assert do.bands(FAR - 1) and not do.bands(FAR)
    c = do.ALL["far 3"]
    worst = [0.0]
    check(ops, worst, prepared(ops, c, FAR), c.name, "prepared")
    check(ops, worst, blur(ops, c, FAR), c.name, "blur")
    acc = torch.zeros(c.I2DF.shape, dtype=torch.float32, device="cuda")
    with pytest.raises(Exception, match="cannot be accumulated in place"):
        prepared(ops, c, FAR, out=acc, add=True)
    assert not acc.any()                             # refused before any launch
    ops.check_status(acc.device)
    print("dark-field re-splat, global gather at R = %d: worst error / bound %.3f" % (FAR, worst[0]))
