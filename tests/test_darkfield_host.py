"""CPU: the dark-field re-splat's test oracle (tests/_darkfield_oracle.py) against the reference's own patch loop, the proof
that its cases reach all 29 bodies of k_df_gather_tiled and the band layouts of k_df_gather_banded, and the yardstick table
the GPU bounds of tests/test_gpu_darkfield.py come from."""
import numpy as np
import pytest

from oracle import paresis_oracle as orc
from tests import _darkfield_oracle as do


def test_oracle_equals_the_per_source_patch_loop():
    """resplat() against the literal loop of RF2:168-186 built from create_gaussian_shape, on one small ragged case."""
    c = do.ALL["mixed 3 33x31"]
    Nx, Ny = c.I2DF.shape
    m = 4
    ref = np.zeros((Nx + 2 * m, Ny + 2 * m))
    sab = np.zeros_like(ref)
    df = c.DF32.astype(np.float64)
    for i in range(Nx):
        for j in range(Ny):
            v = float(c.I2DF[i, j])
            if v == 0:
                continue
            if df[i, j] != 0:
                patch = orc.create_gaussian_shape(df[i, j] / 2)
                h = patch.shape[0] // 2
                assert h == c.half[i, j]
                ref[m + i - h:m + i + h + 1, m + j - h:m + j + h + 1] += patch * v
                sab[m + i - h:m + i + h + 1, m + j - h:m + j + h + 1] += np.abs(patch * v)
            else:
                ref[m + i, m + j] += v
                sab[m + i, m + j] += abs(v)
    ref = ref[m:m + Nx, m:m + Ny] + c.I2
    sab = sab[m:m + Nx, m:m + Ny] + np.abs(c.I2)
    out, S = do.reference(c.name)
    assert np.max(np.abs(out - ref) / S) < 1e-14
    assert np.max(np.abs(S - sab) / S) < 1e-14
    assert np.array_equal(out, S)                    # all weights positive here: the yardstick is the result itself


def test_cases_reach_all_29_tiled_bodies():
    """uniform k selects exactly (k, true), mixed k exactly (k, false), at the declared reach R = k and at R = 14."""
    union = set()
    for name, c in do.CASES.items():
        kind, k = name.split()
        k = int(k)
        want = {(k, kind == "uniform")}
        for R in (k, 14):
            assert do.selection(c.I2DF, c.half, R) == want, (name, R)
        # through k_df_prepare, which marks the sources without weight -1: the same bodies
        assert do.selection(c.I2DF, np.where(c.I2DF != 0, c.half, -1), 14) == want, name
        union |= want
    assert union == {(0, True)} | {(k, u) for k in range(1, 15) for u in (False, True)}
    assert len(union) == 29


def test_selection_rule_on_hand_made_tiles():
    I2DF = np.ones((64, 64), dtype=np.float32)
    half = np.zeros((64, 64), dtype=np.int64)
    half[38, 38] = 5                                 # tile (1, 1); within 3 of no other tile, within 8 of all
    assert do.selection(I2DF, half, 3) == {(0, True), (3, False)}
    assert do.selection(I2DF, half, 8) == {(5, False)}
    I2DF[:] = 0
    I2DF[38, 38] = 1                                 # the only weight has the widest patch: uniform
    assert do.selection(I2DF, half, 14) == {(5, True)}
    assert do.selection(I2DF, np.full((64, 64), 9), 4) == {(4, True)}


def test_band_layouts():
    assert do.bands(15) == [62]
    assert do.bands(16) == [64]
    assert do.bands(17) == [62, 4]
    assert do.bands(31) == [43, 43, 8]
    assert do.bands(40) == [36, 36, 36, 4]
    assert do.bands(48) == [32, 32, 32, 32]
    assert do.bands(63) == [25] * 6 + [8]
    assert do.bands(2032) == [1] * 4096
    assert do.bands(2033) == []                      # the global-memory gather
    for R in range(15, 200):
        assert sum(do.bands(R)) == do.DT + 2 * R


def test_yardstick_table_is_reproduced():
    """|resplat_f32 - resplat| / S per reach, measured here, is the committed table (to 20 %: a numpy whose exp2f rounds a
    few arguments the other way moves the maximum over some thousand pixels by a few per cent), and every dense GPU case has
    an entry."""
    tab = do.measure_yardsticks()
    assert set(tab) == set(do.YARDSTICK)
    for reach in sorted(tab):
        print("reach %2d: yardstick %.3e (table %.3e)" % (reach, tab[reach], do.YARDSTICK[reach]))
        assert 0.8 * do.YARDSTICK[reach] <= tab[reach] <= 1.2 * do.YARDSTICK[reach], reach
    assert 5e-8 < do.YARDSTICK[0] < 7e-8 and 1e-6 < do.YARDSTICK[14] < 2e-6
    assert all(c.reach in do.YARDSTICK for c in do.ALL.values())


@pytest.mark.parametrize("h", list(range(1, 15)) + [17, 40])
def test_single_source_meets_the_derived_bound(h):
    """The float32 restatement of one source's patch stays within single_bound() of the float64 patch, term by term, and
    an unclipped patch sums to the weight within (2h + 1)^2 2^-24: the derivation of the oracle's docstring, checked."""
    pos = (31, 31)
    c, _ = do.single(pos, h)
    ref, S = do.resplat(c.I2DF, c.DF32, c.half, None)
    f32 = do.resplat_f32(c.I2DF, c.DF32, c.half, None).astype(np.float64)
    bnd = do.single_bound(c.DF32[pos], h)
    lo = [max(0, p - h) for p in pos]
    hi = [min(63, p + h) for p in pos]
    win = (slice(lo[0], hi[0] + 1), slice(lo[1], hi[1] + 1))
    b = bnd[lo[0] - pos[0] + h:hi[0] - pos[0] + h + 1, lo[1] - pos[1] + h:hi[1] - pos[1] + h + 1]
    assert np.all(np.abs(f32[win] - ref[win]) <= b * S[win])
    mask = np.ones_like(ref, dtype=bool)
    mask[win] = False
    assert not f32[mask].any() and not ref[mask].any()
    if h <= 31:                                      # unclipped on 64 x 64
        w = float(c.I2DF[pos])
        assert abs(ref.sum() - w) < 1e-14 * w
        assert abs(f32.sum() - w) <= (2 * h + 1) ** 2 * do.U * w
