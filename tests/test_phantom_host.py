"""Contrast phantom, host side (no GPU): the scalars the generator hands its kernels, its output row ranges and its size
check, against what the reference's own generateContrastPhantom.py computed (tests/golden/phantom.npz); the fold cache's
byte bound."""
import numpy as np
import pytest
import torch

from tests._golden import load

SCALARS = ("pix_mm", "r", "rint", "R", "Rint", "h", "origin", "centres", "icentres", "support_end", "cos", "sin", "center")


def _cases(g):
    return ["c%d_" % i for i in range(int(g["n_small"]))] + ["id17_"]


def test_phantom_host_scalars_match_the_reference():
    from paresis_amd.Samples.generateContrastPhantom import phantom_scalars
    g = load("phantom.npz")
    for pre in _cases(g):
        dimX, dimY, pix, angle = (float(v) for v in g[pre + "args"])
        s = phantom_scalars(int(dimX), int(dimY), pix, angle)
        for k in SCALARS:
            got, want = np.asarray(s[k]), g[pre + k]
            if k in ("cos", "sin"):            # libm's last bit may differ between numpy builds
                assert abs(float(got) - float(want)) <= 2e-16, (pre, k, got, want)
            else:
                assert np.array_equal(got, want), (pre, k, got, want)
        assert tuple(s["tube_rows"]) == tuple(int(v) for v in g[pre + "tube_rows"][:2]), pre
        assert tuple(s["support_rows"]) == tuple(int(v) for v in g[pre + "support_rows"][:2]), pre


def test_phantom_wrapped_rows_follow_python_slices():
    """dimX = 30, h = 20: the tube rows slice(-5, 35) wrap to rows 25-29, as the reference's numpy slicing does."""
    from paresis_amd.Samples.generateContrastPhantom import phantom_desc, phantom_scalars
    s = phantom_scalars(30, 160, 250.0, 30.0)
    assert s["h"] == 20 and s["tube_rows"] == (25, 30) and s["support_rows"] == (15, 30)
    d = phantom_desc(30, 160, 250.0, 30.0)
    assert (d.tube_row0, d.tube_row1, d.support_row0, d.support_row1) == (25, 30, 15, 30)
    for m in range(13):
        assert 0 <= d.row0[m] <= d.row1[m] <= 160 and 0 <= d.col0[m] <= d.col1[m] <= 160


def test_phantom_too_small_raises_like_the_reference():
    from paresis_amd.Samples.generateContrastPhantom import phantom_scalars
    g = load("phantom.npz")
    msg = str(g["too_small_message"])
    assert msg == "Image too small for the contrast phantom size"
    with pytest.raises(ValueError, match=msg):
        phantom_scalars(*[float(v) for v in g["too_small_args"]])


def test_phantom_support_window_past_the_slice_raises_like_the_reference():
    """At 1 mm pixels a 32-pixel slice passes the size check (origin = 0) but the support's column window ends at 33: the
    reference's support loop reads sliceTotMat[:, 32] and raises IndexError; 33 pixels fit."""
    from paresis_amd.Samples.generateContrastPhantom import phantom_desc, phantom_scalars
    with pytest.raises(IndexError, match="index 32 is out of bounds for axis 1 with size 32"):
        phantom_scalars(8, 32, 1000.0, 30.0)
    d = phantom_desc(8, 33, 1000.0, 30.0)
    assert d.col1[12] == 33


def test_fold_cache_is_bounded_by_bytes_least_recently_used_out():
    from paresis_amd import ops

    class Fold:
        def __init__(self):
            self.T = torch.zeros((3, 8, 8), dtype=torch.float32)     # 768 bytes

    T1, T2, T3 = torch.zeros(1), torch.zeros(1), torch.zeros(1)
    c = ops.FoldCache(2 * 768)
    f1, f2, f3 = Fold(), Fold(), Fold()
    c.put((T1, (1.0,), (2.0,)), f1)
    c.put((T2, (1.0,), (2.0,)), f2)
    assert c.get((T1, (1.0,), (2.0,))) is f1                       # T1 most recently used now
    assert c.get((T1, (1.0,), (3.0,))) is None                     # coefficients by value
    c.put((T3, (1.0,), (2.0,)), f3)                                 # evicts T2
    assert len(c) == 2 and c.nbytes == 2 * 768
    assert c.get((T2, (1.0,), (2.0,))) is None
    assert c.get((T1, (1.0,), (2.0,))) is f1 and c.get((T3, (1.0,), (2.0,))) is f3
    assert c.get((torch.zeros(1), (1.0,), (2.0,))) is None          # the stack by identity
    c.clear()
    assert len(c) == 0 and c.nbytes == 0
