"""The out= count rule of the four speckle trackers (ops._tracker_args) at their smallest legal shapes.  It comes after the HBM
check, so it needs device tensors; it stops the call before any kernel is launched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_out_must_hold_the_trackers_own_count():
    from paresis_amd import _lib, ops
    ws = {'window': 1, 'search': 1}
    cases = ((ops.lcs, 3, 3, {}, 3, "three"), (ops.lcs_df, 4, 3, {}, 4, "four"), (ops.umpa, 1, 5, ws, 4, "four"),
             (ops.umpa_df, 1, 5, dict(ws, mean=[1.0]), 5, "five"))
    lib = _lib.lib()
    lib.psx_profile_enable(1)
    try:
        for fn, K, n, kw, count, word in cases:
            S = torch.ones((K, n, n), dtype=torch.float32, device="cuda")
            for held in (count - 1, count + 1):
                with pytest.raises(_lib.PsxError, match="out must hold %s tensors" % word):
                    fn(S, S, out=[torch.empty((n, n), dtype=torch.float32, device="cuda") for _ in range(held)], **kw)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 14)
        _lib.check(lib.psx_profile_summary(buf, len(buf)), "psx_profile_summary")
    finally:
        lib.psx_profile_enable(0)
    assert buf.value == b""                                           # no kernel of the library ran
