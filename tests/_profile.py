"""Which kernels a call launched, for the GPU tests that assert the form a dispatch chose."""
import ctypes

import torch

from paresis_amd import _lib


def profile_counts(run):
    """{kernel name: launches} of what run() launches, through psx_profile_*."""
    lib = _lib.lib()
    lib.psx_profile_enable(1)
    try:
        run()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 14)
        _lib.check(lib.psx_profile_summary(buf, len(buf)), "psx_profile_summary")
    finally:
        lib.psx_profile_enable(0)
    return {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines() if l.strip()}
