"""Times the contrast phantom and the material fold at id17_ContrastPhantom's grid (1000 x 3000, 11.71 um): the figures
DESIGN.md section 1 quotes.  One JSON line.

  python tools/phantom_fold_timing.py [--reps 10]

* phantom: generateContrastPhantom's two launches, HIP events around each call after one untimed call, median of --reps;
  plus the per-kernel split from psx_profile_* on one more call.
* fold of the phantom's 13 maps (156 MB read, 36 MB written) into [P_hi, P_lo, A]:
  - warm: --reps folds back to back (the inputs stay in the 256 MB Infinity Cache between calls), mean per fold;
  - cold: before each fold a 1 GiB buffer is written (evicting the maps from the L2 and the Infinity Cache), each fold
    timed alone, median.  This is the figure a position loop sees when other work runs between its folds.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from paresis_amd import ops  # noqa: E402
from paresis_amd._lib import lib  # noqa: E402
from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_lines  # noqa: E402

ARGS = (1000, 3000, 11.710455764075068, 30.0)


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed_each(fn, reps, before=None):
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = _events()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    geom, _ = contrast_phantom_lines(*ARGS)
    torch.cuda.synchronize()
    phantom = timed_each(lambda: contrast_phantom_lines(*ARGS), a.reps)
    lib().psx_profile_enable(1)
    contrast_phantom_lines(*ARGS)
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 14)
    lib().psx_profile_summary(buf, len(buf))
    lib().psx_profile_enable(0)
    kernels = {ln.split()[0]: float(ln.split()[2]) for ln in buf.value.decode().splitlines() if ln.strip()}

    maps = [geom[i] for i in range(13)]
    cp, ca = [-1e4 * (i + 1) for i in range(13)], [-10.0] * 13
    fold = lambda: ops.fold_materials(maps, cp, ca)
    fold()
    torch.cuda.synchronize()
    e0, e1 = _events()
    e0.record()
    for _ in range(a.reps):
        fold()
    e1.record()
    torch.cuda.synchronize()
    warm = e0.elapsed_time(e1) / a.reps
    sweep = torch.empty(1 << 28, dtype=torch.float32, device="cuda")          # 1 GiB
    cold = timed_each(fold, a.reps, before=lambda: sweep.fill_(1.0))
    nbytes = (13 + 3) * 4 * ARGS[0] * ARGS[1]
    print(json.dumps({
        "grid": ARGS, "reps": a.reps,
        "phantom_ms_median": round(statistics.median(phantom), 3), "phantom_kernels_ms": kernels,
        "fold13_warm_ms_mean": round(warm, 4), "fold13_cold_ms_median": round(statistics.median(cold), 4),
        "fold13_cold_GBps": round(nbytes / (statistics.median(cold) * 1e-3) / 1e9, 1),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
