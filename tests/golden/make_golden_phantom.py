#!/usr/bin/env python3
"""The reference's contrast phantom (Samples/generateContrastPhantom.py, run unmodified) -> tests/golden/phantom.npz.

Run, in the build container only, with an interpreter that has scikit-image 0.18 (the generator's `radon`):
        python3.9 tests/golden/make_golden_phantom.py
The module's `radon` is wrapped so that every call records its input slice (as uint8: it holds 0 and 1 only) and its
output line.  Per case "c<i>_": the arguments, the host scalars the generator derives, the tube and support row ranges
(Python slice semantics), the 13 slices, the 13 lines and the 13 maps it returns.  The too-small case stores only that it
raised.  The id17 grid stores the lines and row ranges only (its maps alone would be 312 MB).
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/CodePython"
sys.dont_write_bytecode = True
os.environ["MPLBACKEND"] = "Agg"
import numpy as np  # noqa: E402

_nb = types.ModuleType("numba")
_nb.jit = lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))
sys.modules["numba"] = _nb
for _name in ["fabio", "fabio.edfimage", "fabio.tifimage"]:
    sys.modules[_name] = types.ModuleType(_name)
import matplotlib  # noqa: E402

matplotlib.use("Agg")
from matplotlib import pyplot as plt  # noqa: E402

plt.show = lambda *a, **k: None
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "Samples"))
import generateContrastPhantom as GCP  # noqa: E402

SMALL = [(48, 160, 250.0, 30.0), (64, 171, 230.0, 50.0), (40, 200, 197.5, 0.0), (40, 160, 250.0, 90.0),
         (56, 181, 240.0, 137.5), (30, 160, 250.0, 30.0)]
TOO_SMALL = (40, 100, 250.0, 30.0)
ID17 = (1000, 3000, 11.710455764075068, 30.0)

_calls = []
_radon = GCP.radon


def _recording_radon(image, theta, *a, **k):
    out = _radon(image, theta, *a, **k)
    _calls.append((np.asarray(image).astype(np.uint8), np.asarray(out, dtype=np.float64).copy()))
    return out


GCP.radon = _recording_radon


def host_scalars(dimX, dimY, pixsize, angle):
    """The generator's scalars, by its own expressions (generateContrastPhantom.py:21-48, 67-70)."""
    p = pixsize / 1000
    r = 2 / p
    R = 15 / p
    h = int(10 / 2 // p)
    origin = dimY / 2 - 16 / p
    centres = np.asarray([[22, 7], [16.4, 4.7], [10, 7], [6, 12.5], [6, 19.5], [10, 25], [16.4, 27], [22, 25], [21, 16],
                          [11, 16], [16, 11], [16, 21]], dtype=np.float64) / p + origin
    return dict(pix_mm=p, r=r, rint=int(np.floor(r) + 2), R=R, Rint=int(np.floor(R) + 2), h=h, origin=origin,
                centres=centres, icentres=np.array([[int(np.round(c)) for c in row] for row in centres]),
                support_end=int(np.round(27 / p + origin)), cos=np.cos(np.deg2rad(angle)), sin=np.sin(np.deg2rad(angle)),
                center=dimY // 2)


def main():
    out = {}
    for i, case in enumerate(SMALL + [ID17]):
        dimX, dimY, pix, angle = case
        _calls.clear()
        geom, params = GCP.generateContrastPhantom(dimX, dimY, pix, angle)
        assert len(_calls) == 13
        pre = "c%d_" % i if case != ID17 else "id17_"
        out[pre + "args"] = np.array(case, dtype=np.float64)
        for k, v in host_scalars(*case).items():
            out[pre + k] = np.asarray(v)
        h = out[pre + "h"].item()
        out[pre + "tube_rows"] = np.array(slice(dimX // 2 - h, dimX // 2 + h).indices(dimX))
        out[pre + "support_rows"] = np.array(slice(dimX // 2, dimX // 2 + h).indices(dimX))
        out[pre + "lines"] = np.stack([line[:, 0] for _, line in _calls])
        if case != ID17:
            out[pre + "slices"] = np.packbits(np.stack([s for s, _ in _calls]), axis=-1)
            out[pre + "maps"] = np.stack([np.asarray(g) for g in geom]).astype(np.float64)
        else:
            g = np.stack([np.asarray(g) for g in geom])
            out[pre + "row_nonzero"] = (g != 0).any(axis=2)            # [13, dimX]: which rows hold anything
            out[pre + "row0"] = g[:, int(out[pre + "tube_rows"][0])].astype(np.float64) if h else g[:, 0]
            del g
        if i == 0:
            out["params_smallTubesRadius"] = np.array(params["smallTubesRadius"][0])
            out["params_supportRadius"] = np.array(params["supportRadius"][0])
            out["params_tubes_centers"] = np.array(params["tubes centers"][0], dtype=np.float64)
            out["params_units"] = np.array([params["smallTubesRadius"][1], params["supportRadius"][1],
                                            params["tubes centers"][1]])
        print(case, "done", flush=True)
    try:
        GCP.generateContrastPhantom(*TOO_SMALL)
        raised = ""
    except ValueError as exc:
        raised = str(exc)
    out["too_small_args"] = np.array(TOO_SMALL, dtype=np.float64)
    out["too_small_message"] = np.array(raised)
    out["n_small"] = np.array(len(SMALL))
    np.savez_compressed(os.path.join(HERE, "phantom.npz"), **out)


if __name__ == "__main__":
    main()
