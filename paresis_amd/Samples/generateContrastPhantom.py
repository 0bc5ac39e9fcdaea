"""The contrast phantom (mirror of CodePython/Samples/generateContrastPhantom.py:17-113): 12 material tubes in a solid-water
support, rasterised on a dimY x dimY slice and projected at one angle, one thickness map per material.

`generateContrastPhantom` keeps the reference's name, arguments and units (pixsize in um) and returns the 13 maps as one
[13, dimX, dimY] float32 tensor in HBM (metres).  The host derives every scalar below by the reference's own expressions, in
its order and types (:21-48, 67-70); csrc/phantom.hip does the per-pixel work -- the rasterisation of :50-77 bit for bit and
the projection that scikit-image's `radon(slice, [angle])` (circle=True: the square slice is not padded) computes, without
ever storing the 13 slices.  The reference's figures (plt.show) are not drawn.

Slice windows are clipped to the slice before they reach the kernel (a bounds guard: it changes no result).  A window is
its disc's bounding box plus 2 pixels, and with origin >= 0 every disc lies inside the slice, so a window pixel below 0
(which the reference's numpy indexing wraps to the far edge) or past the slice is outside its disc, where the reference
writes nothing either.  Where the support's window reaches past the last column, the reference's support loop READS
sliceTotMat out of bounds (:73) and raises IndexError: phantom_scalars raises the same.
"""
import ctypes
from ctypes import c_double, c_int, c_void_p

import numpy as np
import torch

from .._lib import PSX_PHANTOM_TUBES, check, lib
from .._tensors import device

NSLICE = PSX_PHANTOM_TUBES + 1
SMALL_TUBES_RADIUS = 2     # mm
TUBES_HEIGHT = 10          # mm
SUPPORT_RADIUS = 15        # mm
TUBES_CENTERS0 = [[22, 7], [16.4, 4.7], [10, 7], [6, 12.5], [6, 19.5], [10, 25], [16.4, 27], [22, 25], [21, 16], [11, 16],
                  [16, 11], [16, 21]]


class PhantomDesc(ctypes.Structure):
    """psx_phantom_desc (include/paresis_hip.h)."""
    _fields_ = [("dimX", c_int), ("dimY", c_int),
                ("ci", c_double * NSLICE), ("cj", c_double * NSLICE),
                ("row0", c_int * NSLICE), ("row1", c_int * NSLICE), ("col0", c_int * NSLICE), ("col1", c_int * NSLICE),
                ("rad2", c_double * NSLICE),
                ("cos_a", c_double), ("sin_a", c_double), ("off_x", c_double), ("off_y", c_double),
                ("pix_mm", c_double),
                ("tube_row0", c_int), ("tube_row1", c_int), ("support_row0", c_int), ("support_row1", c_int)]


def phantom_scalars(dimX, dimY, pixsize, angle):
    """Every scalar of the generator, by its own expressions (generateContrastPhantom.py:21-48, 67-70, 90-103) and
    skimage's radon (its inverse map and rotation centre).  Raises the reference's ValueError when the slice is too small."""
    dimX, dimY = int(dimX), int(dimY)
    pixsize = pixsize / 1000                                    # um to mm
    r = SMALL_TUBES_RADIUS / pixsize                            # pix
    rint = int(np.floor(r) + 2)
    R = SUPPORT_RADIUS / pixsize
    Rint = int(np.floor(R) + 2)
    h = int(TUBES_HEIGHT / 2 // pixsize)
    origin = dimY / 2 - 16 / pixsize
    if origin < 0:
        raise ValueError("Image too small for the contrast phantom size")
    centres = np.asarray(TUBES_CENTERS0, dtype=np.float64) / pixsize + origin
    icentres = np.array([[int(np.round(c)) for c in row] for row in centres])
    support_end = int(np.round(27 / pixsize + origin))
    last_col = int(np.round(dimY / 2)) + Rint - 1                # the support loop's last column (:72), read at :73
    if last_col >= dimY:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (dimY, dimY))
    theta = np.deg2rad(np.asarray([angle], dtype=np.float64))[0]
    cos_a, sin_a = np.cos(theta), np.sin(theta)
    center = dimY // 2                                          # radon: padded_image.shape[0] // 2
    return dict(pix_mm=pixsize, r=r, rint=rint, R=R, Rint=Rint, h=h, origin=origin, centres=centres, icentres=icentres,
                support_end=support_end, cos=float(cos_a), sin=float(sin_a), center=center,
                off_x=float(-center * (cos_a + sin_a - 1)), off_y=float(-center * (cos_a - sin_a - 1)),
                tube_rows=slice(dimX // 2 - h, dimX // 2 + h).indices(dimX)[:2],
                support_rows=slice(dimX // 2, dimX // 2 + h).indices(dimX)[:2])


def phantom_desc(dimX, dimY, pixsize, angle):
    """The kernel's descriptor of phantom_scalars()."""
    s = phantom_scalars(dimX, dimY, pixsize, angle)
    d = PhantomDesc()
    d.dimX, d.dimY = int(dimX), int(dimY)
    clip = lambda v: min(max(int(v), 0), d.dimY)
    for m in range(PSX_PHANTOM_TUBES):                          # :52-59
        ci, cj = s["centres"][m]
        ii, ij = s["icentres"][m]
        d.ci[m], d.cj[m] = float(ci), float(cj)
        d.row0[m], d.row1[m] = clip(ii - s["rint"]), clip(ii + s["rint"])
        d.col0[m], d.col1[m] = clip(ij - s["rint"]), clip(ij + s["rint"])
        d.rad2[m] = s["r"] ** 2
    m = PSX_PHANTOM_TUBES                                       # :67-76, the support
    c = d.dimY / 2
    ic = int(np.round(c))
    d.ci[m] = d.cj[m] = c
    d.row0[m], d.row1[m] = clip(ic - s["Rint"]), clip(max(s["support_end"], ic - s["Rint"]))
    d.col0[m], d.col1[m] = clip(ic - s["Rint"]), clip(ic + s["Rint"])
    d.rad2[m] = s["R"] ** 2
    d.cos_a, d.sin_a, d.off_x, d.off_y = s["cos"], s["sin"], s["off_x"], s["off_y"]
    d.pix_mm = s["pix_mm"]
    t0, t1 = s["tube_rows"]
    s0, s1 = s["support_rows"]
    d.tube_row0, d.tube_row1 = t0, max(t0, t1)
    d.support_row0, d.support_row1 = s0, max(s0, s1)
    return d


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def contrast_phantom_lines(dimX, dimY, pixsize, angle):
    """(geometry [13, dimX, dimY] float32, lines [13, dimY] float64): the maps and the 13 projected lines behind them."""
    d = phantom_desc(dimX, dimY, pixsize, angle)
    dev = device()
    lines = torch.empty((NSLICE, d.dimY), dtype=torch.float64, device=dev)
    geom = torch.empty((NSLICE, d.dimX, d.dimY), dtype=torch.float32, device=dev)
    check(lib().psx_contrast_phantom_f32(ctypes.byref(d), c_void_p(lines.data_ptr()), c_void_p(geom.data_ptr()), _stream()),
          "psx_contrast_phantom_f32")
    return geom, lines


def contrast_phantom_slices(dimX, dimY, pixsize, angle):
    """Debug: the 13 rasterised slices [13, dimY, dimY] uint8 (0/1) in HBM.  Small grids only."""
    d = phantom_desc(dimX, dimY, pixsize, angle)
    out = torch.empty((NSLICE, d.dimY, d.dimY), dtype=torch.uint8, device=device())
    check(lib().psx_contrast_phantom_slices_u8(ctypes.byref(d), c_void_p(out.data_ptr()), _stream()),
          "psx_contrast_phantom_slices_u8")
    return out


def generateContrastPhantom(dimX, dimY, pixsize, angle):
    """(geometry [13, dimX, dimY] float32 in HBM, metres; parameters) -- generateContrastPhantom.py:17-113."""
    geometry, _ = contrast_phantom_lines(dimX, dimY, pixsize, angle)
    parameters = {}
    parameters['smallTubesRadius'] = (SMALL_TUBES_RADIUS, 'mm')
    parameters['supportRadius'] = (SUPPORT_RADIUS, 'mm')
    parameters['tubes centers'] = ([list(c) for c in TUBES_CENTERS0], 'mm')
    return geometry, parameters
