"""A sample the user brings as a volume of material labels, projected at one angle (no counterpart in the reference).

labels [n, m, m] uint8: labels[z] is the slice of height z, in the orientation of contrast_phantom_slices and of
tomography.fbp's volume; label 0 is empty, label k + 1 is the sample's material k.  csrc/volume.hip projects it with the
contrast phantom's model -- scikit-image `radon(slice, [angle])`, circle=True: the slice sampled bilinearly along the rotated
rays -- into one thickness map per material on the study grid (the contract is in include/paresis_hip.h).  Study rows take
the nearest slice (no interpolation across slices); the study pixel may differ from the voxel by a factor of 1/64 to 64.
With dso, the distance in voxels from a point source to the rotation axis, the rays diverge from that source instead
(k_volume_project_cone): the study grid is then the virtual detector through the axis, a ray crosses slices, and the maps
hold path lengths along the rays.

radon's circle is checked here, once per volume, not in the kernel: a label outside (i - c)^2 + (j - c)^2 <= c^2,
c = m // 2, is refused.  With it the rotation axis is study column dimY // 2, as for the phantom.
"""
import numpy as np
import torch

from .. import ops
from .._lib import PSX_VOLUME_MAX_MAT
from .._tensors import device


class DeviceVolume:
    """A checked label volume in HBM with each slice's occupied box: what upload_volume returns."""

    def __init__(self, labels, box, nmat):
        self.labels, self.box, self.nmat = labels, box, nmat


def _as_tensor(labels):
    if isinstance(labels, torch.Tensor):
        return labels
    a = np.asarray(labels)
    if a.dtype != np.uint8:
        raise ValueError("a label volume is uint8, got %s" % a.dtype)
    return torch.from_numpy(np.ascontiguousarray(a))


def check_volume(labels, nmat):
    """ValueError unless labels (a numpy array or a tensor, on any device) is uint8 [n, m, m] with n <= 65535 and
    m <= 8192, holds no label above nmat (1 to 16) and none outside the inscribed circle.  -> the labels as a tensor."""
    nmat = int(nmat)
    if not 1 <= nmat <= PSX_VOLUME_MAX_MAT:
        raise ValueError("a label volume holds 1 to %d materials, got %d" % (PSX_VOLUME_MAX_MAT, nmat))
    t = _as_tensor(labels)
    if t.dtype != torch.uint8:
        raise ValueError("a label volume is uint8, got %s" % t.dtype)
    if t.dim() != 3 or t.shape[1] != t.shape[2] or not 1 <= t.shape[0] <= 65535 or not 1 <= t.shape[1] <= 8192:
        raise ValueError("a label volume is [n <= 65535, m, m] with m <= 8192, got shape %s" % (tuple(t.shape),))
    top = int(t.max())
    if top > nmat:
        raise ValueError("label %d in a volume of %d materials (label k + 1 is material k)" % (top, nmat))
    m = int(t.shape[1])
    d2 = (torch.arange(m, device=t.device) - m // 2) ** 2
    outside = (d2[:, None] + d2[None, :]) > (m // 2) ** 2
    if bool((t.ne(0).any(dim=0) & outside).any()):
        raise ValueError("the volume has a label outside the inscribed circle (i - c)^2 + (j - c)^2 <= c^2, c = %d: the "
                         "projection is scikit-image radon's, which takes the slice inside it" % (m // 2))
    return t


def occupied_box(labels):
    """[n, 4] int32 (row0, row1, col0, col1), half-open: the bounding box of the non-zero labels of each slice of a
    [n, m, m] tensor, zeros for an empty slice."""
    n, m = int(labels.shape[0]), int(labels.shape[1])
    occ = labels.ne(0)
    idx = torch.arange(m, device=labels.device, dtype=torch.int32)
    box = torch.empty((n, 4), dtype=torch.int32, device=labels.device)
    for col, axis in ((0, 2), (2, 1)):
        hit = occ.any(dim=axis)                                          # [n, m]: the rows (the columns) that hold a label
        box[:, col] = torch.where(hit, idx, m).amin(dim=1)
        box[:, col + 1] = torch.where(hit, idx + 1, 0).amax(dim=1)
    box[box[:, 1] <= box[:, 0]] = 0
    return box


def upload_volume(labels, nmat):
    """check_volume, then the labels in HBM with their boxes: once per volume, whatever the number of angles."""
    if isinstance(labels, DeviceVolume):
        if labels.nmat != int(nmat):
            raise ValueError("the volume was uploaded for %d materials, not %d" % (labels.nmat, int(nmat)))
        return labels
    t = check_volume(labels, nmat)
    t = (t if t.is_cuda else t.to(device())).contiguous()
    return DeviceVolume(t, occupied_box(t), int(nmat))


def volume_lines(labels, nmat, voxel_um, dimX, dimY, pixsize_um, angle, dso=None):
    """(geometry [nmat, dimX, dimY] float32 in HBM, metres; lines [nmat, dimX, dimY] float64, voxels; parameters)."""
    v = upload_volume(labels, nmat)
    geom, lines = ops.volume_project(v.labels, v.nmat, angle, (dimX, dimY), float(pixsize_um) / float(voxel_um),
                                     float(voxel_um) * 1e-6, want_lines=True, box=v.box, dso=dso)
    return geom, lines, _parameters(v, voxel_um)


def _parameters(v, voxel_um):
    return {'volumeShape': (tuple(int(x) for x in v.labels.shape), 'voxels'), 'voxelSize': (float(voxel_um), 'um')}


def getVolumeFromFile(labels, nmat, voxel_um, dimX, dimY, pixsize_um, angle, dso=None):
    """(geometry [nmat, dimX, dimY] float32 in HBM, metres; parameters): the volume `labels` (an array, a tensor or an
    upload_volume result) of voxel_um voxels at `angle` degrees on a dimX x dimY grid of pixsize_um pixels.  dso: None for
    the parallel beam, else the source's distance from the rotation axis in voxels (m <= dso <= 1e30)."""
    v = upload_volume(labels, nmat)
    geom = ops.volume_project(v.labels, v.nmat, angle, (dimX, dimY), float(pixsize_um) / float(voxel_um),
                              float(voxel_um) * 1e-6, box=v.box, dso=dso)
    return geom, _parameters(v, voxel_um)


def contrast_phantom_volume(dimX, dimY, pixsize_um):
    """The contrast phantom as a [dimX, dimY, dimY] uint8 label volume in HBM, its voxel the study pixel: label k + 1 on
    contrast_phantom_slices' slice k, the 12 tubes on phantom_scalars' tube rows and the support (label 13) on its
    support rows.  Projected at scale 1 it gives generateContrastPhantom's lines bit for bit."""
    from .generateContrastPhantom import NSLICE, contrast_phantom_slices, phantom_scalars
    s = phantom_scalars(dimX, dimY, pixsize_um, 0.0)
    slices = contrast_phantom_slices(dimX, dimY, pixsize_um, 0.0)
    vol = torch.zeros((int(dimX), int(dimY), int(dimY)), dtype=torch.uint8, device=slices.device)
    for k in range(NSLICE):
        r0, r1 = s["support_rows"] if k == NSLICE - 1 else s["tube_rows"]
        vol[r0:max(r0, r1)] += slices[k] * (k + 1)                     # the 13 slices are disjoint
    return vol
