"""The divergent projection of a labelled voxel volume on the GPU (k_volume_project_cone, ops.volume_project(dso=...))
against the float64 oracle of tests/_cone_oracle.py, bit for bit, and against the parallel kernel at a far source."""
import numpy as np
import pytest
import torch

from tests import _cone_oracle as co
from tests import _volume_oracle as vo

pytestmark = pytest.mark.gpu

ANGLES = (0.0, 30.0, 45.0, 90.0, 135.0, 200.0, -17.0)
SCALES = (1.0 / 3.0, 1.0, 1.7)
NMATS = (1, 3, 16)
HEIGHTS = (1, 3, 8)
SIZES = (1, 2, 5, 33, 64, 65, 130)
FAR = 2.0 ** 70


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _dsos(m):
    return (float(m), 2.5 * m, FAR)


def _leaving_rays(n, m, dims, s, dso):
    """Study rows whose ray is inside [0, n) at some steps of the walk and outside at others."""
    z0 = (np.arange(dims[0]) - dims[0] // 2).astype(np.float64) * s
    g = np.array([co.magnification(dso, r, m // 2) for r in range(m)])
    z = n // 2 + np.floor(z0[:, None] * g[None, :] + 0.5)
    inside = (z >= 0) & (z < n)
    return int((inside.any(axis=1) & ~inside.all(axis=1)).sum())


@pytest.mark.parametrize("m", SIZES)
def test_kernel_matches_oracle(m):
    """Every angle at every scale, the source distance (m, 2.5 m, 2^70), the height, the material count and the study grid
    (smaller or larger than the volume) changing from one combination to the next: the float64 lines equal the oracle's bit
    for bit and the maps are its maps; a second call, a call with each slice's occupied box and a call without lines give the
    same bits; at 2^70 the maps are the parallel kernel's.  Some rays leave the volume through its top or bottom mid-walk."""
    from paresis_amd import ops
    from paresis_amd.Samples.getVolumeFromFile import occupied_box
    vols = {(n, nmat): vo.random_labels(n, m, nmat, seed=100 * n + m + nmat) for n in HEIGHTS for nmat in NMATS}
    dev = {k: torch.from_numpy(v).cuda() for k, v in vols.items()}
    leaving = 0
    voxel_m = 3.7e-6
    for i_s, s in enumerate(SCALES):
        for i_a, angle in enumerate(ANGLES):
            n, nmat = HEIGHTS[(i_s + i_a) % 3], NMATS[(i_a + i_a // 3) % 3]
            dso = _dsos(m)[(2 * i_s + i_a) % 3]
            dims = (max(1, n - 1), max(1, m - 3)) if (i_s + i_a // 4) % 2 else (n + 3, m + 6)
            lab, box = dev[n, nmat], occupied_box(dev[n, nmat])
            geom_ref, lines_ref = co.project(vols[n, nmat], nmat, angle, dims, s, voxel_m, dso)
            geom, lines = ops.volume_project(lab, nmat, angle, dims, s, voxel_m, want_lines=True, dso=dso)
            what = (m, n, s, angle, nmat, dims, dso)
            assert geom.shape == lines.shape == (nmat,) + dims and geom.dtype == torch.float32 and lines.dtype == torch.float64
            assert np.array_equal(_bits(lines.cpu().numpy()), _bits(lines_ref)), what
            assert np.array_equal(geom.cpu().numpy(), geom_ref), what
            leaving += _leaving_rays(n, m, dims, s, dso)
            geom2, lines2 = ops.volume_project(lab, nmat, angle, dims, s, voxel_m, want_lines=True, dso=dso)
            assert torch.equal(lines2, lines) and torch.equal(geom2, geom), what
            geom3, lines3 = ops.volume_project(lab, nmat, angle, dims, s, voxel_m, want_lines=True, box=box, dso=dso)
            assert torch.equal(lines3, lines) and torch.equal(geom3, geom), what
            assert torch.equal(ops.volume_project(lab, nmat, angle, dims, s, voxel_m, box=box, dso=dso), geom), what
            if dso == FAR:
                geom_p, lines_p = ops.volume_project(lab, nmat, angle, dims, s, voxel_m, want_lines=True, box=box)
                assert torch.equal(lines_p, lines) and torch.equal(geom_p, geom), what
    if m >= 5:
        assert leaving > 0


def test_divergence_shows():
    """The oracle's geometry on the device: of two equal blobs the one nearer the source comes out larger, and the same
    volume projects differently from the parallel beam."""
    from paresis_amd import ops
    n, m, dso = 11, 33, 33.0
    h = m // 2
    lab = np.zeros((n, m, m), dtype=np.uint8)
    lab[3:8, h - 12:h - 7, h - 7:h - 2] = 1
    lab[3:8, h + 8:h + 13, h + 3:h + 8] = 2
    t = torch.from_numpy(lab).cuda()
    geom = ops.volume_project(t, 2, 0.0, (31, 65), 1.0, 1.0, dso=dso).cpu().numpy()
    near, far = geom[0] > 0, geom[1] > 0
    assert near.any(axis=0).sum() >= far.any(axis=0).sum() + 2 and near.any(axis=1).sum() >= far.any(axis=1).sum() + 2
    flat = ops.volume_project(t, 2, 0.0, (31, 65), 1.0, 1.0).cpu().numpy()
    assert (flat[0] > 0).any(axis=0).sum() == (flat[1] > 0).any(axis=0).sum() == 5


def test_source_distance_is_checked():
    """dso below m, NaN and the infinities are refused by the library; the sample passes its distance in voxels."""
    from paresis_amd import ops
    from paresis_amd.Sample import AnalyticalSample
    lab = torch.from_numpy(vo.random_labels(2, 8, 2, seed=0)).cuda()
    for dso in (7.999, 0.0, -20.0, float("nan"), float("inf"), -float("inf"), 2e30):
        with pytest.raises(ops.PsxError, match="dso="):
            ops.volume_project(lab, 2, 0.0, (2, 8), 1.0, 1e-6, dso=dso)
    s = AnalyticalSample()
    s.myType, s.myGeometryFunction, s.myMaterials = "sample_of_interest", "getVolumeFromFile", ["a", "b"]
    s.myVolume, s.myVoxelSize, s.myAngle, s.mySourceDistance = lab, 250.0, 30.0, 0.005
    assert abs(s.source_distance_voxels() - 20.0) < 1e-12
    want = ops.volume_project(lab, 2, 30.0, (3, 9), 1.0, 250.0 * 1e-6, dso=s.source_distance_voxels())
    s.getMyGeometry((3, 9), 250.0, 1)
    assert torch.equal(s.geometry_dev(), want)
    s.mySourceDistance = None
    s.getMyGeometry((3, 9), 250.0, 1)
    assert torch.equal(s.geometry_dev(), ops.volume_project(lab, 2, 30.0, (3, 9), 1.0, 250.0 * 1e-6))
    assert not torch.equal(s.geometry_dev(), want)
