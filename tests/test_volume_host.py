"""The labelled voxel volume without a GPU: the float64 oracle of tests/_volume_oracle.py against the phantom's restated
projection (tests/_fbp_oracle.radon_line) and through the filtered back-projection oracle, the C entry point's argument
errors, the loader's checks and the XML tags."""
import ctypes
import types

import numpy as np
import pytest

from tests import _fbp_oracle as fo
from tests import _volume_oracle as vo

ANGLES = (0.0, 90.0, 30.0, -45.0, 137.3)


@pytest.mark.parametrize("m", [1, 2, 5, 33])
def test_oracle_is_radon_line_per_material(m):
    """At s = 1 on a dimY = m grid the contract is k_phantom_lines' map of each material's indicator slice, bit for bit
    (random labels, out to the corners of the slice: the mask is the loader's, not the projection's)."""
    nmat = 3
    lab = vo.random_labels(2, m, nmat, seed=m, in_circle=False)
    for angle in ANGLES:
        _, lines = vo.project(lab, nmat, angle, (2, m), 1.0, 1.0)
        for z in range(2):
            for k in range(nmat):
                want = fo.radon_line((lab[z] == k + 1).astype(np.float64), angle)
                assert np.array_equal(lines[k, z], want), (m, angle, z, k)


def test_oracle_on_the_restated_phantom():
    slices = fo.phantom_slices(64, 500.0)
    assert slices.sum(axis=0).max() == 1                               # disjoint: one label per voxel says it all
    lab = np.zeros((64, 64), dtype=np.uint8)
    for k in range(13):
        lab[slices[k]] = k + 1
    for angle in ANGLES:
        geom, lines = vo.project(lab[None], 13, angle, (1, 64), 1.0, 5e-4)
        for k in range(13):
            assert np.array_equal(lines[k, 0], fo.radon_line(slices[k].astype(np.float64), angle)), (angle, k)
        assert geom.dtype == np.float32 and np.array_equal(geom, (lines * 5e-4).astype(np.float32))


def test_rows_take_the_nearest_slice():
    assert list(vo.rows(4, 4, 1.0)) == [0, 1, 2, 3] and list(vo.rows(5, 5, 1.0)) == [0, 1, 2, 3, 4]
    assert list(vo.rows(2, 6, 0.5)) == [0, 0, 1, 1, 2, 2]                 # floor(t + 0.5): -1.5 -> -1, -0.5 -> 0, 0.5 -> 1
    assert list(vo.rows(8, 3, 2.0)) == [2, 4, 6]
    lab = vo.random_labels(3, 5, 2, seed=1)
    geom, lines = vo.project(lab, 2, 30.0, (7, 4), 1.0, 1.0)
    assert list(vo.rows(3, 7, 1.0)) == [-2, -1, 0, 1, 2, 3, 4]
    assert not lines[:, [0, 1, 5, 6]].any() and not lines[:, 2].any() and lines[1, 4].any()      # slice 0 is empty


def _misclassified(truth, angles):
    """The chiral slice's value map projected per material by the oracle, reconstructed by fo.fbp and classified with
    thresholds halfway between the values: the fraction of the circle's voxels that differ from `truth`'s labels."""
    lab = vo.chiral_slice(64)
    sino = np.zeros((len(angles), 1, 64))
    for a, angle in enumerate(angles):
        _, lines = vo.project(lab[None], 2, angle, (1, 64), 1.0, 1.0)
        sino[a, 0] = vo.CHIRAL_VALUES[0] * lines[0, 0] + vo.CHIRAL_VALUES[1] * lines[1, 0]
    got = vo.classify(fo.fbp(sino, angles)[0])
    inside = vo.circle(64)
    return float((got != truth)[inside].mean()), got


def test_chiral_slice_comes_back_in_its_own_orientation():
    """Projection by this contract and reconstruction by the filtered back-projection contract share one orientation: at
    most 0.5 % of the voxels inside the circle misclassified (a cap; the reference pair alone gives 1 voxel of 3207 on its
    slice), while the mirrored and the transposed slice each miss by more than 5 %."""
    lab = vo.chiral_slice(64)
    angles = np.arange(60) * 3.0
    own, got = _misclassified(lab, angles)
    inside = vo.circle(64)
    flipped = float((got != lab[:, ::-1])[inside].mean())
    transposed = float((got != lab.T)[inside].mean())
    print("chiral slice: misclassified own %.4f, flipped %.4f, transposed %.4f" % (own, flipped, transposed))
    assert own <= 0.005
    assert flipped > 0.05 and transposed > 0.05


def _desc(**kw):
    from paresis_amd import ops
    d = ops.volume_desc(kw.pop("n", 2), kw.pop("m", 8), kw.pop("nmat", 2), 30.0, (kw.pop("dimX", 2), kw.pop("dimY", 8)),
                        kw.pop("s", 1.0), kw.pop("voxel_m", 1e-6))
    assert not kw
    return d


def test_argument_errors_without_gpu():
    """Every refusal is rc -1 with a message that names the entry; nothing is launched."""
    from paresis_amd import _lib
    lib = _lib.lib()
    buf = ctypes.c_void_p(64)                                             # never dereferenced: the checks come first

    def call(desc, labels=buf, geom=buf):
        rc = lib.psx_volume_project_u8(None if desc is None else ctypes.byref(desc), labels, None, geom, None)
        return rc, lib.psx_last_error().decode()

    for args, msg in (((None,), "null descriptor"), ((_desc(), None), "null labels"), ((_desc(), buf, None), "null labels"),
                      ((_desc(nmat=0),), "nmat=0"), ((_desc(nmat=17),), "nmat=17"), ((_desc(m=0),), "m=0"),
                      ((_desc(m=8193),), "m=8193"), ((_desc(n=0),), "n=0"), ((_desc(n=65536),), "n=65536"),
                      ((_desc(s=float("nan")),), "s=nan"), ((_desc(s=100.0),), "s=100"), ((_desc(s=0.01),), "s=0.01"),
                      ((_desc(dimY=(1 << 20) + 1),), "study grid"), ((_desc(dimX=0),), "study grid"),
                      ((_desc(nmat=16, dimX=1 << 18, dimY=1 << 19),), "too large"),
                      ((_desc(voxel_m=float("inf")),), "voxel_m")):
        rc, text = call(*args)
        assert rc == -1 and "psx_volume_project_u8" in text and msg in text, (msg, rc, text)
    assert _lib.ABI_VERSION >= 20 and _lib.PSX_VOLUME_MAX_MAT == 16


def test_check_volume_refusals():
    import torch
    from paresis_amd.Samples.getVolumeFromFile import check_volume, occupied_box
    good = vo.random_labels(3, 9, 2, seed=3)
    assert check_volume(good, 2).shape == (3, 9, 9)
    assert check_volume(torch.from_numpy(good), 16).dtype == torch.uint8
    with pytest.raises(ValueError, match="uint8"):
        check_volume(good.astype(np.int32), 2)
    with pytest.raises(ValueError, match="shape"):
        check_volume(good[:, :, :8], 2)
    with pytest.raises(ValueError, match="shape"):
        check_volume(good[0], 2)
    with pytest.raises(ValueError, match="label 2 in a volume of 1 materials"):
        check_volume(good, 1)
    with pytest.raises(ValueError, match="1 to 16 materials"):
        check_volume(good, 17)
    corner = good.copy()
    corner[1, 0, 8] = 1
    with pytest.raises(ValueError, match="outside the inscribed circle"):
        check_volume(corner, 2)
    edge = np.zeros((1, 9, 9), dtype=np.uint8)
    edge[0, 0, 4] = edge[0, 8, 4] = edge[0, 4, 0] = 1                    # on the circle: (i - 4)^2 + (j - 4)^2 = 16
    check_volume(edge, 1)
    box = occupied_box(torch.from_numpy(np.concatenate([edge, np.zeros_like(edge), good[2:]])))
    assert box.dtype == torch.int32 and box.tolist()[:2] == [[0, 9, 0, 5], [0, 0, 0, 0]]
    i, j = np.nonzero(good[2])
    assert box.tolist()[2] == [i.min(), i.max() + 1, j.min(), j.max() + 1]


SAMPLES_XML = """<listSamples>
    <sample>
        <name>bone_in_water</name>
        <myType>sample_of_interest</myType>
        <myGeometryFunction>getVolumeFromFile</myGeometryFunction>
        <myVolumeFile>%s</myVolumeFile>
        <myVoxelSize unit="um">2.5</myVoxelSize>
        <myMaterials>PMMA,Nylon</myMaterials>
    </sample>
    <sample>
        <name>in_memory</name>
        <myType>sample_of_interest</myType>
        <myGeometryFunction>getVolumeFromFile</myGeometryFunction>
        <myVoxelSize unit="um">4</myVoxelSize>
        <myMaterials>PMMA</myMaterials>
    </sample>
</listSamples>
"""


def test_volume_tags_are_parsed(tmp_path):
    from paresis_amd.Sample import AnalyticalSample
    path = str(tmp_path / "labels.npy")
    np.save(path, vo.random_labels(2, 5, 2, seed=0))
    (tmp_path / "Samples.xml").write_text(SAMPLES_XML % path)
    s = AnalyticalSample(str(tmp_path))
    s.myName = "bone_in_water"
    s.defineCorrectValuesSample()
    assert s.myGeometryFunction == "getVolumeFromFile" and s.myVolumeFile == path and s.myVoxelSize == 2.5
    assert s.myMaterials == ["PMMA", "Nylon"] and s.myVolume is None and s.myAngle == 30
    t = AnalyticalSample(str(tmp_path))
    t.myName = "in_memory"
    t.defineCorrectValuesSample()
    assert t.myVoxelSize == 4.0 and not hasattr(t, "myVolumeFile")
    with pytest.raises(ValueError, match="neither myVolume nor myVolumeFile"):
        t.volume_dev()
    t.myVolume = np.full((1, 3, 3), 2, dtype=np.uint8) * vo.circle(3).astype(np.uint8)
    with pytest.raises(ValueError, match="label 2 in a volume of 1 materials"):     # the check comes before the device
        t.volume_dev()


def test_tomography_takes_both_rotatable_samples_and_no_other():
    from paresis_amd import tomography
    for fn in ("generateContrastPhantom", "getVolumeFromFile"):
        s = types.SimpleNamespace(myGeometryFunction=fn)
        assert tomography._phantom(s) is s
    sphere = types.SimpleNamespace(myGeometryFunction="CreateSampleSphere")
    with pytest.raises(ValueError, match="generateContrastPhantom"):
        tomography._phantom(sphere)
    with pytest.raises(ValueError, match="three-dimensional description.*CreateSampleSphere"):
        tomography.project(sphere, 52.0, [0.0], (4, 4), 1.0)
