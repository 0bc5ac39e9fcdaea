"""The labelled voxel volume on the GPU (csrc/volume.hip, ops.volume_project, Samples/getVolumeFromFile.py, the Sample
class and paresis_amd.tomography) against the float64 oracle of tests/_volume_oracle.py, against the contrast phantom's own
kernels, and through the chain."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import _fbp_oracle as fo
from tests import _volume_oracle as vo
from tests._fbp_oracle import PHANTOM_DELTA

pytestmark = pytest.mark.gpu

ANGLES = (0.0, 90.0, 180.0, 270.0, 30.0, -45.0, 137.3)
SCALES = (1.0, 0.5, 2.0, 0.7)
NMATS = (1, 3, 9, 16)
SHAPES = [(1, 1), (2, 2), (3, 5), (2, 33), (5, 64), (2, 65), (1, 130)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


# -------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_oracle(shape):
    """Every angle at every scale, the material count and the study grid (smaller or larger than the volume) changing from
    one combination to the next: the float64 lines equal the oracle's bit for bit and the maps are its maps; rows outside
    [0, n) are exactly 0; a second call, a call with each slice's occupied box and a call without lines give the same bits."""
    from paresis_amd import ops
    from paresis_amd.Samples.getVolumeFromFile import occupied_box
    n, m = shape
    vols = {nmat: vo.random_labels(n, m, nmat, seed=100 * n + m + nmat) for nmat in NMATS}
    dev = {nmat: torch.from_numpy(v).cuda() for nmat, v in vols.items()}
    boxes = {nmat: occupied_box(t) for nmat, t in dev.items()}
    outside_rows = 0
    for i_s, s in enumerate(SCALES):
        for i_a, angle in enumerate(ANGLES):
            nmat = NMATS[(i_s + i_a) % 4]
            dims = (max(1, n - 1), max(1, m - 3)) if (i_s + i_a // 4) % 2 else (n + 3, m + 6)
            voxel_m = 3.7e-6
            geom_ref, lines_ref = vo.project(vols[nmat], nmat, angle, dims, s, voxel_m)
            geom, lines = ops.volume_project(dev[nmat], nmat, angle, dims, s, voxel_m, want_lines=True)
            what = (shape, s, angle, nmat, dims)
            assert geom.shape == lines.shape == (nmat,) + dims and geom.dtype == torch.float32 and lines.dtype == torch.float64
            assert np.array_equal(_bits(lines.cpu().numpy()), _bits(lines_ref)), what
            assert np.array_equal(geom.cpu().numpy(), geom_ref), what
            out = [x for x, z in enumerate(vo.rows(n, dims[0], s)) if not 0 <= z < n]
            outside_rows += len(out)
            assert not lines[:, out].any() and not geom[:, out].any(), what
            geom2, lines2 = ops.volume_project(dev[nmat], nmat, angle, dims, s, voxel_m, want_lines=True)
            assert torch.equal(lines2, lines) and torch.equal(geom2, geom), what
            geom3, lines3 = ops.volume_project(dev[nmat], nmat, angle, dims, s, voxel_m, want_lines=True, box=boxes[nmat])
            assert torch.equal(lines3, lines) and torch.equal(geom3, geom), what
            assert torch.equal(ops.volume_project(dev[nmat], nmat, angle, dims, s, voxel_m, box=boxes[nmat]), geom), what
    assert outside_rows > 0


def test_binding_checks_come_before_the_kernel():
    from paresis_amd import ops
    lab = torch.from_numpy(vo.random_labels(2, 5, 2, seed=0))
    with pytest.raises(ops.PsxError, match="HBM"):
        ops.volume_project(lab, 2, 0.0, (2, 5), 1.0, 1e-6)
    with pytest.raises(ops.PsxError, match="uint8"):
        ops.volume_project(lab.cuda().int(), 2, 0.0, (2, 5), 1.0, 1e-6)
    with pytest.raises(ops.PsxError, match=r"\[n, m, m\]"):
        ops.volume_project(lab.cuda()[:, :, :4].contiguous(), 2, 0.0, (2, 5), 1.0, 1e-6)
    with pytest.raises(ops.PsxError, match="box"):
        ops.volume_project(lab.cuda(), 2, 0.0, (2, 5), 1.0, 1e-6, box=torch.zeros((3, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ops.PsxError, match="nmat=17"):
        ops.volume_project(lab.cuda(), 17, 0.0, (2, 5), 1.0, 1e-6)
    # a label above nmat is the loader's to refuse; the kernel counts it as empty
    geom = ops.volume_project(lab.cuda(), 1, 30.0, (2, 5), 1.0, 1.0)
    only = lab.clone()
    only[only > 1] = 0
    assert torch.equal(geom, ops.volume_project(only.cuda(), 1, 30.0, (2, 5), 1.0, 1.0))


# ---------------------------------------------------------------------------------- the bridge to the phantom
DIMX, DIMY, PIX_UM, E_KEV = 24, 64, 500.0, 52.0
# beta at 52 keV of the 13 materials, the stand-ins of tests/test_gpu_fbp.py, copied
PHANTOM_BETA = (1.9e-10, 1.6e-10, 1.75e-10, 6.0e-11, 5.2e-11, 7.5e-11, 5.6e-11, 6.4e-11, 1.5e-10, 6.1e-11, 7.0e-14, 7.0e-14, 6.0e-11)


@pytest.fixture(scope="module")
def phantom_volume():
    from paresis_amd.Samples.getVolumeFromFile import contrast_phantom_volume
    vol = contrast_phantom_volume(DIMX, DIMY, PIX_UM)
    assert vol.shape == (DIMX, DIMY, DIMY) and vol.dtype == torch.uint8 and vol.is_cuda
    return vol


def test_phantom_volume_gives_the_phantom(phantom_volume):
    """contrast_phantom_volume through the new kernel: on each material's rows the float64 lines are k_phantom_lines'
    bit for bit, and every map is within one float32 ulp of generateContrastPhantom's (the phantom scales by
    pix_mm * 1e-3, this contract by voxel_m)."""
    from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_lines, phantom_scalars
    from paresis_amd.Samples.getVolumeFromFile import volume_lines
    sc = phantom_scalars(DIMX, DIMY, PIX_UM, 0.0)
    labels = phantom_volume.cpu().numpy()
    slices = fo.phantom_slices(DIMY, PIX_UM)
    t0, t1 = sc["tube_rows"]
    s0, s1 = sc["support_rows"]
    assert all(np.array_equal(labels[t0] == k + 1, slices[k]) for k in range(12)) and not labels[:t0].any()
    assert np.array_equal(labels[s0] == 13, slices[12]) and not labels[t1:].any() and s1 == t1
    for angle in (0.0, 30.0, 90.0, 137.3):
        geom, lines, _ = volume_lines(phantom_volume, 13, PIX_UM, DIMX, DIMY, PIX_UM, angle)
        pgeom, plines = contrast_phantom_lines(DIMX, DIMY, PIX_UM, angle)
        assert geom.shape == pgeom.shape == (13, DIMX, DIMY)
        for k in range(13):
            r0, r1 = (s0, s1) if k == 12 else (t0, t1)
            assert r1 > r0 and torch.equal(lines[k, r0:r1].view(torch.int64),
                                           plines[k].view(torch.int64).expand(r1 - r0, -1)), (angle, k)
            assert not lines[k, :r0].any() and not lines[k, r1:].any()
        a, b = geom.cpu().numpy(), pgeom.cpu().numpy()
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        worst = float((np.abs(a.astype(np.float64) - b) / ulp).max())
        print("angle %.1f: maps differ by at most %.1f ulp on %d of %d pixels" % (angle, worst, int((a != b).sum()), a.size))
        assert worst <= 1.0


def _phantom_sample():
    from paresis_amd.Sample import AnalyticalSample
    s = AnalyticalSample()
    s.myName, s.myType, s.myMaterials = "phantom", "sample_of_interest", ["m%d" % i for i in range(13)]
    s.myGeometryFunction = "generateContrastPhantom"
    s.delta = [[(E_KEV, d)] for d in PHANTOM_DELTA]
    s.beta = [[(E_KEV, b)] for b in PHANTOM_BETA]
    return s


def test_project_of_the_volume_sample_is_the_phantoms(phantom_volume):
    """tomography.project of a getVolumeFromFile sample holding the phantom's volume against the phantom sample, 13
    stand-in delta / beta: per pixel |dphi| <= 3 * 2^-24 * sum_k |c_k| T_k, and logT likewise -- one ulp of a map, and the
    rounding of the two float32 results.  The volume is uploaded once for all angles."""
    from paresis_amd import tomography
    from paresis_amd.getk import k_sample
    angles = [0.0, 30.0, 90.0, 137.3]
    ph = _phantom_sample()
    vs = _phantom_sample()
    vs.myGeometryFunction, vs.myVolume, vs.myVoxelSize = "getVolumeFromFile", phantom_volume, PIX_UM
    want = tomography.project(ph, E_KEV, angles, (DIMX, DIMY), PIX_UM)
    got = tomography.project(vs, E_KEV, angles, (DIMX, DIMY), PIX_UM)
    uploaded = vs.volume_dev()
    assert uploaded.labels.data_ptr() == phantom_volume.data_ptr() and vs.myAngle == 137.3
    k = k_sample(E_KEV)
    for a, angle in enumerate(angles):
        ph.myAngle = angle
        ph.getMyGeometry((DIMX, DIMY), PIX_UM, 1)
        T = ph.geometry_dev().double().cpu().numpy()
        for name, coeff in (("phi", k * np.array(PHANTOM_DELTA)), ("logT", 2 * k * np.array(PHANTOM_BETA))):
            bound = 3 * 2.0 ** -24 * np.einsum("k,kxy->xy", np.abs(coeff), T)
            diff = np.abs(got[name][a].double().cpu().numpy() - want[name][a].double().cpu().numpy())
            print("%s at %.1f: max |diff| %.3e, differing pixels %d, max diff / bound %.3f"
                  % (name, angle, diff.max(), int((diff > 0).sum()), float((diff / np.maximum(bound, 1e-300)).max())))
            assert np.all(diff <= bound), (name, angle)
    assert vs.volume_dev() is uploaded
    vs.myVolume = phantom_volume.clone()                              # another object: checked and uploaded again
    assert vs.volume_dev() is not uploaded


# -------------------------------------------------------------------------------------------------- chain
CH_DIMX, CH_M, CH_OV = 32, 64, 2
CH_DELTA, CH_BETA = (8.7e-8, 1.4e-7), (6.0e-11, 1.5e-10)            # beta in the ratio of vo.CHIRAL_VALUES
CH_ROWS = (4, 28)                                                    # the slices that hold the chiral slice; the others are empty


def _chiral_volume():
    vol = np.zeros((CH_DIMX, CH_M, CH_M), dtype=np.uint8)
    vol[CH_ROWS[0]:CH_ROWS[1]] = vo.chiral_slice(CH_M)
    return vol


def _membrane_maps(point):
    i, j = np.mgrid[0:CH_DIMX, 0:CH_M]
    pattern = np.sin(0.9 * i + 0.3 + 1.7 * point) * np.cos(0.7 * j + 0.9 * point)
    return np.stack([2e-6 * (1 + 0.5 * pattern), np.full((CH_DIMX, CH_M), 1e-4)]).astype(np.float32)


def _chiral_experiment():
    """A 32 x 64 study grid of 500 um pixels (oversampling 2: a 16 x 32 detector), monochromatic, in vacuum, no plate, no
    blur, ray tracing; the sample is the chiral two-material volume at study resolution (voxel = study pixel)."""
    from oracle import paresis_oracle as orc
    from tests._build import build_experiment
    M = (140.0 + 1.6 + 3.6) / (140.0 + 1.6)
    cfg = dict(scintillator=None, dSM=140.0, dMO=1.6, dOD=3.6, meanShotCount=30000.0, ov=CH_OV, pix_um=PIX_UM, M=M,
               inVacuum=True, N=(CH_DIMX, CH_M), spectrum=[(E_KEV, 1.0)], source_size_um=0.0, energy_sampling=1.0,
               det_dims=(CH_DIMX // 2, CH_M // 2), det_pix_um=PIX_UM * 2 * M, psf=0.0, bins=[],
               membrane=orc.Obj(_membrane_maps(0), [[5.0e-7], [9.9e-8]], [[3.0e-9], [5.3e-11]]),
               sample=orc.Obj(np.zeros((2, CH_DIMX, CH_M)), [[d] for d in CH_DELTA], [[b] for b in CH_BETA]),
               air=None, plate=None)
    exp = build_experiment(cfg, "RT", sample_materials=["square", "ell"])
    exp.exp_dict["nbExpPoints"] = 1
    s = exp.mySampleofInterest
    s.myGeometryFunction, s.myVolume, s.myVoxelSize = "getVolumeFromFile", _chiral_volume(), PIX_UM
    return exp


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_scan_of_a_volume_comes_back_in_its_own_orientation():
    """scan (attenuation, ray tracing, 60 angles, one position) -> reconstruct: the mu-weighted centroid of the square lies
    within 0.5 detector pixel of its label centroid (study coordinate x is (x - (ov - 1)/2)/ov on the detector, so a point
    x from the axis' study column sits (x - dimY // 2)/ov from voxel m // 2: the margin of tests/test_gpu_fbp.py), and the
    slice correlates more strongly with the block-averaged truth than with its mirror image or its transpose; the empty
    slices come back without the square."""
    from paresis_amd import tomography
    exp = _chiral_experiment()
    angles = np.arange(60) * 3.0
    sc = tomography.scan(exp, angles)
    assert sc['center'] == tomography.rotation_center(exp) == 15.75
    assert sc['sinograms'][0].shape == (60, CH_DIMX // 2, CH_M // 2)
    mu = tomography.reconstruct(sc)[0].cpu().numpy().astype(np.float64)
    m = CH_M // CH_OV
    assert mu.shape == (CH_DIMX // 2, m, m)
    k = 2 * np.pi * E_KEV * 1e3 * 1.6e-19 / (6.626e-34 * 2.998e8)
    lab = vo.chiral_slice(CH_M)
    row = mu[8]                                                       # detector row 8 = study rows 16, 17
    si, sj = np.nonzero(lab == 1)
    ci, cj = m // 2 + (si.mean() - CH_M // 2) / CH_OV, m // 2 + (sj.mean() - CH_M // 2) / CH_OV
    i, j = np.mgrid[0:m, 0:m]
    hi, hj = (si.max() - si.min() + 1) / 2 / CH_OV + 1.5, (sj.max() - sj.min() + 1) / 2 / CH_OV + 1.5
    w = np.clip(row, 0, None) * ((np.abs(i - ci) <= hi) & (np.abs(j - cj) <= hj))
    gi, gj = (w * i).sum() / w.sum(), (w * j).sum() / w.sum()
    mu_true = 2 * k * np.array((0.0,) + CH_BETA)
    print("square: expected (%.3f, %.3f), centroid (%.3f, %.3f), mu at its centre %.1f of %.1f 1/m"
          % (ci, cj, gi, gj, row[int(round(ci)), int(round(cj))], mu_true[1]))
    assert np.hypot(gi - ci, gj - cj) <= 0.5

    def blocks(slice_labels):
        return mu_true[slice_labels].reshape(m, CH_OV, m, CH_OV).mean(axis=(1, 3))

    own, flipped, transposed = _corr(row, blocks(lab)), _corr(row, blocks(lab[:, ::-1])), _corr(row, blocks(lab.T))
    print("correlation with the truth %.4f, its mirror image %.4f, its transpose %.4f" % (own, flipped, transposed))
    assert own > 0.9 and own > flipped and own > transposed
    empty = mu[0]                                                     # study rows 0, 1: no label
    assert np.abs(empty).max() < 0.05 * mu_true[1]


def _write_xml(tmp_path, volume_file, voxel_um):
    """An XML directory: the package's own files, plus a 16 x 32 detector, the volume sample and their experiment."""
    from paresis_amd import _xml
    d = str(tmp_path / "xml")
    shutil.copytree(_xml._PKG_XML, d)

    def add(name, closing, text):
        path = os.path.join(d, name)
        body = open(path).read()
        assert closing in body
        open(path, "w").write(body.replace(closing, text + closing))

    add("Detectors.xml", "</listDetectors>", """    <detector>
        <name>tiny</name>
        <myDimensions>
            <dimX>16</dimX>
            <dimY>32</dimY>
        </myDimensions>
        <myPixelSize unit="um">6</myPixelSize>
        <myPSF unit="pixel">0</myPSF>
    </detector>
""")
    add("Samples.xml", "</listSamples>", """    <sample>
        <name>chiral_volume</name>
        <myType>sample_of_interest</myType>
        <myGeometryFunction>getVolumeFromFile</myGeometryFunction>
        <myVolumeFile>%s</myVolumeFile>
        <myVoxelSize unit="um">%r</myVoxelSize>
        <myMaterials>PMMA,Nylon</myMaterials>
    </sample>
""" % (volume_file, voxel_um))
    add("Experiment.xml", "</listExperiment>", """    <experiment>
        <name>Chiral_volume_ID17</name>
        <distSourceToMembrane unit="m">140</distSourceToMembrane>
        <distMembraneToObject unit="m">1.6</distMembraneToObject>
        <distObjectToDetector unit="m">3.6</distObjectToDetector>
        <membraneName>Mask_CuSn_From_txt</membraneName>
        <sampleName>chiral_volume</sampleName>
        <sampleType>AnalyticalSample</sampleType>
        <detectorName>tiny</detectorName>
        <sourceName>id17</sourceName>
        <meanShotCount>30000</meanShotCount>
        <inVacuum>True</inVacuum>
    </experiment>
""")
    return d


def test_main_tomography_of_an_xml_volume(tmp_path):
    """main.run(tomography=6) on an XML directory that names a .npy volume: exp_dict['tomographyVolumes'] and the file
    written hold the bits of scan + reconstruct through the API on the same XML."""
    import glob
    from paresis_amd import main, tomography
    from paresis_amd.Experiment import Experiment
    M = (140.0 + 1.6 + 3.6) / (140.0 + 1.6)
    voxel_um = 6.0 / CH_OV / M                                        # the study pixel of the 'tiny' detector: s = 1
    np.save(str(tmp_path / "chiral.npy"), _chiral_volume())
    xml = _write_xml(tmp_path, str(tmp_path / "chiral.npy"), voxel_um)

    def exp_dict():
        return {"experimentName": "Chiral_volume_ID17", "filepath": str(tmp_path) + "/", "overSampling": CH_OV,
                "nbExpPoints": 1, "simulation_type": "RayT", "noise": False, "xmlDir": xml}

    ed = exp_dict()
    main.run(ed, save=True, saving_format=".npy", tomography=6)
    tp = ed['tomographyParams']
    assert tp['angles'] == [0.0, 30.0, 60.0, 90.0, 120.0, 150.0] and tp['center'] == 15.75
    exp = Experiment(exp_dict())
    s = exp.mySampleofInterest
    assert s.myGeometryFunction == "getVolumeFromFile" and s.myVoxelSize == voxel_um and s.myMaterials == ["PMMA", "Nylon"]
    assert exp.exp_dict['studyDimensions'] == [CH_DIMX, CH_M] and tuple(s.geometry_dev().shape) == (2, CH_DIMX, CH_M)
    want = tomography.reconstruct(tomography.scan(exp, tp['angles']))[0]
    assert want.shape == (CH_DIMX // 2, CH_M // 2, CH_M // 2) and float(want.abs().max()) > 0
    assert torch.equal(ed['tomographyVolumes'][0], want)
    files = glob.glob(str(tmp_path) + "/*/tomography/mu_%s.npy" % ed['expID'])
    assert len(files) == 1 and np.array_equal(np.load(files[0]), want.cpu().numpy())
