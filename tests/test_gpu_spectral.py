"""Spectral material decomposition on the GPU (csrc/decompose.hip, ops.decompose, paresis_amd/spectral.py, main.py's --decompose)
against the numpy oracle of tests/_spectral_oracle.py, against known thicknesses, and through the chain."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from tests import _spectral_oracle as so

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ kernel against the oracle
SHAPES = [(1,), (255,), (257,), (3, 257), (64, 65)]      # a block's tail on either side, a second block, two image shapes
MB = [(1, 1), (1, 3), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 8)]
# Unequal bins whose first four keep the two K-edges away from the middle of a wide bin: the column-normalised Abar of (M, B) =
# (4, 4) is then conditioned 38, as with equal bins; a pattern with an edge inside a wide bin gives 460 to 790, and the
# oracle itself does not converge within 12 steps there (cond <= 48 over all the cases below).
UNEQUAL = [4, 3, 5, 2, 7, 1, 12, 9]
SCALE = np.array([0.05, 0.01, 0.004, 0.004])            # metres: each material's thickness at a -ln T of the order of 1
WORST = {}


def bin_sizes(kind, B):
    if kind == "full":                                   # 256 energies exactly
        return [256 // B] * (B - 1) + [256 - (256 // B) * (B - 1)]
    return {"one": [1] * B, "two": [2] * B, "seventeen": [17] * B, "unequal": UNEQUAL[:B]}[kind]


KINDS = ("one", "two", "seventeen", "unequal", "full")


def kernel_case(M, B, kind, shape, unit_v, seed):
    """The tables and data of one comparison: thicknesses drawn per pixel, a few of them negative, their exact -ln T times
    (1 + 1e-3 noise) so that the bins disagree, rounded to float32."""
    sizes = bin_sizes(kind, B)
    E, w, a = so.model_arrays(sizes, M)
    v = np.ones(B) if unit_v else 0.5 + np.arange(1, B + 1) ** 2 / 7.0
    G = so.linear_start(sizes, w, a, v)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = rng.uniform(-0.05, 1.0, (M, n)) * SCALE[:M, None]
    L = -np.log(so.transmission(sizes, w, a, x)) * (1.0 + 1e-3 * rng.standard_normal((B, n)))
    return sizes, w, a, v, G, L.astype(np.float32)


def bound(ref):
    """Per material: 2^-23 |A| for the float32 output, 1e-10 max|A| for a device exp / log of a few ulps (about 10^3 times
    what float64 differs from long double by on these problems)."""
    return 2.0 ** -23 * np.abs(ref) + 1e-10 * np.abs(ref).max(axis=1, keepdims=True)


def compare(tag, got, ref, iterations=12, kind=None):
    """got: ops.decompose's tensors; ref: the oracle's arrays, which must have converged on every pixel it did not flag."""
    x, res, steps = ref
    regular = steps != -1
    assert ((steps[regular] > 0) & (steps[regular] < iterations)).all(), (tag, np.unique(steps))
    gx = got[0].cpu().numpy().astype(np.float64).reshape(x.shape)
    gr, gs = got[1].cpu().numpy().astype(np.float64).ravel(), got[2].cpu().numpy().astype(np.float64).ravel()
    ratio = float((np.abs(gx - x) / bound(x)).max())
    WORST[tag] = ratio
    print("%-28s error/bound %.3f  steps %d..%d  residual %.3g" % (tag, ratio, steps.min(), steps.max(), res[regular].max()))
    assert ratio <= 1.0, (tag, ratio)
    assert (np.abs(gs - steps) <= 1).all(), (tag, gs[np.abs(gs - steps) > 1][:4])
    if kind == "one":
        assert gs.max() <= 2, (tag, gs.max())             # the model is linear: exact after one step
    assert (np.abs(gr[regular] - res[regular]) <= 1e-6 * (1.0 + res[regular])).all() and (gr[~regular] == np.inf).all(), tag


@pytest.mark.parametrize("M,B", MB)
def test_kernel_matches_oracle(M, B):
    """Every bin-size kind with every pixel count, the bin weights unit and unequal in turn; nothing is excluded."""
    from paresis_amd import ops
    for ik, kind in enumerate(KINDS):
        for ish, shape in enumerate(SHAPES):
            unit_v = (ik + ish) % 2 == 0
            sizes, w, a, v, G, L = kernel_case(M, B, kind, shape, unit_v, seed=1000 * M + 100 * B + 10 * ik + ish)
            ref = so.decompose(L, sizes, w, a, v, G)
            dev = torch.from_numpy(L.reshape((B,) + shape)).cuda()
            got = ops.decompose(dev, sizes, w, a, v, G)
            assert tuple(got[0].shape) == (M,) + shape and tuple(got[1].shape) == shape == tuple(got[2].shape)
            compare("M%d B%d %s %s %s" % (M, B, kind, "x".join(map(str, shape)), "v=1" if unit_v else "v"), got, ref, kind=kind)
    print("worst error/bound of M=%d, B=%d: %.3f" % (M, B, max(r for t, r in WORST.items() if t.startswith("M%d B%d " % (M, B)))))


def _special_model():
    sizes = [8, 8, 15]
    E, w, a = so.model_arrays(sizes, 2, exact_weights=True)
    e0 = 0
    for ne in sizes:
        assert sum(w[e0:e0 + ne]) == 1.0 and w[e0:e0 + ne][::-1].sum() == 1.0
        e0 += ne
    v = np.array([1.0, 2.0, 0.5])
    return sizes, w, a, v, so.linear_start(sizes, w, a, v)


def test_special_pixels_in_one_image():
    from paresis_amd import ops
    sizes, w, a, v, G = _special_model()
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 1, (2, 40)) * SCALE[:2, None]
    L = (-np.log(so.transmission(sizes, w, a, x))).astype(np.float32)
    zero, nan, pinf, ninf, deep = 3, 9, 17, 18, 33
    L[:, zero] = 0.0
    L[0, nan], L[1, pinf], L[2, ninf] = np.nan, np.inf, -np.inf
    L[:, deep] = 103.0                                    # T = e^-103: the float32 denormal floor
    t, r, s = (o.cpu().numpy() for o in ops.decompose(torch.from_numpy(L).cuda(), sizes, w, a, v, G))
    assert (t[:, zero] == 0).all() and s[zero] >= 1 and r[zero] == 0
    for p in (nan, pinf, ninf):
        assert (t[:, p] == 0).all() and r[p] == np.inf and s[p] == -1, p
    ref = so.decompose(L, sizes, w, a, v, G)
    assert ref[2][deep] > 0 and ref[2][deep] < 12 and np.isfinite(t[:, deep]).all() and np.isfinite(r[deep])
    assert (np.abs(t[:, deep] - ref[0][:, deep]) <= 2.0 ** -23 * np.abs(ref[0][:, deep]) + 1e-10 * np.abs(ref[0][:, deep]).max()).all()
    compare("special pixels", (torch.from_numpy(t), torch.from_numpy(r), torch.from_numpy(s)), ref)


def test_a_pixel_does_not_depend_on_its_neighbours():
    """The same bits twice; and the same bits for the pixels kept when every other pixel is replaced -- by other data, which
    stops at other steps, and by flagged values."""
    from paresis_amd import ops
    sizes, w, a, v, G, L = kernel_case(3, 4, "unequal", (5, 131), False, seed=77)
    L = L.reshape(4, 5, 131)
    first = ops.decompose(torch.from_numpy(L).cuda(), sizes, w, a, v, G)
    again = ops.decompose(torch.from_numpy(L).cuda(), sizes, w, a, v, G)
    for f, g in zip(first, again):
        assert torch.equal(f, g)
    rng = np.random.default_rng(78)
    keep = rng.random((5, 131)) < 0.3
    other = kernel_case(3, 4, "unequal", (5, 131), False, seed=79)[5].reshape(4, 5, 131) * 3.0
    other[:, rng.random((5, 131)) < 0.3] = np.nan
    other[1, rng.random((5, 131)) < 0.1] = np.inf
    mixed = np.where(keep[None], L, other)
    got = ops.decompose(torch.from_numpy(mixed).cuda(), sizes, w, a, v, G)
    k = torch.from_numpy(keep).cuda()
    assert torch.equal(got[0][:, k], first[0][:, k]) and torch.equal(got[1][k], first[1][k]) and torch.equal(got[2][k], first[2][k])
    assert float(first[2].min()) >= 1 and float(first[2].max()) > float(first[2].min())      # the lanes of a wave stop apart
    assert int((got[2] == -1).sum()) > 100


# ------------------------------------------------------------------------------------------------ physics without the chain
def _model(M, thresholds=(34.0, 50.0)):
    from paresis_amd import spectral
    E, flux = so.spectrum()
    sizes, w = so.split(E, flux, list(thresholds))
    cut = np.cumsum([0] + sizes)
    return spectral.SpectralModel(so.ORDER[:M], [E[cut[b]:cut[b + 1]] for b in range(len(sizes))],
                                  [w[cut[b]:cut[b + 1]] for b in range(len(sizes))], so.coefficients(E, M))


@pytest.mark.parametrize("M", [2, 3])
def test_known_thicknesses_come_back(M):
    """transmission (float32) -> -ln -> decompose on a 33 x 47 grid: each material's thickness comes back within 4 times the
    oracle's own error against the truth on the same float32 data."""
    from paresis_amd import spectral
    model = _model(M)
    i, j = np.mgrid[0:33, 0:47]
    maps = [0.5 + 0.5 * np.sin(0.21 * i + 0.4) * np.cos(0.13 * j), ((i - 16) ** 2 + (j - 23) ** 2 < 150) * 0.8 + 0.1,
            np.exp(-((i - 10) ** 2 + (j - 30) ** 2) / 60.0)][:M]
    truth = np.stack(maps) * SCALE[:M, None, None]
    T = spectral.transmission(model, torch.from_numpy(truth).cuda())
    L = -torch.log(T)
    r = spectral.decompose(L, model)
    v = np.ones(model.bins)
    ox, _, osteps = so.decompose(L.cpu().numpy().reshape(model.bins, -1), model.bin_size, model.w, model.a, v, model.linear_start(v))
    assert (osteps > 0).all() and (osteps < 12).all()
    got = r['thickness'].cpu().numpy().astype(np.float64).reshape(M, -1)
    err = np.abs(got - truth.reshape(M, -1)).max(axis=1)
    oerr = np.abs(ox - truth.reshape(M, -1)).max(axis=1)
    print("M=%d: error against the truth / scale: GPU %s, oracle %s" % (M, err / SCALE[:M], oerr / SCALE[:M]))
    assert (err <= 4 * oerr).all() and (oerr <= 1e-5 * SCALE[:M]).all()
    assert float(r['steps'].min()) >= 1 and float(r['residual'].max()) < 1e-5


def test_beam_hardening_is_what_the_decomposition_removes():
    """5 cm of the soft material behind the whole spectrum in one bin: the monochromatic estimate L/Abar is wrong by more than
    100 times the decomposed thickness's error."""
    from paresis_amd import spectral
    model = _model(1, thresholds=())
    truth = torch.full((1, 4, 4), 0.05, dtype=torch.float64).cuda()
    L = -torch.log(spectral.transmission(model, truth))
    mono = float(L[0, 0, 0]) / float(model.effective()[0, 0])
    dec = float(spectral.decompose(L, model)['thickness'][0, 0, 0])
    print("5 cm soft: monochromatic estimate %.5f m, decomposed %.9f m" % (mono, dec))
    assert abs(mono - 0.05) > 100 * abs(dec - 0.05) and abs(mono - 0.05) > 1e-3


# ------------------------------------------------------------------------------------------------ through the chain
CH_N, CH_OV, CH_PIX_UM = 64, 2, 500.0                    # a 64 x 64 study grid of 500 um pixels: a 32 x 32 detector
CH_ANGLES = [180.0 * k / 8 for k in range(8)]
CH_NAMES = ("SpecSoft", "SpecIodine")
CH_THRESHOLDS = [34.0, 50.0]


def _chain_volume():
    """A soft disc of 25 voxels' radius with a K-edge insert of 6, on the slices 8 .. 55."""
    i, j = np.mgrid[0:CH_N, 0:CH_N]
    lab = np.zeros((CH_N, CH_N), dtype=np.uint8)
    lab[(i - 32) ** 2 + (j - 32) ** 2 <= 25 ** 2] = 1
    lab[(i - 40) ** 2 + (j - 26) ** 2 <= 6 ** 2] = 2
    vol = np.zeros((CH_N, CH_N, CH_N), dtype=np.uint8)
    vol[8:56] = lab
    return vol


def _chain_experiment():
    from oracle import paresis_oracle as orc
    from paresis_amd.getk import k_sample
    from tests._build import build_experiment
    E, flux = so.spectrum(step=4.0)
    k = np.array([k_sample(float(e)) for e in E])
    beta = [list(so.MU[n](E) / (2 * k)) for n in CH_NAMES]
    delta = [list(2e-7 * (30.0 / E) ** 2) for _ in CH_NAMES]
    i, j = np.mgrid[0:CH_N, 0:CH_N]
    membrane = np.stack([2e-6 * (1 + 0.5 * np.sin(0.9 * i + 0.3) * np.cos(0.7 * j)), np.full((CH_N, CH_N), 1e-4)]).astype(np.float32)
    M = (140.0 + 1.6 + 3.6) / (140.0 + 1.6)
    cfg = dict(scintillator=None, dSM=140.0, dMO=1.6, dOD=3.6, meanShotCount=30000.0, ov=CH_OV, pix_um=CH_PIX_UM, M=M,
               inVacuum=True, N=(CH_N, CH_N), spectrum=[(float(e), float(f)) for e, f in zip(E, flux)], source_size_um=0.0,
               energy_sampling=4.0, det_dims=(CH_N // 2, CH_N // 2), det_pix_um=CH_PIX_UM * 2 * M, psf=0.0, bins=list(CH_THRESHOLDS),
               membrane=orc.Obj(membrane, [[5.0e-7] * len(E), [9.9e-8] * len(E)], [[3.0e-9] * len(E), [5.3e-11] * len(E)]),
               sample=orc.Obj(np.zeros((2, CH_N, CH_N)), delta, beta), air=None, plate=None)
    exp = build_experiment(cfg, "RT", sample_materials=list(CH_NAMES))
    exp.exp_dict["nbExpPoints"] = 1
    s = exp.mySampleofInterest
    s.myGeometryFunction, s.myVolume, s.myVoxelSize = "getVolumeFromFile", _chain_volume(), CH_PIX_UM
    return exp


@pytest.fixture(scope="module")
def chain():
    """One scan for the chain's tests: the per-bin sinograms, spectral.scan of the same experiment, the oracle's decomposition
    of those sinograms and the truth -- the sample's own thickness maps at each angle, binned to the detector."""
    from paresis_amd import spectral, tomography
    exp = _chain_experiment()
    model = spectral.model_of(exp)
    assert model.bin_size == [5, 4, 7] and model.names == CH_NAMES
    sc = spectral.scan(exp, CH_ANGLES)
    raw = tomography.scan(exp, CH_ANGLES)
    truth = []
    s, ed = exp.mySampleofInterest, exp.exp_dict
    for angle in CH_ANGLES:
        tomography._turn(s, angle, ed['studyDimensions'], ed['studyPixelSize'], ed['overSampling'])
        g = s.geometry_dev().cpu().numpy().astype(np.float64)
        truth.append(g.reshape(2, CH_N // 2, 2, CH_N // 2, 2).mean(axis=(2, 4)))
    L = np.stack([raw['sinograms'][b].cpu().numpy() for b in range(3)])
    v = np.ones(3)
    ref = so.decompose(L.reshape(3, -1), model.bin_size, model.w, model.a, v, model.linear_start(v))
    return {'exp': exp, 'model': model, 'scan': sc, 'L': L, 'ref': ref, 'truth': np.stack(truth, axis=1)}


def test_scan_is_the_oracles_decomposition_of_the_chains_sinograms(chain):
    sc, (x, res, steps) = chain['scan'], chain['ref']
    assert sc['modality'] == 'materials' and list(sc['sinograms']) == list(CH_NAMES) and sc['angles'] == CH_ANGLES
    shape = (8, CH_N // 2, CH_N // 2)
    assert tuple(sc['residual'].shape) == shape and all(tuple(t.shape) == shape for t in sc['sinograms'].values())
    got = torch.stack([sc['sinograms'][n] for n in CH_NAMES])
    assert ((steps > 0) & (steps < 12)).all()
    gx = got.cpu().numpy().astype(np.float64).reshape(2, -1)
    ratio = float((np.abs(gx - x) / bound(x)).max())
    print("spectral.scan against the oracle on the chain's sinograms: error/bound %.3f" % ratio)
    assert ratio <= 1.0
    assert (np.abs(sc['residual'].cpu().numpy().ravel() - res) <= 1e-6 * (1 + res)).all()


def test_chain_thicknesses_against_the_samples_own(chain):
    """The model's error -- refraction, partial-volume averaging of exp(-mu t) over a detector pixel, the detector's resampling
    -- measured by the CPU oracle on the chain's images; the GPU path stays within twice that, on interior pixels."""
    truth = chain['truth']                                           # [2, 8, 32, 32]
    inner = (slice(None), slice(None), slice(2, -2), slice(2, -2))
    ox = chain['ref'][0].reshape(truth.shape)
    gx = torch.stack([chain['scan']['sinograms'][n] for n in CH_NAMES]).cpu().numpy().astype(np.float64)
    for m, name in enumerate(CH_NAMES):
        scale = truth[m].max()
        oerr, gerr = np.abs(ox - truth)[inner][m], np.abs(gx - truth)[inner][m]
        print("%s: thickness up to %.4f m; error against the sample's own maps: oracle max %.3g rms %.3g, GPU max %.3g rms %.3g (of the "
              "largest thickness)" % (name, scale, oerr.max() / scale, np.sqrt((oerr ** 2).mean()) / scale, gerr.max() / scale,
                                      np.sqrt((gerr ** 2).mean()) / scale))
        assert gerr.max() <= 2 * oerr.max() and np.sqrt((gerr ** 2).mean()) <= 2 * np.sqrt((oerr ** 2).mean())


def test_reconstruct_gives_one_volume_per_material(chain):
    from paresis_amd import spectral
    for options in ({'method': 'fbp'}, {'method': 'sirt', 'iterations': 3, 'nonneg': True}):
        vols = spectral.reconstruct(chain['scan'], **options)
        assert list(vols) == list(CH_NAMES)
        for name, vol in vols.items():
            assert tuple(vol.shape) == (CH_N // 2, CH_N // 2, CH_N // 2) and vol.dtype == torch.float32
            assert bool(torch.isfinite(vol).all())
        soft = vols["SpecSoft"].cpu().numpy()                         # detector row 16 lies in the disc's slices, row 1 in none
        print("%s: soft fraction at the disc's centre %.3f, largest in an empty slice %.3g" % (options['method'], soft[16, 16, 16],
                                                                                              np.abs(soft[1]).max()))
        assert soft[16, 16, 16] > 0.5 and np.abs(soft[1]).max() < 0.05
    with pytest.raises(ValueError, match="needs iterations"):
        spectral.reconstruct(chain['scan'], method='cgls')
    with pytest.raises(ValueError, match="modality"):
        spectral.reconstruct({'modality': 'attenuation'})


# ------------------------------------------------------------------------------------------------ main.run and the command line
def _write_xml(tmp_path, volume_file):
    """An XML directory: the package's own files plus a polychromatic source, a 32 x 32 detector of three bins, the volume
    sample of the two test materials and their experiment."""
    from paresis_amd import _xml
    d = str(tmp_path / "xml")
    shutil.copytree(_xml._PKG_XML, d)

    def add(name, closing, text):
        path = os.path.join(d, name)
        body = open(path).read()
        assert closing in body
        open(path, "w").write(body.replace(closing, text + closing))

    add("Sources.xml", "</listSources>", """    <source>
        <name>spectral_tube</name>
        <myType>Polychromatic</myType>
        <mySize unit="um">0</mySize>
        <sourceVoltage unit="kVp">80</sourceVoltage>
        <myEnergySampling unit="keV">4</myEnergySampling>
    </source>
""")
    add("Detectors.xml", "</listDetectors>", """    <detector>
        <name>three_bins</name>
        <myDimensions>
            <dimX>32</dimX>
            <dimY>32</dimY>
        </myDimensions>
        <myPixelSize unit="um">6</myPixelSize>
        <myPSF unit="pixel">0</myPSF>
        <myBinsThersholds>34,50</myBinsThersholds>
    </detector>
""")
    M = (140.0 + 1.6 + 3.6) / (140.0 + 1.6)
    add("Samples.xml", "</listSamples>", """    <sample>
        <name>spectral_volume</name>
        <myType>sample_of_interest</myType>
        <myGeometryFunction>getVolumeFromFile</myGeometryFunction>
        <myVolumeFile>%s</myVolumeFile>
        <myVoxelSize unit="um">%r</myVoxelSize>
        <myMaterials>SpecSoft,SpecIodine</myMaterials>
    </sample>
""" % (volume_file, 6.0 / CH_OV / M))
    add("Experiment.xml", "</listExperiment>", """    <experiment>
        <name>Spectral_volume</name>
        <distSourceToMembrane unit="m">140</distSourceToMembrane>
        <distMembraneToObject unit="m">1.6</distMembraneToObject>
        <distObjectToDetector unit="m">3.6</distObjectToDetector>
        <membraneName>Mask_CuSn_From_txt</membraneName>
        <sampleName>spectral_volume</sampleName>
        <sampleType>AnalyticalSample</sampleType>
        <detectorName>three_bins</detectorName>
        <sourceName>spectral_tube</sourceName>
        <meanShotCount>30000</meanShotCount>
        <inVacuum>True</inVacuum>
    </experiment>
""")
    return d


@pytest.fixture
def xml_run(tmp_path):
    """The XML directory, with the test materials registered and the tube's spectrum injected for the test's duration.  The
    voxels are 3 um here, so the coefficients are scaled up to keep -ln T of the order of 1."""
    from paresis_amd import materials
    from paresis_amd.getk import k_sample
    from paresis_amd.Source import Source
    np.save(str(tmp_path / "volume.npy"), _chain_volume())
    xml = _write_xml(tmp_path, str(tmp_path / "volume.npy"))
    for name in CH_NAMES:
        materials.register_material(name, lambda e, mu=so.MU[name]: (1e-9, 170.0 * float(mu(e)) / (2.0 * k_sample(e))), "test")
    E, flux = so.spectrum(step=4.0)
    before = Source.spectrum_provider
    Source.spectrum_provider = staticmethod(lambda sd, flu: list(zip(E.tolist(), flux.tolist())))
    yield xml
    Source.spectrum_provider = before
    for name in CH_NAMES:
        materials._REGISTRY.pop(name, None)


def _files(out, fmt):
    return sorted(os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "*", "*", "propag", "materials", "*" + fmt)))


def test_main_run_writes_the_thickness_maps(tmp_path, xml_run):
    from paresis_amd import main, spectral
    ed = {"experimentName": "Spectral_volume", "filepath": str(tmp_path) + "/", "overSampling": CH_OV, "nbExpPoints": 2,
          "simulation_type": "RayT", "noise": False, "xmlDir": xml_run}
    res = main.run(ed, save=True, saving_format=".npy", decompose=True)
    dp, dec = ed['decomposeParams'], ed['decomposition']
    assert dp['materials'] == list(CH_NAMES) and [len(e) for e in dp['energies_keV']] == [5, 4, 7] and 1 < dp['condition'] < 100
    assert [len(w) for w in dp['weights']] == [5, 4, 7] and all(abs(sum(w) - 1) < 1e-12 for w in dp['weights'])
    assert tuple(dec['thickness'].shape) == (2, 32, 32) and float(dec['steps'].min()) >= 1
    files = _files(str(tmp_path), ".npy")
    first = "20_34kev"
    assert [os.path.basename(f) for f in files] == ["residual_%s.npy" % ed['expID']] + ["thickness_%s_%s.npy" % (n, ed['expID'])
                                                                                       for n in sorted(CH_NAMES)]
    assert all(os.sep + first + os.sep in os.sep + f for f in files), files
    for m, name in enumerate(CH_NAMES):
        saved = np.load(glob.glob(str(tmp_path / "*" / first / "propag" / "materials" / ("thickness_%s_*.npy" % name)))[0])
        assert np.array_equal(saved, dec['thickness'][m].cpu().numpy())
    P, W = np.asarray(res[0][2], dtype=np.float32), np.asarray(res[0][3], dtype=np.float32)
    assert P.shape == (3, 32, 32) and W.shape == P.shape
    again = spectral.decompose_run(res, spectral.model_of(_experiment_of(ed, xml_run)))       # the API on the run's own stacks
    assert torch.equal(again['thickness'], dec['thickness']) and torch.equal(again['residual'], dec['residual'])
    soft = dec['thickness'][0].cpu().numpy()
    assert soft[16, 16] > 10 * abs(soft[1, 16]) and soft[16, 16] > 0             # the disc's centre against the empty slices
    with pytest.raises(ValueError, match="not one of the sample"):
        main.run(dict(ed), save=False, decompose=True, decompose_materials=["SpecSoft", "PMMA"])


def _experiment_of(ed, xml):
    from paresis_amd.Experiment import Experiment
    return Experiment({"experimentName": ed["experimentName"], "filepath": ed["filepath"], "overSampling": ed["overSampling"],
                       "nbExpPoints": 1, "simulation_type": ed["simulation_type"], "noise": False, "xmlDir": xml})


def test_command_line_writes_the_thickness_maps(tmp_path, xml_run):
    from paresis_amd import main
    out = str(tmp_path / "cli")
    main.main(["--experiment", "Spectral_volume", "--xml", xml_run, "--out", out, "--format", ".npy", "--no-noise", "--points", "1",
               "--decompose", "--decompose-materials", "SpecIodine,SpecSoft"])
    files = glob.glob(os.path.join(out, "*", "20_34kev", "propag", "materials", "*.npy"))
    names = sorted(os.path.basename(f).rsplit("_", 1)[0] for f in files)
    assert names == ["residual", "thickness_SpecIodine", "thickness_SpecSoft"]
    iodine = np.load([f for f in files if "SpecIodine" in f][0])
    assert iodine.shape == (32, 32) and np.isfinite(iodine).all() and iodine.max() > 0
