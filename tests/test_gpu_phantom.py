"""GPU: the contrast phantom (csrc/phantom.hip) against the reference's own generator (tests/golden/phantom.npz), and the
material fold (csrc/fold.hip) that lets every kernel and both chains take samples of more than PSX_MAX_MAT materials,
against float64 oracles fed the float32 maps the GPU used."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import paresis_oracle as orc
from paresis_amd import _lib
from tests._build import build_experiment, cfg_from_experiment
from tests._golden import experiment_cfg, load, relmax

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _small(g):
    return ["c%d_" % i for i in range(int(g["n_small"]))]


def _args(g, pre):
    dimX, dimY, pix, angle = (float(v) for v in g[pre + "args"])
    return int(dimX), int(dimY), pix, angle


# ------------------------------------------------------------------------------------------------ phantom
def test_phantom_rasterisation_is_bit_equal_to_the_reference():
    from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_slices
    g = load("phantom.npz")
    for pre in _small(g):
        dimX, dimY, pix, angle = _args(g, pre)
        want = np.unpackbits(g[pre + "slices"], axis=-1)[..., :dimY]
        got = contrast_phantom_slices(dimX, dimY, pix, angle).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), pre


def test_phantom_maps_match_the_reference():
    from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_lines, generateContrastPhantom
    g = load("phantom.npz")
    for pre in _small(g):
        dimX, dimY, pix, angle = _args(g, pre)
        geom, params = generateContrastPhantom(dimX, dimY, pix, angle)
        assert geom.dtype == torch.float32 and geom.is_cuda and tuple(geom.shape) == (13, dimX, dimY)
        got, want = geom.cpu().numpy(), g[pre + "maps"]
        for m in range(13):
            assert relmax(got[m], want[m]) <= 1e-6, (pre, m)
            assert np.array_equal(got[m] != 0, want[m] != 0), (pre, m)
        _, lines = contrast_phantom_lines(dimX, dimY, pix, angle)
        assert relmax(lines.cpu().numpy(), g[pre + "lines"]) <= 1e-12, pre
    # the id17 grid (1000 x 3000 at 11.71 um): every row of each map is the recorded line
    dimX, dimY, pix, angle = _args(g, "id17_")
    geom, lines = contrast_phantom_lines(dimX, dimY, pix, angle)
    assert relmax(lines.cpu().numpy(), g["id17_lines"]) <= 1e-12
    nz = g["id17_row_nonzero"]
    want_rows = (g["id17_lines"] * (pix / 1000) * 1e-3).astype(np.float32)
    for m in range(13):
        gm = geom[m]
        rows = (gm != 0).any(dim=1).cpu().numpy()
        assert np.array_equal(rows, nz[m]), m
        r = np.flatnonzero(rows)
        if m < 12:                                                           # row0: the first TUBE row, as recorded
            assert relmax(gm[r[0]].cpu().numpy(), g["id17_row0"][m]) <= 1e-6, m
        assert bool((gm[r] == gm[r[0]]).all()), m                            # every filled row is the same line
        assert relmax(gm[r[0]].cpu().numpy(), want_rows[m]) <= 1e-6, m


def test_analytical_sample_dispatches_to_the_phantom():
    from paresis_amd.Sample import AnalyticalSample
    g = load("phantom.npz")
    s = AnalyticalSample()
    s.myName, s.myType, s.myGeometryFunction = "ContrastPhantomID17", "sample_of_interest", "generateContrastPhantom"
    s.myMaterials = ["m%d" % i for i in range(13)]
    s.getMyGeometry((48, 160), 250.0, 1)
    geo = s.myGeometry
    assert isinstance(geo, torch.Tensor) and geo.is_cuda and geo.dtype == torch.float32 and tuple(geo.shape) == (13, 48, 160)
    assert s.geometry_dev() is geo
    assert relmax(geo.cpu().numpy(), g["c0_maps"]) <= 1e-6                  # c0 is (48, 160, 250 um, 30 deg): angle=30
    p = s.geom_parameters
    assert p["smallTubesRadius"] == (float(g["params_smallTubesRadius"]), "mm")
    assert p["supportRadius"] == (float(g["params_supportRadius"]), "mm")
    assert np.array_equal(np.array(p["tubes centers"][0]), g["params_tubes_centers"]) and p["tubes centers"][1] == "mm"


# --------------------------------------------------------------------------------------------------- fold
def _maps(n, Nx, Ny, seed, pix=3e-6):
    """n smooth float32 thickness maps (sphere chords, metres) of a phantom's magnitude: 0.1-0.5 mm."""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
    out = np.zeros((n, Nx, Ny))
    for m in range(n):
        ci, cj, R = rng.uniform(0.3, 0.7) * Nx, rng.uniform(0.3, 0.7) * Ny, rng.uniform(0.25, 0.45) * min(Nx, Ny)
        out[m] = 2 * np.sqrt(np.maximum(R * R - (ii - ci) ** 2 - (jj - cj) ** 2, 0)) * pix
        out[m] += rng.uniform(0, 2e-5)                                       # a uniform support under every map
    return out.astype(np.float32)


def _coeffs(n, seed, E=52.0):
    """delta / beta of phantom materials at E keV (iodine/gadolinium-loaded water to solid water)."""
    rng = np.random.default_rng(seed + 1000)
    return list(rng.uniform(1.5e-7, 4e-7, n)), list(rng.uniform(5e-11, 2e-9, n))


@pytest.mark.parametrize("n", [9, 13, 16, 40, 70])
def test_fold_kernel_against_float64(n):
    from paresis_amd import ops
    from paresis_amd.getk import k_sample
    Nx, Ny = 67, 45
    T = torch.from_numpy(_maps(n, Nx, Ny, n, pix=1e-5)).cuda()
    delta, beta = _coeffs(n, n)
    k = k_sample(52.0)
    cp, ca = [-k * d for d in delta], [-2 * k * b for b in beta]
    f = ops.fold_materials([T[i] for i in range(n)], cp, ca)
    assert f.n == 3 and f.cphase == [1.0, 1.0, 0.0] and f.catt == [0.0, 0.0, 1.0] and f.folded
    T64 = T.cpu().numpy().astype(np.float64)
    P = np.tensordot(np.array(cp), T64, axes=1)
    A = np.tensordot(np.array(ca), T64, axes=1)
    F = f.T.cpu().numpy().astype(np.float64)
    assert np.max(np.abs(P)) > 100                                          # hundreds of radians: past float32
    assert np.max(np.abs(F[0] + F[1] - P)) <= 1e-12 * np.max(np.abs(P))
    runs = -(-(n - 3) // (64 - 3))                                          # PSX_MAX_FOLD maps per run, 3 carried over
    assert np.all(np.abs(F[2] - A) <= runs * 2 ** -24 * np.abs(A) + 1e-30)  # A rounds to float32 once per run


def _consumers(mats_w, mats_rt, Nx, Ny, E, pix_um, engine):
    """Every consumer of a material stack on one (Nx, Ny) grid: transmission (wave, intensity + phase), attenuated
    accumulation, refraction (single, multi-distance, dark-field split) and Fresnel propagation."""
    from paresis_amd import ops
    from paresis_amd.getk import getk, k_refraction
    out = {}
    out["wave"] = ops.transmit_wave(None, 3.0, mats_w)
    I, phi = ops.transmit_rt(None, 2.0, mats_rt)
    out["I"], out["phi"] = I, phi
    img = torch.full((Nx, Ny), 1.5, dtype=torch.float32, device="cuda")
    out["acc"] = ops.accumulate(torch.zeros_like(img), img, 2.0, mats=mats_rt)
    h, M, z = pix_um * 1e-6, 1.02, 0.8
    ds = z / k_refraction(E) / (h * M) / h
    out["refract"] = ops.refract((Nx, Ny), mats_rt, ds, (Nx, Ny), I0=7500.0)[0]
    out["multi"] = ops.refract_multi((Nx, Ny), mats_rt, [ds, 2 * ds], (Nx, Ny), I0=7500.0)
    mask = torch.zeros((Nx, Ny), dtype=torch.float32, device="cuda")
    mask[:, : Ny // 2] = 1.0
    out["split"] = ops.refract_split((Nx, Ny), mats_rt, ds, (Nx, Ny), mask, I0=7500.0)
    plan = ops.FresnelPlan(Nx, Ny, engine=engine)
    assert plan.engine == engine
    kk = getk(E * 1000)
    inten = torch.zeros((Nx, Ny), dtype=torch.float32, device="cuda")
    plan.propagate([z / (2 * kk * M)], [kk * z / M], (2 * np.pi / (Nx * h), 2 * np.pi / (Ny * h)), amp=float(np.sqrt(7500.0)),
                   mats=mats_w, want_wave=[False], inten_out=[inten])
    out["fresnel"] = inten
    ops.check_status(inten.device)
    return out, (z, M)


@pytest.mark.parametrize("n", [9, 13, 16])
def test_every_consumer_takes_more_than_eight_maps(n):
    from paresis_amd import ops
    from paresis_amd.getk import k_sample
    Nx, Ny, E, pix_um = 131, 97, 52.0, 3.0
    geom = _maps(n, Nx, Ny, 7 * n)
    delta, beta = _coeffs(n, 7 * n)
    k = k_sample(E)
    T = torch.from_numpy(geom).cuda()
    mats_w = ops.MaterialStack(T, cphase=[-k * d for d in delta], catt=[-k * b for b in beta])
    mats_rt = ops.MaterialStack(T, cphase=[-k * d for d in delta], catt=[-2 * k * b for b in beta])
    g64 = geom.astype(np.float64)                                           # the float32 maps the GPU used, widened
    for engine in (_lib.ENGINE_ROCFFT, _lib.ENGINE_LDS):
        out, (z, M) = _consumers(mats_w, mats_rt, Nx, Ny, E, pix_um, engine)
        w_ref = orc.set_wave(np.full((Nx, Ny), 3.0 + 0j), g64, delta, beta, E)
        I_ref, phi_ref, _ = orc.set_wave_rt(np.full((Nx, Ny), 2.0), g64, delta, beta, E, 0)
        assert relmax(out["wave"].cpu().numpy(), w_ref) <= TOL
        assert relmax(out["I"].cpu().numpy(), I_ref) <= TOL
        assert relmax(out["phi"].cpu().numpy(), phi_ref) <= 1e-12
        assert relmax(out["acc"].cpu().numpy(), 1.5 * I_ref) <= TOL
        I7, phi7, _ = orc.set_wave_rt(np.full((Nx, Ny), 7500.0), g64, delta, beta, E, 0)
        ref1 = orc.fast_refraction(I7, phi7, z, E, M, pix_um)[0]
        ref2 = orc.fast_refraction(I7, phi7, 2 * z, E, M, pix_um)[0]
        assert relmax(out["refract"].cpu().numpy(), ref1) <= TOL
        assert relmax(out["multi"][0].cpu().numpy(), ref1) <= TOL and relmax(out["multi"][1].cpu().numpy(), ref2) <= TOL
        split = out["split"]
        assert relmax((split[0] + split[1]).cpu().numpy(), ref1) <= TOL
        ref_f = np.abs(orc.wave_propagation(orc.set_wave(np.full((Nx, Ny), np.sqrt(7500.0) + 0j), g64, delta, beta, E), z, E, M,
                                            (Nx, Ny), pix_um)) ** 2
        assert relmax(out["fresnel"].cpu().numpy(), ref_f) <= TOL, engine


def test_eight_maps_or_fewer_are_not_folded():
    """sample 5 + membrane 2 + air 1 = 8 maps: the same tensors and coefficients reach the kernel, bit for bit a direct
    C-ABI call."""
    from paresis_amd import ops
    from paresis_amd._lib import lib
    Nx, Ny = 64, 48
    Ts = torch.from_numpy(_maps(5, Nx, Ny, 1)).cuda()
    Tm = torch.from_numpy(_maps(2, Nx, Ny, 2)).cuda()
    Ta = torch.from_numpy(_maps(1, Nx, Ny, 3)).cuda()
    s = ops.MaterialStack(Ts, cphase=[-1e4 * (i + 1) for i in range(5)], catt=[-10.0 * (i + 1) for i in range(5)])
    m = ops.MaterialStack(Tm, cphase=[-3e4, -2e4], catt=[-50.0, -5.0])
    a = ops.MaterialStack(Ta, cphase=[0.0], catt=[-1.0])
    st = ops.MaterialStack.concat(a, m, s)
    assert st.n == 8 and not st.folded
    maps = [Ta[0], Tm[0], Tm[1]] + [Ts[i] for i in range(5)]
    assert all(st.map(i).data_ptr() == maps[i].data_ptr() for i in range(8))
    assert st.cphase == a.cphase + m.cphase + s.cphase and st.catt == a.catt + m.catt + s.catt
    I, phi = ops.transmit_rt(None, 2.0, st)
    I2 = torch.empty_like(I)
    phi2 = torch.empty_like(phi)
    Tp = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in maps])
    cp, ca = (ctypes.c_double * 8)(*st.cphase), (ctypes.c_double * 8)(*st.catt)
    rc = lib().psx_transmit_rt_f32(None, ctypes.c_float(2.0), Tp, cp, ca, 8, ctypes.c_void_p(I2.data_ptr()), None,
                                   ctypes.c_void_p(phi2.data_ptr()), I2.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert torch.equal(I, I2) and torch.equal(phi, phi2)
    # one more map folds the largest stack (the sample) only
    s6 = ops.MaterialStack(torch.from_numpy(_maps(6, Nx, Ny, 4)).cuda(), cphase=[-1e4] * 6, catt=[-10.0] * 6)
    st9 = ops.MaterialStack.concat(a, m, s6)
    assert st9.n == 6 and st9.folded and st9.cphase[:3] == a.cphase + m.cphase and st9.cphase[3:] == [1.0, 1.0, 0.0]
    assert st9.map(0).data_ptr() == Ta[0].data_ptr()
    with pytest.raises(ops.PsxError):
        ops.MaterialBatch(st9, [st9.cphase], [st9.catt])
    with pytest.raises(ops.PsxError, match="holds a fold"):                 # its maps belong to one coefficient set
        st9.with_coeffs(catt=[0.0] * st9.n)
    with pytest.raises(ops.PsxError, match="holds a fold"):
        s6.fold().with_coeffs(cphase=[2.0, 2.0, 0.0])
    assert s6.with_coeffs(catt=[0.0] * 6).n == 6                            # the raw stack takes new coefficients


def test_sample_keeps_its_folds_across_positions():
    from paresis_amd.Sample import AnalyticalSample
    s = AnalyticalSample()
    s.myName, s.myType, s.myMaterials = "phantom", "sample_of_interest", ["m%d" % i for i in range(13)]
    s.myGeometry = _maps(13, 40, 30, 5)
    delta, beta = _coeffs(13, 5)
    s.delta = [[(52.0, d)] for d in delta]
    s.beta = [[(52.0, b)] for b in beta]
    f1 = s.stack_rt(52.0).fold()
    assert s.stack_rt(52.0).fold() is f1 and len(s.fold_cache()) == 1
    s.stack_wave(52.0).fold()
    assert len(s.fold_cache()) == 2
    s.myGeometry = _maps(13, 40, 30, 6)                                      # a new geometry drops the old folds
    assert s.stack_rt(52.0).fold() is not f1 and len(s.fold_cache()) == 1


# --------------------------------------------------------------------------------------------------- chains
def _thirteen(cfg, seed):
    """cfg's sample replaced by 13 float32 maps (the sample's thickness shared out, plus a small bump each) with their own
    delta / beta per energy."""
    base = np.asarray(cfg["sample"].geometry[0], dtype=np.float64)
    rng = np.random.default_rng(seed)
    Nx, Ny = base.shape
    w = rng.uniform(0.5, 1.5, 13)
    geom = np.stack([base * w[m] / 13 * 4 for m in range(13)]) + _maps(13, Nx, Ny, seed, pix=1e-7)
    geom = geom.astype(np.float32)
    nE = len(cfg["spectrum"])
    d0, b0 = np.asarray(cfg["sample"].delta)[0], np.asarray(cfg["sample"].beta)[0]
    f = rng.uniform(0.6, 1.8, (13, 2))
    return orc.Obj(geom, [list(d0 * f[m, 0]) for m in range(13)], [list(b0 * f[m, 1]) for m in range(13)])


@pytest.mark.parametrize("sim", ["RT", "Fresnel"])
@pytest.mark.parametrize("tag", ["mono", "poly"])
def test_chains_take_a_thirteen_material_sample(tag, sim):
    """An injected 13-material sample through Experiment.computeSampleAndReferenceImages_{RT,Fresnel} against the oracle.
    The polychromatic grid is below the energy-batching limit: the chain must fall back to the per-energy loop."""
    g = load("experiment.npz")
    key = "%s/%s" % (tag, sim)
    cfg = experiment_cfg(g, key, orc.Obj)
    cfg["sample"] = _thirteen(cfg, 11)
    exp = build_experiment(cfg, sim, sample_materials=["mat%d" % m for m in range(13)])
    if tag == "poly":
        N = tuple(cfg["N"])
        assert N[0] * N[1] <= exp.BATCH_ENERGIES_MAX_PIXELS
        exp.exp_dict["batchEnergies"] = True                                # documented: a folding sample ignores it
    mem = lambda p: np.asarray(g["%s/p%d/membrane" % (key, p)], dtype=np.float32)
    bins = list(cfg["bins"])                                                # point 0 extends them, like the detector's own
    for point in (0, 1):
        exp.myMembrane.myGeometry = mem(point)
        exp.exp_dict["meanEnergy"] = 0
        out = exp.computeSampleAndReferenceImages(point)
        c = dict(cfg)
        c["bins"] = bins
        c["membrane"] = orc.Obj(mem(point).astype(np.float64), cfg["membrane"].delta, cfg["membrane"].beta)
        c["sample"] = orc.Obj(cfg["sample"].geometry, cfg["sample"].delta, cfg["sample"].beta)
        if cfg["air"] is not None:
            c["air"] = orc.Obj(np.asarray(cfg["air"].geometry, dtype=np.float32), cfg["air"].delta, cfg["air"].beta)
        if cfg["plate"] is not None:
            c["plate"] = orc.Obj(np.asarray(cfg["plate"].geometry, dtype=np.float32), cfg["plate"].delta, cfg["plate"].beta)
        ref = orc.compute_fresnel(c, point) if sim == "Fresnel" else orc.compute_rt(c, point)
        bins = c["bins"]
        for i, nm in enumerate(("Sample", "Reference", "Propag", "White")):
            err = relmax(out[i].cpu().numpy(), ref[i])
            assert err <= TOL, (tag, sim, point, nm, err)


# ------------------------------------------------------------------------------------------------ end to end
XML_REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "xml_ref")

# delta, beta at 52 keV: deterministic stand-ins of the order of magnitude of each material (no table of the reference's is
# readable here), scaled as delta ~ E^-2, beta ~ E^-3
ID17_DELTA_BETA_52KEV = {
    "CorticalBoneCB250pct": (1.62e-7, 1.9e-10), "Bone": (1.45e-7, 1.6e-10), "CorticalBoneCB230pct": (1.55e-7, 1.75e-10),
    "Solid Water": (8.7e-8, 6.0e-11), "Adipose": (8.1e-8, 5.2e-11), "InnerBone": (9.6e-8, 7.5e-11), "Breast": (8.5e-8, 5.6e-11),
    "Liver": (9.2e-8, 6.4e-11), "CorticalBoneSB3": (1.40e-7, 1.5e-10), "Brain": (8.9e-8, 6.1e-11), "Air": (1.0e-10, 7.0e-14),
    "SolidWater": (8.7e-8, 6.0e-11), "Cu": (6.3e-7, 4.1e-9), "PMMA": (9.9e-8, 5.3e-11)}


@pytest.fixture
def id17_materials():
    """delta / beta of the 13 phantom materials, the membrane's and air, registered for one test only: the registry, the
    provenance table and the synthetic flag are restored afterwards, so a shared pytest process still sees the contrast
    phantoms stop at the material table (test_host_cpu, reference-XML experiments)."""
    from paresis_amd import materials
    reg, prov, synthetic = dict(materials._REGISTRY), dict(materials._PROVENANCE), materials._allow_synthetic[0]
    try:
        for name, (d, b) in ID17_DELTA_BETA_52KEV.items():
            materials.register_material(name, lambda e, d=d, b=b: (d * (52.0 / e) ** 2, b * (52.0 / e) ** 3),
                                        "test stand-in (tests/test_gpu_phantom.py)")
        yield
    finally:
        materials._REGISTRY.clear()
        materials._REGISTRY.update(reg)
        materials._PROVENANCE.clear()
        materials._PROVENANCE.update(prov)
        materials._allow_synthetic[0] = synthetic


@pytest.mark.parametrize("sim", ["RayT", "Fresnel"])
def test_id17_contrast_phantom_end_to_end(id17_materials, sim):
    """The reference's own id17_ContrastPhantom (tests/fixtures/xml_ref) at oversampling 2: the phantom (13 maps, 1000 x 3000)
    behind the CuSn membrane (2) in air (1), position 0, noise off, against the oracle fed the float32 maps the GPU used.
    Its detector's thresholds (20, 30 keV) lie below the 52 keV monochromatic line, and the reference raises there
    (EXP:297, 426) -- so does the package; the test then puts the one threshold at the line."""
    from paresis_amd.Experiment import Experiment
    ed = {"experimentName": "id17_ContrastPhantom", "filepath": "/tmp/", "overSampling": 2, "nbExpPoints": 1,
          "simulation_type": sim, "noise": False, "xmlDir": XML_REF}
    exp = Experiment(ed)
    assert [int(v) for v in ed["studyDimensions"]] == [1000, 3000]
    geo = exp.mySampleofInterest.myGeometry
    assert isinstance(geo, torch.Tensor) and geo.is_cuda and tuple(geo.shape) == (13, 1000, 3000)
    assert len(exp.myMembrane.myMaterials) == 2 and len(exp.myAirVolume.myMaterials) == 1
    exp.myMembrane.myGeometry = []
    exp.myMembrane.getMyGeometry(ed["studyDimensions"], exp.myMembrane.membranePixelSize, 2, 0, 1)   # main.py:64-65
    assert exp.myDetector.det_param["myBinsThersholds"] == [20.0, 30.0]
    with pytest.raises(Exception, match="outside your source spectrum"):
        exp.computeSampleAndReferenceImages(0)
    exp.myDetector.det_param["myBinsThersholds"] = [52.0]
    cfg = cfg_from_experiment(exp, orc.Obj)
    ed["meanEnergy"] = 0
    out = exp.computeSampleAndReferenceImages(0)
    if sim == "RayT":
        ref = orc.compute_rt(cfg, 0)
        refs, mE = ref[:4], ref[6]
    else:
        ref = orc.compute_fresnel(cfg, 0)
        refs, mE = ref[:4], ref[4]
    for nm, a, r in zip(("Sample", "Reference", "Propag", "White"), out[:4], refs):
        assert np.max(np.abs(r)) > 0 or nm != "Sample"
        err = relmax(a.cpu().numpy(), r)
        assert err <= TOL, (sim, nm, err)
    assert abs(ed["meanEnergy"] - mE) < 1e-4
