"""UMPA on the GPU (csrc/umpa.hip, ops.umpa, retrieval.umpa / retrieve(method='umpa'), main.py --method umpa) against the
float64 numpy oracle of tests/_umpa_oracle.py, whose compare() holds the parity rule: border band bit-exact, fallback masks
equal, interior pixels with gap < 1e-10 excluded (their share <= 1e-4), |ddx|, |ddy| <= 1e-5 px, relative dT <= 1e-5,
|dresidual| <= 1e-7 + 1e-5*residual."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from tests import _retrieval_oracle as orl
from tests import _umpa_oracle as ou

pytestmark = pytest.mark.gpu

KEYS = ('transmission', 'dx', 'dy', 'residual')
MULT = max(1, int(os.environ.get("PSX_FUZZ", "1")))                  # PSX_FUZZ=k: the two 64-pair sweeps under k seeds


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _gpu_umpa(S, R, w, s):
    from paresis_amd import retrieval
    r = retrieval.umpa(_cuda(np.stack(S)), _cuda(np.stack(R)), window=w, search=s)
    assert sorted(r) == sorted(KEYS)
    return {k: _np(v) for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def _warped(n, m, K, dmax):
    return ou.warped_model(n, m, K, seed=n + m + K, dmax=dmax)


# (n, m, K, w, s, dmax): both tile widths (w <= 4: 32, beyond: 16), one to three chunks per candidate row (s <= 3, 4, 8), K = 1,
# both caps at once (1 x 3 interior pixels), and 33 x 21 tiles with ragged edges on both axes.  The oracle alone excludes no
# pixel at any of them (smallest interior gap: 6.0e-8, at 96 x 80).
SHAPES = [(96, 80, 5, 2, 3, 2.5), (301, 173, 16, 3, 3, 3.5), (48, 40, 3, 1, 2, 2.0), (40, 52, 1, 4, 2, 1.5),
          (33, 35, 64, 8, 8, 4.0), (200, 200, 8, 2, 4, 4.0), (520, 648, 4, 2, 2, 2.0)]


@pytest.mark.parametrize("n,m,K,w,s,dmax", SHAPES)
def test_umpa_matches_oracle(n, m, K, w, s, dmax):
    T, Dx, Dy, S, R = _warped(n, m, K, dmax)
    o = ou.umpa(S, R, w, s)
    f = ou.compare(_gpu_umpa(S, R, w, s), o, w, s, label="%dx%d K=%d" % (n, m, K))
    assert f['compared'] > 0


def test_umpa_known_answer():
    """S_k = 0.8 * R_k shifted by (2, -3) (Fourier shift: exact for whole pixels): dy sits on the search boundary and is exactly
    -3, T = 0.8, the residual vanishes; dx = 2 up to the parabola through asymmetric neighbours (the oracle: 0.027)."""
    n, m, K = 64, 72, 4
    rng = np.random.default_rng(10)
    R = [orl.speckle(n, m, rng).astype(np.float32) for _ in range(K)]
    kx, ky = np.fft.fftfreq(n)[:, None], np.fft.fftfreq(m)[None, :]
    ramp = np.exp(-2j * np.pi * (kx * 2.0 + ky * -3.0))
    S = [np.float32(0.8 * np.fft.ifft2(np.fft.fft2(r.astype(np.float64)) * ramp).real) for r in R]
    g = _gpu_umpa(S, R, 2, 3)
    inner = ou.umpa(S, R, 2, 3)['interior']
    assert np.array_equal(g['dy'][inner], np.full(inner.sum(), -3.0, np.float32))
    et = np.abs(g['transmission'][inner].astype(np.float64) - 0.8).max()
    med = np.median(np.abs(g['dx'][inner].astype(np.float64) - 2.0))
    print("known answer: |T-0.8| %.2e, residual max %.2e, median |dx-2| %.4f" % (et, g['residual'][inner].max(), med))
    assert et <= 1e-6
    assert g['residual'][inner].max() <= 1e-10
    assert med <= 0.05


def test_umpa_goes_beyond_lcs():
    """Fields of up to 4 px: on interior pixels with |Dx| or |Dy| > 1.5 px UMPA's median Euclidean error is <= 0.15 px (the
    oracle: 0.057), that of LCS on the same images >= 0.5 px (the oracle: 1.00)."""
    from paresis_amd import retrieval
    n, m, K, w, s, dmax = SHAPES[5]
    T, Dx, Dy, S, R = _warped(n, m, K, dmax)
    St, Rt = _cuda(np.stack(S)), _cuda(np.stack(R))
    u = {k: _np(v) for k, v in retrieval.umpa(St, Rt, window=w, search=s).items()}
    l = {k: _np(v) for k, v in retrieval.lcs(St, Rt).items()}
    band = w + s
    big = (np.abs(Dx) > 1.5) | (np.abs(Dy) > 1.5)
    big[:band] = big[-band:] = False
    big[:, :band] = big[:, -band:] = False
    eu = np.median(np.hypot(u['dx'] - Dx, u['dy'] - Dy)[big])
    el = np.median(np.hypot(l['dx'] - Dx, l['dy'] - Dy)[big])
    print("beyond LCS, %d pixels: median error umpa %.3f px, lcs %.3f px" % (big.sum(), eu, el))
    assert big.sum() > 10000
    assert eu <= 0.15
    assert el >= 0.5


def test_umpa_fallback_bits():
    """A block without reference (every candidate skipped) and a block without sample (T = 0): exactly (1, 0, 0, 0) two pixels
    inside either; everywhere else the parity rule, without a cap on the excluded share."""
    T, Dx, Dy, S, R = ou.warped_model(64, 80, 3, seed=7, dmax=0.8)
    for k in range(3):
        R[k][10:22, 12:24] = 0.0
        S[k][36:48, 50:62] = 0.0
    g = _gpu_umpa(S, R, 1, 1)
    o = ou.umpa(S, R, 1, 1)
    for blk in ((slice(12, 20), slice(14, 22)), (slice(38, 46), slice(52, 60))):
        assert o['fallback'][blk].all()
        for key, v in zip(KEYS, (1.0, 0.0, 0.0, 0.0)):
            assert np.array_equal(g[key][blk], np.full((8, 8), v, np.float32)), key
    ou.compare(g, o, 1, 1, cap=None, label="fallback blocks")


# ------------------------------------------------------------------------------------------ every (w, s), bit for bit
# The host picks one of 16 kernels, tile width 32 (w <= 4) or 16 times s = 1..8, and the LDS layout, the chunks of a candidate
# row, the surplus candidate and the prologue's rows per thread vary with (w, s): all 64 pairs run.  On integer images the
# contract's sums are exact and every later step is one IEEE operation (tests/_umpa_oracle.py), so the four maps are compared
# with np.array_equal over the whole image.  tests/test_umpa_host.py shows that these inputs hold all-skipped, partly skipped,
# T <= 0 and ordinary pixels in several tiles and no exact tie, and that wrong kernels of five kinds would differ on them.
@pytest.mark.parametrize("w,s", ou.PAIRS)
def test_umpa_every_window_and_search_exact(w, s):
    for rep in range(MULT):
        S, R = ou.sweep_instance(w, s, rep)
        o = ou.umpa(S, R, w, s)
        assert o['fallback'].sum() > 9                               # the 3 x 3 all-skipped pixels and the T <= 0 block
        ou.compare_exact(_gpu_umpa(S, R, w, s), o, label="w=%d s=%d K=%d %dx%d" % ((w, s, len(S)) + S[0].shape))


@pytest.mark.parametrize("w,s,period", ou.TIE_CASES)
def test_umpa_ties_take_the_first_minimum(w, s, period):
    """A reference of period (p, q) makes L(u) == L(u + (p, 0)) == L(u + (0, q)) exactly at every interior pixel: the first
    minimum in scan order is asked for, with its parabola.  Both tile widths; one, two and three chunks per candidate row."""
    S, R = ou.tie_instance(w, s, period)
    o = ou.umpa(S, R, w, s)
    f = ou.compare_exact(_gpu_umpa(S, R, w, s), o, ties=True, label="period %s w=%d s=%d" % (period, w, s))
    assert f['ties'] == f['interior'] > 0


@pytest.mark.parametrize("w,s", ou.PAIRS)
def test_umpa_every_window_and_search_warped(w, s):
    """Float images with displacements up to about s - 1/2 under the parity rule, cap 1e-4 (at the committed seed the oracle
    alone excludes no pixel: tests/test_umpa_host.py)."""
    for rep in range(MULT):
        S, R = ou.warped_instance(w, s, rep)
        f = ou.compare(_gpu_umpa(S, R, w, s), ou.umpa(S, R, w, s), w, s, label="warped %dx%d K=%d" % (S[0].shape + (len(S),)))
        assert f['compared'] > 0


@pytest.mark.parametrize("w,s", ou.PAIRS)
def test_umpa_smallest_images(w, s):
    """One interior pixel, and one interior row / column of 40 pixels (two or three tiles along it)."""
    q = 2 * (w + s) + 1
    for shape in ((q, q), (q, q + 39), (q + 39, q)):
        S, R = ou.integer_model(w, s, ou.sweep_K(w, s), seed=4000 + 100 * w + s, shape=shape)
        o = ou.umpa(S, R, w, s)
        assert o['interior'].sum() == (shape[0] - q + 1) * (shape[1] - q + 1)
        ou.compare_exact(_gpu_umpa(S, R, w, s), o, label="w=%d s=%d %dx%d" % ((w, s) + shape))


@pytest.mark.parametrize("w,s", [(4, 8), (5, 1), (8, 7)])
def test_umpa_many_positions_exact(w, s):
    """K = 64 (the most) and 63.  |S| <= 2*4095 + 7 and R <= 4095, so E, B, C <= 64 * 17^2 * 8197^2 = 1.25e12 at w = 8: exact
    integers in float64 (2^53 = 9.0e15) with vmax as everywhere else."""
    for K in (64, 63):
        S, R = ou.integer_model(w, s, K, seed=5000 + K)
        ou.compare_exact(_gpu_umpa(S, R, w, s), ou.umpa(S, R, w, s), label="w=%d s=%d K=%d" % (w, s, K))


def test_umpa_input_forms_streams_and_no_allocation_on_reuse():
    from paresis_amd import ops
    T, Dx, Dy, S, R = _warped(96, 80, 5, 2.5)
    St, Rt = _cuda(np.stack(S)), _cuda(np.stack(R))
    a = ops.umpa(St, Rt)
    assert len(a) == 4
    b = ops.umpa([St[k].clone() for k in range(5)], [Rt[k].clone() for k in range(5)])
    stacks_s = [torch.stack([St[k] * 0.5, St[k], St[k] * 2]) for k in range(5)]
    stacks_r = [torch.stack([Rt[k] * 0.5, Rt[k], Rt[k] * 2]) for k in range(5)]
    c = ops.umpa([s[1] for s in stacks_s], [r[1] for r in stacks_r])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = ops.umpa(St, Rt)
    torch.cuda.current_stream().wait_stream(side)
    for x in (b, c, d):
        for u, v in zip(a, x):
            assert torch.equal(u, v)
    assert not torch.equal(a[1], ops.umpa(St, Rt, window=3, search=2)[1])
    outs = tuple(torch.full_like(a[0], 7.0) for _ in range(4))
    got = ops.umpa(St, Rt, out=outs)
    torch.cuda.synchronize()
    assert all(x is y for x, y in zip(got, outs))
    mem = torch.cuda.memory_allocated()
    ops.umpa(St, Rt, out=outs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem
    for u, v in zip(a, outs):
        assert torch.equal(u, v)


def test_umpa_argument_errors():
    from paresis_amd import ops
    from paresis_amd._lib import PsxError
    img = lambda K, n=16, m=16, dt=torch.float32: torch.ones((K, n, m), dtype=dt, device="cuda")
    for K in (0, 65):
        with pytest.raises(PsxError, match="K=%d" % K):
            ops.umpa(img(K), img(K))
    for kw in ({'window': 0}, {'window': 9}, {'search': 0}, {'search': 9}):
        with pytest.raises(PsxError, match="integer in"):
            ops.umpa(img(2), img(2), **kw)
    with pytest.raises(PsxError, match="smaller than 11x11"):
        ops.umpa(img(2, 16, 10), img(2, 16, 10))
    with pytest.raises(PsxError, match="shape"):
        ops.umpa(img(2), img(2, 16, 17))
    with pytest.raises(PsxError, match="positions"):
        ops.umpa(img(2), img(3))
    with pytest.raises(PsxError, match="float32"):
        ops.umpa(img(2, dt=torch.float64), img(2, dt=torch.float64))
    with pytest.raises(PsxError, match="out must hold four"):
        ops.umpa(img(2), img(2), out=[torch.empty(16, 16, device="cuda")] * 3)
    # the C entry point checks for itself
    import ctypes
    lib = ops.lib()
    x, o = img(1), torch.empty(16, 16, device="cuda")
    ptr = (ctypes.c_void_p * 1)(x.data_ptr())
    po = ctypes.c_void_p(o.data_ptr())
    for K, n, w, s in ((0, 16, 2, 3), (65, 16, 2, 3), (1, 16, 0, 3), (1, 16, 9, 3), (1, 16, 2, 0), (1, 16, 2, 9), (1, 10, 2, 3)):
        assert lib.psx_umpa_f32(ptr, ptr, K, n, 16, w, s, po, po, po, po, None) != 0, (K, n, w, s)
        assert b"psx_umpa_f32" in lib.psx_last_error()


def _run(K, tmp_path, name, **kw):
    from paresis_amd import main
    ed = {"experimentName": "Fil_Nylon_ID17", "filepath": str(tmp_path) + "/" + name + "/", "overSampling": 2,
          "nbExpPoints": K, "simulation_type": "RayT", "noise": False, "seed": 3}
    os.makedirs(ed["filepath"], exist_ok=True)
    return ed, main.run(ed, **kw)


def test_main_retrieve_umpa_writes_maps(tmp_path):
    from paresis_amd import retrieval
    from paresis_amd.InputOutput.pagailleIO import openImage
    ed, res = _run(3, tmp_path, "three", save=True, saving_format=".tif", retrieve=True, method='umpa')
    files = sorted(glob.glob(ed["filepath"] + "*/retrieval/*.tif"))
    name = lambda f: os.path.basename(f).split("_")[0]
    assert sorted(name(f) for f in files) == ["dx", "dy", "phi", "residual", "transmission"], files
    maps = {name(f): openImage(f) for f in files}
    S = [_np(res[p][0])[0] for p in sorted(res)]
    R = [_np(res[p][1])[0] for p in sorted(res)]
    o = ou.umpa(S, R, 2, 3)
    ou.compare({k: np.asarray(maps[k], dtype=np.float32) for k in KEYS}, o, 2, 3, label="the chain's images")
    assert np.isfinite(maps['phi']).all() and np.abs(maps['phi']).max() > 0
    # the CLI on the run's directory writes the same bytes
    run_dir = os.path.dirname(os.path.dirname(files[0]))
    p = ed['retrievalParams']
    before = {f: open(f, "rb").read() for f in files}
    for f in files:
        os.remove(f)
    retrieval.main([run_dir, "--method", "umpa", "--energy", repr(p['energy_keV']), "--pixel-um", repr(p['pixel_um']),
                    "--distance", repr(p['distance_m']), "--magnification", repr(p['magnification'])])
    for f in files:
        assert open(f, "rb").read() == before[f], f
    # one position is enough, and other window / search values arrive
    ed1, res1 = _run(1, tmp_path, "one", save=True, saving_format=".npy", retrieve=True, method='umpa', window=3, search=2)
    files1 = sorted(glob.glob(ed1["filepath"] + "*/retrieval/*.npy"))
    assert sorted(name(f) for f in files1) == ["dx", "dy", "phi", "residual", "transmission"], files1
    o1 = ou.umpa([_np(res1[0][0])[0]], [_np(res1[0][1])[0]], 3, 2)
    ou.compare({name(f): np.asarray(openImage(f), dtype=np.float32) for f in files1 if name(f) in KEYS}, o1, 3, 2,
               label="one position")


# ------------------------------------------------------------------------------------ end to end with |D| > 1 pixel
# The nylon wire of Fil_Nylon_ID17 with its delta times DELTA_FACTOR (beta unchanged): the wire's edges then displace the
# speckles by many pixels.  CPU calibration: oracle.compute_rt over 12 positions -- shifted copies of one synthetic sphere
# membrane -- in this configuration (ov = 2, mono 52 keV, no noise), then both numpy oracles (UMPA w = 2, s = 3; LCS) against
# e2e.truths on the mask 1 <= max(|dx_t|, |dy_t|) <= s - 1 = 2, 8 px inside the frame.  Median Euclidean error in pixels,
# UMPA / LCS = ratio (mask size), per delta factor:
#   2: 0.295 / 1.120 = 0.264 (61)      3: 0.218 / 1.088 = 0.200 (159)     4: 0.189 / 1.176 = 0.160 (323)
#   5: 0.169 / 1.191 = 0.142 (576)     6: 0.169 / 1.220 = 0.139 (920)     7: 0.163 / 1.258 = 0.129 (1353)
#   8: 0.150 / 1.273 = 0.118 (1860)    9: 0.128 / 1.275 = 0.101 (2420)   10: 0.117 / 1.287 = 0.091 (3017)
# Factor 10 has the lowest ratio and, with 8 and 9, the 1500 pixels asked for (max |D_true| 17 px: beyond the mask).  The
# calibration is below 0.35, so the GPU run must reach 0.5.
DELTA_FACTOR = 10.0
E2E_EXPERIMENT = "Fil_DenseNylon_ID17"
E2E_MAX_RATIO = 0.5

_E2E_SAMPLE = """    <sample>
        <name>filDenseNylon</name>
        <myType>sample_of_interest</myType>
        <myGeometryFunction>CreateSampleCylindre</myGeometryFunction>
        <myRadius unit="um">700</myRadius>
        <myOrientation unit="degree">30</myOrientation>
        <myMaterials>DenseNylon</myMaterials>
    </sample>
</listSamples>"""

_E2E_EXPERIMENT = """    <experiment>
        <name>%s</name>
        <distSourceToMembrane unit="m">140</distSourceToMembrane>
        <distMembraneToObject unit="m">1.6</distMembraneToObject>
        <distObjectToDetector unit="m">3.6</distObjectToDetector>
        <membraneName>Mask_CuSn_From_txt</membraneName>
        <sampleName>filDenseNylon</sampleName>
        <sampleType>AnalyticalSample</sampleType>
        <detectorName>sCMOS_ESRF</detectorName>
        <sourceName>id17</sourceName>
        <meanShotCount>30000</meanShotCount>
        <inVacuum>True</inVacuum>
    </experiment>
</listExperiment>""" % E2E_EXPERIMENT


def _write_xml(directory):
    """The package's four XML files plus the dense nylon wire and its experiment (as tests/_retrieval_df_e2e.write_xml)."""
    import shutil
    from paresis_amd import _xml
    os.makedirs(directory, exist_ok=True)
    for nm in ("Experiment.xml", "Samples.xml", "Detectors.xml", "Sources.xml"):
        shutil.copy(os.path.join(_xml._PKG_XML, nm), os.path.join(directory, nm))
    for nm, tail, add in (("Samples.xml", "</listSamples>", _E2E_SAMPLE), ("Experiment.xml", "</listExperiment>", _E2E_EXPERIMENT)):
        p = os.path.join(directory, nm)
        s = open(p).read()
        assert s.rstrip().endswith(tail)
        open(p, "w").write(s.rstrip()[:-len(tail)] + add + "\n")
    return directory


def test_end_to_end_beyond_one_pixel(tmp_path):
    from paresis_amd import main, materials, retrieval
    from paresis_amd.Experiment import Experiment
    from tests import _retrieval_e2e as e2e

    def dense(e):
        d, b = materials.delta_beta("Nylon", e)
        return DELTA_FACTOR * d, b

    xml_dir = _write_xml(str(tmp_path / "xml"))
    ed = {"experimentName": E2E_EXPERIMENT, "filepath": str(tmp_path) + "/run/", "overSampling": 2, "nbExpPoints": 12,
          "simulation_type": "RayT", "noise": False, "seed": 3, "xmlDir": xml_dir}
    os.makedirs(ed["filepath"], exist_ok=True)
    materials.register_material("DenseNylon", dense, "test: Nylon with delta times %g" % DELTA_FACTOR)
    try:
        res = main.run(ed, save=False, retrieve=True, method='umpa')
        exp = Experiment(dict(ed, filepath=str(tmp_path) + "/probe/"))
        T, delta = _np(exp.mySampleofInterest.myGeometry)[0], exp.mySampleofInterest.delta[0][0][1]
    finally:
        materials._REGISTRY.pop("DenseNylon", None)
        materials._PROVENANCE.pop("DenseNylon", None)
    params = ed['retrievalParams']
    w, s = 2, 3
    u = retrieval.retrieve(res, params, method='umpa', window=w, search=s)[0]
    l = retrieval.retrieve(res, params)[0]
    dx_t, dy_t, _ = e2e.truths(_np(res[0][4]), _np(res[0][5]), T, delta, params['energy_keV'])
    big = np.maximum(np.abs(dx_t), np.abs(dy_t))
    m = (big >= 1) & (big <= s - 1)
    m[:8] = m[-8:] = False
    m[:, :8] = m[:, -8:] = False
    eu = np.median(np.hypot(_np(u['dx']) - dx_t, _np(u['dy']) - dy_t)[m])
    el = np.median(np.hypot(_np(l['dx']) - dx_t, _np(l['dy']) - dy_t)[m])
    print("e2e |D| > 1: mask %d, max |D_true| %.1f, median error umpa %.3f px, lcs %.3f px, ratio %.3f"
          % (m.sum(), big.max(), eu, el, eu / el))
    assert m.sum() >= 1500
    assert eu / el <= E2E_MAX_RATIO
