"""The host side of the spectral material decomposition (paresis_amd/spectral.py, psx_decompose_f32's argument checks, main.py's
options) and the numpy oracle the GPU tests compare against (tests/_spectral_oracle.py).  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import _spectral_oracle as so

NAMES = list(so.ORDER)
THRESHOLDS = [34.0, 50.0]


def _experiment(names=("SpecSoft", "SpecIodine"), thresholds=THRESHOLDS, air=False, plate=False, N=(8, 6)):
    """A tests/_build.py experiment on the 20-80 keV spectrum sampled at 2 keV, its materials the oracle module's."""
    from oracle import paresis_oracle as orc
    from paresis_amd.getk import k_sample
    from tests._build import build_experiment
    E, flux = so.spectrum()
    k = np.array([k_sample(float(e)) for e in E])

    def obj(mus, thickness):
        beta = [list(mu(E) / (2 * k)) for mu in mus]
        delta = [[1e-7] * len(E) for _ in mus]
        return orc.Obj(np.stack([np.full(N, t, dtype=np.float32) for t in thickness]), delta, beta)

    M = (140.0 + 1.6 + 3.6) / (140.0 + 1.6)
    cfg = dict(scintillator=None, dSM=140.0, dMO=1.6, dOD=3.6, meanShotCount=30000.0, ov=2, pix_um=3.0, M=M, inVacuum=not air,
               N=N, spectrum=[(float(e), float(f)) for e, f in zip(E, flux)], source_size_um=0.0, energy_sampling=2.0,
               det_dims=(N[0] // 2, N[1] // 2), det_pix_um=6.0 * M, psf=0.0, bins=list(thresholds),
               membrane=obj([so.mu_soft, so.mu_soft], [1e-6, 1e-4]), sample=obj([so.MU.get(n, so.mu_soft) for n in names], [0.0] * len(names)),
               air=obj([lambda e: 0.02 * so.mu_soft(e)], [3.0]) if air else None,
               plate=obj([so.mu_bone], [2e-3]) if plate else None)
    return build_experiment(cfg, "RT", sample_materials=list(names)), E, flux


def test_model_of_takes_the_bins_and_the_flat_fields_shares():
    from paresis_amd import spectral
    exp, E, flux = _experiment()
    model = spectral.model_of(exp)
    assert model.names == ("SpecSoft", "SpecIodine") and model.bin_size == [8, 8, 15] and model.bins == 3
    assert [list(e) for e in model.energies] == [list(E[:8]), list(E[8:16]), list(E[16:])]
    e0 = 0
    for ne in model.bin_size:                            # in vacuum, no plate, no scintillator: the spectrum's own shares
        w = model.w[e0:e0 + ne]
        assert abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, flux[e0:e0 + ne] / flux[e0:e0 + ne].sum(), rtol=1e-14, atol=0)
        e0 += ne
    assert np.allclose(model.a, np.stack([so.mu_soft(E), so.mu_iodine(E)]), rtol=1e-13, atol=0)
    sizes, w = so.split(E, flux, THRESHOLDS)             # the oracle module's own split is the chain's
    assert sizes == model.bin_size and np.allclose(w, model.w, rtol=1e-14, atol=0)
    assert np.allclose(model.effective(), so.effective(sizes, w, model.a), rtol=1e-14, atol=0)
    one = spectral.model_of(exp, ["SpecIodine"])
    assert one.names == ("SpecIodine",) and np.allclose(one.a[0], so.mu_iodine(E), rtol=1e-13, atol=0)


def test_air_and_plate_harden_the_weights():
    from paresis_amd import spectral
    exp, E, flux = _experiment(air=True, plate=True)
    model = spectral.model_of(exp)
    att = flux * np.exp(-0.02 * so.mu_soft(E) * 3.0 - so.mu_bone(E) * float(np.float32(2e-3)))   # the maps are float32
    e0 = 0
    for ne in model.bin_size:
        assert np.allclose(model.w[e0:e0 + ne], att[e0:e0 + ne] / att[e0:e0 + ne].sum(), rtol=1e-12, atol=0)
        e0 += ne
    exp.myPlate.myGeometry = exp.myPlate.myGeometry.copy()
    exp.myPlate.myGeometry[0, 1, 1] *= 2
    with pytest.raises(ValueError, match="plate.*not uniform"):
        spectral.model_of(exp)


def test_leftover_energies_are_dropped():
    """Thresholds the caller has closed already, the last below the spectrum's end: the energies above it are computed by the
    chain and never detected."""
    from paresis_amd import spectral
    exp, E, _ = _experiment()
    exp._bins_ready = True
    model = spectral.model_of(exp)
    assert model.bin_size == [8, 8] and float(model.energies[-1][-1]) == 50.0 and model.a.shape == (2, 16)


def test_model_errors():
    from paresis_amd import spectral
    exp, _, _ = _experiment()
    with pytest.raises(ValueError, match="not one of the sample"):
        spectral.model_of(exp, ["SpecSoft", "Water"])
    with pytest.raises(ValueError, match="each material once"):
        spectral.model_of(exp, ["SpecSoft", "SpecSoft"])
    exp, _, _ = _experiment(thresholds=[76.0, 77.0, 78.0, 79.0])
    with pytest.raises(ValueError, match="closed by no energy"):
        spectral.model_of(exp)
    exp, _, _ = _experiment(names=NAMES, thresholds=[50.0])
    with pytest.raises(ValueError, match="4 materials cannot be told apart from 2 energy bins"):
        spectral.model_of(exp)
    assert spectral.model_of(exp, NAMES[:2]).bins == 2
    exp, _, _ = _experiment(names=NAMES + ["SpecSoft2"], thresholds=[30.0, 40.0, 50.0, 60.0])
    with pytest.raises(ValueError, match="4 materials at most"):
        spectral.model_of(exp)


def test_rank_deficiency_names_the_condition_number():
    """Two materials of one energy dependence -- the synthetic stand-ins of the shipped ones all scale as E^-3."""
    from paresis_amd import materials, spectral
    E, flux = so.spectrum()
    sizes, w = so.split(E, flux, THRESHOLDS)
    beta = np.stack([np.array([materials._synthetic(n)(float(e))[1] for e in E]) for n in ("PMMA", "Nylon")])
    ws = [w[:8], w[8:16], w[16:]]
    es = [E[:8], E[8:16], E[16:]]
    model = spectral.SpectralModel(("PMMA", "Nylon"), es, ws, beta * E[None, :] * 1e13)
    assert model.condition() > 1e12
    with pytest.raises(ValueError, match=r"condition number .* > 1e\+08.*E\^-3"):
        model.check_rank()
    good = spectral.SpectralModel(("SpecSoft", "SpecBone", "SpecIodine"), es, ws, so.coefficients(E, 3))
    A = good.effective()
    assert abs(good.condition() - np.linalg.cond(A / np.linalg.norm(A, axis=0))) < 1e-9 and good.check_rank() <= 30
    assert good.condition() < np.linalg.cond(A)          # the columns' units do not count
    with pytest.raises(ValueError, match="sum to"):
        spectral.SpectralModel(("a",), [E[:2]], [[0.5, 0.6]], [[1.0, 2.0]])
    with pytest.raises(ValueError, match="2 materials cannot be told apart from 1 energy bins"):
        spectral.SpectralModel(("a", "b"), [E[:2]], [[0.5, 0.5]], [[1.0, 2.0], [2.0, 1.0]])


def test_transmission_and_monochromatic_on_the_host():
    import torch
    from paresis_amd import spectral
    E, flux = so.spectrum()
    sizes, w = so.split(E, flux, THRESHOLDS)
    a = so.coefficients(E, 2)
    model = spectral.SpectralModel(NAMES[:2], [E[:8], E[8:16], E[16:]], [w[:8], w[8:16], w[16:]], a)
    t = np.random.default_rng(3).uniform(0, 1, (2, 5, 7)) * np.array([0.05, 0.01])[:, None, None]
    T = spectral.transmission(model, torch.from_numpy(t))
    assert T.dtype == torch.float32 and tuple(T.shape) == (3, 5, 7)
    ref = so.transmission(sizes, w, a, t.reshape(2, -1)).reshape(3, 5, 7)
    assert np.array_equal(T.numpy(), ref.astype(np.float32)) or np.abs(T.numpy() - ref).max() <= 2.0 ** -24
    mono = spectral.monochromatic(torch.from_numpy(t), model, 60.0)
    assert np.allclose(mono.numpy(), so.mu_soft(60.0) * t[0] + so.mu_bone(60.0) * t[1], rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match="not one of the model's energies"):
        spectral.monochromatic(torch.from_numpy(t), model, 61.0)


@pytest.mark.parametrize("M,thresholds", [(1, []), (2, THRESHOLDS), (3, THRESHOLDS), (4, [34.0, 42.0, 50.0])])
def test_oracle_recovers_known_thicknesses(M, thresholds):
    """From exact float64 data the oracle returns the thicknesses to rounding, within 7 steps, and float64 agrees with long
    double to 1e-13 of the scale; from the same data rounded to float32 the error is of the size of that rounding times the
    problem's conditioning."""
    E, flux = so.spectrum()
    sizes, w = so.split(E, flux, thresholds)
    a = so.coefficients(E, M)
    v = np.ones(len(sizes))
    G = so.linear_start(sizes, w, a, v)
    scale = np.array([0.05, 0.01, 0.004, 0.004])[:M]
    x = np.random.default_rng(5).uniform(0, 1, (M, 300)) * scale[:, None]
    L = -np.log(so.transmission(sizes, w, a, x))
    got, res, steps = so.decompose(L, sizes, w, a, v, G)
    assert steps.min() >= 1 and steps.max() <= 7
    assert (np.abs(got - x).max(axis=1) <= 1e-12 * scale).all() and res.max() < 1e-13
    ld, _, _ = so.decompose(L, sizes, w, a, v, G, dtype=np.longdouble)
    assert ld.dtype == np.longdouble and (np.abs(got - ld).max(axis=1) <= 1e-13 * scale).all()
    got32, _, steps32 = so.decompose(L.astype(np.float32), sizes, w, a, v, G)
    assert steps32.max() <= 7 and (np.abs(got32 - x).max(axis=1) <= 1e-5 * scale).all()


def test_oracle_flags_and_single_energy_bins():
    E = np.array([30.0, 60.0])
    a = so.coefficients(E, 2)
    sizes, w, v = [1, 1], np.ones(2), np.array([1.0, 2.5])
    G = so.linear_start(sizes, w, a, v)
    x = np.array([[0.03, 0.0, 0.01], [0.004, 0.0, -0.001]])
    L = (a.T @ x).astype(np.float32).astype(np.float64)
    L[1, 1] = np.nan
    got, res, steps = so.decompose(L, sizes, w, a, v, G)
    assert steps[1] == -1 and res[1] == np.inf and (got[:, 1] == 0).all()
    assert (steps[[0, 2]] >= 1).all() and (steps[[0, 2]] <= 2).all()            # the model is linear: exact after one step
    assert np.allclose(got[:, [0, 2]], np.linalg.solve(a.T, L[:, [0, 2]]), rtol=1e-12, atol=0)
    bad, _, st = so.decompose(L[:, :1], sizes, w, np.stack([a[0], a[0]]), v, G)     # proportional materials: no pivot
    assert st[0] == -2 and np.array_equal(bad[:, 0], G @ L[:, 0])


def _call(lib, **over):
    """psx_decompose_f32 with valid host-side arguments and made-up device addresses, `over` replacing some: none of these
    calls may get as far as the GPU."""
    B, M, E = 3, 2, 5
    keep = []

    def arr(ctype, vals):
        keep.append((ctype * len(vals))(*vals))
        return keep[-1]

    args = dict(logT=arr(ctypes.c_void_p, [4096, 8192, 12288]), B=B, bin_size=arr(ctypes.c_int, [2, 2, 1]),
                w=arr(ctypes.c_double, [0.5, 0.5, 0.5, 0.5, 1.0]), a=arr(ctypes.c_double, [1.0] * (M * E)), M=M,
                v=arr(ctypes.c_double, [1.0] * B), G=arr(ctypes.c_double, [0.0] * (M * B)), iterations=12, tol=1e-13, n=10,
                thickness=arr(ctypes.c_void_p, [16384, 20480]), residual=None, steps=None, stream=None)
    args.update(over)
    for k in ("logT", "thickness"):
        if isinstance(args[k], list):
            args[k] = arr(ctypes.c_void_p, args[k])
    if isinstance(args["bin_size"], list):
        args["bin_size"] = arr(ctypes.c_int, args["bin_size"])
    rc = lib.psx_decompose_f32(*[args[k] for k in ("logT", "B", "bin_size", "w", "a", "M", "v", "G", "iterations", "tol", "n",
                                                   "thickness", "residual", "steps", "stream")])
    return rc, lib.psx_last_error().decode()


def test_abi_argument_errors_come_before_any_gpu_call():
    from paresis_amd import _lib
    lib = _lib.lib()
    assert _lib.ABI_VERSION >= 22 and lib.psx_abi_version() == _lib.ABI_VERSION
    assert (_lib.PSX_DECOMP_MAX_MAT, _lib.PSX_DECOMP_MAX_BINS, _lib.PSX_DECOMP_MAX_ENERGIES) == (4, 8, 256)
    cases = [(dict(logT=None), "null logT"), (dict(bin_size=None), "null bin_size"), (dict(w=None), "null w"),
             (dict(a=None), "null a"), (dict(v=None), "null v"), (dict(G=None), "null G"), (dict(thickness=None), "null thickness"),
             (dict(logT=[4096, None, 12288]), "logT[1] is null"), (dict(thickness=[16384, None]), "thickness[1] is null"),
             (dict(B=0), "B=0"), (dict(B=9), "B=9"), (dict(M=0), "M=0"), (dict(M=5, B=8), "M=5"), (dict(M=3, B=2), "M=3"),
             (dict(bin_size=[2, 0, 3]), "bin_size[1]=0"), (dict(bin_size=[100, 100, 57]), "more than 256"),
             (dict(iterations=0), "iterations=0"), (dict(tol=-1e-3), "tol="), (dict(tol=float("nan")), "tol="),
             (dict(tol=float("inf")), "tol="), (dict(n=0), "n=0"), (dict(n=-5), "n=-5")]
    for over, text in cases:
        rc, msg = _call(lib, **over)
        assert rc == -1 and "psx_decompose_f32" in msg and text in msg, (over, rc, msg)


def test_ops_decompose_checks_on_the_host():
    import torch
    from paresis_amd import ops
    L = torch.zeros((3, 4), dtype=torch.float32)
    a = [[1.0] * 5, [2.0] * 5]
    good = dict(bin_size=[2, 2, 1], w=[0.5, 0.5, 0.5, 0.5, 1.0], a=a, v=[1.0] * 3, G=[[0.0] * 3] * 2)
    for over, text in ((dict(bin_size=[2, 2]), "bin_size"), (dict(w=[1.0]), "sum of bin_size"), (dict(v=[1.0, 0.0, 1.0]), "v must"),
                       (dict(G=[[0.0] * 3]), "G must be 2 x 3"), (dict(iterations=0), "iterations"), (dict(tol=-1.0), "tol"),
                       (dict(a=[[1.0] * 5] * 4), "M=4 materials")):
        with pytest.raises(ops.PsxError, match=text):
            ops.decompose(L, **dict(good, **over))
    with pytest.raises(ops.PsxError, match="HBM"):                     # everything else is right: only the device is not
        ops.decompose(L, **good)


def test_main_options(tmp_path, capsys):
    from paresis_amd import main
    with pytest.raises(SystemExit) as e:
        main.main(["--out", str(tmp_path), "--decompose-materials", "PMMA"])
    assert e.value.code == 2 and "--decompose-materials is an option of --decompose" in capsys.readouterr().err
    with pytest.raises(ValueError, match="decompose_materials is an option of decompose"):
        main.run({"nbExpPoints": 1}, decompose_materials=["PMMA"])
