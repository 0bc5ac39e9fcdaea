"""Paganin retrieval without a GPU: the float64 oracle of the contract (tests/_paganin_oracle.py), the filter's units against
the oracle chains, the discovery of main.run's propagation images, and the argument checks that come before any device."""
import os

import numpy as np
import pytest
import torch

from tests import _paganin_oracle as po


def test_oracle_known_answer():
    """t a cosine series on the extension, r formed spectrally from exp(-mu t): the oracle returns t.  Bound: x is rounded to
    float32 once (6e-8*max|r - 1| per pixel, damped by the filter), so 1e-6*max|r - 1|/(mu*c_min) in thickness."""
    for (n, m), alpha, mu in (((48, 40), 3.0, 22.0), ((33, 57), 400.0, 50.0), ((2, 2), 0.0, 22.0)):
        t, r = po.known_answer(n, m, alpha, mu)
        o = po.paganin(r, None, alpha, mu)
        assert o['thickness'].dtype == np.float32 and o['contact'].dtype == np.float32
        bound = 1e-6 * max(np.abs(r - 1).max(), 1e-3) / (mu * np.exp(-mu * t).min()) + 1.2e-7 * t.max()
        assert np.abs(o['thickness'] - t).max() <= bound, (n, m, alpha)
        assert np.abs(o['contact'] - np.exp(-mu * t)).max() <= 1e-6


def test_oracle_guards_and_dc():
    I, I0 = po.image_pair(12, 9, seed=1)
    I0[0, 0], I0[1, 1], I0[2, 2], I0[3, 3] = 0.0, -5.0, np.nan, np.inf
    I[4, 4] = np.nan
    r = po.ratio(I, I0)
    assert all(r[i, i] == 1.0 for i in range(5)) and np.isfinite(r).all()
    o = po.paganin(I, I0, 3.0, 22.0)
    assert np.isfinite(o['contact']).all() and np.isfinite(o['thickness']).all()
    # the filter passes the mean of the extension unchanged
    assert abs(o['y'].mean() - (r - 1).astype(np.float32).astype(np.float64).mean()) < 1e-12
    # a dark region without a filter: c <= 0 takes the finite floor
    dark = np.ones((6, 5), np.float32)
    dark[2:4, 1:3] = -0.5
    dark[0, 0] = -1.0
    o = po.paganin(dark, None, 0.0, 22.0)
    floor = np.float32(-np.log(po.FLT_MIN) / 22.0)
    assert np.all(o['thickness'][2:4, 1:3] == floor) and o['thickness'][0, 0] == floor
    assert np.abs(o['thickness'][dark == 1.0]).max() < 1e-15


# The issue's table: max|thickness - bin2(T)|/max T of the blob experiment through the CPU oracle chains, alpha from z*M (the
# contract), z, z/M, and without a filter
BLOB_TABLE = {"RT": (0.042, 0.13, 0.22, 0.36), "Fresnel": (0.034, 0.18, 0.28, 0.96)}


@pytest.mark.parametrize("sim", ["RT", "Fresnel"])
def test_blob_calibration_pins_alpha(sim):
    from oracle import paresis_oracle as orc
    from paresis_amd import retrieval
    cfg, T = po.blob_cfg()
    out = orc.compute_rt(cfg, 0) if sim == "RT" else orc.compute_fresnel(cfg, 0)
    P, W = out[2][0], out[3][0]
    kw = po.blob_params(cfg)
    alpha, mu = retrieval.paganin_alpha(**kw)
    M = kw['magnification']
    assert M == 2.0
    got = [po.blob_error(po.paganin(P, W, a, mu)['thickness'], T) for a in (alpha, alpha / M, alpha / M ** 2, 0.0)]
    print("blob %s: z*M %.4f, z %.4f, z/M %.4f, no filter %.4f" % ((sim,) + tuple(got)))
    for g, want in zip(got, BLOB_TABLE[sim]):
        assert abs(g - want) <= 0.2 * want, (sim, got)
    assert got[0] == min(got) and got[0] <= 0.08


def test_paganin_alpha_hand_values():
    from paresis_amd import retrieval, synth
    from paresis_amd.getk import getk
    d, b = synth.DELTA_BETA_52KEV["Nylon"]
    alpha, mu = retrieval.paganin_alpha(d, b, 52.0, 6.0, 3.6, 1.0254)
    assert abs(alpha - 440.7) < 0.05 and abs(mu - 22.105) < 5e-4
    assert mu == 2 * getk(52e3) * b and alpha == 3.6 * 1.0254 * d / (mu * 6e-6 ** 2)
    # ov-free and linear in z*M; no phase contrast, no filter
    a2, _ = retrieval.paganin_alpha(d, b, 52.0, 6.0, 1.8, 2.0508)
    assert abs(a2 - alpha) <= 1e-12 * alpha
    assert retrieval.paganin_alpha(0.0, b, 52.0, 6.0, 3.6, 1.0)[0] == 0.0
    for bad in (dict(beta=0.0), dict(beta=-1e-11), dict(delta=-1e-8), dict(delta=float("nan")), dict(pixel_um=0.0),
                dict(magnification=0.0), dict(energy_keV=0.0), dict(distance_m=-1.0)):
        kw = dict(delta=d, beta=b, energy_keV=52.0, pixel_um=6.0, distance_m=3.6, magnification=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            retrieval.paganin_alpha(**kw)


def test_argument_errors_before_any_device():
    from paresis_amd import ops, retrieval
    from paresis_amd._lib import PsxError
    img = lambda B, n=8, m=8: torch.ones((B, n, m), dtype=torch.float32)
    with pytest.raises(PsxError, match="B=0"):
        ops.paganin(img(0), None, 1.0, 1.0, None)
    with pytest.raises(PsxError, match="B=65"):
        ops.paganin(img(65), None, 1.0, 1.0, None)
    with pytest.raises(PsxError, match=r"\[B, n, m\]"):
        ops.paganin(torch.ones(8, 8), None, 1.0, 1.0, None)
    with pytest.raises(PsxError, match="whites holds 2"):
        ops.paganin(img(3), img(2), 1.0, 1.0, None)
    with pytest.raises(PsxError, match="alpha must hold one value per image"):
        ops.paganin(img(3), None, [1.0, 2.0], 1.0, None)
    for alpha, mu, what in ((-1.0, 1.0, "alpha"), (float("nan"), 1.0, "alpha"), (1.0, 0.0, "mu"), (1.0, float("inf"), "mu"),
                            ([0.0, 1.0, -2.0], 1.0, "alpha"), (1.0, [1.0, 1.0, -1.0], "mu")):
        with pytest.raises(PsxError, match=what + " must be finite"):
            ops.paganin(img(3), None, alpha, mu, None)
    with pytest.raises(PsxError, match="plan must be an ops.IntegratePlan"):
        ops.paganin(img(3), None, 1.0, 1.0, None)
    kw = dict(delta=1e-7, beta=4e-11, energy_keV=52.0, pixel_um=6.0, distance_m=3.6, magnification=1.0)
    with pytest.raises(PsxError, match="HBM"):                            # CPU tensors: no CPU path
        retrieval.paganin(torch.ones(8, 8), **kw)
    with pytest.raises(PsxError, match="HBM"):
        retrieval.paganin(img(2), img(2), **kw)
    with pytest.raises(ValueError, match="one value per image"):
        retrieval.paganin(img(3), **dict(kw, delta=[1e-7, 2e-7]))
    with pytest.raises(ValueError, match="no propagation image"):
        retrieval.retrieve_propagation({0: (img(1), img(1))}, {}, (1e-7, 4e-11))
    with pytest.raises(ValueError, match="no propagation image"):
        retrieval.retrieve_propagation({1: (img(1),) * 4}, {}, (1e-7, 4e-11))


def _layout(root, exp_id, fmt, bins=None, drop=None):
    """main.run's propagation files: <bin dir>/propag/PropagImage_<id>_<fmt> and <bin dir>/White_<id>_<fmt>."""
    from paresis_amd.InputOutput.pagailleIO import save_image
    rng = np.random.default_rng(0)
    dirs = [str(root) + "/"] if bins is None else [str(root) + "/%s/" % b for b in bins]
    for d in dirs:
        os.makedirs(d + "propag/", exist_ok=True)
        os.makedirs(d + "sample/", exist_ok=True)
        if drop != "propag":
            save_image(rng.random((5, 4)).astype(np.float32), d + "propag/PropagImage_" + exp_id + "_" + fmt)
        if drop != "white":
            save_image(rng.random((5, 4)).astype(np.float32), d + "White_" + exp_id + "_" + fmt)
    return dirs


@pytest.mark.parametrize("fmt", [".tif", ".edf", ".npy"])
def test_discover_propagation(tmp_path, fmt):
    from paresis_amd.retrieval import discover_propagation
    _layout(tmp_path / "one", "20260101-120000", fmt)
    (tmp_path / "one" / "DF.tif").write_bytes(b"")
    os.makedirs(tmp_path / "one" / "propag" / "retrieval")               # an earlier retrieval's output is no input
    (tmp_path / "one" / "propag" / "retrieval" / ("contact_20260101-120000" + fmt)).write_bytes(b"")
    (d, exp_id, f, pg, wh), = discover_propagation(str(tmp_path / "one"))
    assert d == str(tmp_path / "one") and exp_id == "20260101-120000" and f == fmt
    assert pg == os.path.join(d, "propag", "PropagImage_20260101-120000_" + fmt)
    assert wh == os.path.join(d, "White_20260101-120000_" + fmt)
    _layout(tmp_path / "two", "X1", fmt, bins=["20_30kev", "30_40kev"])
    found = discover_propagation(str(tmp_path / "two"))
    assert [x[0] for x in found] == [str(tmp_path / "two" / "20_30kev"), str(tmp_path / "two" / "30_40kev")]


def test_discover_propagation_errors(tmp_path):
    from paresis_amd.retrieval import discover_propagation
    _layout(tmp_path / "a", "X", ".tif", drop="white")
    with pytest.raises(ValueError, match="has no flat field"):
        discover_propagation(str(tmp_path / "a"))
    _layout(tmp_path / "b", "X", ".tif", drop="propag")
    with pytest.raises(ValueError, match="has no propagation image"):
        discover_propagation(str(tmp_path / "b"))
    _layout(tmp_path / "c", "X", ".tif")
    _layout(tmp_path / "c", "Y", ".tif")
    with pytest.raises(ValueError, match="several runs"):
        discover_propagation(str(tmp_path / "c"))
    (tmp_path / "d").mkdir()
    with pytest.raises(ValueError, match="no propag/PropagImage_"):
        discover_propagation(str(tmp_path / "d"))


def test_propagation_material_rules():
    from paresis_amd.Experiment import Experiment
    from paresis_amd.retrieval import propagation_material
    exp = Experiment({"experimentName": "Fil_Nylon_ID17", "filepath": "/tmp/", "overSampling": 2, "nbExpPoints": 1,
                      "simulation_type": "RayT"})
    assert propagation_material(exp) == "Nylon" and propagation_material(exp, "Nylon") == "Nylon"
    with pytest.raises(ValueError, match="not one of the sample of interest's"):
        propagation_material(exp, "PMMA")
    exp.mySampleofInterest.myMaterials = ["PMMA", "Nylon"]
    assert propagation_material(exp) == "PMMA" and propagation_material(exp, "Nylon") == "Nylon"
    exp.mySampleofInterest.myMaterials = []
    with pytest.raises(ValueError, match="names no material"):
        propagation_material(exp)


def test_command_line_rules(tmp_path, capsys):
    from paresis_amd import main, retrieval
    phys = ["--energy", "52", "--pixel-um", "6", "--distance", "3.6", "--magnification", "1.02"]
    prop = [str(tmp_path), "--propagation", "--delta", "9.5e-8", "--beta", "4.2e-11"]
    for extra, msg in ((["--method", "umpa"], "none of the tracker options"), (["--dark-field"], "none of the tracker options"),
                       (["--max-shift", "1"], "none of the tracker options"), (["--window", "3"], "none of the tracker options"),
                       (["--search", "2"], "none of the tracker options")):
        with pytest.raises(SystemExit):
            retrieval.main(prop + phys + extra)
        assert msg in capsys.readouterr().err
    with pytest.raises(SystemExit):
        retrieval.main(prop)                                              # no physical parameters
    assert "--propagation needs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        retrieval.main([str(tmp_path), "--propagation", "--delta", "9.5e-8"] + phys)
    assert "--propagation needs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        retrieval.main([str(tmp_path), "--propagation", "--delta", "9.5e-8", "--beta", "0"] + phys)
    assert "beta must be finite and > 0" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        retrieval.main([str(tmp_path), "--delta", "9.5e-8"] + phys)
    assert "options of --propagation" in capsys.readouterr().err
    with pytest.raises(ValueError, match="no propag/PropagImage_"):      # the rules passed: discovery comes next, no GPU yet
        retrieval.main(prop + phys)
    with pytest.raises(SystemExit):
        main.main(["--out", str(tmp_path / "o"), "--material", "Nylon"])
    assert "--material is an option of --retrieve-propagation" in capsys.readouterr().err
    with pytest.raises(ValueError, match="material is an option of propagation"):
        main.run({"experimentName": "Fil_Nylon_ID17", "nbExpPoints": 1}, material="Nylon")
