"""Differential phase tomography without a GPU: the float64 oracle of tests/_hilbert_oracle.py against the ramp on analytic
sinograms and on the restated phantom (so that the GPU tests compare against the right operator), the float32 yardstick of the
GPU parity bound, the contract's constants, and every refusal the differential route adds."""
import argparse
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import _fbp_oracle as fo
from tests import _hilbert_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("P", [64, 128, 1024])
def test_response_is_imaginary_odd_and_zero_at_dc_and_nyquist(P):
    G = ho.hilbert_transform(P)
    assert np.abs(G.real).max() < 1e-15
    assert np.abs(G.imag + np.roll(G.imag[::-1], 1)).max() < 1e-15
    for name in ho.FILTERS:
        Ho = ho.hilbert_response(P, name)
        assert Ho[0] == 0.0 and Ho[P // 2] == 0.0
        assert np.abs(Ho + np.roll(Ho[::-1], 1)).max() < (1e-15 if name == "hilbert" else 2.0 / P)   # the Hann window of an even
        # length is even about P/2 - 1/2, not about P/2: the device takes the odd part, as it takes the ramp's even part
    # -i sgn(f)/pi away from DC and Nyquist: Ho = -1/pi on the positive frequencies
    Ho = ho.hilbert_response(P, "hilbert")
    assert np.abs(Ho[P // 8:3 * P // 8] + 1 / np.pi).max() < 0.02 and np.all(Ho[1:P // 2] < 0) and np.all(Ho[P // 2 + 1:] > 0)


@pytest.mark.parametrize("m", [2, 5, 32, 33, 64])
def test_hilbert_filter_is_the_direct_convolution(m):
    """P >= 2m: every lag |k - j| < m is inside the kernel, so q[k] = sum_j g[k - j] line[j], linear and not wrapped."""
    rng = np.random.default_rng(m)
    line = rng.normal(size=m)
    g = ho.hilbert_kernel(fo.pad_length(m))
    j = np.arange(m)
    direct = (g[(j[:, None] - j[None, :]) % len(g)] * line[None, :]).sum(axis=1)
    q = ho.filter_lines(line[None, None, :], "hilbert")[0, 0]
    assert np.abs(q - direct).max() <= 1e-13 * np.abs(direct).max()
    assert g[1] == 2 / np.pi ** 2 and g[-1] == -g[1] and g[2] == 0 and g[len(g) // 2] == 0


@pytest.mark.parametrize("case", ho.BLOB_CASES, ids=lambda c: "m%d-A%d" % c[:2])
def test_hilbert_of_the_derivative_is_the_ramp(case):
    """Three Gaussian blobs, analytic p and dp/du: fbp_hilbert(dp/du) = fbp_ramp(p) to discretisation -- within twice the gap
    first seen per case -- and the other sign of the kernel misses by the whole volume, twice over."""
    m, A, center, gap = case
    theta, p, dp = ho.blob_sinograms(m, A, center)
    ramp = fo.fbp(p, theta, center, "ramp")
    peak = np.abs(ramp).max()
    got = np.abs(ho.fbp(dp, theta, center, "hilbert") - ramp).max() / peak
    wrong = np.abs(ho.fbp(dp, theta, center, "hilbert", sign=-1.0) - ramp).max() / peak
    print("blobs m=%d A=%d: gap %.3e (bound %.1e), wrong sign %.3f, peak %.3f" % (m, A, got, 2 * gap, wrong, peak))
    assert got <= 2 * gap
    assert 1.9 <= wrong <= 2.1
    assert 0.5 < peak < 1.5                                   # the blobs themselves came back: amplitudes 1, -0.6, 0.8


def test_restated_phantom_delta_comes_back_from_central_differences():
    """The 13-material delta slice through central differences of its sinogram and the Hilbert filter: the mean over each
    material's interior within 3 % of the largest delta (twice the 1.48 % first seen; the ramp on the sinogram itself gives
    0.47 %)."""
    slices = fo.phantom_slices(64, 500.0)
    theta = np.arange(90) * 2.0
    sino = np.stack([np.stack([fo.radon_line(s.astype(np.float64), a) for s in slices]) for a in theta])
    delta = np.array(fo.PHANTOM_DELTA)
    line = np.einsum("akm,k->am", sino, delta)[:, None, :]
    vol = ho.fbp(ho.central_differences(line), theta)[0]
    err = [abs(vol[fo.interior(slices[k])].mean() - delta[k]) / delta.max() for k in range(13)]
    print("worst interior mean error / max delta: %.4f" % max(err))
    assert max(err) <= 0.03


@pytest.mark.parametrize("shape", ho.SHAPES[:5] + ho.EXTRA_SHAPES)
def test_float32_yardstick(shape):
    """The float32 / complex64 restatement reproduces F32_ERROR_HILBERT, in the manner of tests/test_fbp_host.py (the
    512-pixel shape is left to the table, as there)."""
    A, n, m = shape
    theta, sino = fo.case_angles(A), fo.case_sino(A, n, m)
    worst = 0.0
    for flt in ho.FILTERS:
        for c in fo.case_centers(m):
            ref = ho.fbp(sino, theta, c, flt, False)
            worst = max(worst, float(np.abs(ho.fbp_f32(sino, theta, c, flt, False) - ref).max() / np.abs(ref).max()))
    print("float32 restatement at %s: %.3e (table %.3e)" % (shape, worst, ho.F32_ERROR_HILBERT[shape]))
    assert 0 < worst <= 1.25 * ho.F32_ERROR_HILBERT[shape]
    assert sorted(ho.F32_ERROR_HILBERT) == sorted(ho.SHAPES) and [fo.pad_length(k) for k in (32, 33)] == [64, 128]


def test_plan_create_refuses_every_other_filter():
    from paresis_amd import _lib
    lib = _lib.lib()
    th = (ctypes.c_double * 3)(0.0, 60.0, 120.0)
    for flt in (3, 15, 18, -1):
        h = ctypes.c_void_p(None)
        rc = lib.psx_fbp_plan_create(3, 8, th, 4.0, flt, 1, 0, ctypes.byref(h))
        text = lib.psx_last_error().decode()
        assert rc == -1 and not h.value and "filter" in text and str(flt) in text, (flt, rc, text)


def test_tables_and_header_agree():
    from paresis_amd import _lib
    assert _lib.FBP_FILTERS == {"ramp": 0, "hann": 1, "none": 2}
    assert _lib.FBP_DIFFERENTIAL_FILTERS == {"hilbert": 16, "hilbert-hann": 17}
    assert _lib.ABI_VERSION >= 21 and _lib.lib().psx_abi_version() == _lib.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "paresis_hip.h")).read()
    values = {}
    for name, expr in re.findall(r"^#define (PSX_FBP_[A-Z_]+)\s+(\([^)]*\)|\d+)", text, flags=re.M):
        values[name] = eval(expr, {"__builtins__": {}}, dict(values))
    assert values["PSX_FBP_DIFFERENTIAL"] == 16
    assert values["PSX_FBP_HILBERT"] == _lib.FBP_DIFFERENTIAL_FILTERS["hilbert"] == 16
    assert values["PSX_FBP_HILBERT_HANN"] == _lib.FBP_DIFFERENTIAL_FILTERS["hilbert-hann"] == 17
    assert "(PSX_FBP_DIFFERENTIAL | PSX_FBP_HANN)" in text and "(PSX_FBP_DIFFERENTIAL | PSX_FBP_RAMP)" in text
    assert [values[k] for k in ("PSX_FBP_RAMP", "PSX_FBP_HANN", "PSX_FBP_NONE")] == [0, 1, 2]


def test_binding_takes_the_new_names_and_checks_before_the_device():
    import torch
    from paresis_amd import ops, tomography
    with pytest.raises(ops.PsxError, match="filter.*hilbert.*shepp"):
        ops.FbpPlan([0.0, 90.0], 8, filter="shepp")
    with pytest.raises(ops.PsxError, match="filter"):
        ops.FbpPlan([0.0, 90.0], 8, filter="hilbert_hann")
    with pytest.raises(ops.PsxError, match="no CPU path|HBM"):               # a known name: on to the tensor's own check
        tomography.fbp(torch.zeros((2, 1, 8)), [0.0, 90.0], filter="hilbert")


def _scanned(**over):
    sc = {'sinograms': {}, 'angles': [0.0, 90.0], 'center': 4.0, 'voxel_m': 1e-6, 'modality': 'phase', 'differential': True,
          'energy_keV': 52.0}
    sc.update(over)
    return sc


def test_reconstruct_refusals():
    from paresis_amd import tomography
    assert tomography.DIFFERENTIAL_FILTER_OF == {'ramp': 'hilbert', 'hann': 'hilbert-hann'}
    assert tomography.reconstruct(_scanned()) == {} and tomography.reconstruct(_scanned(), filter='hann') == {}
    with pytest.raises(ValueError, match="filter"):
        tomography.reconstruct(_scanned(), filter='none')
    for method, extra in (('sirt', {}), ('cgls', {}), ('tv', {'weight': 0.1})):
        with pytest.raises(ValueError, match="differential"):
            tomography.reconstruct(_scanned(), method=method, iterations=3, **extra)
    with pytest.raises(ValueError, match="differential"):
        tomography.reconstruct(_scanned(modality='attenuation'))
    integral = _scanned()
    del integral['differential']                                # a dict from before the key: an integral scan, any method
    assert tomography.reconstruct(integral, method='sirt', iterations=3) == {}
    assert tomography.reconstruct(_scanned(differential=False), filter='none') == {}


def test_run_option_refusals():
    from paresis_amd import main, tomography
    tomography.check_run_options(4, 'phase', 'fbp', 0, None)                  # the positional form of before
    tomography.check_run_options(4, 'phase', 'fbp', 0, None, True)
    tomography.check_run_options(4, 'phase', 'fbp', 0, None, differential=True)
    tomography.check_run_options(0, 'attenuation', 'fbp', 0, None, differential=False)
    for args, msg in (((0, 'attenuation', 'fbp', 0, None), "tomography_differential is an option of tomography"),
                      ((4, 'attenuation', 'fbp', 0, None), "differential is an option of modality 'phase'"),
                      ((4, 'phase', 'sirt', 3, None), "method 'fbp'"), ((4, 'phase', 'cgls', 3, None), "method 'fbp'"),
                      ((4, 'phase', 'tv', 3, 0.1), "method 'fbp'")):
        with pytest.raises(ValueError, match=msg):
            tomography.check_run_options(*args, differential=True)
    ed = {"experimentName": "x", "filepath": "/nonexistent/", "overSampling": 2, "nbExpPoints": 3, "simulation_type": "RayT"}
    with pytest.raises(ValueError, match="differential is an option of modality 'phase'"):
        main.run(dict(ed), save=False, tomography=4, tomography_differential=True)
    with pytest.raises(ValueError, match="tomography_differential is an option of tomography"):
        main.run(dict(ed), save=False, tomography_differential=True)
    with pytest.raises(ValueError, match="method 'fbp'"):
        main.run(dict(ed), save=False, tomography=4, tomography_modality='phase', tomography_method='sirt',
                 tomography_iterations=2, tomography_differential=True)


def test_scan_refuses_differential_attenuation():
    from paresis_amd import tomography
    exp = types.SimpleNamespace(exp_dict={"nbExpPoints": 3},
                                mySampleofInterest=types.SimpleNamespace(myGeometryFunction="generateContrastPhantom"))
    with pytest.raises(ValueError, match="differential is an option of modality 'phase'"):
        tomography.scan(exp, [0.0], modality="attenuation", differential=True)
    with pytest.raises(ValueError, match="differential is an option of modality 'phase'"):
        tomography.scan(exp, [0.0], differential=True)
    assert tomography.MODALITIES == ("attenuation", "phase")


def test_cli_option_parses_and_is_refused_out_of_place(capsys, tmp_path):
    from paresis_amd import main, tomography
    ap = argparse.ArgumentParser()
    tomography.add_tomography_options(ap)
    assert ap.parse_args([]).tomography_differential is False
    a = ap.parse_args(["--tomography", "4", "--tomography-modality", "phase", "--tomography-differential"])
    assert a.tomography_differential is True and a.tomography_modality == "phase"
    tomography.check_tomography_options(ap, a)                                # in place: no error
    phase = ["--tomography", "4", "--tomography-modality", "phase", "--points", "3"]
    for argv, msg in ((["--tomography-differential"], "--tomography-differential is an option of --tomography"),
                      (["--tomography", "4", "--tomography-differential"],
                       "--tomography-differential goes with --tomography-modality phase and --tomography-method fbp"),
                      (phase + ["--tomography-method", "sirt", "--tomography-iterations", "3", "--tomography-differential"],
                       "--tomography-differential goes with --tomography-modality phase and --tomography-method fbp"),
                      (phase + ["--tomography-method", "tv", "--tomography-iterations", "3", "--tomography-weight", "0.1",
                                "--tomography-differential"],
                       "--tomography-differential goes with --tomography-modality phase and --tomography-method fbp")):
        with pytest.raises(SystemExit):
            main.main(["--out", str(tmp_path / "o")] + argv)
        assert msg in capsys.readouterr().err, argv
