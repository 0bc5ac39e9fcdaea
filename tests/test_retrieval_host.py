"""Phase retrieval without a GPU: the float64 oracle of the contract (tests/_retrieval_oracle.py), the unit conversion of
paresis_amd.retrieval, the CLI's discovery of main.run's layout, and the argument checks that come before any device."""
import numpy as np
import pytest
import torch

from tests import _retrieval_oracle as orl


def test_oracle_recovers_exact_model():
    T, Dx, Dy, S, R = orl.exact_model(64, 48, 6, seed=1)
    r = orl.lcs(S, R, dtype=np.float64, return_mask=True)
    assert not r['fallback'].any()
    assert np.abs(r['transmission'] - T).max() < 1e-10
    assert np.abs(r['dx'] - Dx).max() < 1e-10
    assert np.abs(r['dy'] - Dy).max() < 1e-10


def test_oracle_k3_solve_is_exact():
    """Three positions: three equations, three unknowns -- the fit interpolates every R_k."""
    rng = np.random.default_rng(3)
    R = [orl.speckle(40, 30, rng).astype(np.float32) for _ in range(3)]
    S = [orl.speckle(40, 30, rng).astype(np.float32) for _ in range(3)]
    M, v = orl.normal_equations(S, R)
    x = np.linalg.solve(M, v[..., None])[..., 0]
    for k in range(3):
        g0, g1 = orl.gradients(R[k])
        fit = x[..., 0] * S[k] + x[..., 1] * g0 + x[..., 2] * g1
        assert np.abs(fit - R[k]).max() / np.abs(R[k]).max() < 1e-9


def test_oracle_fallback_and_clamp():
    T, Dx, Dy, S, R = orl.exact_model(40, 40, 5, seed=2, dmax=2.0)
    for k in range(5):                                   # a flat reference block: zero gradient columns
        R[k][10:20, 10:20] = 5000.0
        S[k][10:20, 10:20] = 4000.0
    r = orl.lcs(S, R, return_mask=True)
    inner = (slice(11, 19), slice(11, 19))
    assert r['fallback'][inner].all()
    assert np.all(r['transmission'][inner] == 1.0) and np.all(r['dx'][inner] == 0.0) and np.all(r['dy'][inner] == 0.0)
    c = orl.lcs(S, R, max_shift=0.75)
    assert np.abs(Dx).max() > 1.0
    assert c['dx'].max() == np.float32(0.75) and c['dx'].min() == np.float32(-0.75)
    assert np.all(np.abs(c['dx']) <= np.float32(0.75)) and np.all(np.abs(c['dy']) <= np.float32(0.75))


def test_oracle_integration_known_answer():
    """phi evenly extended (a cosine series on the 2n x 2m grid): its spectral gradients integrate back to phi - mean."""
    n, m = 48, 40
    rng = np.random.default_rng(4)
    i = np.arange(n)[:, None] + 0.5
    j = np.arange(m)[None, :] + 0.5
    phi = np.zeros((n, m))
    gx = np.zeros((n, m))
    gy = np.zeros((n, m))
    for _ in range(6):                                   # cos(pi a i/n) cos(pi b j/m): even about the borders
        a, b = rng.integers(0, 6, 2)
        c = rng.standard_normal()
        ca, cb = np.cos(np.pi * a * i / n), np.cos(np.pi * b * j / m)
        phi += c * ca * cb
    # gradients of the extension, formed spectrally (the extension is periodic; its spectrum is what FC inverts)
    E = np.concatenate([phi, phi[::-1, :]], 0)
    E = np.concatenate([E, E[:, ::-1]], 1)
    kx = 2 * np.pi * np.fft.fftfreq(2 * n)[:, None]
    ky = 2 * np.pi * np.fft.fftfreq(2 * m)[None, :]
    F = np.fft.fft2(E)
    gx = np.fft.ifft2(1j * kx * F).real[:n, :m]
    gy = np.fft.ifft2(1j * ky * F).real[:n, :m]
    out = orl.integrate(gx, gy)
    assert np.abs(out - (phi - phi.mean())).max() < 1e-10


def test_phase_gradient_inverts_the_chain_displacement():
    """A linear phase ramp on the study grid (ov = 2) -> the chain's displacement (RF2:54-56) -> the detector's 2x2 binning ->
    phase_gradient returns the binned ramp's slope per detector pixel."""
    from paresis_amd.getk import getk, k_refraction
    from paresis_amd.retrieval import phase_gradient
    E, p_um, z, M, ov = 52.0, 6.0, 3.6, 145.2 / 141.6, 2
    h = p_um / ov / M * 1e-6                              # study pixel (EXP:188)
    a0, a1 = 0.013, -0.021                                # rad per study pixel
    N = 16
    phi = a0 * np.arange(N)[:, None] + a1 * np.arange(N)[None, :]
    dphix, dphiy = np.gradient(phi, h, edge_order=2)       # RF2:54
    Dx = dphix * z / k_refraction(E) / (h * M)            # RF2:55 (study pixels)
    Dy = dphiy * z / k_refraction(E) / (h * M)
    bin2 = lambda a: a.reshape(N // ov, ov, N // ov, ov).mean(axis=(1, 3))
    dx, dy = bin2(Dx) / ov, bin2(Dy) / ov                 # detector pixels
    gx, gy = phase_gradient(dx, dy, E, p_um, z, M)
    binned = bin2(phi)
    sx = binned[1, 0] - binned[0, 0]                      # the binned ramp's slope per detector pixel
    sy = binned[0, 1] - binned[0, 0]
    assert abs(getk(E * 1e3) - k_refraction(E)) / getk(E * 1e3) < 1e-14
    assert np.abs(gx - sx).max() < 1e-12 * abs(sx) + 1e-15 and np.abs(gy - sy).max() < 1e-12 * abs(sy) + 1e-15
    assert np.abs(gx - sx).max() / abs(sx) < 1e-12


def _layout(root, exp_id, positions, fmt, bins=None, drop=None):
    """main.run's directory layout (main.py: sample/sampleImage_<id>_NN, ref/ReferenceImage_<id>_NN, per bin directory)."""
    from paresis_amd.InputOutput.pagailleIO import save_image
    rng = np.random.default_rng(0)
    dirs = [str(root) + "/"] if bins is None else [str(root) + "/%s/" % b for b in bins]
    for d in dirs:
        for p in positions:
            for sub, name in (("sample/", "sampleImage_"), ("ref/", "ReferenceImage_")):
                if drop == (sub, p):
                    continue
                import os
                os.makedirs(d + sub, exist_ok=True)
                save_image(rng.random((5, 4)).astype(np.float32), d + sub + name + exp_id + "_" + "%2.2d" % p + fmt)
    return dirs


@pytest.mark.parametrize("fmt", [".tif", ".edf", ".npy"])
def test_cli_discovery_single_bin(tmp_path, fmt):
    from paresis_amd.retrieval import discover
    _layout(tmp_path, "20260101-120000", [0, 1, 2, 3], fmt)
    (tmp_path / "DF.tif").write_bytes(b"")
    found = discover(str(tmp_path))
    assert len(found) == 1
    d, exp_id, f, pairs = found[0]
    assert d == str(tmp_path) and exp_id == "20260101-120000" and f == fmt
    assert [p for p, _, _ in pairs] == [0, 1, 2, 3]
    for p, s, r in pairs:
        assert s.endswith("sample/sampleImage_20260101-120000_%2.2d%s" % (p, fmt))
        assert r.endswith("ref/ReferenceImage_20260101-120000_%2.2d%s" % (p, fmt))


def test_cli_discovery_two_bins(tmp_path):
    from paresis_amd.retrieval import discover
    _layout(tmp_path, "X1", [0, 1, 2], ".tif", bins=["20_30kev", "30_40kev"])
    found = discover(str(tmp_path))
    assert [f[0] for f in found] == [str(tmp_path / "20_30kev"), str(tmp_path / "30_40kev")]
    assert all(len(f[3]) == 3 for f in found)


def test_cli_discovery_errors(tmp_path):
    from paresis_amd.retrieval import discover
    _layout(tmp_path / "a", "X", [0, 1, 2, 3], ".tif", drop=("ref/", 2))
    with pytest.raises(ValueError, match="no reference partner"):
        discover(str(tmp_path / "a"))
    _layout(tmp_path / "b", "X", [0, 1], ".npy")
    with pytest.raises(ValueError, match="at least 3 positions"):
        discover(str(tmp_path / "b"))
    (tmp_path / "c").mkdir()
    with pytest.raises(ValueError, match="no sample/ and ref/"):
        discover(str(tmp_path / "c"))


def test_argument_errors_before_any_device():
    from paresis_amd import ops
    from paresis_amd._lib import PsxError
    img = lambda K, n=8, m=8: torch.ones((K, n, m), dtype=torch.float32)
    with pytest.raises(PsxError, match="K=2"):
        ops.lcs(img(2), img(2))
    with pytest.raises(PsxError, match="K=65"):
        ops.lcs(img(65), img(65))
    with pytest.raises(PsxError, match="shape"):
        ops.lcs([torch.ones(8, 8), torch.ones(8, 8), torch.ones(8, 9)], img(3))
    with pytest.raises(PsxError, match="positions"):
        ops.lcs(img(3), img(4))
    with pytest.raises(PsxError, match="HBM"):                            # CPU tensors: no CPU path
        ops.lcs(img(3), img(3))
    with pytest.raises(PsxError, match="HBM"):
        ops.lcs([t for t in img(3)], [t for t in img(3)])
