"""The kernel-spectrum tables of the power-of-two line kernels are stored in the order the lanes of the middle stage load them
(csrc/fresnel_p2_dev.hpp, namespace spectrum): every compiled form of k_fresnel_p2 / k_fresnel_p2x must still meet each point of
a transformed line with its own bin.

White complex noise in: with a flat spectrum ONE misplaced bin shows at about 1e-3 of the peak, far above the tolerance (a
smooth wave would hide it).  All distances differ, so the two spectra of a DUAL round cannot be swapped unseen.  Whole complex
fields and the intensity images against the float64 oracle, tolerance and norm of
test_gpu_kernels.py::test_fresnel_power_of_two_lines_and_wrapped_outputs.  The 24-sample axis runs on k_fresnel_lines, whose
tables keep their order."""
import functools

import numpy as np
import pytest
import torch

from oracle import paresis_oracle as orc
from tests._golden import relmax

pytestmark = pytest.mark.gpu

TOL = 1e-5
ZS = (0.4, 2.3, 5.2, 7.2)
E, PIX, MAG, AMP = 52.0, 2.9, 1.03, 1.25
DL, BL = np.array([6.2e-7, 9.9e-8]), np.array([4e-9, 4.5e-11])

# one long axis per radix (R1 = 4, 8, 16, 32), each on either axis: every radix runs as pass 1 and as pass 2
SHAPES = [(512, 24), (24, 1024), (2048, 24), (24, 4096), (24, 512), (1024, 24), (24, 2048), (4096, 24)]


@pytest.fixture(scope="module")
def ops():
    from paresis_amd import ops as _ops
    from paresis_amd._lib import lib
    assert lib().psx_device_ok() == 1, lib().psx_last_error()
    return _ops


def dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()      # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def case(shape, nz):
    """Inputs and the oracle's fields at the first nz distances of ZS for one grid (computed once, shared by the cases, read only)."""
    Nx, Ny = shape
    rng = np.random.default_rng(11 + Nx + 3 * Ny)
    T64 = rng.uniform(0.0, 3e-5, size=(2, Nx, Ny))
    w_in = rng.normal(size=(Nx, Ny)) + 1j * rng.normal(size=(Nx, Ny))
    T32 = T64.astype(np.float32).astype(np.float64)
    w0 = orc.set_wave(AMP * w_in.astype(np.complex64).astype(np.complex128), T32, DL, BL, E)
    refs = [orc.wave_propagation(w0, z, E, MAG, (Nx, Ny), PIX) for z in ZS[:nz]]
    for a in (T64, w_in, *refs):
        a.setflags(write=False)
    return T64, w_in, refs


def check(ops, shape, nd, nz, queue=False):
    Nx, Ny = shape
    T64, w_in, refs = case(shape, nz)
    zs = ZS[:nd]
    k = orc.k_sample(E)
    m = ops.MaterialStack(dev(T64, torch.float32), cphase=-k * DL, catt=-k * BL)
    kk = orc.getk(E * 1000)
    du = (2 * np.pi / (Nx * PIX * 1e-6), 2 * np.pi / (Ny * PIX * 1e-6))
    plan = ops.FresnelPlan(Nx, Ny, max_dist=nd, engine=2)
    assert plan.engine == 2
    if queue:
        plan.work_queue(True)
    inten = [torch.zeros((Nx, Ny), dtype=torch.float32, device="cuda") for _ in zs]
    outs = plan.propagate([z / (2 * kk * MAG) for z in zs], [kk * z / MAG for z in zs], du, wave_in=dev(w_in, torch.complex64),
                          amp=AMP, mats=m, inten_out=inten)
    for z, o, it, ref in zip(zs, outs, inten, refs):
        ew, ei = relmax(o.cpu().numpy(), ref), relmax(it.cpu().numpy(), np.abs(ref) ** 2)
        print("shape %s nd %d queue %d z %.1f: field %.2e intensity %.2e" % (shape, nd, queue, z, ew, ei))
        assert ew < TOL, (shape, nd, z)
        assert ei < TOL, (shape, nd, z)
    plan.close()


@pytest.mark.parametrize("nd", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_radix_in_either_pass(ops, shape, nd):
    """R1 = 4, 8, 16, 32 as pass 1 (one distance: plain rounds; several: DUAL rounds, an odd count leaves a pair half empty) and
    as pass 2."""
    check(ops, shape, nd, 4)


def test_work_queue_forms(ops):
    """The QUEUE instantiations read the same table."""
    check(ops, (4096, 24), 4, 4, queue=True)


@pytest.mark.parametrize("shape,nd", [((16384, 24), 1), ((24, 16384), 3)])
def test_two_round_kernel(ops, shape, nd):
    """fresnel_p2x.hip: the (bin, bin + M) pairs of both rounds, both halves of a slab's pairs."""
    check(ops, shape, nd, nd)
