"""Pass 1 of the LDS Fresnel engine with several distances (DUAL rounds of k_fresnel_p2, csrc/fresnel_p2.hip): the first pair of
distances of a line group transforms the line forward, the loader waves keep the line after forward stage A in registers and
the later pairs start from that snapshot.

The grids are the smallest that still take those rounds on the device at hand: a workgroup runs the pairs of a line group in
consecutive rounds only when the groups alone occupy every CU, so the line count is CU count x lines per round + 1 (one more
group than CUs, the last one not full where a round holds several lines).  One grid per radix R1 = 32, 16, 8, 4, one with 5
wrapped outputs per line and one with none (and a zero fill behind the samples).

Every call of n distances is held to
  1. the same plan called with at most two distances at a time -- calls that never take a snapshot (one pair per line group; a
     single distance runs the plain rounds): every output bit for bit;
  2. the float64 oracle, whole complex fields and intensity images, norm and tolerance of
     test_gpu_kernels.py::test_fresnel_power_of_two_lines_and_wrapped_outputs.
White complex noise in: one misplaced point of a restored line shows at about 1e-3 of the peak.  All distances differ."""
import functools

import numpy as np
import pytest
import torch

from oracle import paresis_oracle as orc
from tests._golden import relmax

pytestmark = pytest.mark.gpu

TOL = 1e-5
ZS = (0.4, 2.3, 5.2, 7.2, 1.1, 3.6, 6.1, 0.9)
E, PIX, MAG, AMP = 52.0, 2.9, 1.03, 1.25
DL, BL = np.array([6.2e-7, 9.9e-8]), np.array([4e-9, 4.5e-11])

# (samples of a pass-1 line, image lines per DUAL round): R1 = 32, 16, 8, 4; 5 wrapped outputs; none (2 N + 29 < 1024)
LINES = {4096: 1, 2048: 2, 1024: 4, 512: 8, 500: 8, 497: 8}
RADIX_LINES = (4096, 2048, 1024, 512)


@pytest.fixture(scope="module")
def ops():
    from paresis_amd import ops as _ops
    from paresis_amd._lib import lib
    assert lib().psx_device_ok() == 1, lib().psx_last_error()
    return _ops


def shape_of(nx):
    """One more line group than the device has CUs, the last one a single line."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return nx, cus * LINES[nx] + 1


def dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()      # a copy: the shared inputs are read-only


@functools.lru_cache(maxsize=None)
def inputs(shape):
    Nx, Ny = shape
    rng = np.random.default_rng(23 + Nx + 3 * Ny)
    T64 = rng.uniform(0.0, 3e-5, size=(2, Nx, Ny))
    w_in = rng.normal(size=(Nx, Ny)) + 1j * rng.normal(size=(Nx, Ny))
    T32 = T64.astype(np.float32).astype(np.float64)
    w0 = orc.set_wave(AMP * w_in.astype(np.complex64).astype(np.complex128), T32, DL, BL, E)
    for a in (T64, w_in, w0):
        a.setflags(write=False)
    return T64, w_in, w0


@functools.lru_cache(maxsize=None)
def reference(shape, z):
    """The oracle's field at one distance (computed once, shared by the cases, read only)."""
    ref = orc.wave_propagation(inputs(shape)[2], z, E, MAG, shape, PIX)
    ref.setflags(write=False)
    return ref


def check(ops, nx, nd, queue=False, want_wave=True, want_inten=True, add=False):
    shape = Nx, Ny = shape_of(nx)
    T64, w_in, _ = inputs(shape)
    zs = ZS[:nd]
    k = orc.k_sample(E)
    m = ops.MaterialStack(dev(T64, torch.float32), cphase=-k * DL, catt=-k * BL)
    kk = orc.getk(E * 1000)
    du = (2 * np.pi / (Nx * PIX * 1e-6), 2 * np.pi / (Ny * PIX * 1e-6))
    plan = ops.FresnelPlan(Nx, Ny, max_dist=nd, engine=2)
    assert plan.engine == 2
    if queue:
        plan.work_queue(True)
    w = dev(w_in, torch.complex64)
    base = torch.full((Nx, Ny), 0.75 if add else 0.0, dtype=torch.float32, device="cuda")

    def call(idx):
        inten = [base.clone() for _ in idx] if want_inten else None
        outs = plan.propagate([zs[i] / (2 * kk * MAG) for i in idx], [kk * zs[i] / MAG for i in idx], du, wave_in=w, amp=AMP, mats=m,
                              want_wave=[want_wave] * len(idx), inten_out=inten, add=add)
        return outs, inten if want_inten else [None] * len(idx)

    outs, inten = call(list(range(nd)))
    for first in range(0, nd, 2):
        idx = list(range(first, min(first + 2, nd)))
        o2, i2 = call(idx)
        for i, o, it in zip(idx, o2, i2):
            if want_wave:
                assert torch.equal(outs[i], o), (shape, nd, i, "field differs from the call of distances %s" % idx)
            if want_inten:
                assert torch.equal(inten[i], it), (shape, nd, i, "intensity differs from the call of distances %s" % idx)
    for i, z in enumerate(zs):
        ref = reference(shape, z)
        ew = relmax(outs[i].cpu().numpy(), ref) if want_wave else 0.0
        ei = relmax(inten[i].cpu().numpy() - (0.75 if add else 0.0), np.abs(ref) ** 2) if want_inten else 0.0
        print("shape %s nd %d queue %d z %.1f: field %.2e intensity %.2e" % (shape, nd, queue, z, ew, ei))
        assert ew < TOL, (shape, nd, z)
        assert ei < TOL, (shape, nd, z)
    plan.close()


@pytest.mark.parametrize("nd", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("nx", sorted(LINES, reverse=True))
def test_later_pairs_start_from_the_snapshot(ops, nx, nd):
    """2 distances: one pair, no snapshot.  3 and 5: the last pair's second result is dropped.  5 and 8: the snapshot is written
    back more than once."""
    check(ops, nx, nd)


@pytest.mark.parametrize("nd", [3, 8])
@pytest.mark.parametrize("nx", RADIX_LINES)
def test_work_queue_rounds(ops, nx, nd):
    """The QUEUE instantiations: units are claimed in a line group's first round only."""
    check(ops, nx, nd, queue=True)


@pytest.mark.parametrize("nx", RADIX_LINES)
def test_fields_alone(ops, nx):
    check(ops, nx, 5, want_inten=False)


@pytest.mark.parametrize("nx", RADIX_LINES)
def test_intensities_added_to_an_image(ops, nx):
    """add=True: the intensity of every distance is added to what its image holds (0.75 everywhere)."""
    check(ops, nx, 4, want_wave=False, add=True)
