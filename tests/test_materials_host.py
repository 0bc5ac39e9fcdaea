"""CPU: the float64 references, the test stacks and the derived bounds of tests/_materials_oracle.py, checked without a GPU.

- every map of every stack the GPU file uses matters: a map dropped, two coefficients swapped or the pad map T[0] given a
  second helping moves the reference by more than 100 tolerances (no exceptions);
- a CORRECT kernel fits the bounds: a numpy float32 emulation of each kernel's operation order, with every hardware
  function pushed to the error the derivation grants it, stays inside on every generated stack;
- the bounds have teeth: four wrong kernels break them.

The emulation's float64 sums are a product and an add where the device has one fma: 2^-53 of a term apart, 2^-29 of the
float32 roundings the bounds are made of."""
import numpy as np
import pytest

from tests import _materials_oracle as mo

F = np.float32
LOG2E = 1.4426950408889634
INV_TWO_PI = 0.15915494309189533576888376337251


@pytest.fixture(scope="module")
def stacks():
    return [mo.thin(st) for st in mo.gpu_stacks()]


def _within_one_ulp(y64, rng):
    """A float32 neighbour of y64 picked at random: what a '1 ulp' function may return."""
    r = y64.astype(F)
    lo = np.where(r.astype(np.float64) <= y64, r, np.nextafter(r, F(-np.inf)))
    hi = np.where(r.astype(np.float64) <= y64, np.nextafter(r, F(np.inf)), r)
    return np.where(rng.integers(0, 2, y64.shape) == 1, hi, lo).astype(F)


def _expf(x32, rng):
    with np.errstate(under="ignore"):
        return _within_one_ulp(np.exp(x32.astype(np.float64)), rng)


def _exp_att(la, rng):
    with np.errstate(under="ignore"):
        return _within_one_ulp(np.exp2((la * LOG2E).astype(F).astype(np.float64)), rng)        # common.hpp exp_att


def _cis(ph, rng):
    """common.hpp cis_f64 with v_sin_f32 / v_cos_f32 at their measured 1.25e-7, sign at random."""
    t = ph * INV_TWO_PI
    rev = (t - np.rint(t)).astype(F).astype(np.float64)
    e = lambda: F(1.25e-7) * rng.choice(np.array([-1, 1], dtype=F), ph.shape)
    return np.cos(2 * np.pi * rev).astype(F) + e(), np.sin(2 * np.pi * rev).astype(F) + e()


def _sums(st, wrong=None):
    """(ph, la) as mats_eval forms them; `wrong`: 'ph32' / 'la32' (the sum in float32), 'drop' (the last map left out),
    'pad' (the pad slot, T[0], under map 0's coefficients)."""
    cp, ca = list(st.cphase), list(st.catt)
    T = [st.T[i] for i in range(st.n)]
    if wrong == "drop":
        cp[-1], ca[-1] = 0.0, 0.0
    if wrong == "pad":
        T, cp, ca = T + [st.T[0]], cp + [st.cphase[0]], ca + [st.catt[0]]
    ph, la = np.zeros(st.shape), np.zeros(st.shape)
    ph32, la32 = np.zeros(st.shape, F), np.zeros(st.shape, F)
    for t, p, a in zip(T, cp, ca):
        ph = ph + p * t.astype(np.float64)
        la = la + a * t.astype(np.float64)
        ph32 = ph32 + F(p) * t
        la32 = la32 + F(a) * t
    return (ph32.astype(np.float64) if wrong == "ph32" else ph), (la32.astype(np.float64) if wrong == "la32" else la)


def _emulate(st, rng, wrong=None):
    """Margins (err / bound) of an emulated k_transmit_wave, k_transmit_rt and k_accumulate on st: {quantity: margin}."""
    shape = st.shape
    amp, I0, scale = 1.37, 0.83, 1.21
    w_in = (rng.uniform(0.5, 1.5, shape) + 1j * rng.uniform(-1, 1, shape)).astype(np.complex64)
    I_in, img, acc0 = (rng.uniform(0.5, 2.0, shape).astype(F) for _ in range(3))
    phi_in = rng.uniform(-50, 50, shape)
    ph, la = _sums(st, wrong)
    out = {}
    # k_transmit_wave (transmit.hip): a = amp * exp_att(la); o = a * (w * cis)
    c, s = _cis(ph, rng)
    a = F(amp) * _exp_att(la, rng)
    wx, wy = w_in.real, w_in.imag
    o = (a * (wx * c - wy * s)).astype(np.float64) + 1j * (a * (wx * s + wy * c)).astype(np.float64)
    ref, rla = mo.ref_wave(st, amp, w_in)
    out["wave"] = mo.margin(np.abs(o - ref), mo.bound_wave(rla, ref))
    # k_transmit_rt: I0 * Iin * expf((float)la);  phin + ph
    I = (F(I0) * I_in) * _expf(la.astype(F), rng)
    rI, rphi, _ = mo.ref_rt(st, I0, I_in, phi_in)
    out["I"] = mo.margin(np.abs(I.astype(np.float64) - rI), mo.bound_intensity(rla, rI))
    out["phi"] = mo.margin(np.abs(((phi_in + ph) - rphi).astype(np.float64)), mo.bound_phi(st, phi_in))
    # k_accumulate: v = scale * img; v *= expf((float)la); acc + v
    v = (F(scale) * img) * _expf(la.astype(F), rng)
    racc, bacc, _ = mo.ref_accumulate([st], [img], [scale], acc0)
    out["acc"] = mo.margin(np.abs((acc0 + v).astype(np.float64) - racc), bacc)
    rsto, bsto, _ = mo.ref_accumulate([st], [img], [scale], None)
    out["store"] = mo.margin(np.abs(v.astype(np.float64) - rsto), bsto)
    return out


def test_every_map_of_every_gpu_stack_matters(stacks):
    exceptions = []
    for st in stacks:
        for label, changes in mo.how_much_each_map_matters(st).items():
            if min(changes) <= mo.MATTERS:
                exceptions.append((st.name, label, changes))
    assert not exceptions, exceptions


@pytest.mark.parametrize("nmat", [5, 6, 7, 8])
def test_every_map_of_the_split_membrane_matters(nmat):
    st = mo.membrane_split(nmat)[0]
    for label, changes in mo.how_much_each_map_matters(st).items():
        assert min(changes) > mo.MATTERS, (label, changes)


def test_the_stacks_are_what_they_claim():
    for nmat in mo.RANGE_NMAT:
        for phase in mo.RANGE_PHASE:
            st = mo.range_stack(nmat, phase)
            ph, la = mo.exponents(st)
            assert abs(np.min(ph) + phase) <= 1e-9 * phase and abs(np.min(la) - mo.RANGE_LA) < 1e-9
            assert np.max(la) > -8.0 and np.sum(la < -40) > 100                # spread over 0 ... -80
            assert np.exp(np.min(la)) * 0.25 > mo.TINY32                       # the dimmest result stays a normal float32
    assert abs(np.min(mo.exponents(mo.opaque_stack())[1]) + 200.0) < 1e-9
    for st in mo.gpu_stacks():
        if st.n > 1:
            assert len(set(st.cphase)) == st.n and len(set(st.catt)) == st.n, st.name


def test_a_correct_kernel_fits_the_bounds(stacks):
    rng = np.random.default_rng(5)
    worst = {}
    for st in stacks:
        if st.name == "opaque":                                               # results below the normal range: not pinned
            continue
        for q, m in _emulate(st, rng).items():
            worst[q] = max(worst.get(q, 0.0), m)
            assert m <= 1.0, (st.name, q, m)
    print("emulated kernels, worst err / bound:", {q: round(m, 3) for q, m in worst.items()})


def test_the_bounds_have_teeth():
    rng = np.random.default_rng(6)
    # the phase summed in float32 at 1e4 rad: 1e4 * u rad per rounding against 7e-7
    for nmat in mo.RANGE_NMAT:
        assert _emulate(mo.range_stack(nmat, 1e4), rng, "ph32")["wave"] > 1.0, nmat
    # the log-attenuation summed in float32 at -80: products and partial sums of up to 64 u each against (80 + 4) u in all
    m = _emulate(mo.range_stack(7, 5.0), rng, "la32")
    assert m["I"] > 1.0 and m["store"] > 1.0 and m["wave"] > 1.0, m
    # a table gone wrong: the last map dropped, the pad slot under map 0's coefficients
    for st in mo.gpu_stacks():
        if st.n == 0 or st.name == "opaque":
            continue
        st = mo.thin(st)
        for wrong in ("drop", "pad"):
            m = _emulate(st, rng, wrong)
            assert min(m["wave"], m["I"], m["phi"], m["store"]) > mo.MATTERS, (st.name, wrong, m)
