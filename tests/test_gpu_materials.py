"""GPU: every consumer of the material stack against the plain float64 references of tests/_materials_oracle.py, per pixel
and against DERIVED bounds (their derivation is in that module's docstring; tests/test_materials_host.py checks them on the
CPU): every map count 0 ... 8 (5, 6 and 7 run the NM = 8 kernels on pack_mats' padding), phases up to 1e6 rad,
log-attenuations down to -80 (and -200), the sizes at which the elementwise skeletons change path, unaligned maps, and
psx_status_scan_f32.  Fresnel outputs at z != 0 follow the suite's rule: max|out - ref| / max|ref| < 1e-5 against
orc.wave_propagation of the reference wave.

Run with -s: each test prints the worst err / bound it met (1.0 = at the bound)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import paresis_oracle as orc
from paresis_amd import _lib
from tests import _materials_oracle as mo
from tests._golden import relmax
from tests._profile import profile_counts

pytestmark = pytest.mark.gpu

TOL = 1e-5
E_KEV, PIX_UM, MAG = 52.0, 2.9, 1.02
ENGINES = (_lib.ENGINE_ROCFFT, _lib.ENGINE_LDS)
_DEV_STACKS = {}


@pytest.fixture(scope="module")
def ops():
    from paresis_amd import ops as _ops
    from paresis_amd._lib import lib
    assert lib().psx_device_ok() == 1, lib().psx_last_error()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def shifted(a, off):
    """a on the device, starting `off` elements into its buffer: off = 1 ... 3 floats break the 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off * buf.element_size()
    return v


def images2d(st):
    """A 1-D stack's pixels as one image row (a MaterialStack holds 2-D maps)."""
    return (1,) + st.shape if len(st.shape) == 1 else st.shape


def gstack(ops, st, offsets=None):
    """The device MaterialStack of st (None for no maps); offsets: every map cut from its own buffer at that float offset,
    the stack assembled through MaterialStack.concat of single-map stacks."""
    if st.n == 0:
        return None
    key = (st.name, offsets)
    if key not in _DEV_STACKS:
        shape = images2d(st)
        if offsets is None:
            m = ops.MaterialStack(dev(st.T.reshape((st.n,) + shape)), cphase=st.cphase, catt=st.catt)
        else:
            m = ops.MaterialStack.concat(*[ops.MaterialStack(shifted(st.T[i].reshape(shape), offsets[i % len(offsets)])[None],
                                                             cphase=[st.cphase[i]], catt=[st.catt[i]]) for i in range(st.n)])
            assert any(m.map(i).data_ptr() % 16 for i in range(st.n))
        _DEV_STACKS[key] = m
    return _DEV_STACKS[key]


def scaled(st, s):
    """st under the coefficients of another energy (a source's or an image's own)."""
    return st.with_coeffs([c * s for c in st.cphase], [c * s for c in st.catt])


def gscaled(m, s):
    return None if m is None else m.with_coeffs([c * s for c in m.cphase], [c * s for c in m.catt])


def report(what, m):
    print("materials: %-44s worst err/bound %.3f" % (what, m))
    assert m <= 1.0, (what, m)


@functools.lru_cache(maxsize=4)
def inputs(shape, seed):
    """(wave, I, img, acc, phi) of a test, shared by its checks: read-only."""
    rng = np.random.default_rng(seed)
    w = (rng.uniform(0.5, 1.5, shape) + 1j * rng.uniform(-1, 1, shape)).astype(np.complex64)
    I, img, acc = (rng.uniform(0.5, 2.0, shape).astype(np.float32) for _ in range(3))
    phi = rng.uniform(-50, 50, shape)
    return w, I, img, acc, phi


def fresnel_scalars(shape, z):
    kk = orc.getk(E_KEV * 1000)
    du = (2 * np.pi / (shape[0] * PIX_UM * 1e-6), 2 * np.pi / (shape[1] * PIX_UM * 1e-6))
    return z / (2 * kk * MAG), kk * z / MAG, du


# ----------------------------------------------------------------------------------- the checks, one per consumer
def check_transmit_wave(ops, st, m, seed, w_off=0):
    shape = images2d(st)
    w_in = inputs(shape, seed)[0]
    worst = 0.0
    for wi in ([w_in, None] if st.n else [w_in]):                              # no maps and no wave: nothing gives the shape
        ref, la = mo.ref_wave(st, 1.37, None if wi is None else wi.reshape(st.shape))
        d = None if wi is None else (shifted(wi, w_off) if w_off else dev(wi))
        out = ops.transmit_wave(d, 1.37, m)
        worst = max(worst, mo.margin(np.abs(host(out).reshape(st.shape) - ref), mo.bound_wave(la, ref)))
        if d is not None:                                                      # in place: the same kernel, the same bits
            w = d.clone()
            assert ops.transmit_wave(w, 1.37, m, out=w) is w and torch.equal(w, out)
    return worst


def check_transmit_rt(ops, st, m, seed, off=0):
    shape = images2d(st)
    _, I_in, _, _, phi_in = inputs(shape, seed)
    worst_I = worst_phi = 0.0
    for use_I in (True, False):
        for use_phi in (True, False):
            for want_phi in (True, False):
                ref_I, ref_phi, la = mo.ref_rt(st, 0.83, I_in.reshape(st.shape) if use_I else None,
                                               phi_in.reshape(st.shape) if use_phi else None)
                dI = (shifted(I_in, off) if off else dev(I_in)) if use_I else None
                out = None if (use_I or st.n) else torch.empty(shape, dtype=torch.float32, device="cuda")
                I, phi = ops.transmit_rt(dI, 0.83, m, phi_in=dev(phi_in) if use_phi else None, want_phi=want_phi, out=out)
                assert (phi is not None) == want_phi
                worst_I = max(worst_I, mo.margin(np.abs(host(I).reshape(st.shape) - ref_I), mo.bound_intensity(la, ref_I)))
                if want_phi:
                    err = np.abs(host(phi).reshape(st.shape).astype(np.longdouble) - ref_phi).astype(np.float64)
                    worst_phi = max(worst_phi, mo.margin(err, mo.bound_phi(st, phi_in.reshape(st.shape) if use_phi else None)))
    return worst_I, worst_phi


def check_sums(ops, sums, acc, weight, calls=1):
    """The reduction alone, independent of expf: sums[0] against the float64 sum of the GPU's own image, sums[1] = weight
    times that; `calls` identical calls into one buffer add up."""
    s = host(ops.fold_sums(sums))
    own = calls * float(np.sum(host(acc).astype(np.float64)))
    assert abs(s[0] - own) <= 1e-12 * abs(own), (s[0], own)
    assert abs(s[1] - f64(weight) * s[0]) <= 1e-12 * abs(s[1]), (s, weight)


def f64(x):
    return float(ctypes.c_double(x).value)


def check_accumulate(ops, st, m, seed, off=0):
    """k_accumulate and k_accumulate_sum: add on and off, acc=None; returns (worst accumulate, worst accumulate_sum)."""
    shape = images2d(st)
    _, _, img, acc0, _ = inputs(shape, seed)
    put = (lambda a: shifted(a, off)) if off else dev
    dimg = put(img)
    worst, worst_s = 0.0, 0.0
    for add in (False, True):
        ref, bound, terms = mo.ref_accumulate([st], [img.reshape(st.shape)], [1.21], acc0.reshape(st.shape) if add else None)
        acc = put(acc0)
        assert ops.accumulate(acc, dimg, 1.21, m, add=add) is acc
        worst = max(worst, mo.margin(np.abs(host(acc).reshape(st.shape) - ref), bound))
        acc, sums = put(acc0), ops.new_sums(dimg.device)
        ops.accumulate_sum(acc, dimg, sums, 24.5, scale=1.21, mats=m, add=add)
        worst_s = max(worst_s, mo.margin(np.abs(host(acc).reshape(st.shape) - ref), bound))
        if not add:
            check_sums(ops, sums, acc, 24.5)
            ops.accumulate_sum(acc, dimg, sums, 24.5, scale=1.21, mats=m, add=False)
            check_sums(ops, sums, acc, 24.5, calls=2)
            only = ops.new_sums(dimg.device)                                  # acc=None: the reduction without the image
            ops.accumulate_sum(None, dimg, only, 24.5, scale=1.21, mats=m)
            check_sums(ops, only, acc, 24.5)
    return worst, worst_s


def check_accumulate_many(ops, st, m, seed, counts, off=0):
    """k_accumulate_many with `counts` images, each under its own coefficients: per pixel against the reference, bit for bit the
    chain of accumulate_sum calls, the sums to rounding, and acc=None."""
    shape = images2d(st)
    rng = np.random.default_rng(seed)
    put = (lambda a: shifted(a, off)) if off else dev
    acc0 = rng.uniform(0.5, 2.0, shape).astype(np.float32)
    worst = 0.0
    for ne in counts:
        imgs = [rng.uniform(0.5, 2.0, shape).astype(np.float32) for _ in range(ne)]
        dimgs = [put(a) for a in imgs]
        scales = [1.0 + 0.1 * e for e in range(ne)]
        weights = [20.0 + 2 * e for e in range(ne)]
        sts = [scaled(st, mo.SOURCE_SCALE[e % 3]) for e in range(ne)]
        mats = None if m is None else [gscaled(m, mo.SOURCE_SCALE[e % 3]) for e in range(ne)]
        for add in (False, True):
            ref, bound, terms = mo.ref_accumulate(sts, [a.reshape(st.shape) for a in imgs], scales,
                                                  acc0.reshape(st.shape) if add else None)
            a1, a2 = put(acc0), put(acc0)
            s1, s2, s3 = (ops.new_sums(a1.device) for _ in range(3))
            ops.accumulate_many(a2, dimgs, s2, weights, scales=scales, mats=mats, add=add)
            worst = max(worst, mo.margin(np.abs(host(a2).reshape(st.shape) - ref), bound))
            for e in range(ne):
                ops.accumulate_sum(a1, dimgs[e], s1, weights[e], scale=scales[e], mats=None if mats is None else mats[e],
                                   add=add or e > 0)
            assert torch.equal(a1, a2), (st.name, ne, add)
            ops.accumulate_many(None, dimgs, s3, weights, scales=scales, mats=mats, add=add)
            f1, f2, f3 = (host(ops.fold_sums(s)) for s in (s1, s2, s3))
            assert np.allclose(f1, f2, rtol=1e-12, atol=0) and np.allclose(f3, f2, rtol=1e-12, atol=0), (f1, f2, f3)
            # against the reference: every term within its (|la| + 4) u |v| (nothing is added to an image here)
            slack = sum(float(np.sum(mo.bound_intensity(mo.exponents(s)[1] if s.n else 0.0, v) - mo.U * np.abs(v)))
                        for s, v in zip(sts, terms))
            want = (sum(float(np.sum(v)) for v in terms), sum(w * float(np.sum(v)) for w, v in zip(weights, terms)))
            assert abs(f2[0] - want[0]) <= slack + 1e-12 * want[0] and abs(f2[1] - want[1]) <= max(weights) * slack + 1e-12 * want[1]
    return worst


def check_propagate(ops, st, m, seed, engine, with_wave):
    """FresnelPlan.propagate over [z, 0, z']: the z = 0 output per pixel (k_pad_transmit / k_source_out), the others by the
    suite's rule (k_pad_transmit / k_source_transposed, both tile paths on a grid with Ny % 4 == 0)."""
    shape = st.shape
    w_in = inputs(shape, seed)[0] if with_wave else None
    plan = ops.FresnelPlan(shape[0], shape[1], engine=engine)
    assert plan.engine == engine
    zs = [1.6, 0.0, 0.45]
    sc = [fresnel_scalars(shape, z) for z in zs]
    inten = [torch.full(shape, 0.5, dtype=torch.float32, device="cuda") for _ in zs]
    outs = plan.propagate([s[0] for s in sc], [s[1] for s in sc], sc[0][2], wave_in=None if w_in is None else dev(w_in), amp=1.37,
                          mats=m, inten_out=inten, inten_scale=[1.0, 2.0, 0.5], add=True)
    ref0, la = mo.ref_wave(st, 1.37, w_in)
    worst = mo.margin(np.abs(host(outs[1]) - ref0), mo.bound_wave(la, ref0))
    for z, o, it, isc in zip(zs, outs, inten, [1.0, 2.0, 0.5]):
        ref = orc.wave_propagation(ref0, z, E_KEV, MAG, shape, PIX_UM)
        assert relmax(host(o), ref) < TOL, (st.name, engine, z)
        assert relmax(host(it), 0.5 + isc * np.abs(ref) ** 2) < TOL, (st.name, engine, z)
    plan.close()
    return worst


def check_propagate_sources(ops, st, m, seed):
    """3 sources x 2 distances on the LDS engine, each source under its own coefficients: ONE batched pre-pass (the profile
    counts it), bit for bit one propagate call per source, and the suite's rule against the oracle."""
    shape = st.shape
    ns, nd = 3, 2
    w = inputs(shape, seed)[0]
    waves = [None, w, None]
    dw = [None if a is None else dev(a) for a in waves]
    amp = [1.0 + 0.25 * s for s in range(ns)]
    zs = [[0.8 + 0.5 * s + 1.1 * d for d in range(nd)] for s in range(ns)]
    sc = [[fresnel_scalars(shape, z) for z in r] for r in zs]
    a, gph, du = [[c[0] for c in r] for r in sc], [[c[1] for c in r] for r in sc], sc[0][0][2]
    scale = [[0.5 + s + d for d in range(nd)] for s in range(ns)]
    mats = None if m is None else [gscaled(m, mo.SOURCE_SCALE[s]) for s in range(ns)]
    plan = ops.FresnelPlan(shape[0], shape[1], max_dist=nd, engine=_lib.ENGINE_LDS)
    assert plan.engine == _lib.ENGINE_LDS
    io = [[torch.empty(shape, device="cuda") for _ in range(nd)] for _ in range(ns)]
    got = []
    counts = profile_counts(lambda: got.append(plan.propagate_sources(a, gph, du, wave_in=dw, amp=amp, mats=mats, inten_out=io,
                                                                      inten_scale=scale)))
    assert counts.get("k_source_transposed") == 1, ("the three sources did not take the batched pre-pass", st.name, counts)
    got = got[0]
    for s in range(ns):
        io1 = [torch.empty(shape, device="cuda") for _ in range(nd)]
        one = plan.propagate(a[s], gph[s], du, wave_in=dw[s], amp=amp[s], mats=None if mats is None else mats[s],
                             inten_out=io1, inten_scale=scale[s])
        ref0, _ = mo.ref_wave(scaled(st, mo.SOURCE_SCALE[s]), amp[s], waves[s])
        for d in range(nd):
            assert torch.equal(got[s][d], one[d]) and torch.equal(io[s][d], io1[d]), (st.name, s, d)
            ref = orc.wave_propagation(ref0, zs[s][d], E_KEV, MAG, shape, PIX_UM)
            assert relmax(host(got[s][d]), ref) < TOL, (st.name, s, d)
            assert relmax(host(io[s][d]), scale[s][d] * np.abs(ref) ** 2) < TOL, (st.name, s, d)
    plan.close()


# ------------------------------------------------------------------------------- a. every count, every consumer
@pytest.mark.parametrize("nmat", range(0, 9))
def test_transmit_every_count(ops, nmat):
    for shape in mo.GRIDS:
        st = mo.count_stack(nmat, shape)
        m = gstack(ops, st)
        report("k_transmit_wave %d maps %dx%d" % ((nmat,) + shape), check_transmit_wave(ops, st, m, nmat))
        wI, wphi = check_transmit_rt(ops, st, m, nmat)
        report("k_transmit_rt I %d maps %dx%d" % ((nmat,) + shape), wI)
        report("k_transmit_rt phi %d maps %dx%d" % ((nmat,) + shape), wphi)


@pytest.mark.parametrize("nmat", range(0, 9))
def test_accumulate_every_count(ops, nmat):
    for shape in mo.GRIDS:
        st = mo.count_stack(nmat, shape)
        m = gstack(ops, st)
        wa, ws = check_accumulate(ops, st, m, nmat)
        report("k_accumulate %d maps %dx%d" % ((nmat,) + shape), wa)
        report("k_accumulate_sum %d maps %dx%d" % ((nmat,) + shape), ws)
        report("k_accumulate_many %d maps %dx%d" % ((nmat,) + shape),
               check_accumulate_many(ops, st, m, nmat, (1, 3, _lib.PSX_MAX_SRC + 1)))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("nmat", range(0, 9))
def test_fresnel_fused_load_every_count(ops, nmat, engine):
    for shape in mo.GRIDS:
        st = mo.count_stack(nmat, shape)
        m = gstack(ops, st)
        for with_wave in (False, True):
            report("%s %d maps %dx%d wave_in=%d" % (("k_pad_transmit" if engine == _lib.ENGINE_ROCFFT else "k_source_out", nmat) + shape
                                                   + (with_wave,)), check_propagate(ops, st, m, nmat, engine, with_wave))


@pytest.mark.parametrize("nmat", range(0, 9))
def test_propagate_sources_every_count(ops, nmat):
    for shape in mo.GRIDS:
        st = mo.count_stack(nmat, shape)
        check_propagate_sources(ops, st, gstack(ops, st), nmat)


@pytest.mark.parametrize("nmat", [5, 6, 7, 8])
def test_refraction_every_entry_point_above_four_maps(ops, nmat):
    """refract, refract_multi, refract_split and refract_batch on the split membrane of test_refraction_more_than_four_maps
    against the oracle on the equivalent (I, phi)."""
    st, delta, beta, (z, E, M, pix) = mo.membrane_split(nmat)
    m = gstack(ops, st)
    N = st.shape
    geom = st.T.astype(np.float64)
    h = pix * 1e-6
    dscale = lambda zz: zz / orc.k_refraction(E) / (h * M) / h
    I_ref, phi_ref, _ = orc.set_wave_rt(np.full(N, 7500.0), geom, delta, beta, E, 0)
    zs = (z, 0.5 * z)
    refs = [orc.fast_refraction(I_ref.copy(), phi_ref.copy(), zz, E, M, pix)[0] for zz in zs]
    single = ops.refract(N, m, dscale(z), N, I0=7500.0)[0]
    assert relmax(host(single), refs[0]) < TOL
    for o, ref in zip(ops.refract_multi(N, m, [dscale(zz) for zz in zs], N, I0=7500.0), refs):
        assert relmax(host(o), ref) < TOL
    # the split: the sources under mask == 0 and the others, refracted apart
    mask = np.zeros(N, dtype=np.float32)
    mask[40:130, 60:170] = 1.0
    o0, o1 = ops.refract_split(N, m, dscale(z), N, dev(mask), I0=7500.0)
    for o, keep in ((o0, mask == 0), (o1, mask != 0)):
        ref = orc.fast_refraction(I_ref * keep, phi_ref.copy(), z, E, M, pix)[0]
        assert relmax(host(o), ref) < TOL
    # the batch: three refractions over the same maps, each under its own coefficients and distance
    ne = 3
    mats = [gscaled(m, mo.SOURCE_SCALE[e]) for e in range(ne)]
    outs = ops.refract_batch(N, mats, [dscale(z * (1 - 0.2 * e)) for e in range(ne)], N, I0=[7500.0 + 100 * e for e in range(ne)])
    for e in range(ne):
        s = mo.SOURCE_SCALE[e]
        I_e, phi_e, _ = orc.set_wave_rt(np.full(N, 7500.0 + 100 * e), geom, [d * s for d in delta], [b * s for b in beta], E, 0)
        ref = orc.fast_refraction(I_e, phi_e, z * (1 - 0.2 * e), E, M, pix)[0]
        assert relmax(host(outs[e]), ref) < TOL, e
    ops.check_status(single.device)


def test_unaligned_maps_through_concat(ops):
    """Three maps cut from 1-D buffers at float offsets 1, 2 and 3, assembled by MaterialStack.concat: every 16-byte path off."""
    st = mo.unaligned_stack()
    m = gstack(ops, st, offsets=(1, 2, 3))
    report("k_transmit_wave unaligned", check_transmit_wave(ops, st, m, 3, w_off=1))
    wI, wphi = check_transmit_rt(ops, st, m, 3, off=1)
    report("k_transmit_rt I unaligned", wI)
    report("k_transmit_rt phi unaligned", wphi)
    wa, ws = check_accumulate(ops, st, m, 3)
    report("k_accumulate unaligned maps", wa)
    report("k_accumulate_sum unaligned maps", ws)
    report("k_accumulate_many unaligned maps", check_accumulate_many(ops, st, m, 3, (3,)))
    for engine in ENGINES:
        report("fused load unaligned maps engine %d" % engine, check_propagate(ops, st, m, 3, engine, True))
    check_propagate_sources(ops, st, m, 3)


# ------------------------------------------------------------------------------------------------------ b. range
@pytest.mark.parametrize("phase", mo.RANGE_PHASE)
@pytest.mark.parametrize("nmat", mo.RANGE_NMAT)
def test_range_of_phase_and_attenuation(ops, nmat, phase):
    """Phase sums up to 5, 1e4 and 1e6 rad with log-attenuations over 0 ... -80, per pixel: the bound does not know the phase."""
    st = mo.range_stack(nmat, phase)
    m = gstack(ops, st)
    tag = "%d maps %g rad" % (nmat, phase)
    report("k_transmit_wave " + tag, check_transmit_wave(ops, st, m, 17))
    wI, wphi = check_transmit_rt(ops, st, m, 17)
    report("k_transmit_rt I " + tag, wI)
    report("k_transmit_rt phi " + tag, wphi)
    wa, ws = check_accumulate(ops, st, m, 17)
    report("k_accumulate " + tag, wa)
    report("k_accumulate_sum " + tag, ws)
    report("k_accumulate_many " + tag, check_accumulate_many(ops, st, m, 17, (3,)))
    for engine in ENGINES:
        report("%s %s" % ("k_pad_transmit" if engine == _lib.ENGINE_ROCFFT else "k_source_out", tag),
               check_propagate(ops, st, m, 17, engine, True))


def test_opaque_stack_stays_finite(ops):
    """la down to -200: exp(la) is far below float32.  Finite, no negative intensity, nothing above the reference by more than
    its bound plus the smallest normal float32; pixels whose result is a normal float32 keep the bound.  What v_exp_f32 gives
    between zero and the smallest normal is not pinned."""
    st = mo.opaque_stack()
    m = gstack(ops, st)
    w_in, I_in, img, _, _ = inputs(st.shape, 23)

    def judge(what, got, ref, bound, intensity):
        assert np.all(np.isfinite(got)), what
        if intensity:
            assert np.all(got >= 0), what
        assert np.all(np.abs(got) <= np.abs(ref) + bound + mo.TINY32), what
        normal = np.abs(ref) > 4 * mo.TINY32
        assert normal.any() and (~normal).any()
        report(what + " (normal pixels)", mo.margin(np.abs(got - ref)[normal], bound[normal]))

    ref, la = mo.ref_wave(st, 1.37, w_in)
    judge("k_transmit_wave opaque", host(ops.transmit_wave(dev(w_in), 1.37, m)), ref, mo.bound_wave(la, ref), False)
    rI, _, _ = mo.ref_rt(st, 0.83, I_in)
    judge("k_transmit_rt opaque", host(ops.transmit_rt(dev(I_in), 0.83, m, want_phi=False)[0]), rI, mo.bound_intensity(la, rI), True)
    racc, bacc, _ = mo.ref_accumulate([st], [img], [1.21], None)
    acc = torch.ones(st.shape, device="cuda")
    judge("k_accumulate opaque", host(ops.accumulate(acc, dev(img), 1.21, m, add=False)), racc, bacc, True)
    sums = ops.new_sums(acc.device)
    judge("k_accumulate_sum opaque", host(ops.accumulate_sum(acc, dev(img), sums, 2.0, scale=1.21, mats=m, add=False)), racc, bacc, True)
    assert np.all(np.isfinite(host(sums)))
    judge("k_accumulate_many opaque", host(ops.accumulate_many(acc, [dev(img)], sums, [2.0], scales=[1.21], mats=[m], add=False)),
          racc, bacc, True)
    for engine in ENGINES:
        plan = ops.FresnelPlan(st.shape[0], st.shape[1], engine=engine)
        out = plan.propagate([0.0], [0.0], fresnel_scalars(st.shape, 0.0)[2], wave_in=dev(w_in), amp=1.37, mats=m)[0]
        judge("fused load opaque engine %d" % engine, host(out), ref, mo.bound_wave(la, ref), False)
        plan.close()


# -------------------------------------------------------------------------------------- c. elementwise skeletons
@pytest.mark.parametrize("n", mo.SIZES)
def test_elementwise_sizes(ops, n):
    """One pixel, the 4-pixel vector edge, ragged tails, past k_accumulate_sum's 1024 x 256 x 4 pixels per trip and past
    ew_grid's 16384 blocks; aligned, and with the images and maps 1 ... 3 floats off the 16-byte alignment."""
    st = mo.size_stack(n)
    for off, offsets in ((0, None), (1, (1, 2, 3))):
        m = gstack(ops, st, offsets=offsets)
        tag = "n=%d %s" % (n, "aligned" if off == 0 else "misaligned")
        report("k_transmit_wave " + tag, check_transmit_wave(ops, st, m, n % 1000, w_off=off))
        _, I_in, _, _, phi_in = inputs(images2d(st), n % 1000)
        ref_I, ref_phi, la = mo.ref_rt(st, 0.83, I_in.reshape(st.shape), phi_in.reshape(st.shape))
        I, phi = ops.transmit_rt(shifted(I_in, off) if off else dev(I_in), 0.83, m, phi_in=dev(phi_in))
        report("k_transmit_rt I " + tag, mo.margin(np.abs(host(I).reshape(st.shape) - ref_I), mo.bound_intensity(la, ref_I)))
        report("k_transmit_rt phi " + tag, mo.margin(np.abs(host(phi).reshape(st.shape).astype(np.longdouble) - ref_phi).astype(np.float64),
                                                     mo.bound_phi(st, phi_in.reshape(st.shape))))
        wa, ws = check_accumulate(ops, st, m, n % 1000, off=off)
        report("k_accumulate " + tag, wa)
        report("k_accumulate_sum " + tag, ws)
        report("k_accumulate_many " + tag, check_accumulate_many(ops, st, m, n % 1000, (2,), off=off))
    _DEV_STACKS.clear()                                                       # the large stacks are of no use to a later test


# ------------------------------------------------------------------------------------------------ d. status scan
def test_status_scan(ops):
    from paresis_amd._lib import PsxError
    device = torch.device("cuda", torch.cuda.current_device())
    ops.check_status(device)
    sizes = (4 * 256 + 37, 16384 * 256 + 1029)                               # a ragged last block; a second, ragged grid-stride trip
    for n in sizes:
        tail = n - 20                                                         # inside the ragged tail
        base = torch.full((n,), 1.5, dtype=torch.float32, device="cuda")
        for bad in (float("nan"), float("inf"), float("-inf"), 3.1e38):
            for pos in (0, n // 2, n - 1, tail):
                img = base.clone()
                img[pos] = bad
                ops.status_scan(img)
                with pytest.raises(PsxError, match="nans or insane"):
                    ops.check_status(device, "status scan")
                assert int(ops.status_word(device).item()) == 0, "the status word is restored by the check"
            if n > 100000:
                break                                                         # the long image: NaN at every position is enough
        good = base.clone()
        for pos, v in ((0, 3.0e38), (n // 2, -3.0e38), (n - 1, 0.0), (tail, 1e-45), (tail + 1, -1e-40), (1, -0.0)):
            good[pos] = v
        ops.status_scan(good)
        ops.check_status(device, "status scan")
        assert int(ops.status_word(device).item()) == 0
