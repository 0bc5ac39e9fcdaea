"""The material stack's consumers in plain numpy float64, the test stacks, and DERIVED per-pixel error bounds.

A material stack is up to PSX_MAX_MAT float32 thickness maps T_i with a phase and an attenuation coefficient each.  Every
consumer forms the two exponents  ph = sum cphase_i T_i  and  la = sum catt_i T_i  per pixel and then one of

    wave = amp * w_in * exp(la) * exp(i ph)          k_transmit_wave, k_pad_transmit, k_source_out, k_source_transposed(_batch)
    I    = I0 * I_in * exp(la)                       k_transmit_rt, the refraction staging
    phi  = phi_in + ph                               k_transmit_rt (float64 on the device)
    acc (+)= scale * img * exp(la)                   k_accumulate, k_accumulate_sum, k_accumulate_many

The references below are fed the float32 maps, images and scalars the GPU gets, widened to float64 (phi: to long double,
whose 64-bit mantissa leaves the reference 2^-11 of the device's float64 rounding).

The bounds (u = 2^-24, the float32 unit roundoff; a float32 rounding is relative u, a "1 ulp" function relative 2u), each
term beside the code line it comes from.  They are derived, never fitted to what a GPU printed:

attenuation factor, relative (|la| + 2) u
    common.hpp  mats_eval:  la = fma(catt_i, (double)T_i, la)    float64: nmat * 2^-53 |la|, 2^-29 of the terms below
    transmit.hip            expf((float)la)                      (float)la: |la| u ABSOLUTE in the exponent = |la| u relative
    common.hpp  exp_att:    exp2f((float)(la * log2 e))          the product is float64; the rounding is |la| log2(e) u in the
                                                                 base-2 exponent = ln 2 * |la| log2(e) u = |la| u relative
    expf (OCML) / v_exp_f32: within 1 ulp                        2 u

intensity and accumulation, absolute (|la| + 4) u |v| + u |acc + v|,  v = scale * img * exp(la)
    transmit.hip  I0 * Iin * expf(..) ;  scale * img, v * expf(..)     two float32 products: 2 u on top of the factor's
    transmit.hip  acc[p] + v                                          the add rounds the total: u |acc + v| (a store of v
                                                                       alone rounds nothing more: the term is then slack)
    Several images (k_accumulate_many, or one call per image) repeat both terms per image, the add on the running total.

wave, |out - ref| <= |ref| [(|la| + 4) u + 7e-7]
    amplitude path: amp * exp_att(la), a * w           the factor, two products: (|la| + 4) u
    phasor path (common.hpp cis_f64):
        v_sin_f32 / v_cos_f32, max |error| 1.25e-7 each (measured, comment above cis_f64): sqrt 2 * 1.25e-7 = 1.77e-7 as a vector
        rev = (float)(t - rint t), |rev| <= 0.5: 0.5 u revolutions = 2 pi * 0.5 u = 1.9e-7 rad
        w.x*c - w.y*s, w.x*s + w.y*c: two products and a sum per component, each component <= u (|w| + |component|),
            as a vector (sqrt 2 + 1) u |w| = 1.44e-7 |w|   (contracted to fma: less)
        float64 phase sum and t = ph / 2 pi: nmat * 2^-53 |ph| rad, 1e-9 at 1e6 rad
    sum 5.1e-7, stated as 7e-7.  Nothing in the phasor path scales with ph: the reduction is float64.

phi, absolute  nmat * 2^-52 sum |cphase_i T_i| + 2^-52 |phi_in|
    mats_eval: nmat float64 fma roundings of partial sums <= sum |cphase_i T_i|; transmit.hip `phin[p] + ph`: one more of the
    total.  Each is 2^-53 of its operand; the bound carries a factor two.
"""
import os

import numpy as np

U = 2.0 ** -24
EPS64 = 2.0 ** -52
HW_PHASOR = 7e-7
TINY32 = float(np.finfo(np.float32).tiny)
MATTERS = 100.0                       # every map moves the reference by more than this many tolerances


# ------------------------------------------------------------------------------------------------------ stacks
class Stack:
    def __init__(self, name, T, cphase, catt):
        self.name, self.T = name, T
        self.cphase, self.catt = [float(v) for v in cphase], [float(v) for v in catt]
        self.n, self.shape = T.shape[0], tuple(T.shape[1:])
        self._exponents = {}                                                   # exponents() of this stack, by dtype

    def with_coeffs(self, cphase, catt):
        return Stack(self.name, self.T, cphase, catt)


def maps(nmat, shape, seed, pix=3e-6):
    """nmat smooth float32 thickness maps (sphere chords over a uniform support, metres; 0.1 mm in magnitude) as _maps() of
    tests/test_gpu_phantom.py makes them; a 1-D shape takes the chords of the same spheres along a line."""
    rng = np.random.default_rng(seed)
    out = np.zeros((nmat,) + tuple(shape))
    for m in range(nmat):
        c0, c1, R = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.25, 0.45)
        if len(shape) == 2:
            Nx, Ny = shape
            ii, jj = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
            Rp = R * min(Nx, Ny)
            out[m] = 2 * np.sqrt(np.maximum(Rp * Rp - (ii - c0 * Nx) ** 2 - (jj - c1 * Ny) ** 2, 0)) * pix
        else:
            n = shape[0]
            x = (np.arange(n) - c0 * n) / max(R * n, 1.0)
            out[m] = 1.2e-4 * np.sqrt(np.maximum(1 - x * x, 0))
        out[m] += rng.uniform(5e-6, 2e-5)                                    # a uniform support under every map
    return out.astype(np.float32)


def stack(name, nmat, shape, seed, phase_max=30.0, la_min=-2.0):
    """A stack whose phase sum reaches -phase_max rad and whose log-attenuation reaches la_min at its thickest pixel (and a few
    per cent of that on the bare support).  Each map its own coefficients: the weights are a shuffled ladder, no two closer
    than 0.8 / (nmat - 1) of 0.6 ... 1.4, phase and attenuation shuffled apart."""
    T = maps(nmat, shape, seed)
    if nmat == 0:
        return Stack(name, T, [], [])
    rng = np.random.default_rng(seed + 1000)
    T64 = T.astype(np.float64)
    ladder = np.linspace(0.6, 1.4, nmat) if nmat > 1 else np.array([1.0])
    rp, ra = rng.permutation(ladder), rng.permutation(ladder)
    cphase = -phase_max * rp / np.max(np.tensordot(rp, T64, axes=1))
    catt = la_min * ra / np.max(np.tensordot(ra, T64, axes=1))
    return Stack(name, T, cphase, catt)


def membrane_split(nmat):
    """The stack of test_refraction_more_than_four_maps: the golden membrane map tiled to 200 x 200 and split into nmat float32
    slices with their own delta / beta.  Returns (Stack, delta, beta, (z, E, M, pix))."""
    from oracle import paresis_oracle as orc
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refraction.npz"))
    z, E, M, pix = (float(v) for v in g["0/params"])
    T0 = g["0/T"]
    reps = (int(np.ceil(200 / T0.shape[0])), int(np.ceil(200 / T0.shape[1])))
    T = np.tile(T0, reps)[:200, :200].astype(np.float32)
    rng = np.random.default_rng(nmat)
    frac = rng.uniform(0.5, 1.5, nmat)
    geom = np.stack([(T * f).astype(np.float32) for f in frac])
    delta, beta = list(rng.uniform(1e-7, 6e-7, nmat)), list(rng.uniform(1e-10, 4e-9, nmat))
    kk = orc.k_sample(E)
    return (Stack("membrane%d" % nmat, geom, [-kk * d for d in delta], [-2 * kk * b for b in beta]), delta, beta,
            (z, E, M, pix))


GRIDS = [(131, 100), (67, 45)]        # Ny % 4 == 0: vector AND ragged 64 x 64 tiles;  no vector tile at all
RANGE_NMAT = (1, 4, 7)
RANGE_PHASE = (5.0, 1e4, 1e6)         # the goldens' reach; the physical ceiling; far beyond: the bound does not move
RANGE_LA = -80.0
SIZES = (1, 3, 4, 5, 1023, 4099, 1048576 + 3075, 4194304 + 1029)
SOURCE_SCALE = (1.0, 0.71, 0.53)      # coefficient scale of source / image e (an energy's own delta, beta): e % 3


def count_stack(nmat, shape):
    return stack("count%d_%dx%d" % ((nmat,) + tuple(shape)), nmat, shape, 100 * shape[0] + nmat)


def range_stack(nmat, phase):
    return stack("range%d_%g" % (nmat, phase), nmat, GRIDS[0], 7000 + nmat, phase_max=phase, la_min=RANGE_LA)


def size_stack(n):
    return stack("size%d" % n, 3 if n < 100000 else 2, (n,), 300 + n % 97)


def opaque_stack():
    return stack("opaque", 4, GRIDS[1], 41, la_min=-200.0)


def unaligned_stack():
    return stack("unaligned", 3, GRIDS[0], 53)


def gpu_stacks():
    """Every generated stack tests/test_gpu_materials.py uses (tests/test_materials_host.py walks them)."""
    for shape in GRIDS:
        for nmat in range(0, 9):
            yield count_stack(nmat, shape)
    for nmat in RANGE_NMAT:
        for phase in RANGE_PHASE:
            yield range_stack(nmat, phase)
    for n in SIZES:
        yield size_stack(n)
    yield opaque_stack()
    yield unaligned_stack()


# -------------------------------------------------------------------------------------------------- references
def f32(x):
    """The float32 a scalar argument becomes on its way through the C ABI, widened."""
    return float(np.float32(x))


def exponents(st, dtype=np.float64):
    """(ph, la) = (sum cphase_i T_i, sum catt_i T_i) in `dtype`, map after map as the kernels do."""
    if dtype not in st._exponents:
        ph, la = np.zeros(st.shape, dtype=dtype), np.zeros(st.shape, dtype=dtype)
        for i in range(st.n):
            t = st.T[i].astype(dtype)
            ph = ph + dtype(st.cphase[i]) * t
            la = la + dtype(st.catt[i]) * t
        st._exponents[dtype] = (ph, la)
    return st._exponents[dtype]


def ref_wave(st, amp, w_in=None):
    """(wave, la): amp * w_in * exp(la) * exp(i ph); w_in None = the unit wave."""
    ph, la = exponents(st)
    w = f32(amp) * np.exp(la) * np.exp(1j * ph)
    if w_in is not None:
        w = w * w_in.astype(np.complex128)
    return w, la


def ref_rt(st, I0, I_in=None, phi_in=None):
    """(I, phi, la): I0 * I_in * exp(la) in float64, phi_in + ph in long double."""
    _, la = exponents(st)
    ph, _ = exponents(st, np.longdouble)
    I = f32(I0) * np.exp(la)
    if I_in is not None:
        I = I * I_in.astype(np.float64)
    if phi_in is not None:
        ph = ph + phi_in.astype(np.longdouble)
    return I, ph, la


def ref_accumulate(stacks, imgs, scales, acc0=None):
    """acc0 + sum_e scales[e] * imgs[e] * exp(la_e), stacks[e] the image's stack (None: no attenuation), added in list order;
    acc0 None: the first term is stored.  Returns (acc, bound, terms): the bound sums (|la_e| + 4) u |v_e| per image and
    u |running total| per add."""
    total = None if acc0 is None else acc0.astype(np.float64)
    bound, terms = 0.0, []
    for st, img, sc in zip(stacks, imgs, scales):
        la = exponents(st)[1] if st is not None and st.n else np.zeros(img.shape)
        v = f32(sc) * img.astype(np.float64) * np.exp(la)
        terms.append(v)
        total = v if total is None else total + v
        bound = bound + bound_intensity(la, v, total)
    return total, bound, terms


# ------------------------------------------------------------------------------------------------------ bounds
def bound_att(la):
    return (np.abs(la) + 2) * U


def bound_intensity(la, v, total=None):
    return (np.abs(la) + 4) * U * np.abs(v) + U * np.abs(v if total is None else total)


def bound_wave(la, ref):
    return np.abs(ref) * ((np.abs(la) + 4) * U + HW_PHASOR)


def bound_phi(st, phi_in=None):
    s = np.zeros(st.shape)
    for i in range(st.n):
        s = s + np.abs(st.cphase[i] * st.T[i].astype(np.float64))
    return st.n * EPS64 * s + (EPS64 * np.abs(phi_in.astype(np.float64)) if phi_in is not None else 0.0)


def margin(err, bound):
    """max err / bound over the pixels (0 / 0 = 0: where the bound is zero the result must be exact)."""
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


# --------------------------------------------------------------------------------------------- every map matters
def mutations(st):
    """The ways a kernel can get the table wrong, as (label, cphase, catt) over the same maps: a map dropped, the coefficients
    of two neighbours swapped, the pad map T[0] taken once more with map 0's coefficients."""
    for i in range(st.n):
        yield ("drop%d" % i, [0.0 if j == i else c for j, c in enumerate(st.cphase)],
               [0.0 if j == i else c for j, c in enumerate(st.catt)])
    for i in range(st.n - 1):
        cp, ca = list(st.cphase), list(st.catt)
        cp[i], cp[i + 1], ca[i], ca[i + 1] = cp[i + 1], cp[i], ca[i + 1], ca[i]
        yield "swap%d" % i, cp, ca
    if st.n:
        yield "pad", [2 * st.cphase[0]] + st.cphase[1:], [2 * st.catt[0]] + st.catt[1:]


def thin(st, cap=60000):
    """st on at most about `cap` pixels (every k-th): what holds at some pixel of the subset holds at some pixel."""
    npix = int(np.prod(st.shape))
    if npix <= cap:
        return st
    k = npix // cap
    return Stack(st.name, np.ascontiguousarray(st.T.reshape(st.n, -1)[:, ::k]), st.cphase, st.catt)


def how_much_each_map_matters(st):
    """For every mutation, the largest change of each reference in units of that pixel's tolerance: {label: (wave, I, phi)}.
    I stands for the accumulated image too (the same v and the same leading term)."""
    st = thin(st)
    w, la = ref_wave(st, 1.0)
    I, ph, _ = ref_rt(st, 1.0)
    out = {}
    for label, cp, ca in mutations(st):
        mt = st.with_coeffs(cp, ca)
        w2, _ = ref_wave(mt, 1.0)
        I2, ph2, _ = ref_rt(mt, 1.0)
        out[label] = (margin(np.abs(w2 - w), bound_wave(la, w)), margin(np.abs(I2 - I), bound_intensity(la, I)),
                      margin(np.abs((ph2 - ph).astype(np.float64)), bound_phi(st) + EPS64))
    return out
