"""Tensor-level operators: PyTorch-ROCm tensors in HBM -> libparesis_hip.so (ctypes) on the current HIP stream.

PyTorch is plumbing here (device memory, streams, torch.distributed); all arithmetic on the hot path runs in the
hand-written HIP kernels behind the C ABI.  Every function checks devices/dtypes/shapes on the host before a kernel is
launched, and raises PsxError on any failure -- there is no CPU fallback.
"""
import ctypes
import math
from ctypes import c_double, c_float, c_int, c_void_p

import torch

from . import _lib
from ._lib import PsxError, check, lib

MARGIN_FRESNEL = 15   # Experiment.py:236
MARGIN_DETECTOR = 15  # Detector.py:92


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(None)


def _ptrs(tensors):
    """The void* host array of a sequence of tensors for the C ABI; None gives NULL."""
    tensors = list(tensors)
    return (c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _need(t, dtype, name, shape=None):
    if not isinstance(t, torch.Tensor):
        raise PsxError("%s must be a torch.Tensor, got %r" % (name, type(t)))
    if not t.is_cuda:
        raise PsxError("%s must live in HBM (cuda/ROCm tensor); got device %s. There is no CPU path." % (name, t.device))
    if t.dtype != dtype:
        raise PsxError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise PsxError("%s must be contiguous (row-major [Nx][Ny])" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise PsxError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def _on(t, name, device, what="the plan"):
    """t, when it is on `device`; `what` names who else is there, for the message."""
    if t.device != device:
        raise PsxError("%s is on %s, %s on %s" % (name, t.device, what, device))
    return t


class MaterialStack:
    """Thickness maps [nmat, Nx, Ny] float32 in HBM + per-map coefficients (see include/paresis_hip.h, "Materials").

    Any number of maps: a kernel takes at most PSX_MAX_MAT, so a stack of more is handed to it FOLDED -- psx_fold_materials_f32
    sums the phase in float64 into a float32 hi/lo pair and the log-attenuation into one float32 map, the stack [P_hi, P_lo, A]
    with cphase (1, 1, 0) and catt (0, 0, 1), which gives every consumer the same exponents to ~1e-14 relative.  A stack of
    PSX_MAX_MAT maps or fewer is passed as it is.  fold_cache (a FoldCache, e.g. the sample's) keeps folds across calls."""

    def __init__(self, T, cphase=None, catt=None, fold_cache=None):
        if T is None:
            self.T, self.n = None, 0
        else:
            _need(T, torch.float32, "thickness stack")
            if T.dim() != 3:
                raise PsxError("Sample Geometry has the wrong nb of dim [material, x, y]")   # Sample.py:263-264
            self.T, self.n = T, T.shape[0]
        self.cphase = [0.0] * self.n if cphase is None else [float(v) for v in cphase]
        self.catt = [0.0] * self.n if catt is None else [float(v) for v in catt]
        if len(self.cphase) != self.n or len(self.catt) != self.n:
            raise PsxError("coefficient lists must have one entry per material")
        self.fold_cache = fold_cache
        self.folded = False           # maps of its own per coefficient set (a fold, or a concat holding one)

    @staticmethod
    def concat(*stacks):
        """Materials of several objects seen by one kernel (e.g. membrane phase + sample phase, Experiment.py:469).  When
        they hold more than PSX_MAX_MAT maps, the stack with the most maps (the sample) is replaced by its fold, then the
        next, until they fit."""
        stacks = [s for s in stacks if s is not None and s.n > 0]
        if not stacks:
            return MaterialStack(None)
        while sum(s.n for s in stacks) > _lib.PSX_MAX_MAT:
            i = max(range(len(stacks)), key=lambda j: stacks[j].n)
            if stacks[i].n <= _FOLD_MAPS:
                raise PsxError("%d stacks of %d maps cannot be folded to %d" % (len(stacks), sum(s.n for s in stacks),
                                                                                 _lib.PSX_MAX_MAT))
            stacks[i] = stacks[i].fold()
        out = MaterialStack.__new__(MaterialStack)
        out.T = None
        out.n = sum(s.n for s in stacks)
        out.cphase = [c for s in stacks for c in s.cphase]
        out.catt = [c for s in stacks for c in s.catt]
        out._maps = [s.map(i) for s in stacks for i in range(s.n)]
        out.fold_cache = None
        out.folded = any(s.folded for s in stacks)
        out._parts = stacks           # keeps the folds alive as long as the stack
        return out

    def map(self, i):
        if self.T is not None:
            return self.T[i]
        return self._maps[i]

    def with_coeffs(self, cphase=None, catt=None):
        """The same maps under other coefficients.  Not for a fold or a stack holding one: its maps are [P_hi, P_lo, A] of
        ONE coefficient set (take the raw stack's with_coeffs, then fold or concat)."""
        if self.folded:
            raise PsxError("with_coeffs: this stack holds a fold, whose maps belong to one coefficient set")
        out = MaterialStack.__new__(MaterialStack)
        out.T, out.n = self.T, self.n
        if self.T is None and self.n:
            out._maps = self._maps
            out._parts = getattr(self, "_parts", None)
        out.cphase = list(self.cphase) if cphase is None else [float(v) for v in cphase]
        out.catt = list(self.catt) if catt is None else [float(v) for v in catt]
        out.fold_cache = self.fold_cache
        out.folded = self.folded
        return out

    def fold(self):
        """The equivalent 3-map stack [P_hi, P_lo, A] (cphase 1, 1, 0; catt 0, 0, 1) -- from fold_cache when it holds it."""
        key = None
        if self.T is not None and self.fold_cache is not None:
            key = (self.T, tuple(self.cphase), tuple(self.catt))
            hit = self.fold_cache.get(key)
            if hit is not None:
                return hit
        out = fold_materials([self.map(i) for i in range(self.n)], self.cphase, self.catt)
        if key is not None:
            self.fold_cache.put(key, out)
        return out

    def cargs(self, shape=None):
        """(T** host array, cphase*, catt*, nmat) for the C ABI; keeps the ctypes arrays alive on self.  A stack of more than
        PSX_MAX_MAT maps passes its fold (kept on self while it lives)."""
        if self.n > _lib.PSX_MAX_MAT:
            self._fold = self.fold()
            return self._fold.cargs(shape)
        maps = [self.map(i) for i in range(self.n)]
        for i, m in enumerate(maps):
            _need(m, torch.float32, "thickness map %d" % i, shape)
        self._c = (_ptrs(maps or [None]),
                   (c_double * max(1, self.n))(*self.cphase), (c_double * max(1, self.n))(*self.catt))
        return self._c[0], self._c[1], self._c[2], self.n


_FOLD_MAPS = 3


def fold_materials(maps, cphase, catt):
    """psx_fold_materials_f32 over any number of float32 maps of one shape: a MaterialStack [P_hi, P_lo, A] (float32 [3, Nx,
    Ny] in HBM) with cphase (1, 1, 0) and catt (0, 0, 1).  More than PSX_MAX_FOLD maps fold in runs, each run's fold
    carried into the next as its first three maps (the phase pair exactly; A rounds to float32 once per run)."""
    n = len(maps)
    if n == 0 or len(cphase) != n or len(catt) != n:
        raise PsxError("fold_materials: %d maps, %d phase and %d attenuation coefficients" % (n, len(cphase), len(catt)))
    shape = tuple(maps[0].shape)
    for i, m in enumerate(maps):
        _need(m, torch.float32, "thickness map %d" % i, shape)
    out = torch.empty((_FOLD_MAPS,) + shape, dtype=torch.float32, device=maps[0].device)
    ms, cp, ca = list(maps), [float(v) for v in cphase], [float(v) for v in catt]
    while True:
        k = min(len(ms), _lib.PSX_MAX_FOLD)
        check(lib().psx_fold_materials_f32(_ptrs(ms[:k]), (c_double * k)(*cp[:k]),
                                           (c_double * k)(*ca[:k]), k, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                           out[0].numel(), _stream()), "psx_fold_materials_f32")
        if k == len(ms):
            break
        # the next run reads this run's fold in place: its output is a new buffer
        prev, out = out, torch.empty_like(out)
        ms = [prev[0], prev[1], prev[2]] + ms[k:]
        cp = [1.0, 1.0, 0.0] + cp[k:]
        ca = [0.0, 0.0, 1.0] + ca[k:]
    st = MaterialStack(out, cphase=[1.0, 1.0, 0.0], catt=[0.0, 0.0, 1.0])
    st.folded = True
    return st


class FoldCache:
    """Folds of an object's thickness stacks, keyed by (stack tensor, cphase, catt): the stack is matched by IDENTITY (an
    id() alone can be reused by a new tensor), the coefficients by value.  Bounded by bytes, the least recently used out
    first (the most recent fold always stays)."""

    def __init__(self, max_bytes):
        self.max_bytes = int(max_bytes)
        self._entries = {}            # (id(T), cphase, catt) -> (T, stack, bytes), least recently used first
        self.nbytes = 0

    def _k(self, key):
        return (id(key[0]),) + tuple(key[1:])

    def get(self, key):
        k = self._k(key)
        hit = self._entries.get(k)
        if hit is None or hit[0] is not key[0]:
            return None
        self._entries[k] = self._entries.pop(k)
        return hit[1]

    def put(self, key, stack):
        k = self._k(key)
        old = self._entries.pop(k, None)
        if old is not None:
            self.nbytes -= old[2]
        nb = stack.T.numel() * stack.T.element_size()
        while self._entries and self.nbytes + nb > self.max_bytes:
            self.nbytes -= self._entries.pop(next(iter(self._entries)))[2]
        self._entries[k] = (key[0], stack, nb)
        self.nbytes += nb

    def clear(self):
        self._entries.clear()
        self.nbytes = 0

    def __len__(self):
        return len(self._entries)


_NO_MATS = None


def _mats(m):
    global _NO_MATS
    if m is None:
        if _NO_MATS is None:
            _NO_MATS = MaterialStack(None)
        return _NO_MATS
    return m


class MaterialBatch:
    """The materials of a batch of sources over the same maps (the energies of a detector bin): `base` carries the maps,
    cphase[s][i] / catt[s][i] the coefficients of source s.  What a list of per-source MaterialStack objects says, without
    building them (and re-checking their maps) for every membrane position: the coefficients depend on the energy only."""

    def __init__(self, base, cphase, catt):
        self.base = _unfolded(_mats(base), "MaterialBatch")
        self.cphase = [[float(v) for v in r] for r in cphase]
        self.catt = [[float(v) for v in r] for r in catt]
        if any(len(r) != self.base.n for r in self.cphase) or any(len(r) != self.base.n for r in self.catt):
            raise PsxError("MaterialBatch: one coefficient per material and source")
        self.n = self.base.n

    def rebase(self, base):
        """The same coefficients over another position's maps."""
        out = MaterialBatch.__new__(MaterialBatch)
        out.base, out.cphase, out.catt, out.n = _unfolded(_mats(base), "MaterialBatch.rebase"), self.cphase, self.catt, self.n
        if out.base.n != self.n:
            raise PsxError("MaterialBatch.rebase: %d maps for %d coefficients" % (out.base.n, self.n))
        return out


def _unfolded(m, what):
    """m, when its maps can serve other coefficients: a stack that folds (more than PSX_MAX_MAT maps) or holds a fold has
    maps of its own for each coefficient set, so the sources of a batch cannot share them."""
    if m.n > _lib.PSX_MAX_MAT or m.folded:
        raise PsxError("%s: a stack of more than %d maps folds per coefficient set; its sources cannot share maps (take one "
                       "call per source)" % (what, _lib.PSX_MAX_MAT))
    return m


def _batch_mats(mats, ns, shape, what):
    """(T** host array, nmat, cphase[ns][nmat], catt[ns][nmat]) from a MaterialBatch or from one MaterialStack per source."""
    if isinstance(mats, MaterialBatch):
        if len(mats.cphase) != ns:
            raise PsxError("%s: %d coefficient rows for %d sources" % (what, len(mats.cphase), ns))
        return mats.base.cargs(shape)[0], mats.n, mats.cphase, mats.catt
    mats = [_mats(None)] * ns if mats is None else [_unfolded(_mats(m), what) for m in mats]
    nm = mats[0].n
    T = mats[0].cargs(shape)[0]
    for m in mats[1:]:
        if m.n != nm or any(m.map(i).data_ptr() != mats[0].map(i).data_ptr() for i in range(nm)):
            raise PsxError("%s: every source must use the same thickness maps" % what)
    return T, nm, [m.cphase for m in mats], [m.catt for m in mats]


_workspaces = {}
_status_words = {}


def _workspace(device, nbytes):
    # one scratch buffer per (device, stream): calls issued on different streams may overlap on the GPU
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def status_word(device):
    """Per-device status word the kernels OR error bits into (PSX_STATUS_*)."""
    w = _status_words.get(device.index)
    if w is None:
        w = torch.zeros(1, dtype=torch.int32, device=device)
        _status_words[device.index] = w
    return w


def check_status(device, what="refraction"):
    """Synchronising read of the status word; raises like refractionFileNumba2.py:81-82 and clears it."""
    w = status_word(device)
    v = int(w.item())
    if v:
        w.zero_()
        if v & _lib.STATUS_NONFINITE:
            raise PsxError("The calculated intensity refractive includes some nans or insane values (%s)" % what)
        raise PsxError("device status %d after %s" % (v, what))


# --------------------------------------------------------------------------------------------- transmission
def transmit_wave(wave_in, amp, mats, out=None):
    """K1 (Sample.py:279): out = amp * wave_in * exp(sum catt*T) * exp(i sum cphase*T).  wave_in None = unit wave."""
    mats = _mats(mats)
    ref = wave_in if wave_in is not None else mats.map(0)
    shape = tuple(ref.shape)
    if wave_in is not None:
        _need(wave_in, torch.complex64, "wave_in")
    if out is None:
        out = torch.empty(shape, dtype=torch.complex64, device=ref.device)
    _need(out, torch.complex64, "wave_out", shape)
    T, cp, ca, n = mats.cargs(shape)
    check(lib().psx_transmit_wave_c64(_ptr(wave_in), c_float(amp), T, cp, ca, n, _ptr(out), out.numel(), _stream()),
          "psx_transmit_wave_c64")
    return out


def fill(t, value):
    """t[:] = value through the library's own elementwise kernel (K2 with no input image and no material): the hot loop
    launches no PyTorch kernel -- the first launch of one (fill, cat, reduce) makes PyTorch load its code object for that
    kernel family, a one-off 15-40 ms host stall that showed up at membrane position 0 (position loop)."""
    _need(t, torch.float32, "fill target")
    check(lib().psx_transmit_rt_f32(None, c_float(value), None, None, None, 0, _ptr(t), None, None, t.numel(), _stream()),
          "psx_transmit_rt_f32 (fill)")
    return t


def transmit_rt(I_in, I0, mats, phi_in=None, want_phi=True, shape=None, out=None):
    """K2 (Sample.py:347-348): I = I0*I_in*exp(sum catt*T); phi = phi_in + sum cphase*T (float64)."""
    mats = _mats(mats)
    ref = I_in if I_in is not None else (mats.map(0) if mats.n else out)
    shape = tuple(ref.shape)
    if I_in is not None:
        _need(I_in, torch.float32, "I_in")
    if phi_in is not None:
        _need(phi_in, torch.float64, "phi_in", shape)
    if out is not None:
        _need(out, torch.float32, "I_out", shape)
    I_out = out if out is not None else torch.empty(shape, dtype=torch.float32, device=ref.device)
    phi_out = torch.empty(shape, dtype=torch.float64, device=ref.device) if want_phi else None
    T, cp, ca, n = mats.cargs(shape)
    check(lib().psx_transmit_rt_f32(_ptr(I_in), c_float(I0), T, cp, ca, n, _ptr(I_out), _ptr(phi_in), _ptr(phi_out),
                                    I_out.numel(), _stream()), "psx_transmit_rt_f32")
    return I_out, phi_out


def accumulate(acc, img, scale=1.0, mats=None, add=True):
    """acc (+)= scale*img*exp(sum catt*T)  (Experiment.py:351-358, 478-483)."""
    mats = _mats(mats)
    _need(acc, torch.float32, "acc")
    _need(img, torch.float32, "img", acc.shape)
    T, cp, ca, n = mats.cargs(tuple(acc.shape))
    check(lib().psx_accumulate_f32(_ptr(acc), _ptr(img), c_float(scale), T, ca, n, 1 if add else 0, acc.numel(),
                                   _stream()), "psx_accumulate_f32")
    return acc


def new_sums(device):
    return torch.zeros((_lib.PSX_SUM_SLOTS, _lib.PSX_SUM_STRIDE), dtype=torch.float64, device=device)


def fold_sums(sums):
    """[sum S, sum weight*S] (float64 tensor of 2, still in HBM) of a new_sums() buffer."""
    return sums[:, :2].sum(dim=0)


def accumulate_sum(acc, img, sums, weight, scale=1.0, mats=None, add=True):
    """accumulate() that also reduces what it adds: sums[0] += sum(v), sums[1] += weight*sum(v), v = scale*img*att
    (Experiment.py:360-361, 485-486).  sums: float64 [SUM_SLOTS, SUM_STRIDE] in HBM from new_sums() -- the kernel's
    workgroups add into 32 slots 128 bytes apart; fold_sums() gives the two totals.  acc may be None (reduction only)."""
    mats = _mats(mats)
    _need(img, torch.float32, "img")
    if acc is not None:
        _need(acc, torch.float32, "acc", img.shape)
    _need(sums, torch.float64, "sums", (_lib.PSX_SUM_SLOTS, _lib.PSX_SUM_STRIDE))
    T, cp, ca, n = mats.cargs(tuple(img.shape))
    check(lib().psx_accumulate_sum_f32(_ptr(acc), _ptr(img), c_float(scale), T, ca, n, 1 if add else 0, img.numel(),
                                       _ptr(sums), c_double(weight), _stream()), "psx_accumulate_sum_f32")
    return acc


def accumulate_many(acc, imgs, sums, weights, scales=None, mats=None, add=True):
    """accumulate_sum() over the images of several energies in ONE pass per PSX_MAX_SRC images, added in list order exactly
    as one accumulate_sum call per image would: acc (+)= sum_e scales[e] * imgs[e] * att_e, sums += (sum, sum of
    weights[e] * term).  mats[e]: MaterialStack of image e (same maps, own attenuation coefficients) or None."""
    ne = len(imgs)
    scales = [1.0] * ne if scales is None else [float(v) for v in scales]
    shape = tuple(imgs[0].shape)
    for i, t in enumerate(imgs):
        _need(t, torch.float32, "imgs[%d]" % i, shape)
    if acc is not None:
        _need(acc, torch.float32, "acc", shape)
    if sums is not None:
        _need(sums, torch.float64, "sums", (_lib.PSX_SUM_SLOTS, _lib.PSX_SUM_STRIDE))
    T, nm, _, cat = _batch_mats(mats, ne, shape, "accumulate_many")
    for e0 in range(0, ne, _lib.PSX_MAX_SRC):
        el = range(e0, min(ne, e0 + _lib.PSX_MAX_SRC))
        n = len(el)
        check(lib().psx_accumulate_many_f32(
            _ptr(acc), _ptrs(imgs[e] for e in el), (c_float * n)(*[scales[e] for e in el]), n, T,
            (c_double * max(1, n * nm))(*[c for e in el for c in cat[e]]), nm, 1 if (add or e0 > 0) else 0,
            imgs[0].numel(), _ptr(sums), (c_double * n)(*[float(weights[e]) for e in el]), _stream()),
            "psx_accumulate_many_f32")
    return acc


# ----------------------------------------------------------------------------------------------- refraction
def _refract_io(shape, outs, k, add, mats=None, I_in=None, phi_in=None, on=None, name="I_out",
                missing="existing output images"):
    """The preamble the refraction wrappers share; returns (Nx, Ny, device, outs).  The optional inputs I_in / phi_in are
    checked; the device is that of `on`, else of the first input given, else of the maps; the k output images are allocated
    there (not with add=True, which needs the `missing` ones) or checked under `name` (numbered where it holds a %d)."""
    Nx, Ny = int(shape[0]), int(shape[1])
    if on is None:
        on = I_in if I_in is not None else (phi_in if phi_in is not None else mats.map(0))
    dev = on.device
    if I_in is not None:
        _need(I_in, torch.float32, "I_in", (Nx, Ny))
    if phi_in is not None:
        _need(phi_in, torch.float64, "phi_in", (Nx, Ny))
    if outs is None:
        if add:
            raise PsxError("add=True needs " + missing)
        outs = [torch.empty((Nx, Ny), dtype=torch.float32, device=dev) for _ in range(k)]
    for e, t in enumerate(outs):
        _need(t, torch.float32, name % e if "%" in name else name, (Nx, Ny))
    return Nx, Ny, dev, outs


def refract(shape, mats, dscale, clamp, margin=15, I_in=None, I0=1.0, phi_in=None, out=None, out_scale=1.0, add=False,
            want_D=False, I_mut=None):
    """K9-K13 (refractionFileNumba2.py:25-86 + 198-263).  Returns (I_out, Dx|None, Dy|None); Dx,Dy are padded."""
    mats = _mats(mats)
    Nx, Ny, dev, (out,) = _refract_io(shape, None if out is None else [out], 1, add, mats, I_in, phi_in,
                                      missing="an existing output image")
    Dx = Dy = None
    if want_D:
        Dx = torch.empty((Nx + 2 * margin, Ny + 2 * margin), dtype=torch.float32, device=dev)
        Dy = torch.empty_like(Dx)
    if I_mut is not None and (I_in is None or I_mut.data_ptr() != I_in.data_ptr()):
        raise PsxError("I_mut must alias I_in")
    ws = _workspace(dev, lib().psx_refract_workspace_bytes(Nx, Ny))
    T, cp, ca, n = mats.cargs((Nx, Ny))
    check(lib().psx_refract_f32(_ptr(I_in), c_float(I0), T, cp, ca, n, _ptr(phi_in), _ptr(out), c_float(out_scale),
                                1 if add else 0, _ptr(Dx), _ptr(Dy), _ptr(I_mut), Nx, Ny, int(margin), c_double(dscale),
                                c_double(clamp[0]), c_double(clamp[1]), _ptr(status_word(dev)), _ptr(ws), _stream()),
          "psx_refract_f32")
    return out, Dx, Dy


def refract_split(shape, mats, dscale, clamp, mask, margin=15, I_in=None, I0=1.0, phi_in=None, outs=None, out_scale=1.0,
                  add=False):
    """fastRefractionDF's split and its two refractions (RF2:147-154) in one call (psx_refract_split_f32): returns
    (refraction of the sources where mask == 0, refraction of the sources where mask != 0); mask: float32 [Nx][Ny]."""
    mats = _mats(mats)
    _need(mask, torch.float32, "mask", (int(shape[0]), int(shape[1])))
    Nx, Ny, dev, outs = _refract_io(shape, outs, 2, add, mats, I_in, phi_in, on=mask)
    ws = _workspace(dev, lib().psx_refract_multi_workspace_bytes(Nx, Ny, 2))
    T, cp, ca, n = mats.cargs((Nx, Ny))
    check(lib().psx_refract_split_f32(_ptr(I_in), _ptr(mask), c_float(I0), T, cp, ca, n, _ptr(phi_in), _ptr(outs[0]),
                                      _ptr(outs[1]), c_float(out_scale), 1 if add else 0, Nx, Ny, int(margin), c_double(dscale),
                                      c_double(clamp[0]), c_double(clamp[1]), _ptr(status_word(dev)), _ptr(ws), _stream()),
          "psx_refract_split_f32")
    return outs[0], outs[1]


def refract_batch(shape, mats, dscales, clamp, margin=15, I_in=None, I0=None, outs=None, out_scale=1.0, add=False):
    """Several refractions over the SAME thickness maps in one launch per kernel (the energies of a detector bin,
    EXP:448-486): mats[e] (same maps, own coefficients), dscales[e], I_in[e] (all or None) or the uniform I0[e], outs[e].
    Every image is what refract() gives for that refraction.  Returns the list of output images."""
    ne = len(dscales)
    Nx, Ny = int(shape[0]), int(shape[1])
    T, nm, cph, cat = _batch_mats(mats, ne, (Nx, Ny), "refract_batch")
    maps = (mats.base if isinstance(mats, MaterialBatch) else _mats(mats[0])).map(0)
    for e, t in enumerate(I_in if I_in is not None else ()):
        _need(t, torch.float32, "I_in[%d]" % e, (Nx, Ny))
    _, _, dev, outs = _refract_io(shape, outs, ne, add, on=maps, name="outs[%d]")
    I0 = [1.0] * ne if I0 is None else [float(v) for v in I0]
    for e0 in range(0, ne, _lib.PSX_MAX_SRC):
        el = range(e0, min(ne, e0 + _lib.PSX_MAX_SRC))
        n = len(el)
        ws = _workspace(dev, lib().psx_refract_batch_workspace_bytes(Nx, Ny, n))
        check(lib().psx_refract_batch_f32(
            n, _ptrs(I_in[e] for e in el) if I_in is not None else None,
            (c_float * n)(*[I0[e] for e in el]), T,
            (c_double * (n * nm))(*[c for e in el for c in cph[e]]),
            (c_double * (n * nm))(*[c for e in el for c in cat[e]]), nm,
            _ptrs(outs[e] for e in el), c_float(out_scale), 1 if add else 0, Nx, Ny, int(margin),
            (c_double * n)(*[float(dscales[e]) for e in el]), c_double(clamp[0]), c_double(clamp[1]),
            _ptr(status_word(dev)), _ptr(ws), _stream()), "psx_refract_batch_f32")
    return outs


def refract_multi(shape, mats, dscales, clamp, margin=15, I_in=None, I0=1.0, phi_in=None, outs=None, out_scale=1.0,
                  add=False):
    """A propagation-distance batch of K9-K13: len(dscales) refractions of the SAME source (I_in/I0, mats, phi_in) in
    one launch per kernel (psx_refract_multi_f32); the thickness maps are read once per tile for all distances.
    Returns the list of images, each identical to refract(..., dscale=dscales[d])[0]."""
    mats = _mats(mats)
    nd = len(dscales)
    if outs is not None and len(outs) != nd:
        raise PsxError("refract_multi: %d output images for %d distances" % (len(outs), nd))
    Nx, Ny, dev, outs = _refract_io(shape, outs, nd, add, mats, I_in, phi_in)
    ws = _workspace(dev, lib().psx_refract_multi_workspace_bytes(Nx, Ny, nd))
    T, cp, ca, n = mats.cargs((Nx, Ny))
    dsc = (c_double * nd)(*[float(x) for x in dscales])
    check(lib().psx_refract_multi_f32(_ptr(I_in), c_float(I0), T, cp, ca, n, _ptr(phi_in), _ptrs(outs), c_float(out_scale),
                                      1 if add else 0, None, None, None, Nx, Ny, int(margin), dsc, nd,
                                      c_double(clamp[0]), c_double(clamp[1]), _ptr(status_word(dev)), _ptr(ws),
                                      _stream()), "psx_refract_multi_f32")
    return outs


def set_refract_halo(halo):
    """Gather halo of the refraction tile kernel: 4, 6, 8, 12 or 16 pixels (psx_refract_set_halo; a speed knob -- the halo decides
    which shares are gathered in the tiles and which are replayed, so the last bit of an image may depend on it)."""
    check(lib().psx_refract_set_halo(int(halo)), "psx_refract_set_halo")


def tune_refract_halo(call, halos=(4, 6, 8), reps=2):
    """Picks the gather halo by MEASUREMENT: `call()` (a refraction with the caller's real arguments) is timed with each halo --
    one untimed run, then `reps` runs between two events -- and the fastest stays set.  Which halo wins depends on how many
    rays travel further than it (the far-ray replay costs ~11 global atomics per ns): 4 or 6 pixels at oversampling 2, 12 at
    oversampling 4 with the bench's membranes (pass halos=(4, 6, 8, 12, 16) there).  The images agree to float rounding whatever the choice (a pixel's sum is split
    differently between tile gather and replay: the last bit may move -- a reproducible run fixes the halo by rule instead).
    One host synchronisation per candidate: meant for the set-up of a run, not for its loop.  Returns (halo, {halo: ms})."""
    times = {}
    for h in halos:
        set_refract_halo(h)
        call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        times[h] = e0.elapsed_time(e1) / reps
    best = min(times, key=times.get)
    set_refract_halo(best)
    return best, times


def darkfield_blur(I2DF, DF, I2, R):
    """Variable-width Gaussian re-splat of fastRefractionDF (refractionFileNumba2.py:168-186): returns
    I2 + sum_s I2DF[s] * gaussian_shape(DF[s]/2) centred on s.  DF in pixels at the target pixels; R = max half-size."""
    _need(I2DF, torch.float32, "I2DF")
    _need(DF, torch.float32, "DF", I2DF.shape)
    if I2 is not None:
        _need(I2, torch.float32, "I2", I2DF.shape)
    out = torch.empty_like(I2DF)
    Nx, Ny = I2DF.shape
    ws = torch.empty(lib().psx_darkfield_workspace_bytes(Nx, Ny), dtype=torch.uint8, device=I2DF.device)
    check(lib().psx_darkfield_blur_f32(_ptr(I2DF), _ptr(DF), _ptr(I2), _ptr(out), Nx, Ny, int(R), _ptr(ws), _stream()),
          "psx_darkfield_blur_f32")
    return out


def darkfield_split(I, DF_rad, num, den, limit):
    """The front of fastRefractionDF in one pass (psx_darkfield_split_f32); DF_px = DF_rad * num / den, float64, in the
    reference's order (RF2:114: num = propagationDistance, den = studyPixelSize*1e-6*magnification).  Returns (I_nodf, I_df, DF_px float32, prep,
    words): words = two device uint64 holding the float64 bit patterns of max(DF_px) before / after the DF > limit -> 0 rule
    -- read them with darkfield_maxima() only when the caller does not know the maximum (one host synchronisation)."""
    _need(I, torch.float32, "I")
    _need(DF_rad, torch.float64, "darkField", I.shape)
    Nx, Ny = I.shape
    dev = I.device
    I_nodf, I_df, DF_px = (torch.empty((Nx, Ny), dtype=torch.float32, device=dev) for _ in range(3))
    prep = torch.empty(lib().psx_darkfield_workspace_bytes(Nx, Ny), dtype=torch.uint8, device=dev)
    words = torch.empty(2, dtype=torch.int64, device=dev)
    check(lib().psx_darkfield_split_f32(_ptr(I), _ptr(DF_rad), c_double(num), c_double(den), c_double(limit), _ptr(I_nodf), _ptr(I_df),
                                        _ptr(DF_px), _ptr(prep), _ptr(words), Nx, Ny, _stream()), "psx_darkfield_split_f32")
    return I_nodf, I_df, DF_px, prep, words


def darkfield_maxima(words):
    """(max DF_px, max DF_px after the DF > limit rule) from the device words of darkfield_split: ONE device-to-host copy."""
    import numpy as np
    w = words.cpu().numpy().view(np.float64)
    return float(w[0]), float(w[1])


def darkfield_blur_prepared(I2DF, DF, prep, I2, R, scan=True, out=None, add=False):
    """darkfield_blur() on the patch table darkfield_split() made from the width map; scan: NaN / inf in the result raise
    the device status word (RF2:190-193), checked by the kernel that stores it.  out / add: the result is stored into (added
    to) an existing image -- the chain's sum over energies without a pass of its own."""
    _need(I2DF, torch.float32, "I2DF")
    _need(DF, torch.float32, "DF", I2DF.shape)
    if out is None:
        if add:
            raise PsxError("add=True needs an existing output image")
        out = torch.empty_like(I2DF)
    _need(out, torch.float32, "out", I2DF.shape)
    Nx, Ny = I2DF.shape
    check(lib().psx_darkfield_blur_prepared_f32(_ptr(I2DF), _ptr(DF), _ptr(prep), _ptr(I2), _ptr(out), Nx, Ny, int(R),
                                                _ptr(status_word(I2DF.device)) if scan else None, 1 if add else 0, _stream()),
          "psx_darkfield_blur_prepared_f32")
    return out


def darkfield_merge(I, a, b):
    """I[:] = a + b through the library (no PyTorch kernel in the dark-field path)."""
    check(lib().psx_darkfield_merge_f32(_ptr(I), _ptr(a), _ptr(b), I.numel(), _stream()), "psx_darkfield_merge_f32")
    return I


def repad(src, margin_src, margin_dst, shape):
    """The centre `shape` of a map padded by margin_src, re-padded with zeros to margin_dst (psx_repad_f32)."""
    Nx, Ny = int(shape[0]), int(shape[1])
    _need(src, torch.float32, "src", (Nx + 2 * margin_src, Ny + 2 * margin_src))
    dst = torch.empty((Nx + 2 * margin_dst, Ny + 2 * margin_dst), dtype=torch.float32, device=src.device)
    check(lib().psx_repad_f32(_ptr(src), int(margin_src), _ptr(dst), int(margin_dst), Nx, Ny, _stream()), "psx_repad_f32")
    return dst


def set_deterministic(on=True):
    """Order-independent sums in the scatter paths that otherwise use float atomics (far rays, fastloop): fixed-point
    deposits, bitwise reproducible results, a few per cent slower.  Per host thread; off by default in the
    library, ON around the Experiment class's ray-tracing chain unless exp_dict['reproducible'] is False."""
    check(lib().psx_set_deterministic(1 if on else 0), "psx_set_deterministic")


def get_deterministic():
    return bool(lib().psx_get_deterministic())


def set_deterministic_scale(scale=0.0):
    """The replay's fixed-point unit from the caller's intensity scale (psx_set_deterministic_scale); 0: from the call's own
    measured maximum (the default)."""
    check(lib().psx_set_deterministic_scale(c_float(float(scale))), "psx_set_deterministic_scale")


def get_deterministic_scale():
    """The calling thread's replay scale (psx_get_deterministic_scale; 0 = the unit comes from each call's measured maximum)."""
    return float(lib().psx_get_deterministic_scale())


class deterministic:
    """with ops.deterministic(on[, scale]): ... -- sets the mode (and the unit's scale) and puts back what the caller had, mode AND
    scale: scopes nest (Experiment.refraction inside the ray-tracing chain's scope keeps the chain's fixed unit; a user's own
    psx_set_deterministic_scale survives a call of the class).  scale=None keeps the caller's scale."""

    def __init__(self, on=True, scale=0.0):
        self.on = bool(on)
        self.scale = None if scale is None else (float(scale) if on else 0.0)

    def __enter__(self):
        self.prev, self.prev_scale = get_deterministic(), get_deterministic_scale()
        set_deterministic(self.on)
        if self.scale is not None:
            set_deterministic_scale(self.scale)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        set_deterministic_scale(self.prev_scale)
        return False


def clock_probe():
    """Shader clock in MHz the device sustains right now (psx_clock_probe: a 30 us spin on every CU behind what is queued on the
    current stream, which it synchronises).  Diagnostics: the boxes of a pool differ by > 10 % in what they sustain."""
    mhz = c_float(0.0)
    check(lib().psx_clock_probe(ctypes.byref(mhz), _stream()), "psx_clock_probe")
    return float(mhz.value)


def debug_switch(name, value=1):
    """A diagnostic A/B switch of the library (psx_debug_switch; include/paresis_hip.h lists the names).  Process-wide, off by
    default; for tools and tests -- the library never reads the environment."""
    check(lib().psx_debug_switch(str(name).encode(), int(value)), "psx_debug_switch")


def debug_switches_active():
    """'name=value ...' of every diagnostic switch that is not at its default ('' = a clean product run)."""
    buf = ctypes.create_string_buffer(512)
    check(lib().psx_debug_switches_active(buf, len(buf)), "psx_debug_switches_active")
    return buf.value.decode()


def fastloop(I, Dx, Dy, I2):
    """fastloopNumba (refractionFileNumba2.py:198-263) on explicit float32 displacement maps; accumulates into I2."""
    _need(I, torch.float32, "I")
    for nm, t in (("Dx", Dx), ("Dy", Dy), ("I2", I2)):
        _need(t, torch.float32, nm, I.shape)
    check(lib().psx_fastloop_f32(_ptr(I), _ptr(Dx), _ptr(Dy), _ptr(I2), I.shape[0], I.shape[1], _stream()),
          "psx_fastloop_f32")
    return I2


# ---------------------------------------------------------------------------------------------- plan handles
class _Plan:
    """A plan of the library: its `device`, the handle `_h` (both set by _create, from the subclass's __init__) and
    `_destroy`, the name of the symbol that frees it.  close() may be called any number of times; a plan that is dropped
    closes itself."""
    _destroy = None

    def _create(self, device, symbol, *args):
        """The plan's device (None: the current one) and, on it, the handle: symbol(*args, &handle)."""
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._h = c_void_p(None)
        with torch.cuda.device(self.device):
            check(getattr(lib(), symbol)(*args, ctypes.byref(self._h)), symbol)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib(), self._destroy)(self._h)
            self._h = c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# -------------------------------------------------------------------------------------------------- Fresnel
class FresnelPlan(_Plan):
    """psx_fresnel_plan for one study grid (Experiment.wavePropagation, Experiment.py:219-252)."""
    _destroy = "psx_fresnel_plan_destroy"

    def __init__(self, Nx, Ny, margin=MARGIN_FRESNEL, max_dist=4, engine=_lib.ENGINE_AUTO, device=None):
        self.Nx, self.Ny, self.margin, self.max_dist = int(Nx), int(Ny), int(margin), int(max_dist)
        self._create(device, "psx_fresnel_plan_create", self.Nx, self.Ny, self.margin, self.max_dist, int(engine))
        self.engine = lib().psx_fresnel_plan_engine(self._h)
        self.bytes = lib().psx_fresnel_plan_bytes(self._h)

    def work_queue(self, on=True):
        """Line groups through a queue instead of static shares (psx_fresnel_plan_work_queue): for runs whose transfers or
        other streams share the GPU with the propagations."""
        check(lib().psx_fresnel_plan_work_queue(self._h, 1 if on else 0), "psx_fresnel_plan_work_queue")

    def propagate(self, a, gphase, du, wave_in=None, amp=1.0, mats=None, want_wave=None, inten_out=None,
                  inten_scale=None, add=False):
        """One input wave -> len(a) distances.  a[d]=z/(2kM), gphase[d]=kz/M, du=(du_x,du_y)=2*pi/(N*h).

        want_wave[d]: return the complex field; inten_out[d]: float32 image that receives inten_scale[d]*|.|^2
        (added when add=True).  Returns the list of complex outputs (None where not wanted)."""
        mats = _mats(mats)
        nd = len(a)
        shape = (self.Nx, self.Ny)
        if wave_in is not None:
            _need(wave_in, torch.complex64, "wave_in", shape)
        want_wave = [True] * nd if want_wave is None else list(want_wave)
        inten_out = [None] * nd if inten_out is None else list(inten_out)
        inten_scale = [1.0] * nd if inten_scale is None else [float(s) for s in inten_scale]
        waves = [torch.empty(shape, dtype=torch.complex64, device=self.device) if w else None for w in want_wave]
        for i, t in enumerate(inten_out):
            if t is not None:
                _need(t, torch.float32, "inten_out[%d]" % i, shape)
        T, cp, ca, n = mats.cargs(shape)
        check(lib().psx_fresnel_propagate(self._h, _ptr(wave_in), c_float(amp), T, cp, ca, n, nd,
                                          (c_double * nd)(*[float(v) for v in a]),
                                          (c_double * nd)(*[float(v) for v in gphase]), c_double(du[0]), c_double(du[1]),
                                          _ptrs(waves), _ptrs(inten_out), (c_float * nd)(*inten_scale), 1 if add else 0,
                                          _stream()),
              "psx_fresnel_propagate")
        return waves


    def propagate_sources(self, a, gphase, du, wave_in=None, amp=None, mats=None, want_wave=None, inten_out=None,
                          inten_scale=None):
        """Several source waves over the SAME thickness maps in one call (the energies of a detector bin, EXP:317-361):
        a[s][d], gphase[s][d]; wave_in[s] (or None), amp[s]; mats[s]: MaterialStack of source s (same maps, own coefficients);
        want_wave[d]; inten_out[s][d] (float32 image or None), inten_scale[s][d].  Every (source, distance) result is what
        propagate() gives for that source; nothing is accumulated.  Returns waves[s][d] (None where not wanted).  More than
        PSX_MAX_SRC sources are taken in chunks."""
        ns, nd = len(a), len(a[0])
        shape = (self.Nx, self.Ny)
        T, nm, cph, cat = _batch_mats(mats, ns, shape, "propagate_sources")
        amp = [1.0] * ns if amp is None else [float(v) for v in amp]
        want_wave = [True] * nd if want_wave is None else list(want_wave)
        inten_out = [[None] * nd for _ in range(ns)] if inten_out is None else [list(r) for r in inten_out]
        inten_scale = [[1.0] * nd for _ in range(ns)] if inten_scale is None else [[float(v) for v in r] for r in inten_scale]
        waves = [[torch.empty(shape, dtype=torch.complex64, device=self.device) if w else None for w in want_wave]
                 for _ in range(ns)]
        for s0 in range(0, ns, _lib.PSX_MAX_SRC):
            sl = range(s0, min(ns, s0 + _lib.PSX_MAX_SRC))
            n = len(sl)
            for s in sl:
                if wave_in is not None and wave_in[s] is not None:
                    _need(wave_in[s], torch.complex64, "wave_in[%d]" % s, shape)
                for d, t in enumerate(inten_out[s]):
                    if t is not None:
                        _need(t, torch.float32, "inten_out[%d][%d]" % (s, d), shape)
            wi = _ptrs(None if wave_in is None else wave_in[s] for s in sl)
            wo, io = _ptrs(waves[s][d] for s in sl for d in range(nd)), _ptrs(inten_out[s][d] for s in sl for d in range(nd))
            check(lib().psx_fresnel_propagate_sources(
                self._h, n, nd, wi, (c_float * n)(*[amp[s] for s in sl]), T,
                (c_double * max(1, n * nm))(*[c for s in sl for c in cph[s]]),
                (c_double * max(1, n * nm))(*[c for s in sl for c in cat[s]]), nm,
                (c_double * (n * nd))(*[float(a[s][d]) for s in sl for d in range(nd)]),
                (c_double * (n * nd))(*[float(gphase[s][d]) for s in sl for d in range(nd)]), c_double(du[0]), c_double(du[1]),
                wo, io, (c_float * (n * nd))(*[inten_scale[s][d] for s in sl for d in range(nd)]), _stream()),
                "psx_fresnel_propagate_sources")
        return waves


# ------------------------------------------------------------------------------------------------- detector
class DetectorPlan(_Plan):
    """psx_detector_plan: the composed blur/bin/PSF operator of Detector.detection (Detector.py:79-119)."""
    _destroy = "psx_detector_plan_destroy"

    def __init__(self, Nx, Ny, ov, nx, ny, sigma_src, sigma_psf, margin=MARGIN_DETECTOR, device=None):
        self.Nx, self.Ny, self.nx, self.ny = int(Nx), int(Ny), int(nx), int(ny)
        self._create(device, "psx_detector_plan_create", self.Nx, self.Ny, int(ov), self.nx, self.ny, int(margin),
                     c_double(sigma_src), c_double(sigma_psf))

    INFO_FIELDS = ("fx_W", "fy_W", "bx_W", "by_W", "front_ok", "front_cheap", "front_RT", "back_ok", "back_RT", "back_stencil",
                   "pitch2", "fy_n_out")

    def info(self):
        """What the plan decided (psx_detector_plan_info, host only): the band widths of the four operators, whether the fused
        pairs fit (and the front's halos are cheap), their rows per tile, whether the PSF stage is a plain stencil, and the
        pitch and row length of the fused front's intermediate image."""
        buf = (c_int * _lib.PSX_DETECTOR_PLAN_INFO)()
        n = lib().psx_detector_plan_info(self._h, buf, len(buf))
        if n != len(self.INFO_FIELDS):
            raise _lib.PsxError("psx_detector_plan_info wrote %d of %d fields" % (n, len(self.INFO_FIELDS)))
        return dict(zip(self.INFO_FIELDS, (int(v) for v in buf)))

    def detect(self, img, out=None):
        _need(img, torch.float32, "img", (self.Nx, self.Ny))
        if out is None:
            out = torch.empty((self.nx, self.ny), dtype=torch.float32, device=img.device)
        _need(out, torch.float32, "out", (self.nx, self.ny))
        check(lib().psx_detect_f32(self._h, _ptr(img), _ptr(out), _stream()), "psx_detect_f32")
        return out

    def detect_many(self, imgs, outs=None):
        """detect() of several images of this plan's shape -- the images of an energy bin -- PSX_MAX_DETECT per call: fused
        stages take them in one launch each; every image comes out exactly as detect() of it alone would."""
        outs = [None] * len(imgs) if outs is None else list(outs)
        for k, img in enumerate(imgs):
            _need(img, torch.float32, "imgs[%d]" % k, (self.Nx, self.Ny))
            if outs[k] is None:
                outs[k] = torch.empty((self.nx, self.ny), dtype=torch.float32, device=img.device)
            _need(outs[k], torch.float32, "outs[%d]" % k, (self.nx, self.ny))
        for k0 in range(0, len(imgs), _lib.PSX_MAX_DETECT):
            part_in, part_out = imgs[k0:k0 + _lib.PSX_MAX_DETECT], outs[k0:k0 + _lib.PSX_MAX_DETECT]
            check(lib().psx_detect_multi_f32(self._h, _ptrs(part_in), _ptrs(part_out), len(part_in), _stream()),
                  "psx_detect_multi_f32")
        return outs


def detector_operator_host(N, ov, n, sigma_src, sigma_psf, margin=MARGIN_DETECTOR):
    """One axis of the composed detector operator, built on the host (no GPU): (start[n], weights[n][W])."""
    import numpy as np
    wcap = 4096
    start = (c_int * n)()
    weights = (c_float * (n * wcap))()
    W = c_int(0)
    check(lib().psx_detector_operator_host(int(N), int(ov), int(n), int(margin), c_double(sigma_src), c_double(sigma_psf),
                                           start, weights, wcap, ctypes.byref(W)), "psx_detector_operator_host")
    w = np.frombuffer(weights, dtype=np.float32).reshape(n, wcap)[:, :W.value].copy()
    return np.frombuffer(start, dtype=np.int32).copy(), w


def resize(img, sx, sy):
    """Detector.resize (Detector.py:185-198): identity when sizes match, else s x s block sums, s = Nx//sx."""
    _need(img, torch.float32, "img")
    if img.shape[0] == sx and img.shape[1] == sy:
        return img
    out = torch.empty((sx, sy), dtype=torch.float32, device=img.device)
    check(lib().psx_resize_f32(_ptr(img), img.shape[0], img.shape[1], _ptr(out), int(sx), int(sy), _stream()),
          "psx_resize_f32")
    return out


def poisson(lam, seed):
    """Shot noise (Detector.py:113-115) from a counter-based generator keyed by (seed, pixel)."""
    _need(lam, torch.float32, "lam")
    out = torch.empty_like(lam)
    check(lib().psx_poisson_f32(_ptr(lam), _ptr(out), lam.numel(), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _stream()),
          "psx_poisson_f32")
    return out


def poisson_key(seed, pointNum=0, ibin=0, kind=0):
    """64-bit generator key of one detector image: a hash of WHAT is drawn -- the user's seed, the membrane position, the
    energy bin and the image kind (0 sample, 1 reference, 2 propagation, 3 white) -- so the noise of an image does not
    depend on call order or on how the positions are sharded over GPUs (splitmix64 finaliser per field)."""
    m = (1 << 64) - 1
    h = 0x9E3779B97F4A7C15
    for v in (int(seed), int(pointNum), int(ibin), int(kind)):
        h = (h ^ (v & m)) & m
        h = (h + 0x9E3779B97F4A7C15) & m
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & m
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & m
        h = h ^ (h >> 31)
    return h


def poisson_multi(imgs, seeds):
    """In-place shot noise on several equally sized images in ONE launch, image i under key seeds[i]."""
    if not imgs:
        return imgs
    if len(imgs) > _lib.PSX_MAX_POISSON or len(seeds) != len(imgs):
        raise PsxError("poisson_multi: 1..%d images with one key each" % _lib.PSX_MAX_POISSON)
    for i, t in enumerate(imgs):
        _need(t, torch.float32, "imgs[%d]" % i, imgs[0].shape)
    sd = (ctypes.c_uint64 * len(imgs))(*[int(v) & (2 ** 64 - 1) for v in seeds])
    check(lib().psx_poisson_multi_f32(_ptrs(imgs), sd, len(imgs), imgs[0].numel(), _stream()), "psx_poisson_multi_f32")
    return imgs


def pack_counts(src, dst, index0, exc, exc_count, overflow):
    """dst (int16 storage, read as uint16) = src as 16-bit photon counts; counts >= 65535 leave the escape code 65535 and
    (index0 + p, count) in the exception table exc (int32 [cap, 2]; exc_count int32 [1] counts them); overflow (int32 [1])
    is raised when src is not all integers in [0, 2^24] or the table is full -- dst is then not to be used."""
    _need(src, torch.float32, "src")
    _need(dst, torch.int16, "dst", src.shape)
    _need(exc, torch.int32, "exc")
    _need(exc_count, torch.int32, "exc_count")
    _need(overflow, torch.int32, "overflow")
    check(lib().psx_pack_counts_u16(_ptr(src), _ptr(dst), src.numel(), int(index0), _ptr(exc), _ptr(exc_count),
                                    exc.numel() // 2, _ptr(overflow), _stream()), "psx_pack_counts_u16")
    return dst


def unpack_counts(src, dst, exc=None, exc_count=None):
    """dst (float32) = the 16-bit counts of src (int16 storage, read as uint16), then the exceptions of pack_counts."""
    _need(src, torch.int16, "src")
    _need(dst, torch.float32, "dst", src.shape)
    cap = 0
    if exc is not None:
        _need(exc, torch.int32, "exc")
        _need(exc_count, torch.int32, "exc_count")
        cap = exc.numel() // 2
    check(lib().psx_unpack_counts_u16(_ptr(src), _ptr(dst), src.numel(), _ptr(exc) if cap else None,
                                      _ptr(exc_count) if cap else None, cap, _stream()), "psx_unpack_counts_u16")
    return dst


def status_scan(img):
    _need(img, torch.float32, "img")
    check(lib().psx_status_scan_f32(_ptr(img), img.numel(), _ptr(status_word(img.device)), _stream()),
          "psx_status_scan_f32")


def _positions(imgs, name, kmin=3):
    """The K images of one side of an LCS call as a list of 2-D tensors: a [K, n, m] tensor, or a sequence of K 2-D tensors
    (e.g. the bin slices S[ibin] of the chains' [nbins, n, m] stacks).  Counts and shapes only: devices come after both
    sides are known, so that the message names the first thing that is wrong."""
    if isinstance(imgs, torch.Tensor):
        if imgs.dim() != 3:
            raise PsxError("%s must be [K, n, m] or a sequence of K [n, m] images; got shape %s" % (name, tuple(imgs.shape)))
        imgs = [imgs[k] for k in range(imgs.shape[0])]
    imgs = list(imgs)
    K = len(imgs)
    if K < kmin or K > _lib.PSX_MAX_LCS:
        raise PsxError("%s: K=%d positions outside [%d, %d]" % (name, K, kmin, _lib.PSX_MAX_LCS))
    for k, t in enumerate(imgs):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise PsxError("%s[%d] must be a 2-D tensor" % (name, k))
        if tuple(t.shape) != tuple(imgs[0].shape):
            raise PsxError("%s[%d] has shape %s, %s[0] %s" % (name, k, tuple(t.shape), name, tuple(imgs[0].shape)))
    return imgs


_NO_MEAN = object()      # _tracker_args: the tracker takes no reference means (None means "compute them")
_COUNT_WORDS = {3: "three", 4: "four", 5: "five"}


def _out_count(out, names):
    if len(out) != len(names):
        raise PsxError("out must hold %s tensors (%s)" % (_COUNT_WORDS[len(names)], ", ".join(names)))


def _tracker_args(sample, reference, kmin, names, out, max_shift=None, window_search=None, mean=_NO_MEAN):
    """The front end of the four speckle trackers (lcs, lcs_df, umpa, umpa_df), the checks in the order their callers document:
    K in [kmin, PSX_MAX_LCS] on both sides (_positions), window / search and the smallest image they allow (UMPA), equal
    counts, the reference means (umpa_df: host-only, so they and the number of out= tensors come before any device
    check), equal shapes, float32 images in HBM on one device, max_shift > 0 or None (LCS), and out= tensors of the n x m
    shape (`names`, one per output map), or new ones.  -> (S, R, device, out, mean)"""
    S = _positions(sample, "sample", min(kmin, 3))
    R = _positions(reference, "reference", min(kmin, 3))
    for nm, imgs in (("sample", S), ("reference", R)):
        if len(imgs) < kmin:      # LCS-DF: one position more than LCS, whose own floor _positions has reported
            raise PsxError("%s: K=%d positions outside [%d, %d]: dark field has four unknowns" % (nm, len(imgs), kmin, _lib.PSX_MAX_LCS))
    if window_search is not None:
        for nm, v, cap in zip(("window", "search"), window_search, (_lib.PSX_MAX_UMPA_WINDOW, _lib.PSX_MAX_UMPA_SEARCH)):
            if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= cap:
                raise PsxError("%s must be an integer in [1, %d], got %r" % (nm, cap, v))
        least = 2 * (int(window_search[0]) + int(window_search[1])) + 1
        if S[0].shape[0] < least or S[0].shape[1] < least:
            raise PsxError("images %dx%d smaller than %dx%d = 2*(window+search)+1" % (tuple(S[0].shape) + (least, least)))
    K = len(S)
    if K != len(R):
        raise PsxError("sample has %d positions, reference %d" % (K, len(R)))
    if mean is not _NO_MEAN:
        if mean is not None:
            try:
                mean = [float(v) for v in mean]
            except (TypeError, ValueError):
                raise PsxError("mean must be a sequence of %d finite floats, got %r" % (K, mean))
            if len(mean) != K:
                raise PsxError("mean must hold one value per position (%d), got %d" % (K, len(mean)))
            if not all(math.isfinite(v) for v in mean):
                raise PsxError("mean must be finite, got %r" % (mean,))
        if out is not None:
            out = tuple(out)
            _out_count(out, names)
    shape = tuple(S[0].shape)
    if tuple(R[0].shape) != shape:
        raise PsxError("reference images have shape %s, sample images %s" % (tuple(R[0].shape), shape))
    if shape[0] < 3 or shape[1] < 3:
        raise PsxError("images %dx%d smaller than 3x3" % shape)
    dev = S[0].device
    for nm, imgs in (("sample", S), ("reference", R)):
        for k, t in enumerate(imgs):
            _need(t, torch.float32, "%s[%d]" % (nm, k))
            _on(t, "%s[%d]" % (nm, k), dev, "sample[0]")
    if max_shift is not None and not float(max_shift) > 0.0:
        raise PsxError("max_shift must be > 0 pixels (None: no clamp), got %r" % (max_shift,))
    if out is None:
        out = tuple(torch.empty(shape, dtype=torch.float32, device=dev) for _ in names)
    else:
        out = tuple(out)
        _out_count(out, names)
        for nm, t in zip(names, out):
            _need(t, torch.float32, "out " + nm, shape)
            _on(t, "out " + nm, dev, "the images")
    return S, R, dev, out, mean


def lcs(sample, reference, max_shift=None, out=None):
    """LCS speckle tracking of one energy bin (psx_lcs_f32): K in [3, PSX_MAX_LCS] sample / reference pairs of n x m float32
    images in HBM -> (transmission, dx, dy), n x m float32.  dx is the displacement along axis 0, dy along axis 1, in pixels,
    with the sign of the chain's Dxreal / Dyreal.  max_shift (pixels, > 0) clamps dx and dy; None: no clamp.  out: three
    caller-owned n x m float32 tensors (transmission, dx, dy) to write into."""
    S, R, dev, out, _ = _tracker_args(sample, reference, 3, ("transmission", "dx", "dy"), out, max_shift=max_shift)
    with torch.cuda.device(dev):
        check(lib().psx_lcs_f32(_ptrs(S), _ptrs(R), len(S), *S[0].shape, c_float(float(max_shift or 0)), *map(_ptr, out), _stream()),
              "psx_lcs_f32")
    return out


def lcs_df(sample, reference, max_shift=None, out=None):
    """LCS-DF speckle tracking of one energy bin (psx_lcs_df_f32): ops.lcs with a dark-field column, the 5-point Laplacian of
    each reference image (the diffusion term of the X-ray Fokker-Planck model).  K in [4, PSX_MAX_LCS] sample / reference
    pairs in the forms ops.lcs takes -> (transmission, dx, dy, df), n x m float32.  dx, dy as ops.lcs (max_shift clamps these
    two only); df is the diffusion coefficient in detector pixels^2 (a Gaussian blur of per-axis variance s^2 gives
    df = s^2/2), not clamped.  out: four caller-owned n x m float32 tensors (transmission, dx, dy, df) to write into."""
    S, R, dev, out, _ = _tracker_args(sample, reference, 4, ("transmission", "dx", "dy", "df"), out, max_shift=max_shift)
    with torch.cuda.device(dev):
        check(lib().psx_lcs_df_f32(_ptrs(S), _ptrs(R), len(S), *S[0].shape, c_float(float(max_shift or 0)), *map(_ptr, out), _stream()),
              "psx_lcs_df_f32")
    return out


def umpa(sample, reference, window=2, search=3, out=None):
    """UMPA windowed speckle tracking of one energy bin (psx_umpa_f32): K in [1, PSX_MAX_LCS] sample / reference pairs in the
    forms ops.lcs takes -> (transmission, dx, dy, residual), n x m float32.  Per interior pixel, the integer shift u = (a, b),
    |a|, |b| <= search, that minimises the float64 least-squares cost of S_k(q) ~ T*R_k(q - u) over a uniform
    (2*window+1)^2 window (no Hamming taper) and all K positions, refined per axis by a parabola through the neighbouring
    costs; dx along axis 0, dy along axis 1, the sign of ops.lcs.  residual = cost/sum S^2 at the minimum.  Pixels closer
    than window+search to a border are exactly (1, 0, 0, 0).  window in [1, PSX_MAX_UMPA_WINDOW], search in
    [1, PSX_MAX_UMPA_SEARCH], n, m >= 2*(window+search)+1.  out: four caller-owned n x m float32 tensors to write into."""
    S, R, dev, out, _ = _tracker_args(sample, reference, 1, ("transmission", "dx", "dy", "residual"), out,
                                      window_search=(window, search))
    with torch.cuda.device(dev):
        check(lib().psx_umpa_f32(_ptrs(S), _ptrs(R), len(S), *S[0].shape, int(window), int(search), *map(_ptr, out), _stream()),
              "psx_umpa_f32")
    return out


def umpa_df(sample, reference, window=2, search=3, mean=None, out=None):
    """UMPA with its dark-field term (psx_umpa_df_f32): ops.umpa under the model S_k(q) ~ T*[mu_k + V*(R_k(q - u) - mu_k)], mu_k
    the mean of reference frame k -> (transmission, dx, dy, visibility, residual), n x m float32.  V is the ratio of the
    speckle visibility behind the sample to that of the reference: 1 where nothing scatters, below 1 where the sample
    blurs the speckle.  It is not clamped (noise and model error give values above 1 or below 0) and it is NOT converted
    to a scattering angle: that depends on the speckle's spectrum.  Border-band and fallback pixels are exactly
    (1, 0, 0, 1, 0).  mean: K finite floats, the mu_k; None computes each reference frame's mean in float64 on the device
    and copies the K values to the host, which SYNCHRONISES the stream -- pass the means to stay asynchronous.  Everything
    else (window, search, sizes, input forms) as ops.umpa.  out: five caller-owned n x m float32 tensors to write into."""
    S, R, dev, out, mean = _tracker_args(sample, reference, 1, ("transmission", "dx", "dy", "visibility", "residual"), out,
                                         window_search=(window, search), mean=mean)
    with torch.cuda.device(dev):
        if mean is None:
            mean = torch.stack([t.mean(dtype=torch.float64) for t in R]).tolist()      # one copy to the host: synchronises
        check(lib().psx_umpa_df_f32(_ptrs(S), _ptrs(R), (c_double * len(S))(*mean), len(S), *S[0].shape, int(window), int(search),
                                    *map(_ptr, out), _stream()), "psx_umpa_df_f32")
    return out


class IntegratePlan(_Plan):
    """psx_integrate_plan for one n x m grid: Frankot-Chellappa integration of a gradient field with mirror extension
    (rocFFT on the 2n x 2m complex64 grid the plan owns; `bytes` reports it with rocFFT's work buffer)."""
    _destroy = "psx_integrate_plan_destroy"

    def __init__(self, n, m, device=None):
        self.n, self.m = int(n), int(m)
        self._create(device, "psx_integrate_plan_create", self.n, self.m)
        self.bytes = lib().psx_integrate_plan_bytes(self._h)

    def integrate(self, gx, gy, scale=1.0, out=None):
        """phi (n x m float32, radians, zero mean over the extension) whose gradient is scale*(gx, gy), in radians per pixel
        along axis 0 / axis 1.  Calls on one plan are ordered on the current stream (they share its buffer)."""
        shape = (self.n, self.m)
        _need(gx, torch.float32, "gx", shape)
        _need(gy, torch.float32, "gy", shape)
        _on(gx, "gx", self.device)
        _on(gy, "gy", self.device)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            _need(out, torch.float32, "out", shape)
        with torch.cuda.device(self.device):
            check(lib().psx_integrate_f32(self._h, _ptr(gx), _ptr(gy), c_double(scale), _ptr(out), _stream()),
                  "psx_integrate_f32")
        return out

    def paganin(self, images, whites, alpha, mu, out=None):
        """ops.paganin on this plan."""
        return paganin(images, whites, alpha, mu, self, out=out)


def _image_list(imgs, name, B=None):
    """B images as a list of 2-D tensors from a [B, n, m] tensor or a sequence of B [n, m] tensors (ops.lcs's two forms);
    entries of a sequence may be None.  Counts only: dtypes, shapes and devices are the caller's to check."""
    if isinstance(imgs, torch.Tensor):
        if imgs.dim() != 3:
            raise PsxError("%s must be [B, n, m] or a sequence of B [n, m] images; got shape %s" % (name, tuple(imgs.shape)))
        imgs = [imgs[b] for b in range(imgs.shape[0])]
    imgs = list(imgs)
    if B is None and not 1 <= len(imgs) <= _lib.PSX_MAX_PAGANIN:
        raise PsxError("%s: B=%d images outside [1, %d]" % (name, len(imgs), _lib.PSX_MAX_PAGANIN))
    if B is not None and len(imgs) != B:
        raise PsxError("%s holds %d images, images %d" % (name, len(imgs), B))
    return imgs


def _per_image(v, name, B):
    """A scalar, or a sequence of B of them -> B floats."""
    try:
        v = [float(v)] * B if not hasattr(v, "__len__") else [float(x) for x in v]
    except (TypeError, ValueError):
        raise PsxError("%s must be a number or a sequence of %d numbers, got %r" % (name, B, v))
    if len(v) != B:
        raise PsxError("%s must hold one value per image (%d), got %d" % (name, B, len(v)))
    return v


def paganin(images, whites, alpha, mu, plan, out=None):
    """Paganin's single-material phase retrieval of B propagation images (psx_paganin_f32; the contract is in
    include/paresis_hip.h): images, a [B, n, m] float32 tensor in HBM or a sequence of B n x m ones (ops.lcs's input forms),
    B in [1, PSX_MAX_PAGANIN]; whites, the flat fields in the same forms, None for none (entries of a sequence may be None);
    alpha (>= 0, detector px^2) and mu (> 0, 1/m), one number for all images or B of them; plan, an IntegratePlan of the
    images' shape, whose buffer and transforms the call uses -> (contact, thickness), two [B, n, m] float32 tensors:
    contact = exp(-mu*t) as retrieved, thickness = t in metres.  out: (contact, thickness) to write into, each a
    [B, n, m] tensor, a sequence of B n x m tensors, or None for a map that is not wanted (not both); they are returned as
    given.  Two images share one transform; calls on one plan are ordered on the current stream."""
    I = _image_list(images, "images")
    B = len(I)
    W = [None] * B if whites is None else _image_list(whites, "whites", B)
    alpha, mu = _per_image(alpha, "alpha", B), _per_image(mu, "mu", B)
    for b in range(B):
        if not (math.isfinite(alpha[b]) and alpha[b] >= 0.0):
            raise PsxError("alpha must be finite and >= 0, got %r" % alpha[b])
        if not (math.isfinite(mu[b]) and mu[b] > 0.0):
            raise PsxError("mu must be finite and > 0, got %r" % mu[b])
    if not isinstance(plan, IntegratePlan):
        raise PsxError("plan must be an ops.IntegratePlan, got %r" % type(plan))
    shape = (plan.n, plan.m)
    for nm, imgs in (("images", I), ("whites", W)):
        for b, t in enumerate(imgs):
            if t is None and nm == "whites":
                continue
            _need(t, torch.float32, "%s[%d]" % (nm, b), shape)
            _on(t, "%s[%d]" % (nm, b), plan.device)
    if out is None:
        out = tuple(torch.empty((B,) + shape, dtype=torch.float32, device=plan.device) for _ in range(2))
    else:
        out = tuple(out)
        if len(out) != 2:
            raise PsxError("out must hold two entries (contact, thickness), either of which may be None")
        if out[0] is None and out[1] is None:
            raise PsxError("out asks for neither contact nor thickness")
    lists = []
    for nm, o in zip(("contact", "thickness"), out):
        if o is None:
            lists.append(None)
            continue
        lst = _image_list(o, "out " + nm, B)
        for b, t in enumerate(lst):
            _need(t, torch.float32, "out %s[%d]" % (nm, b), shape)
            _on(t, "out %s[%d]" % (nm, b), plan.device)
        lists.append(lst)
    with torch.cuda.device(plan.device):
        check(lib().psx_paganin_f32(plan._h, B, _ptrs(I), None if whites is None else _ptrs(W), (c_double * B)(*alpha),
                                    (c_double * B)(*mu), None if lists[0] is None else _ptrs(lists[0]),
                                    None if lists[1] is None else _ptrs(lists[1]), _stream()), "psx_paganin_f32")
    return out


# --------------------------------------------------------------------------------------- spectral material decomposition
def decompose(logT, bin_size, w, a, v, G, iterations=12, tol=1e-13, out=None):
    """Projection-domain material decomposition of B energy bins (psx_decompose_f32; the contract is in
    include/paresis_hip.h): logT, a [B, ...] float32 tensor in HBM or a sequence of B equal-shaped ones, L_b = -ln of bin
    b's transmission; bin_size, the B numbers of energies per bin (their sum E <= PSX_DECOMP_MAX_ENERGIES); w, the E
    weights bin after bin; a, the [M][E] attenuation coefficients in 1/m (M <= B, M <= PSX_DECOMP_MAX_MAT); v, the B bin
    weights (> 0); G, the M x B matrix of the linearised start -- host numbers all (paresis_amd.spectral builds them)
    -> (thickness [M, ...] in metres, residual [...], steps [...]), float32.  out: three such tensors to write into."""
    L = [logT[b] for b in range(logT.shape[0])] if isinstance(logT, torch.Tensor) else list(logT)
    B = len(L)
    if not 1 <= B <= _lib.PSX_DECOMP_MAX_BINS:
        raise PsxError("logT: B=%d bins outside [1, %d]" % (B, _lib.PSX_DECOMP_MAX_BINS))
    bin_size = [int(s) for s in bin_size]
    E = sum(bin_size)
    if len(bin_size) != B or min(bin_size) < 1 or E > _lib.PSX_DECOMP_MAX_ENERGIES:
        raise PsxError("bin_size must hold %d counts >= 1 summing to %d at most, got %r" % (B, _lib.PSX_DECOMP_MAX_ENERGIES, bin_size))
    w = [float(x) for x in w]
    a = [[float(x) for x in row] for row in a]
    v = [float(x) for x in v]
    G = [[float(x) for x in row] for row in G]
    M = len(a)
    if not 1 <= M <= min(B, _lib.PSX_DECOMP_MAX_MAT):
        raise PsxError("a: M=%d materials outside [1, %d] (B=%d bins)" % (M, min(B, _lib.PSX_DECOMP_MAX_MAT), B))
    if len(w) != E or any(len(row) != E for row in a):
        raise PsxError("w and every row of a must hold %d values (the sum of bin_size)" % E)
    if len(v) != B or not all(math.isfinite(x) and x > 0.0 for x in v):
        raise PsxError("v must hold %d finite weights > 0, got %r" % (B, v))
    if len(G) != M or any(len(row) != B for row in G):
        raise PsxError("G must be %d x %d" % (M, B))
    if isinstance(iterations, bool) or int(iterations) != iterations or int(iterations) < 1:
        raise PsxError("iterations must be an integer >= 1, got %r" % (iterations,))
    if not (math.isfinite(float(tol)) and float(tol) >= 0.0):
        raise PsxError("tol must be finite and >= 0, got %r" % (tol,))
    shape = tuple(L[0].shape) if isinstance(L[0], torch.Tensor) else None
    for b, t in enumerate(L):
        _need(t, torch.float32, "logT[%d]" % b, shape)
        _on(t, "logT[%d]" % b, L[0].device, "logT[0]")
    n = L[0].numel()
    if n < 1:
        raise PsxError("logT holds no pixel: shape %s" % (shape,))
    dev = L[0].device
    if out is None:
        out = (torch.empty((M,) + shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev),
               torch.empty(shape, dtype=torch.float32, device=dev))
    else:
        out = tuple(out)
        _out_count(out, ("thickness", "residual", "steps"))
        for nm, t, sh in zip(("thickness", "residual", "steps"), out, ((M,) + shape, shape, shape)):
            _need(t, torch.float32, "out " + nm, sh)
            _on(t, "out " + nm, dev, "logT")
    flat = [x for row in a for x in row]
    with torch.cuda.device(dev):
        check(lib().psx_decompose_f32(_ptrs(L), B, (c_int * B)(*bin_size), (c_double * E)(*w), (c_double * (M * E))(*flat), M,
                                      (c_double * B)(*v), (c_double * (M * B))(*[x for row in G for x in row]), int(iterations),
                                      c_double(float(tol)), n, _ptrs([out[0][m] for m in range(M)]), _ptr(out[1]), _ptr(out[2]),
                                      _stream()), "psx_decompose_f32")
    return out


# --------------------------------------------------------------------------------------- filtered back-projection
class FbpPlan(_Plan):
    """psx_fbp_plan (the contract is in include/paresis_hip.h): parallel-beam filtered back-projection of [A, n, m] sinograms
    at the A angles `theta_deg` (degrees, any values) about detector column `center` (None: m // 2, radon's), with filter
    'ramp', 'hann' or 'none' -- or 'hilbert' / 'hilbert-hann' for a DIFFERENTIAL sinogram, d/d(column) per detector pixel
    (_lib.FBP_DIFFERENTIAL_FILTERS) --, onto [n, m, m] volumes, zero outside the inscribed circle when `circle`.  The plan owns the
    angle and filter tables, the rocFFT plans and the filtered sinogram of max_rows detector rows (0: the library's
    choice), so n may differ from call to call; `bytes` reports them."""
    _destroy = "psx_fbp_plan_destroy"

    def __init__(self, theta_deg, m, center=None, filter="ramp", circle=True, max_rows=0, device=None):
        try:
            theta = [float(v) for v in theta_deg]
        except (TypeError, ValueError):
            raise PsxError("theta_deg must be a sequence of angles in degrees, got %r" % (theta_deg,))
        filters = dict(_lib.FBP_FILTERS, **_lib.FBP_DIFFERENTIAL_FILTERS)
        if filter not in filters:
            raise PsxError("filter must be one of %s, got %r" % (sorted(filters), filter))
        self.theta, self.m, self.filter, self.circle = tuple(theta), int(m), filter, bool(circle)
        self.center = float(self.m // 2 if center is None else center)
        self._create(device, "psx_fbp_plan_create", len(theta), self.m, (c_double * len(theta))(*theta), c_double(self.center),
                     filters[filter], int(self.circle), int(max_rows))
        self.bytes = lib().psx_fbp_plan_bytes(self._h)

    def fbp(self, sino, out=None):
        """ops.fbp on this plan."""
        return fbp(sino, self, out=out)

    def project(self, vol, out=None):
        """ops.fbp_project on this plan."""
        return fbp_project(vol, self, out=out)

    def adjoint(self, sino, out=None):
        """ops.fbp_adjoint on this plan."""
        return fbp_adjoint(sino, self, out=out)


def fbp(sino, plan, out=None):
    """Filtered back-projection (psx_fbp_f32): sino, an [A, n, m] float32 tensor in HBM (A, m the plan's; any n >= 1) ->
    the [n, m, m] float32 volume, vol[r] the slice of detector row r.  out: a caller-owned [n, m, m] float32 tensor to write
    into.  Calls on one plan are ordered on the current stream (they share its buffer)."""
    return _fbp_call("psx_fbp_f32", plan, sino, "sino", out, False)


def _fbp_rows(plan, x, what, volume):
    """n of x, a float32 tensor in HBM of a shape the plan takes: a volume [n, m, m] or a sinogram [A, n, m]."""
    A, m = len(plan.theta), plan.m
    _need(x, torch.float32, what)
    if volume:
        ok, axis, takes = x.dim() == 3 and x.shape[1] == m and x.shape[2] == m, 0, "[n >= 1, %d, %d]" % (m, m)
    else:
        ok, axis, takes = x.dim() == 3 and x.shape[0] == A and x.shape[2] == m, 1, "[%d, n >= 1, %d]" % (A, m)
    if not ok or x.shape[axis] < 1:
        raise PsxError("%s has shape %s, the plan takes %s" % (what, tuple(x.shape), takes))
    return int(x.shape[axis])


def _fbp_call(name, plan, x, what, out, to_sino):
    """One of the plan's three operators: x is a sinogram [A, n, m] (-> a volume [n, m, m]) or, with to_sino, a volume
    (-> a sinogram).  Every check comes before the device is touched."""
    if not isinstance(plan, FbpPlan):
        raise PsxError("plan must be an ops.FbpPlan, got %r" % type(plan))
    n = _fbp_rows(plan, x, what, to_sino)
    shape = (len(plan.theta), n, plan.m) if to_sino else (n, plan.m, plan.m)
    _on(x, what, plan.device)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=plan.device)
    else:
        _need(out, torch.float32, "out", shape)
        _on(out, "out", plan.device)
    with torch.cuda.device(plan.device):
        check(getattr(lib(), name)(plan._h, _ptr(x), n, _ptr(out), _stream()), name)
    return out


def fbp_project(vol, plan, out=None):
    """The plan's forward projector (psx_fbp_project_f32; the contract is in include/paresis_hip.h): vol, an [n, m, m]
    float32 tensor in HBM -> the [A, n, m] float32 sinogram B^T vol, the exact transpose of the back-projector's
    interpolation (the lit voxels only when the plan has `circle`), unscaled: line integrals in pixels, what ops.fbp
    consumes.  The plan's filter is ignored.  Deterministic: two calls return the same bits.  out: a caller-owned
    [A, n, m] float32 tensor to write into."""
    return _fbp_call("psx_fbp_project_f32", plan, vol, "vol", out, True)


def fbp_adjoint(sino, plan, out=None):
    """The plan's back-projector without filter and scale (psx_fbp_adjoint_f32): sino [A, n, m] -> B sino, [n, m, m]; on a
    'none' plan ops.fbp is float32(pi/(2A)) times it.  The plan's filter is ignored.  out: a caller-owned [n, m, m]
    float32 tensor.  Calls on one plan are ordered on the current stream (they share its buffer)."""
    return _fbp_call("psx_fbp_adjoint_f32", plan, sino, "sino", out, False)


def fbp_tv_step(plan, weight, nonneg, u, c, x, xbar_in, xbar_out, px_in, py_in, px_out, py_out):
    """The voxel step of total-variation reconstruction on the plan's projector pair (psx_fbp_tv_step_f32; the contract is
    in include/paresis_hip.h), one launch for the n slices: the TV dual (px_in, py_in) takes its step of 1/2 along the
    forward differences of xbar_in and is projected onto |p| <= weight -> (px_out, py_out); x, in place, takes its step
    x - tau*(u + grad^T p'), tau = 1/(c + the voxel's number of active differences), and is clamped at 0 with nonneg;
    xbar_out = 2 x' - x.  u = B y and c = B 1 (ops.fbp_adjoint).  All nine are [n, m, m] float32 tensors in HBM on the
    plan's device, m the plan's; an _out tensor shares no storage with any other (neighbouring tiles read the _in ones).
    Every check comes before the device is touched.  -> (x, xbar_out, px_out, py_out)."""
    if not isinstance(plan, FbpPlan):
        raise PsxError("plan must be an ops.FbpPlan, got %r" % type(plan))
    try:
        weight = float(weight)
    except (TypeError, ValueError):
        raise PsxError("weight must be a number, got %r" % (weight,))
    if not (weight >= 0.0 and weight != float("inf")):
        raise PsxError("weight must be finite and >= 0, got %r" % (weight,))
    shape = (_fbp_rows(plan, x, "x", True), plan.m, plan.m)
    named = (("u", u), ("c", c), ("x", x), ("xbar_in", xbar_in), ("px_in", px_in), ("py_in", py_in),
             ("xbar_out", xbar_out), ("px_out", px_out), ("py_out", py_out))
    for nm, t in named:
        _need(t, torch.float32, nm, shape)
        _on(t, nm, plan.device)
    for k, (nm, t) in enumerate(named[6:]):
        for other, o in named[:6 + k]:
            if t.data_ptr() == o.data_ptr():
                raise PsxError("%s shares its storage with %s: the step reads its neighbours' inputs" % (nm, other))
    with torch.cuda.device(plan.device):
        check(lib().psx_fbp_tv_step_f32(plan._h, shape[0], c_double(weight), int(bool(nonneg)), _ptr(u), _ptr(c), _ptr(x),
                                        _ptr(xbar_in), _ptr(xbar_out), _ptr(px_in), _ptr(py_in), _ptr(px_out), _ptr(py_out),
                                        _stream()), "psx_fbp_tv_step_f32")
    return x, xbar_out, px_out, py_out

# ------------------------------------------------------------------------------------------------------ FDK
class FdkPlan(_Plan):
    """psx_fdk_plan (the contract is in include/paresis_hip.h): FDK reconstruction of [A, n, m] cone-beam sinograms on the
    virtual detector through the rotation axis, taken at the A angles `theta_deg` (degrees, a full turn) from a point source
    `dso` voxels (m <= dso <= 1e30) from the axis, about detector column `center` (None: m // 2) and optical-axis row
    `vcenter` (None: (n - 1)/2; any real), with filter 'ramp', 'hann' or 'none', onto [n, m, m] volumes.  The plan owns the
    filtered sinogram of all n rows besides a parallel plan's tables; `bytes` reports them."""
    _destroy = "psx_fdk_plan_destroy"

    def __init__(self, theta_deg, n, m, dso, center=None, vcenter=None, filter="ramp", circle=True, device=None):
        try:
            theta = [float(v) for v in theta_deg]
        except (TypeError, ValueError):
            raise PsxError("theta_deg must be a sequence of angles in degrees, got %r" % (theta_deg,))
        if filter not in _lib.FBP_FILTERS:
            raise PsxError("filter must be one of %s, got %r" % (sorted(_lib.FBP_FILTERS), filter))
        self.theta, self.n, self.m, self.filter, self.circle = tuple(theta), int(n), int(m), filter, bool(circle)
        self.dso = float(dso)
        self.center = float(self.m // 2 if center is None else center)
        self.vcenter = float((self.n - 1) / 2.0 if vcenter is None else vcenter)
        self._create(device, "psx_fdk_plan_create", len(theta), self.n, self.m, (c_double * len(theta))(*theta),
                     c_double(self.center), c_double(self.vcenter), c_double(self.dso), _lib.FBP_FILTERS[filter],
                     int(self.circle))
        self.bytes = lib().psx_fdk_plan_bytes(self._h)

    def fdk(self, sino, out=None):
        """ops.fdk on this plan."""
        return fdk(sino, self, out=out)


def fdk(sino, plan, out=None):
    """FDK reconstruction (psx_fdk_f32): sino, an [A, n, m] float32 tensor in HBM (A, n, m the plan's) -> the [n, m, m]
    float32 volume, slice Z at height Z - vcenter.  out: a caller-owned [n, m, m] float32 tensor to write into.
    Deterministic; calls on one plan are ordered on the current stream (they share its buffers)."""
    if not isinstance(plan, FdkPlan):
        raise PsxError("plan must be an ops.FdkPlan, got %r" % type(plan))
    _need(sino, torch.float32, "sino", (len(plan.theta), plan.n, plan.m))
    _on(sino, "sino", plan.device)
    shape = (plan.n, plan.m, plan.m)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=plan.device)
    else:
        _need(out, torch.float32, "out", shape)
        _on(out, "out", plan.device)
    with torch.cuda.device(plan.device):
        check(lib().psx_fdk_f32(plan._h, _ptr(sino), _ptr(out), _stream()), "psx_fdk_f32")
    return out


class VolumeDesc(ctypes.Structure):
    """psx_volume_desc (include/paresis_hip.h)."""
    _fields_ = [("n", c_int), ("m", c_int), ("nmat", c_int), ("dimX", c_int), ("dimY", c_int),
                ("cos_a", c_double), ("sin_a", c_double), ("off_x", c_double), ("off_y", c_double),
                ("s", c_double), ("voxel_m", c_double), ("box", c_void_p)]


def volume_desc(n, m, nmat, angle_deg, dims, scale, voxel_m, box=None):
    """The kernel's descriptor: the scalars of the contract by the phantom's own expressions (phantom_scalars: skimage
    radon's inverse map about c = m // 2)."""
    import numpy as np
    theta = np.deg2rad(np.asarray([angle_deg], dtype=np.float64))[0]
    cos_a, sin_a = np.cos(theta), np.sin(theta)
    center = int(m) // 2
    d = VolumeDesc()
    d.n, d.m, d.nmat, d.dimX, d.dimY = int(n), int(m), int(nmat), int(dims[0]), int(dims[1])
    d.cos_a, d.sin_a = float(cos_a), float(sin_a)
    d.off_x, d.off_y = float(-center * (cos_a + sin_a - 1)), float(-center * (cos_a - sin_a - 1))
    d.s, d.voxel_m = float(scale), float(voxel_m)
    d.box = None if box is None else box.data_ptr()
    return d


def volume_project(labels, nmat, angle_deg, dims, scale, voxel_m, want_lines=False, box=None, dso=None):
    """The thickness maps of a labelled voxel volume at one angle (psx_volume_project_u8; the contract is in
    include/paresis_hip.h): labels [n, m, m] uint8 in HBM, label k + 1 = material k < nmat -> geom [nmat, dimX, dimY]
    float32 (metres) on the dims = (dimX, dimY) study grid, whose pixel is `scale` voxels of voxel_m metres; with want_lines
    also the float64 line integrals in voxels, (geom, lines).  box: an [n, 4] int32 tensor of each slice's occupied
    (row0, row1, col0, col1), half-open, which only spares work; None: the whole slice.  The kernel applies no circle mask
    and ignores labels above nmat: Samples.getVolumeFromFile.check_volume is the loader's check.
    dso: None for the parallel beam; otherwise the distance in voxels, m <= dso <= 1e30, from a point source to the rotation
    axis, and the projection is the divergent one (psx_volume_project_cone_u8): the study grid is the virtual detector
    through the axis, the lines are path lengths in voxels along the diverging rays."""
    _need(labels, torch.uint8, "labels")
    if labels.dim() != 3 or labels.shape[1] != labels.shape[2]:
        raise PsxError("labels must be [n, m, m], got shape %s" % (tuple(labels.shape),))
    n, m = int(labels.shape[0]), int(labels.shape[1])
    if box is not None:
        _need(box, torch.int32, "box", (n, 4))
        _on(box, "box", labels.device, "labels")
    d = volume_desc(n, m, nmat, angle_deg, dims, scale, voxel_m, box)
    if d.nmat < 1 or d.dimX < 1 or d.dimY < 1:
        raise PsxError("volume_project: nmat=%d, study grid %d x %d" % (d.nmat, d.dimX, d.dimY))
    with torch.cuda.device(labels.device):
        geom = torch.empty((d.nmat, d.dimX, d.dimY), dtype=torch.float32, device=labels.device)
        lines = torch.empty((d.nmat, d.dimX, d.dimY), dtype=torch.float64, device=labels.device) if want_lines else None
        if dso is None:
            check(lib().psx_volume_project_u8(ctypes.byref(d), _ptr(labels), _ptr(lines), _ptr(geom), _stream()),
                  "psx_volume_project_u8")
        else:
            check(lib().psx_volume_project_cone_u8(ctypes.byref(d), c_double(float(dso)), _ptr(labels), _ptr(lines), _ptr(geom),
                                                   _stream()), "psx_volume_project_cone_u8")
    return (geom, lines) if want_lines else geom
