"""The three entry points of csrc/membrane.hip -- psx_membrane_f32 (host arrays, tiles binned on the host, float64 sums),
psx_membrane_layer_f32 and psx_membrane_layers_f32 (resident list, fixed-point sums in LDS) -- called through the C ABI on lists
built for the purpose (tests/_membrane_oracle.py) and held, PER PIXEL, to the numpy reference there:

    |gpu(p) - ref(p)| <= 2^-23 |ref(p)| + scale n(p) 2^-36        and        gpu(p) == 0.0f where n(p) = 0

on every pixel the reference does not flag rim-ambiguous (tests/test_membrane_host.py: none in a built list, at most 1e-4 of the
hit pixels in a random one).  The first term is one float32 ulp of the pixel's own value -- half of it the rounding of the store,
the rest for the ~1e-13 of the kernel's square root and the order of the float64 sum --, the second the accumulator's unit of
2^-36 pixel for each of the n(p) chords.  Every case asserts, from psx_membrane_plan_info, that it reaches the staging condition
it is named for."""
import ctypes
from ctypes import c_double, c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

from tests import _membrane_oracle as mo

pytestmark = pytest.mark.gpu

DP = ctypes.POINTER(c_double)
E_ARG = -1                          # PSX_E_ARG


def _lib():
    from paresis_amd._lib import lib
    return lib()


def _dp(a):
    return a.ctypes.data_as(DP)


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ints(v):
    return (c_int * max(1, len(v)))(*[int(a) for a in v])


class Plan:
    def __init__(self, x, y, r):
        from paresis_amd._lib import check
        self.x, self.y, self.r = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, y, r))
        self.h = c_void_p(None)
        check(_lib().psx_membrane_plan_create(_dp(self.x), _dp(self.y), _dp(self.r), len(self.r), ctypes.byref(self.h)), "plan")
        buf = (c_int * len(mo.INFO_FIELDS))()
        assert _lib().psx_membrane_plan_info(self.h, buf, len(buf)) == len(mo.INFO_FIELDS)
        self.info = dict(zip(mo.INFO_FIELDS, (int(v) for v in buf)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib().psx_membrane_plan_destroy(self.h)
        self.h = None


def fresh(c, fill=np.nan):
    return torch.full((c.dimX, c.dimY), fill, dtype=torch.float32, device="cuda")


def run_layers(plan, c, offs, out, accumulate=0, support=None, support_value=0.0):
    from paresis_amd._lib import check
    check(_lib().psx_membrane_layers_f32(plan.h, len(offs), _ints([o[0] for o in offs]), _ints([o[1] for o in offs]), c.dimX, c.dimY,
                                         c.margin, c.margin2, c_double(c.scale), accumulate, c_void_p(out.data_ptr()),
                                         c_void_p(support.data_ptr()) if support is not None else None, c_float(support_value),
                                         _stream()), "psx_membrane_layers_f32")
    torch.cuda.synchronize()
    return out


def run_layer(plan, c, off, out, accumulate=0):
    from paresis_amd._lib import check
    check(_lib().psx_membrane_layer_f32(plan.h, int(off[0]), int(off[1]), c.dimX, c.dimY, c.margin, c.margin2, c_double(c.scale),
                                        accumulate, c_void_p(out.data_ptr()), _stream()), "psx_membrane_layer_f32")
    torch.cuda.synchronize()
    return out


def run_host(c, layers, out, accumulate=0):
    """psx_membrane_f32 on the spheres of the given layers as ONE list (a sum over spheres is a sum over layers of spheres), so
    that every chord of the call is summed in float64 before the single store."""
    from paresis_amd._lib import check
    xf = np.ascontiguousarray(np.concatenate([mo.layer_coords(c, l)[0] for l in layers] or [np.zeros(0)]))
    yf = np.ascontiguousarray(np.concatenate([mo.layer_coords(c, l)[1] for l in layers] or [np.zeros(0)]))
    r = np.ascontiguousarray(np.concatenate([c.r for l in layers] or [np.zeros(0)]))
    check(_lib().psx_membrane_f32(_dp(xf), _dp(yf), _dp(r), len(r), c.dimX, c.dimY, c.margin, c.margin2, c_double(c.scale), accumulate,
                                  c_void_p(out.data_ptr()), _stream()), "psx_membrane_f32")
    torch.cuda.synchronize()
    return out


def held(gpu, ref3, scale, what):
    """Assert the per-pixel bound of the module docstring; returns the worst |error| / bound over the pixels with chords."""
    ref, cnt, amb = ref3
    g = gpu.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(g)), (what, "not finite")
    use = ~amb
    bound = 2.0 ** -23 * np.abs(ref) + scale * cnt * mo.ACC_UNIT
    err = np.abs(g - ref)
    zero = use & (cnt == 0)
    assert np.all(g[zero] == 0.0), (what, "a pixel without a chord is not 0", int((g[zero] != 0).sum()))
    bad = use & (err > bound)
    if bad.any():
        i, j = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0)), err.shape)
        raise AssertionError("%s: %d pixels beyond the bound; worst at (%d, %d): gpu %.9g ref %.17g n %d, error %.3g, bound %.3g"
                             % (what, int(bad.sum()), i, j, g[i, j], ref[i, j], cnt[i, j], err[i, j], bound[i, j]))
    hit = use & (cnt > 0)
    return float((err[hit] / bound[hit]).max()) if hit.any() else 0.0


def expect_staging(name, c, info, st):
    """What a case is named for, from the plan's own account of the build."""
    assert st["kept"] == info["kept"], (name, st, info)
    if name.startswith("row-"):
        count = int(name.split("-")[1])
        assert info["ncx"] == 1 and st["staged"] == st["hits"] == count == len(c.r)      # one job holds them all, all splatted
        assert st["batches"] == -(-count // info["ML_CAP"])
        assert count - info["ML_CAP"] in (-1, 0, 1) or count - 2 * info["ML_CAP"] in (0, 1) or count > 6 * info["ML_CAP"]
    elif name.startswith("jobs-rows"):
        assert len(c.offs) == 1 and st["rows"] > info["ML_SEGS"]                         # one layer, more than a round of jobs
    elif name.startswith("jobs-"):
        jobs = int(name.split("-")[1])
        assert st["jobs"] == jobs == len(c.offs) * st["rows"]
        assert jobs - info["ML_SEGS"] in (-1, 0, 1) or jobs > 2 * info["ML_SEGS"]
    elif name.startswith("layers-"):
        nl = int(name.split("-")[1])
        assert nl == len(c.offs) and st["launches"] == -(-nl // info["ML_MAX"])
        assert nl == 1 or nl - info["ML_MAX"] in (-1, 0, 1) or nl - 2 * info["ML_MAX"] in (0, 1)
    elif name.startswith("random-"):
        assert st["staged"] > info["ML_CAP"] and st["hits"] > info["ML_CAP"]
    elif name == "radius-300":
        assert info["rmax_int"] == 301 > 4 * max(info["MLX"], info["MLY"])
    elif name == "radius-plan-max":
        assert info["rmax_int"] == 1 << 14
    elif name.startswith("radius-tiny"):
        assert info["kept"] == int((c.r > 1e-6).sum()) < len(c.r)                       # the plan leaves the tiny ones out
    elif name == "none-valid":
        assert info["kept"] == 1 and st["hits"] == 0        # one entry is a sphere, outside the admission bound
    elif name == "empty":
        assert info["kept"] == 0 and len(c.r) == 0
    elif name.startswith("admission"):
        assert info["kept"] == len(c.r) - 10                                            # r <= 0 and the non-finite entries
    elif name == "offsets":
        assert st["staged"] > 0


def test_grids_straddle_the_tiles_of_this_build():
    with Plan([1.0], [1.0], [1.0]) as p:
        X, Y = p.info["MLX"], p.info["MLY"]
    assert set(mo.GRIDS) == {(1, 1), (X - 1, Y - 1), (X, Y), (X + 1, Y + 1), (2 * X, 2 * Y), (2 * X + 6, 2 * Y + 2)}
    assert p.info["MC"] == 32 == X                      # the built lists put spheres on multiples of 32: cell and tile corners


@pytest.mark.parametrize("name", list(mo.cases()))
def test_entry_points_against_the_reference(name):
    """All three entry points on one case.  psx_membrane_layers_f32 renders every layer in one call; psx_membrane_f32 gets the
    spheres of all layers as one list; psx_membrane_layer_f32 is held layer by layer to that layer's own reference."""
    c = mo.cases()[name]
    ref = mo.reference(name)
    nl = len(c.offs)
    with Plan(c.x, c.y, c.r) as plan:
        st = mo.staging(plan.info, c)
        expect_staging(name, c, plan.info, st)
        w_layers = held(run_layers(plan, c, c.offs, fresh(c)), ref, c.scale, name + " layers")
        w_layer = max(held(run_layer(plan, c, c.offs[l], fresh(c)), mo.layer_reference(name, l), c.scale, "%s layer %d" % (name, l))
                      for l in range(nl))
    w_host = held(run_host(c, range(nl), fresh(c)), ref, c.scale, name + " host")
    print("%s: %d spheres kept, %d layers, %s; worst error / bound: host %.3f layer %.3f layers %.3f"
          % (name, plan.info["kept"], nl, {k: st[k] for k in ("rows", "jobs", "rounds", "launches", "staged", "hits", "batches")},
             w_host, w_layer, w_layers))


def test_no_layer_stores_zeros():
    c = mo.cases()["grid-33x65"]
    with Plan(c.x, c.y, c.r) as plan:
        out, sup = fresh(c), fresh(c)
        run_layers(plan, c, (), out, support=sup, support_value=0.25)
        assert bool((out == 0).all()) and bool((sup == 0.25).all())


def test_plan_refuses_a_radius_the_accumulator_cannot_hold():
    """2^14 pixels and more: the plan refuses (a chord in 2^-36 pixel no longer fits the rounding offset of the splat), the
    host-binned entry point, which sums in float64, takes it and is right."""
    c = mo.cases()["radius-plan-max"]
    for big in (2.0 ** 14, 2.0 ** 14 + 0.125, 999999.875):
        r = c.r.copy()
        r[0] = big
        h = c_void_p(None)
        x, y = np.ascontiguousarray(c.x), np.ascontiguousarray(c.y)
        assert _lib().psx_membrane_plan_create(_dp(x), _dp(y), _dp(r), len(r), ctypes.byref(h)) == E_ARG and not h.value
        assert b"radius" in _lib().psx_last_error()
        cc = c._replace(r=r)
        xf, yf, _ = mo.layer_coords(cc, 0)
        ref = mo.splat(xf, yf, r, c.dimX, c.dimY, c.margin, c.margin2, c.scale)
        assert not ref[2].any() and ref[1].min() >= 1
        held(run_host(cc, [0], fresh(c)), ref, c.scale, "host r = %r" % big)
    r = c.r.copy()
    r[1] = 0.0                                           # what is not kept is not measured
    r[0] = np.inf
    with Plan(c.x, c.y, r) as plan:
        assert plan.info["kept"] == 0


def _old(c, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand((c.dimX, c.dimY), generator=g, dtype=torch.float32) * 3e-5 - 1e-5).cuda()


@pytest.mark.parametrize("name", ["grid-70x130", "grid-64x128", "layers-8", "random-1"])
def test_accumulate_adds_the_same_values_bit_for_bit(name):
    """accumulate = 1 leaves float32(old + v), v being what the same call stores with accumulate = 0; both scales."""
    c = mo.cases()[name]
    assert c.scale == (1.0 if name in ("grid-64x128", "layers-8") else mo.PIX_SCALE) and len(c.offs) <= 8
    old = _old(c, 7) if c.scale != 1.0 else _old(c, 7) * 1e6
    with Plan(c.x, c.y, c.r) as plan:
        assert len(c.offs) <= plan.info["ML_MAX"]
        v = run_layers(plan, c, c.offs, fresh(c))
        assert torch.equal(run_layers(plan, c, c.offs, old.clone(), accumulate=1), old + v)
        v = run_layer(plan, c, c.offs[0], fresh(c))
        assert torch.equal(run_layer(plan, c, c.offs[0], old.clone(), accumulate=1), old + v)
    v = run_host(c, range(len(c.offs)), fresh(c))
    assert float(v.max()) > 0 and torch.equal(run_host(c, range(len(c.offs)), old.clone(), accumulate=1), old + v)


@pytest.mark.parametrize("name", ["layers-1", "layers-9", "layers-17"])
def test_support_map_is_filled_once(name):
    """...by the first launch, also when the layers take several; a null support changes nothing of the membrane."""
    c = mo.cases()[name]
    with Plan(c.x, c.y, c.r) as plan:
        sup = fresh(c)
        a = run_layers(plan, c, c.offs, fresh(c), support=sup, support_value=0.006)
        assert bool((sup == np.float32(0.006)).all())
        b = run_layers(plan, c, c.offs, fresh(c))
        assert torch.equal(a, b)
        # accumulate = 1 over several launches adds to the caller's map, and the support is still written, not added to
        old = _old(c, 3) * 1e6
        sup = fresh(c, 1.0)
        got = run_layers(plan, c, c.offs, old.clone(), accumulate=1, support=sup, support_value=0.006)
        assert bool((sup == np.float32(0.006)).all())
        want = old.clone()
        M = plan.info["ML_MAX"]
        for l0 in range(0, len(c.offs), M):
            want = want + run_layers(plan, c, c.offs[l0:l0 + M], fresh(c))
        assert torch.equal(got, want)


def test_order_independence_bit_for_bit():
    """The layers kernel sums integers: the same bits from the same call twice, from the list in another order (other cells'
    order, other batches) and from the layers in another order."""
    for name in ("random-1", "row-200", "layers-8", "jobs-18"):
        c = mo.cases()[name]
        with Plan(c.x, c.y, c.r) as plan:
            assert len(c.offs) <= plan.info["ML_MAX"]
            a = run_layers(plan, c, c.offs, fresh(c))
            assert torch.equal(a, run_layers(plan, c, c.offs, fresh(c)))
            for offs in [c.offs[::-1]] + [[c.offs[i] for i in np.random.default_rng(s).permutation(len(c.offs))] for s in (1, 2)]:
                assert sorted(offs) == sorted(c.offs)
                assert torch.equal(a, run_layers(plan, c, offs, fresh(c))), (name, "layers permuted", offs)
        for seed in (1, 2):
            perm = np.random.default_rng(seed).permutation(len(c.r))
            with Plan(c.x[perm], c.y[perm], c.r[perm]) as plan:
                assert torch.equal(a, run_layers(plan, c, c.offs, fresh(c))), (name, "list shuffled", seed)
        assert float(a.max()) > 0


def test_bad_arguments_launch_nothing():
    c = mo.cases()["grid-33x65"]
    L = _lib()
    sentinel = 12345.0
    out = fresh(c, sentinel)
    o, st, sc = c_void_p(out.data_ptr()), _stream(), c_double(1.0)
    x, y, r = (np.ascontiguousarray(v) for v in (c.x, c.y, c.r))
    zero = _ints([0])
    with Plan(c.x, c.y, c.r) as plan:
        h = plan.h
        calls = [
            L.psx_membrane_layers_f32(None, 1, zero, zero, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, None, c_float(0), st),
            L.psx_membrane_layers_f32(h, 1, zero, zero, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, None, None, c_float(0), st),
            L.psx_membrane_layers_f32(h, 1, None, zero, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, None, c_float(0), st),
            L.psx_membrane_layers_f32(h, 1, zero, None, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, None, c_float(0), st),
            L.psx_membrane_layers_f32(h, -1, zero, zero, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, None, c_float(0), st),
            L.psx_membrane_layers_f32(h, 1, zero, zero, 0, c.dimY, c.margin, c.margin2, sc, 0, o, None, c_float(0), st),
            L.psx_membrane_layers_f32(h, 1, zero, zero, c.dimX, -4, c.margin, c.margin2, sc, 0, o, None, c_float(0), st),
            L.psx_membrane_layers_f32(h, 1, zero, zero, c.dimX, c.dimY, -1, 0, sc, 0, o, None, c_float(0), st),
            L.psx_membrane_layer_f32(None, 0, 0, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_layer_f32(h, 0, 0, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, None, st),
            L.psx_membrane_layer_f32(h, 0, 0, -1, c.dimY, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_layer_f32(h, 0, 0, c.dimX, 0, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_layer_f32(h, 0, 0, c.dimX, c.dimY, -2, -1, sc, 0, o, st),
            L.psx_membrane_f32(_dp(x), _dp(y), _dp(r), len(r), c.dimX, c.dimY, c.margin, c.margin2, sc, 0, None, st),
            L.psx_membrane_f32(None, _dp(y), _dp(r), len(r), c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_f32(_dp(x), None, _dp(r), len(r), c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_f32(_dp(x), _dp(y), None, len(r), c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_f32(_dp(x), _dp(y), _dp(r), -1, c.dimX, c.dimY, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_f32(_dp(x), _dp(y), _dp(r), len(r), 0, c.dimY, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_f32(_dp(x), _dp(y), _dp(r), len(r), c.dimX, -1, c.margin, c.margin2, sc, 0, o, st),
            L.psx_membrane_f32(_dp(x), _dp(y), _dp(r), len(r), c.dimX, c.dimY, -1, 0, sc, 0, o, st),
            L.psx_membrane_plan_create(_dp(x), _dp(y), _dp(r), len(r), None),
        ]
        hh = c_void_p(None)
        calls += [L.psx_membrane_plan_create(None, _dp(y), _dp(r), len(r), ctypes.byref(hh)),
                  L.psx_membrane_plan_create(_dp(x), _dp(y), _dp(r), -1, ctypes.byref(hh))]
        assert not hh.value
        torch.cuda.synchronize()
        assert calls == [E_ARG] * len(calls), calls
        assert bool((out == sentinel).all())                   # nothing was launched
        buf = (c_int * 10)(*([-7] * 10))
        assert L.psx_membrane_plan_info(h, None, 10) == 0 and L.psx_membrane_plan_info(h, buf, 0) == 0 and list(buf) == [-7] * 10
        assert L.psx_membrane_plan_info(h, buf, 3) == 3 and list(buf)[:4] == [plan.info["kept"], plan.info["ncx"], plan.info["ncy"], -7]
    # n = 0 with null arrays is a list, not an error
    hh = c_void_p(None)
    assert L.psx_membrane_plan_create(None, None, None, 0, ctypes.byref(hh)) == 0 and hh.value
    c0 = mo.cases()["empty"]
    out = fresh(c0)
    assert L.psx_membrane_layer_f32(hh, 3, -4, c0.dimX, c0.dimY, c0.margin, c0.margin2, sc, 0, c_void_p(out.data_ptr()), st) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    L.psx_membrane_plan_destroy(hh)
    out = fresh(c0)
    assert L.psx_membrane_f32(None, None, None, 0, c0.dimX, c0.dimY, c0.margin, c0.margin2, sc, 0, c_void_p(out.data_ptr()), st) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())


def test_wrapper_plan_cache_evicts_and_rebuilds():
    """getMembraneSegmentedFromFile keeps eight plans: after nine distinct lists the first is gone, and asking for it again
    renders ITS membrane (against the project oracle, as tests/test_gpu_main.py holds the wrapper), not a stale neighbour's."""
    import types
    from oracle import paresis_oracle as orc
    from paresis_amd import synth
    from paresis_amd.Samples import getMembraneFromFile as GM
    from tests._golden import relmax
    smp = types.SimpleNamespace(myMeanSphereRadius=15.0, myNbOfLayers=2)
    dimX, dimY, pix = 40, 72, 1.45
    lists = [synth.sphere_list(seed=500 + k) for k in range(9)]

    def render(k):
        return GM.getMembraneSegmentedFromFile(smp, dimX, dimY, pix, 5, 6000.0, sphere_list=lists[k])[0][0].cpu().numpy()

    GM._plans.clear()
    maps = [render(k) for k in range(9)]
    assert len(GM._plans) == 8                              # the first list's plan was evicted
    again = render(0)
    assert len(GM._plans) == 8 and np.array_equal(again, maps[0])
    assert all(not np.array_equal(maps[0], m) for m in maps[1:])
    ref = orc.membrane_segmented(lists[0], dimX, dimY, pix, 15.0, 2, 6000.0, synth.position_seed(5))[0]
    assert ref.max() > 0 and relmax(again, ref) < 2e-7
    ref8 = orc.membrane_segmented(lists[8], dimX, dimY, pix, 15.0, 2, 6000.0, synth.position_seed(5))[0]
    assert relmax(maps[8], ref8) < 2e-7 and relmax(again, ref8) > 1e-3
