"""Time the phase retrieval's kernels against their byte price.

    python tools/time_retrieval.py [--reps 20] [--host] [--umpa-only] [--paganin] [--fbp] [--project] [--tv] [--volume] [--decompose] [--fdk]

k_lcs reads 2K images and writes 3: 4*n*m*(2K + 3) bytes; k_lcs_df (LCS-DF, the dark-field column) reads the same and writes
4: 4*n*m*(2K + 4).  The two are timed in the same process, alternating launch by launch on the same inputs.  The
integration's extended grid is 2n x 2m complex64.  Times are HIP-event pairs per launch (psx_profile_summary), after warm-up,
on a GPU the process has to itself.  --host adds the float64
numpy oracle's time at the same sizes -- HOST time, one run, for scale only.

k_umpa (UMPA, window w, search s) reads 2K images and writes 4: the same 4*n*m*(2K + 4) bytes from HBM, but it is bound by its
float64 product sums: n*m*(2s+1)^2*K useful FMAs, set against the v_fma_f64 rate that tools/valu_bench measures (FMA64_CYCLES
per wave64 instruction and SIMD).  Its cases end with time(w = 4)/time(w = 1): the separable window sums keep it below 3,
direct ones would give about 9.  k_umpa_df (its dark-field variant, ops.umpa_df with the means given, so that nothing
synchronises) writes 5 maps and is timed in the same process, alternating with k_umpa launch by launch on the same inputs: two
box passes more in the prologue against (2s+1)^2 in the search, and a 2 x 2 solve per candidate.

--paganin times psx_paganin_f32 alone (B images of one shape with their flat fields, both maps): per pair of images the pack
reads 4 n x m float32 images and writes the extended grid, the filter reads and writes it, the crop reads its corner and writes
4 maps; the two rocFFT transforms are the integration's.

--fbp times psx_fbp_f32 alone at (A, n, m) = (720, 64, 1024): the filter (pack, two rocFFT passes per row pair, the multiply)
against the bytes it moves, and k_fbp_backproject against its two prices per voxel, angle and detector row: two 4-byte LDS
reads (as half of two ds_read_b128 that serve four rows) at 256 B per clock and CU, and two float32 FMAs.  The multiply of
the Hilbert filter (k_fbp_filter_hilbert, a plan with filter 'hilbert' on the same input) is listed beside the ramp's.

--project times the matched pair at (720, 64, 1024) and (90, 24, 64): k_fbp_project (psx_fbp_project_f32) and
psx_fbp_adjoint_f32 (k_fbp_pack + k_fbp_backproject at scale 1).  The projector's prices per voxel, angle and detector row: the
bytes it stages (every angle re-reads the slice: 4 B, from cache), three 4-byte LDS reads (three candidates, each a quarter
of a ds_read_b128 that serves four rows), two useful float32 FMAs out of the three it issues, and the float64 chain of a
candidate (two FMAs, floor, two additions, two comparisons, one conversion: 8 quarter-rate instructions) shared by four rows.

--tv times k_fbp_tv_step (psx_fbp_tv_step_f32), the voxel step of total-variation reconstruction, at (n, m) = (8, 512) and
(2, 2048): per voxel it reads six floats and writes four, 40 B, set against the HBM rate a copy achieves (6.3 TB/s of the
8 TB/s peak, MI355X_MICROARCH.md).  Beside it: the same step written with torch operations (torch_tv_step below, kept in
this tool only: the baseline the kernel replaces), timed with a host clock around a synchronised loop, and the share of a
whole iteration of tomography.tv at 90 angles that the two projector calls take.

--volume times k_volume_project (psx_volume_project_u8) on a (dimX, dimY) = (512, 2048) study grid at 30 degrees, voxel =
study pixel: on contrast_phantom_volume (13 materials, [512, 2048, 2048] labels) with and without the slices' occupied
boxes, and on a random 8-material volume of the same size (every voxel inside the circle its own label: four different
labels at most steps).  The baseline is psx_contrast_phantom_f32 at that grid (k_phantom_lines + k_phantom_maps), which is
how the same maps are made from the 13 analytic discs.  The byte price is one read of the labels and one write of the maps.

--decompose times k_decompose (psx_decompose_f32, the spectral material decomposition) at 2048 x 2048 pixels, M = 2 materials,
B = 3 bins of 8, 8 and 15 energies (a 20-80 keV spectrum sampled at 2 keV): its price is the float64 exp, one per pixel, energy
and Gauss-Newton step plus one pass for the residual, counted from the steps the kernel reports and set against the v_fma_f64
rate -- the time is given as float64 FMA slots per exp.  Beside it: the same iteration written with torch operations in
float64 (torch_decompose below, kept in this tool only; every pixel takes the kernel's largest step count), timed with a host
clock around a synchronised loop.

--fdk times the cone beam's kernels beside their parallel counterparts at (A, n, m) = (360, 64, 512): k_fdk_backproject beside
k_fbp_backproject on one sinogram (per voxel, angle and slice FDK reads four samples from cache where the parallel kernel
reads two from LDS, and forms a row coordinate in float64), and k_volume_project_cone beside k_volume_project on a random
8-material volume of 64 slices of 512 x 512 at 30 degrees (the cone kernel reads its labels from global memory and divides
once per step).
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from paresis_amd import ops, retrieval  # noqa: E402
from paresis_amd._lib import lib  # noqa: E402

PEAK = 8e12
FMA64_CYCLES, CLOCK, SIMDS = 4.0, 2.4e9, 256 * 4        # tools/valu_bench: cycles per wave64 v_fma_f64 and SIMD
FMA64_PEAK = SIMDS * 64 / FMA64_CYCLES * CLOCK          # float64 FMAs per second, all lanes busy


def summary():
    buf = ctypes.create_string_buffer(1 << 16)
    ops.check(lib().psx_profile_summary(buf, len(buf)), "psx_profile_summary")
    out = {}
    for line in buf.value.decode().splitlines():
        name, count, ms = line.split()
        out[name] = (int(count), float(ms))
    return out


def case(n, m, K, reps, host):
    g = torch.Generator(device="cuda").manual_seed(n + K)
    S = 1e4 * (1 + 0.3 * torch.rand((K, n, m), device="cuda", generator=g))
    R = 1e4 * (1 + 0.3 * torch.rand((K, n, m), device="cuda", generator=g))
    outs = tuple(torch.empty((n, m), device="cuda") for _ in range(3))
    outs_df = tuple(torch.empty((n, m), device="cuda") for _ in range(4))
    phi = torch.empty((n, m), device="cuda")
    for _ in range(3):
        ops.lcs(S, R, out=outs)
        ops.lcs_df(S, R, out=outs_df)
        retrieval.integrate(outs[1], outs[2], out=phi)
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        ops.lcs(S, R, out=outs)
        ops.lcs_df(S, R, out=outs_df)
        retrieval.integrate(outs[1], outs[2], out=phi)
    torch.cuda.synchronize()
    s = summary()
    lib().psx_profile_enable(0)
    per = {k: v[1] / v[0] * 1e3 for k, v in s.items()}       # us per call
    price = 4.0 * n * m * (2 * K + 3)
    t = per["k_lcs"]
    print("%dx%d K=%d  k_lcs %.1f us  price %.1f MB (%.1f us at 8 TB/s)  achieved %.2f TB/s = %.2f of 8 TB/s"
          % (n, m, K, t, price / 1e6, price / PEAK * 1e6, price / (t * 1e-6) / 1e12, price / (t * 1e-6) / PEAK))
    price_df = 4.0 * n * m * (2 * K + 4)
    tdf = per["k_lcs_df"]
    print("%dx%d K=%d  k_lcs_df %.1f us = %.2f x k_lcs  price %.1f MB (%.1f us at 8 TB/s)  achieved %.2f TB/s = %.2f of 8 TB/s"
          % (n, m, K, tdf, tdf / t, price_df / 1e6, price_df / PEAK * 1e6, price_df / (tdf * 1e-6) / 1e12,
             price_df / (tdf * 1e-6) / PEAK))
    kern = sum(v for k, v in per.items() if k.startswith("k_integ"))
    fft = sum(v for k, v in per.items() if k.startswith("rocfft_integrate"))
    grid = 4.0 * n * m * 8
    print("    integrate %.1f us = kernels %.1f us (%s) + rocFFT %.1f us (%s); extended grid %.1f MiB per pass"
          % (kern + fft, kern, ", ".join("%s %.1f" % (k, v) for k, v in per.items() if k.startswith("k_integ")), fft,
             ", ".join("%s %.1f" % (k, v) for k, v in per.items() if k.startswith("rocfft")), grid / 2 ** 20))
    if host:
        from tests import _retrieval_oracle as orl
        Sh, Rh = list(S.cpu().numpy()), list(R.cpu().numpy())
        t0 = time.perf_counter()
        r = orl.lcs(Sh, Rh)
        t1 = time.perf_counter()
        orl.integrate(r['dx'], r['dy'])
        t2 = time.perf_counter()
        from tests import _retrieval_df_oracle as odf
        odf.lcs_df(Sh, Rh)
        t3 = time.perf_counter()
        print("    numpy oracle (HOST time): lcs %.2f s, integrate %.2f s, lcs_df %.2f s" % (t1 - t0, t2 - t1, t3 - t2))


def umpa_case(n, m, K, w, s, reps):
    g = torch.Generator(device="cuda").manual_seed(n + K)
    S = 1e4 * (1 + 0.3 * torch.rand((K, n, m), device="cuda", generator=g))
    R = 1e4 * (1 + 0.3 * torch.rand((K, n, m), device="cuda", generator=g))
    outs = tuple(torch.empty((n, m), device="cuda") for _ in range(4))
    outs_df = tuple(torch.empty((n, m), device="cuda") for _ in range(5))
    mean = R.mean(dim=(1, 2), dtype=torch.float64).tolist()
    for _ in range(3):
        ops.umpa(S, R, window=w, search=s, out=outs)
        ops.umpa_df(S, R, window=w, search=s, mean=mean, out=outs_df)
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        ops.umpa(S, R, window=w, search=s, out=outs)
        ops.umpa_df(S, R, window=w, search=s, mean=mean, out=outs_df)
    torch.cuda.synchronize()
    prof = summary()
    lib().psx_profile_enable(0)
    t, tdf = (prof[k][1] / prof[k][0] * 1e-3 for k in ("k_umpa", "k_umpa_df"))
    price = 4.0 * n * m * (2 * K + 4)
    fma = float(n) * m * (2 * s + 1) ** 2 * K
    print("%dx%d K=%d w=%d s=%d  k_umpa %.1f us  price %.1f MB (%.1f us at 8 TB/s)  %.2f G FMA64 (%.1f us at %.1f T FMA/s) = %.2f of "
          "the float64 FMA rate" % (n, m, K, w, s, t * 1e6, price / 1e6, price / PEAK * 1e6, fma / 1e9, fma / FMA64_PEAK * 1e6,
                                    FMA64_PEAK / 1e12, fma / t / FMA64_PEAK))
    print("%dx%d K=%d w=%d s=%d  k_umpa_df %.1f us = %.3f x k_umpa" % (n, m, K, w, s, tdf * 1e6, tdf / t))
    return t


def paganin_case(n, m, B, reps):
    g = torch.Generator(device="cuda").manual_seed(n + B)
    W = 1e4 * (1 + 0.1 * torch.rand((B, n, m), device="cuda", generator=g))
    I = W * (1 + 0.3 * (torch.rand((B, n, m), device="cuda", generator=g) - 0.5))
    outs = (torch.empty((B, n, m), device="cuda"), torch.empty((B, n, m), device="cuda"))
    plan = retrieval._plan(I.device, n, m)
    for _ in range(3):
        ops.paganin(I, W, 3.0, 22.0, plan, out=outs)
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        ops.paganin(I, W, 3.0, 22.0, plan, out=outs)
    torch.cuda.synchronize()
    s = summary()
    lib().psx_profile_enable(0)
    pairs = (B + 1) // 2
    per = {k: v[1] / (reps * pairs) * 1e3 for k, v in s.items()}       # us per pair of images
    grid = 4.0 * n * m * 8
    price = {"k_pag_pack": 16.0 * n * m + grid, "k_pag_filter": 2 * grid, "k_pag_crop": grid / 4 + 16.0 * n * m}
    kern = sum(per[k] for k in price)
    fft = sum(v for k, v in per.items() if k.startswith("rocfft_paganin"))
    print("%dx%d B=%d  paganin per pair %.1f us = kernels %.1f us + rocFFT %.1f us (%s)"
          % (n, m, B, kern + fft, kern, fft, ", ".join("%s %.1f" % (k, v) for k, v in per.items() if k.startswith("rocfft"))))
    for k, b in price.items():
        print("    %s %.1f us  price %.1f MB (%.1f us at 8 TB/s) = %.2f of 8 TB/s" % (k, per[k], b / 1e6, b / PEAK * 1e6,
                                                                                        b / (per[k] * 1e-6) / PEAK))


LDS_PEAK = 256 * 256 * CLOCK                            # bytes per second: 256 B per clock and CU
FMA32_PEAK = SIMDS * 64 / 2.0 * CLOCK                   # float32 FMAs per second: a wave64 v_fma_f32 takes 2 cycles of a SIMD


def fbp_case(A, n, m, reps):
    g = torch.Generator(device="cuda").manual_seed(A + n)
    sino = 1.0 + torch.rand((A, n, m), device="cuda", generator=g)
    plan = ops.FbpPlan([180.0 * a / A for a in range(A)], m)
    vol = torch.empty((n, m, m), device="cuda")
    for _ in range(2):
        ops.fbp(sino, plan, out=vol)
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        ops.fbp(sino, plan, out=vol)
    torch.cuda.synchronize()
    s = summary()
    lib().psx_profile_enable(0)
    per = {k: v[1] / reps * 1e3 for k, v in s.items()}       # us per call (all launches of a kernel in one call)
    P = 64
    while P < 2 * m:
        P *= 2
    pairs = (n + 1) // 2
    grid = 8.0 * pairs * A * P
    price = {"k_fbp_pack": 4.0 * A * n * m + grid, "k_fbp_filter": 2 * grid}
    fft = sum(v for k, v in per.items() if k.startswith("rocfft_fbp"))
    print("A=%d n=%d m=%d  plan %.0f MiB  filter per call %.1f us = kernels %.1f us + rocFFT %.1f us (%s, %d launches each)"
          % (A, n, m, plan.bytes / 2 ** 20, per["k_fbp_pack"] + per["k_fbp_filter"] + fft, per["k_fbp_pack"] + per["k_fbp_filter"],
             fft, ", ".join("%s %.1f" % (k, v) for k, v in per.items() if k.startswith("rocfft")), pairs))
    # the Hilbert filter's step (a differential sinogram) on the same input: the same loads and stores as the ramp's
    hilbert = ops.FbpPlan(plan.theta, m, filter="hilbert")
    for _ in range(2):
        ops.fbp(sino, hilbert, out=vol)
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        ops.fbp(sino, hilbert, out=vol)
    torch.cuda.synchronize()
    per["k_fbp_filter_hilbert"] = summary()["k_fbp_filter_hilbert"][1] / reps * 1e3
    lib().psx_profile_enable(0)
    hilbert.close()
    price["k_fbp_filter_hilbert"] = price["k_fbp_filter"]
    for k, b in price.items():
        print("    %s %.1f us  price %.1f MB (%.1f us at 8 TB/s) = %.2f of 8 TB/s" % (k, per[k], b / 1e6, b / PEAK * 1e6,
                                                                                        b / (per[k] * 1e-6) / PEAK))
    print("    k_fbp_filter_hilbert / k_fbp_filter = %.3f" % (per["k_fbp_filter_hilbert"] / per["k_fbp_filter"]))
    t = per["k_fbp_backproject"] * 1e-6
    work = float(m) * m * A * n
    lds, fma = 8.0 * work, 2.0 * work
    print("    k_fbp_backproject %.1f us per call (%d launches)  LDS reads %.1f GB (%.1f us at %.0f TB/s) = %.2f of the LDS rate;  "
          "%.1f G FMA32 (%.1f us at %.1f T FMA/s) = %.2f of the float32 FMA rate"
          % (t * 1e6, s["k_fbp_backproject"][0] // reps, lds / 1e9, lds / LDS_PEAK * 1e6, LDS_PEAK / 1e12, lds / t / LDS_PEAK,
             fma / 1e9, fma / FMA32_PEAK * 1e6, FMA32_PEAK / 1e12, fma / t / FMA32_PEAK))


def project_case(A, n, m, reps):
    g = torch.Generator(device="cuda").manual_seed(A + n)
    vol = 1.0 + torch.rand((n, m, m), device="cuda", generator=g)
    plan = ops.FbpPlan([180.0 * a / A for a in range(A)], m, filter="none")
    sino = torch.empty((A, n, m), device="cuda")
    back = torch.empty_like(vol)
    for _ in range(2):
        ops.fbp_project(vol, plan, out=sino)
        ops.fbp_adjoint(sino, plan, out=back)
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        ops.fbp_project(vol, plan, out=sino)
        ops.fbp_adjoint(sino, plan, out=back)
    torch.cuda.synchronize()
    s = summary()
    lib().psx_profile_enable(0)
    per = {k: v[1] / reps * 1e3 for k, v in s.items()}       # us per call
    work = float(m) * m * A * n
    t = per["k_fbp_project"] * 1e-6
    staged, lds, fma, f64 = 4.0 * work, 12.0 * work, 2.0 * work, 6.0 * work
    print("A=%d n=%d m=%d  k_fbp_project %.1f us per call (%d launches)  staged %.1f GB (%.1f us at 8 TB/s) = %.2f of 8 TB/s;  "
          "LDS reads %.1f GB (%.1f us at %.0f TB/s) = %.2f of the LDS rate;  %.1f G useful FMA32 (%.1f us) = %.2f of the float32 "
          "FMA rate;  %.1f G float64 instructions (%.1f us at %.1f T/s) = %.2f of the float64 rate"
          % (A, n, m, t * 1e6, s["k_fbp_project"][0] // reps, staged / 1e9, staged / PEAK * 1e6, staged / t / PEAK,
             lds / 1e9, lds / LDS_PEAK * 1e6, LDS_PEAK / 1e12, lds / t / LDS_PEAK, fma / 1e9, fma / FMA32_PEAK * 1e6,
             fma / t / FMA32_PEAK, f64 / 1e9, f64 / FMA64_PEAK * 1e6, FMA64_PEAK / 1e12, f64 / t / FMA64_PEAK))
    tb = per["k_fbp_backproject"] * 1e-6
    print("    psx_fbp_adjoint_f32 %.1f us per call = k_fbp_pack %.1f us + k_fbp_backproject %.1f us (%d launches): LDS reads "
          "%.2f of the LDS rate, %.2f of the float32 FMA rate;  k_fbp_project / k_fbp_backproject = %.2f"
          % (per["k_fbp_pack"] + per["k_fbp_backproject"], per["k_fbp_pack"], per["k_fbp_backproject"],
             s["k_fbp_backproject"][0] // reps, 8.0 * work / tb / LDS_PEAK, 2.0 * work / tb / FMA32_PEAK, t / tb))


HBM_ACHIEVABLE = 6.3e12                                 # bytes per second: a float4 copy (MI355X_MICROARCH.md)


def torch_tv_step(lam, nonneg, ax, ay, tau, u, x, xbar, px, py):
    """psx_fbp_tv_step_f32's arithmetic with torch operations -> (x', xbar', px', py').  ax, ay: the active differences as
    float32 [m, m] masks; tau: the primal step [n, m, m]."""
    gx, gy = torch.zeros_like(xbar), torch.zeros_like(xbar)
    gx[:, :-1, :] = xbar[:, 1:, :] - xbar[:, :-1, :]
    gy[:, :, :-1] = xbar[:, :, 1:] - xbar[:, :, :-1]
    tx, ty = px + 0.5 * (gx * ax), py + 0.5 * (gy * ay)
    nr = torch.sqrt(tx * tx + ty * ty)
    s = torch.where(nr > lam, lam / nr.clamp(min=1e-30), torch.ones_like(nr))
    pxn, pyn = tx * s, ty * s
    a, b = pxn * ax, pyn * ay
    d = -a - b
    d[:, 1:, :] += a[:, :-1, :]
    d[:, :, 1:] += b[:, :, :-1]
    xn = x - tau * (u + d)
    if nonneg:
        xn = xn.clamp(min=0)
    return xn, 2 * xn - x, pxn, pyn


def _host_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def tv_case(n, m, A, reps):
    from paresis_amd import tomography
    g = torch.Generator(device="cuda").manual_seed(n + m)
    rand = lambda: torch.rand((n, m, m), device="cuda", generator=g) - 0.5
    plan = ops.FbpPlan([180.0 * a / A for a in range(A)], m, filter="none")
    u, x, xbar, px, py = rand(), rand(), rand(), rand(), rand()
    c = ops.fbp_adjoint(torch.ones((A, n, m), device="cuda"), plan)
    xbar2, px2, py2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    lam = 0.3
    for _ in range(3):
        ops.fbp_tv_step(plan, lam, True, u, c, x.clone(), xbar, xbar2, px, py, px2, py2)
    torch.cuda.synchronize()
    xs = x.clone()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        ops.fbp_tv_step(plan, lam, True, u, c, xs, xbar, xbar2, px, py, px2, py2)
    torch.cuda.synchronize()
    t = summary()["k_fbp_tv_step"]
    lib().psx_profile_enable(0)
    t = t[1] / t[0] * 1e-3
    price = 40.0 * n * m * m
    print("n=%d m=%d  k_fbp_tv_step %.1f us  price %.1f MB (%.1f us at %.1f TB/s) = %.2f of the achievable HBM rate, %.2f of 8 TB/s"
          % (n, m, t * 1e6, price / 1e6, price / HBM_ACHIEVABLE * 1e6, HBM_ACHIEVABLE / 1e12, price / t / HBM_ACHIEVABLE,
             price / t / PEAK))
    lit = tomography._lit(m, True, x.device)
    ax, ay = torch.zeros((m, m), device="cuda"), torch.zeros((m, m), device="cuda")
    ax[:-1, :] = (lit[:-1, :] & lit[1:, :]).float()
    ay[:, :-1] = (lit[:, :-1] & lit[:, 1:]).float()
    deg = ax + ay
    deg[1:, :] += ax[:-1, :]
    deg[:, 1:] += ay[:, :-1]
    tau = tomography._reciprocal(c + deg)
    want = ops.fbp_tv_step(plan, lam, True, u, c, x.clone(), xbar, xbar2, px, py, px2, py2)
    got = torch_tv_step(lam, True, ax, ay, tau, u, x, xbar, px, py)
    worst = max(float((a - b).abs().max()) for a, b in zip(got, want))
    t_kernel = _host_us(lambda: ops.fbp_tv_step(plan, lam, True, u, c, xs, xbar, xbar2, px, py, px2, py2), reps)
    t_torch = _host_us(lambda: torch_tv_step(lam, True, ax, ay, tau, u, x, xbar, px, py), reps)
    print("    the step with torch operations %.1f us per call (host clock; the kernel the same way %.1f us): %.1f times the kernel; "
          "largest difference between the two %.1e" % (t_torch, t_kernel, t_torch / t_kernel, worst))
    b = ops.fbp_project(x, plan)
    tomography.tv(b, plan.theta, 2, lam, nonneg=True)
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    tomography.tv(b, plan.theta, reps, lam, nonneg=True)
    torch.cuda.synchronize()
    s = summary()
    lib().psx_profile_enable(0)
    per = {k: v[1] / reps * 1e3 for k, v in s.items()}        # us per iteration (the two set-up projections are in: 2/reps more)
    proj = per["k_fbp_project"] + per["k_fbp_pack"] + per["k_fbp_backproject"]
    t_iter = _host_us(lambda: tomography.tv(b, plan.theta, reps, lam, nonneg=True), 1) / reps
    print("    tomography.tv at %d angles: %.1f us per iteration (host clock) = projectors %.1f us (project %.1f, adjoint %.1f) = %.2f "
          "of it + k_fbp_tv_step %.1f us = %.3f + torch's dual update and launches"
          % (A, t_iter, proj, per["k_fbp_project"], per["k_fbp_pack"] + per["k_fbp_backproject"], proj / t_iter,
             per["k_fbp_tv_step"], per["k_fbp_tv_step"] / t_iter))
    plan.close()


def _kernel_us(names, fn, reps):
    """Mean HIP-event time in us of the kernels `names` over `reps` calls of fn, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    lib().psx_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    s = summary()
    lib().psx_profile_enable(0)
    return [s[k][1] / s[k][0] * 1e3 for k in names]


def volume_case(dimX, dimY, pix_um, reps):
    from paresis_amd.Samples.generateContrastPhantom import contrast_phantom_lines
    from paresis_amd.Samples.getVolumeFromFile import contrast_phantom_volume, upload_volume
    angle, voxel_m = 30.0, pix_um * 1e-6
    t_lines, t_maps = _kernel_us(("k_phantom_lines", "k_phantom_maps"),
                                 lambda: contrast_phantom_lines(dimX, dimY, pix_um, angle), reps)
    base = t_lines + t_maps
    print("dimX=%d dimY=%d  psx_contrast_phantom_f32 %.1f us (k_phantom_lines %.1f + k_phantom_maps %.1f)"
          % (dimX, dimY, base, t_lines, t_maps))
    want = contrast_phantom_lines(dimX, dimY, pix_um, angle)[0]

    def run(name, v, nmat, box):
        (t,) = _kernel_us(("k_volume_project",), lambda: ops.volume_project(v.labels, nmat, angle, (dimX, dimY), 1.0, voxel_m,
                                                                            box=v.box if box else None), reps)
        price = v.labels.numel() + 4.0 * nmat * dimX * dimY
        print("    %-34s k_volume_project %9.1f us = %7.1f x the phantom's kernels; price %.0f MB (%.0f us at 8 TB/s) = %.3f of peak"
              % (name, t, t / base, price / 1e6, price / PEAK * 1e6, price / (t * 1e-6) / PEAK))
        return t

    v = upload_volume(contrast_phantom_volume(dimX, dimY, pix_um), 13)
    got = ops.volume_project(v.labels, 13, angle, (dimX, dimY), 1.0, voxel_m, box=v.box)
    print("    the phantom's volume gives the phantom's maps: largest difference %.1e m of %.1e m"
          % (float((got - want).abs().max()), float(want.abs().max())))
    run("phantom volume, occupied boxes", v, 13, True)
    run("phantom volume, whole slices", v, 13, False)
    del v, got
    g = torch.Generator(device="cuda").manual_seed(dimX + dimY)
    d2 = (torch.arange(dimY, device="cuda") - dimY // 2) ** 2
    inside = (d2[:, None] + d2[None, :] <= (dimY // 2) ** 2).to(torch.uint8)
    lab = torch.randint(1, 9, (dimX, dimY, dimY), device="cuda", generator=g, dtype=torch.uint8) * inside
    v = upload_volume(lab, 8)
    run("random 8-material volume", v, 8, True)


def fdk_case(A, n, m, reps):
    """The cone beam's two kernels beside their parallel counterparts: k_fdk_backproject / k_fbp_backproject on one [A, n, m]
    sinogram, k_volume_project_cone / k_volume_project on an n-slice random 8-material volume of m x m slices at 30 degrees
    (s = 1, the study grid n x m), the source 3 m voxels from the axis."""
    from paresis_amd.Samples.getVolumeFromFile import upload_volume
    theta = [360.0 * a / A for a in range(A)]
    dso = 3.0 * m
    g = torch.Generator(device="cuda").manual_seed(A + n + m)
    sino = torch.rand((A, n, m), device="cuda", generator=g, dtype=torch.float32)
    flat, cone = ops.FbpPlan(theta, m), ops.FdkPlan(theta, n, m, dso)
    (t_fbp,) = _kernel_us(("k_fbp_backproject",), lambda: ops.fbp(sino, flat), reps)
    t_fdk, t_unpack = _kernel_us(("k_fdk_backproject", "k_fdk_unpack"), lambda: ops.fdk(sino, cone), reps)
    updates = float(A) * n * m * m
    print("A=%d n=%d m=%d  k_fbp_backproject %.1f us (%.2f G voxel-angles/s)  k_fdk_backproject %.1f us (%.2f G/s) = %.2f x; "
          "k_fdk_unpack %.1f us; plans %.1f and %.1f MB"
          % (A, n, m, t_fbp, updates / t_fbp / 1e3, t_fdk, updates / t_fdk / 1e3, t_fdk / t_fbp, t_unpack, flat.bytes / 1e6,
             cone.bytes / 1e6))
    d2 = (torch.arange(m, device="cuda") - m // 2) ** 2
    inside = (d2[:, None] + d2[None, :] <= (m // 2) ** 2).to(torch.uint8)
    lab = torch.randint(1, 9, (n, m, m), device="cuda", generator=g, dtype=torch.uint8) * inside
    v = upload_volume(lab, 8)
    (t_par,) = _kernel_us(("k_volume_project",), lambda: ops.volume_project(v.labels, 8, 30.0, (n, m), 1.0, 1e-6, box=v.box), reps)
    (t_cone,) = _kernel_us(("k_volume_project_cone",),
                           lambda: ops.volume_project(v.labels, 8, 30.0, (n, m), 1.0, 1e-6, box=v.box, dso=dso), reps)
    steps = float(n) * m * m
    print("    %d slices of %d x %d, 8 materials: k_volume_project %.1f us (%.2f G steps/s)  k_volume_project_cone %.1f us "
          "(%.2f G steps/s) = %.2f x" % (n, m, m, t_par, steps / t_par / 1e3, t_cone, steps / t_cone / 1e3, t_cone / t_par))


def _decompose_model():
    """20-80 keV at 2 keV in bins of 8, 8 and 15 energies; a soft and a bone-like material (1/m)."""
    E = np.arange(20.0, 81.0, 2.0)
    t = (E - 18.0) / 62.0
    flux = t * (1.2 - t) ** 2 + 0.02
    sizes = [8, 8, 15]
    cut = np.cumsum([0] + sizes)
    w = np.concatenate([flux[cut[b]:cut[b + 1]] / flux[cut[b]:cut[b + 1]].sum() for b in range(3)])
    a = np.stack([54.0 * (20.0 / E) ** 4 + 18.0 * (60.0 / E), 700.0 * (20.0 / E) ** 3.2 + 38.0 * (60.0 / E) ** 0.8])
    return sizes, w, a


def torch_decompose(L, sizes, w, a, v, G, steps):
    """`steps` Gauss-Newton steps of psx_decompose_f32's iteration for M = 2 on every pixel, in float64 torch operations."""
    L = L.double()
    x = torch.einsum("mb,bn->mn", G, L)
    for _ in range(steps):
        N00 = N01 = N11 = r0 = r1 = 0.0
        e0 = 0
        for b, ne in enumerate(sizes):
            ab = a[:, e0:e0 + ne]
            s = w[e0:e0 + ne, None] * torch.exp(-(ab.T @ x))
            T = s.sum(dim=0)
            g = (ab @ s) / T
            r = L[b] + torch.log(T)
            N00, N01, N11 = N00 + v[b] * g[0] * g[0], N01 + v[b] * g[0] * g[1], N11 + v[b] * g[1] * g[1]
            r0, r1 = r0 + v[b] * g[0] * r, r1 + v[b] * g[1] * r
            e0 += ne
        det = N00 * N11 - N01 * N01
        x = x + torch.stack([(N11 * r0 - N01 * r1) / det, (N00 * r1 - N01 * r0) / det])
    return x


def decompose_case(n, m, reps):
    sizes, w, a = _decompose_model()
    B, E = len(sizes), sum(sizes)
    v = np.ones(B)
    cut = np.cumsum([0] + sizes)
    A = np.stack([a[:, cut[b]:cut[b + 1]] @ w[cut[b]:cut[b + 1]] for b in range(B)])
    G = np.linalg.solve(A.T @ A, A.T)
    g = torch.Generator(device="cuda").manual_seed(n + m)
    x = torch.rand((2, n * m), device="cuda", generator=g, dtype=torch.float64) * torch.tensor([[0.05], [0.01]], device="cuda")
    wd, ad = torch.from_numpy(w).cuda(), torch.from_numpy(a).cuda()
    L = torch.stack([-torch.log((wd[cut[b]:cut[b + 1], None] * torch.exp(-(ad[:, cut[b]:cut[b + 1]].T @ x))).sum(dim=0))
                     for b in range(B)]).float().reshape(B, n, m).contiguous()
    out = ops.decompose(L, sizes, w, a, v, G)
    steps = out[2]
    kmax, ksum = int(steps.max()), float(steps.double().sum())
    (t,) = _kernel_us(("k_decompose",), lambda: ops.decompose(L, sizes, w, a, v, G, out=out), reps)
    exps = (ksum + n * m) * E
    print("n=%d m=%d M=2 B=3 E=%d  k_decompose %9.1f us; steps %d..%d (mean %.2f); %.3g float64 exps = %.2f ns per pixel, %.1f float64 "
          "FMA slots per exp (at %.3g FMA/s)" % (n, m, E, t, int(steps.min()), kmax, ksum / (n * m), exps, t * 1e3 / (n * m),
                                                  t * 1e-6 * FMA64_PEAK / exps, FMA64_PEAK))
    Gd, Lf = torch.from_numpy(G).cuda(), L.reshape(B, -1)
    ref = torch_decompose(Lf, sizes, wd, ad, v, Gd, kmax)
    print("    torch_decompose agrees to %.1e m of %.1e m" % (float((ref - out[0].reshape(2, -1).double()).abs().max()), float(ref.abs().max())))
    t_torch = _host_us(lambda: torch_decompose(Lf, sizes, wd, ad, v, Gd, kmax), max(reps // 4, 2))
    print("    the same %d steps in torch operations %9.1f us = %.1f x k_decompose" % (kmax, t_torch, t_torch / t))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--umpa-only", action="store_true")
    ap.add_argument("--paganin", action="store_true", help="time psx_paganin_f32 only")
    ap.add_argument("--fbp", action="store_true", help="time psx_fbp_f32 only")
    ap.add_argument("--project", action="store_true", help="time psx_fbp_project_f32 and psx_fbp_adjoint_f32 only")
    ap.add_argument("--tv", action="store_true", help="time psx_fbp_tv_step_f32 and an iteration of tomography.tv only")
    ap.add_argument("--volume", action="store_true", help="time psx_volume_project_u8 against psx_contrast_phantom_f32 only")
    ap.add_argument("--decompose", action="store_true", help="time psx_decompose_f32 against the same iteration in torch operations only")
    ap.add_argument("--fdk", action="store_true",
                    help="time k_fdk_backproject beside k_fbp_backproject and k_volume_project_cone beside k_volume_project only")
    a = ap.parse_args()
    if a.fdk:
        fdk_case(360, 64, 512, max(a.reps // 4, 2))
        return
    if a.decompose:
        decompose_case(2048, 2048, a.reps)
        return
    if a.volume:
        volume_case(512, 2048, 20.0, max(a.reps // 4, 2))
        return
    if a.tv:
        tv_case(8, 512, 90, a.reps)
        tv_case(2, 2048, 90, max(a.reps // 2, 2))
        return
    if a.project:
        project_case(720, 64, 1024, max(a.reps // 4, 2))
        project_case(90, 24, 64, a.reps)
        return
    if a.fbp:
        fbp_case(720, 64, 1024, max(a.reps // 4, 2))
        fbp_case(90, 24, 64, a.reps)
        return
    if a.paganin:
        for n, m, B in ((2048, 2048, 2), (2048, 2048, 8), (200, 200, 2)):
            paganin_case(n, m, B, a.reps)
        return
    for n, m, K in () if a.umpa_only else ((2048, 2048, 16), (2048, 2048, 64), (200, 200, 12)):
        case(n, m, K, a.reps, a.host)
    umpa_case(2048, 2048, 16, 2, 3, a.reps)
    umpa_case(200, 200, 12, 2, 3, a.reps)
    t1 = umpa_case(2048, 2048, 16, 1, 3, a.reps)
    t4 = umpa_case(2048, 2048, 16, 4, 3, a.reps)
    print("k_umpa 2048x2048 K=16 s=3: time(w=4)/time(w=1) = %.2f" % (t4 / t1))
    umpa_case(2048, 2048, 16, 8, 8, max(a.reps // 10, 2))


if __name__ == "__main__":
    main()
