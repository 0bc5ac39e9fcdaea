// fbp.hip -- filtered back-projection of a stack of projections (psx_fbp_*; the contract is in include/paresis_hip.h).
//   k_fbp_pack     Z[rp][a][k] = (sino[a][r0+2rp][k], sino[a][r0+2rp+1][k]) for k < m, 0 up to the line's length L: two
//                  detector rows per complex line (L = P with a filter, m without)
//   rocFFT         P-point forward transforms, A lines per row pair and launch
//   k_fbp_filter   Z *= He/P, He the even part of the real filter H (float64 table): the pair stays separable.  The Hilbert
//                  filters of a differential sinogram: Z *= i Ho/P, Ho the odd part -- Hermitian too, so the same holds
//   rocFFT         inverse; Z.x / Z.y are now the filtered lines of the two rows
//   k_fbp_backproject   one workgroup per 16 x 16 tile of the slice and block of 4 detector rows (two row pairs)
// The filtered sinogram is never cropped or copied: the back-projector reads the float2 lines of Z as they are, and a row
// pair of Z is the (row, row + 1) interleave its LDS image wants.
//   k_fbp_project  the back-projector's exact transpose, volume -> sinogram, in the gather form: one workgroup per angle,
//                  run of 64 samples and block of 4 detector rows (psx_fbp_project_f32; psx_fbp_adjoint_f32 is pack +
//                  back-projection at scale 1)
//   k_fbp_tv_step  the voxel step of total-variation reconstruction on the pair (psx_fbp_tv_step_f32): dual projection,
//                  divergence, primal step, clamp and over-relaxation in one launch
//   FDK (psx_fdk_*; cone beam, full turn): k_fbp_pack with the cosine pre-weight, the same filter, k_fdk_unpack into the
//                  plan's filtered sinogram of all rows, k_fdk_backproject: a thread per voxel column and block of 8 slices
#include "fresnel_plan.hpp"

#include <complex>
#include <vector>

using namespace psx;

namespace {

constexpr int FBP_TILE = 16;     // slice tile: 16 x 16 voxels, one per thread
constexpr int FBP_ROWS = 4;      // detector rows per workgroup: one float4 of LDS per sample
constexpr int FBP_CHUNK = 32;    // angles staged per round
// Samples of one line a tile can reach: u = (j-h) c - (i-h) s + center spans 15 (|c| + |s|) <= 21.3 over the tile, so
// floor(u) takes at most 23 values from floor(u_min) on and the interpolation reads one more: 24.  The segment starts one
// sample below floor(u_min) (u_min is evaluated at a corner by another thread, to ~1e-12) and has one to spare above:
// 26 = ceil(sqrt(2) * 16) + 3.
constexpr int FBP_SEG = 26;

// The contract's geometry (include/paresis_hip.h, "the matched projector pair"), stated once: the projector is the
// back-projector's exact transpose because both take u and its tap from here.  Voxel (i, j), h = m / 2, lies at the detector
// coordinate u = (j - h) cos - (i - h) sin + center, in float64, the sine's product first: dj = j - h, ndi = -(i - h).
__device__ __forceinline__ double fbp_u(double dj, double ndi, double c, double s, double center) {
    return fma(dj, c, fma(ndi, s, center));
}

// u interpolates between sample fl = floor(u), with the weight w0 = 1 - w1, and fl + 1, with w1 = (float)(u - fl)
struct FbpTap { double fl; float w0, w1; };
__device__ __forceinline__ FbpTap fbp_tap(double u) {
    const double fl = floor(u);
    const float w1 = (float)(u - fl);
    return {fl, 1.0f - w1, w1};
}

// Voxel (i, j) is inside the inscribed circle, or the plan has none.  W, the integer type of the squares, is each caller's
// own: int is exact for indices inside the slice (m <= PSX_FBP_MAX_M), int64_t for any int.
template <typename W> __device__ __forceinline__ bool fbp_lit(int i, int j, int h, int circle) {
    return !circle || (W)(i - h) * (i - h) + (W)(j - h) * (j - h) <= (W)h * h;
}

// FDK's pre-weight of sample (r, k), the cosine of the ray's angle to the optical axis (include/paresis_hip.h, "FDK"); the
// parallel beam has none
struct ConeWeight { double dso, center, vcenter; };
struct NoWeight {};
__device__ __forceinline__ float fbp_weighted(float p, int, int, const NoWeight &) { return p; }
__device__ __forceinline__ float fbp_weighted(float p, int r, int k, const ConeWeight &c) {
#pragma clang fp contract(off)
    const double dk = (double)k - c.center, dr = (double)r - c.vcenter;
    return (float)((double)p * c.dso / sqrt(c.dso * c.dso + dk * dk + dr * dr));
}

template <typename Weight>
__global__ __launch_bounds__(256) void k_fbp_pack(const float *__restrict__ sino, float2 *__restrict__ Z, int A, int n, int m,
                                                  int L, int r0, int npairs, Weight wt) {
    const int64_t N = (int64_t)npairs * A * L;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(p % L);
        const int64_t la = p / L;
        const int a = (int)(la % A), rp = (int)(la / A);
        float2 z = make_float2(0.f, 0.f);
        if (k < m) {
            const int r = r0 + 2 * rp;
            const int64_t q = ((int64_t)a * n + r) * m + k;
            z.x = fbp_weighted(sino[q], r, k, wt);
            if (r + 1 < n) z.y = fbp_weighted(sino[q + m], r + 1, k, wt);
        }
        Z[p] = z;
    }
}

// Z *= T[k] for the even table of the ramp filters, Z *= i T[k] for the odd table of the Hilbert filters (DIFFERENTIAL):
// either multiplier is Hermitian, so the two rows of a pair stay in Z.x and Z.y
template <bool DIFFERENTIAL>
__global__ __launch_bounds__(256) void k_fbp_filter(float2 *__restrict__ Z, const double *__restrict__ T, int P, int64_t N) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const double w = T[p & (P - 1)];
        const float2 z = Z[p];
        Z[p] = DIFFERENTIAL ? make_float2((float)(-(double)z.y * w), (float)((double)z.x * w))
                            : make_float2((float)((double)z.x * w), (float)((double)z.y * w));
    }
}

struct FbpArgs {
    const float2 *Z;          // [npairs][A][L]
    const double *cs;         // [A] cos, then [A] sin
    float *vol;               // [n][m][m]
    double center;
    float scale;              // pi / (2A)
    int A, n, m, L, r0, npairs, circle;
};

__global__ __launch_bounds__(256) void k_fbp_backproject(FbpArgs p) {
    __shared__ float4 seg[FBP_CHUNK][FBP_SEG];       // seg[a][k] = the four rows' sample base[a] + k
    __shared__ double scos[FBP_CHUNK], ssin[FBP_CHUNK];
    __shared__ int sbase[FBP_CHUNK];

    const int tid = threadIdx.x;
    const int h = p.m / 2;
    const int j0 = blockIdx.x * FBP_TILE, i0 = blockIdx.y * FBP_TILE;
    const int j = j0 + (tid & (FBP_TILE - 1)), i = i0 + (tid >> 4);
    const int rb = p.r0 + blockIdx.z * FBP_ROWS;                // first detector row of this workgroup
    const int pair0 = blockIdx.z * (FBP_ROWS / 2);              // its first row pair in Z
    const bool voxel = i < p.m && j < p.m;
    const bool lit = voxel && fbp_lit<int64_t>(i, j, h, p.circle);

    // a tile whose nearest point to the axis is outside the circle holds zeros only (the same for the whole workgroup)
    bool dark = false;
    if (p.circle) {
        const int i1 = min(i0 + FBP_TILE, p.m) - 1, j1 = min(j0 + FBP_TILE, p.m) - 1;
        const int64_t di = (h < i0 ? i0 : h > i1 ? i1 : h) - h, dj = (h < j0 ? j0 : h > j1 ? j1 : h) - h;
        dark = di * di + dj * dj > (int64_t)h * h;
    }

    float acc[FBP_ROWS] = {0.f, 0.f, 0.f, 0.f};
    if (!dark) {
        const double dj = (double)(j - h), ndi = -(double)(i - h);
        // the tile's corners, overhang included: every thread's u lies between their extremes
        const double cj0 = (double)(j0 - h), cj1 = (double)(j0 + FBP_TILE - 1 - h);
        const double ci0 = -(double)(i0 - h), ci1 = -(double)(i0 + FBP_TILE - 1 - h);
        for (int a0 = 0; a0 < p.A; a0 += FBP_CHUNK) {
            const int na = min(FBP_CHUNK, p.A - a0);
            if (tid < na) {
                const double c = p.cs[a0 + tid], s = p.cs[p.A + a0 + tid];
                const double u00 = fbp_u(cj0, ci0, c, s, p.center), u01 = fbp_u(cj1, ci0, c, s, p.center);
                const double u10 = fbp_u(cj0, ci1, c, s, p.center), u11 = fbp_u(cj1, ci1, c, s, p.center);
                scos[tid] = c;
                ssin[tid] = s;
                sbase[tid] = (int)floor(fmin(fmin(u00, u01), fmin(u10, u11))) - 1;
            }
            __syncthreads();
            // stage: one float2 (a row pair) per element, k fastest so that a wave reads whole segments of the lines
            for (int e = tid; e < na * (FBP_ROWS / 2) * FBP_SEG; e += 256) {
                const int k = e % FBP_SEG, t = e / FBP_SEG;
                const int pp = t % (FBP_ROWS / 2), a = t / (FBP_ROWS / 2);
                const int g = sbase[a] + k, pair = pair0 + pp;
                float2 v = make_float2(0.f, 0.f);
                if (g >= 0 && g < p.m && pair < p.npairs) v = p.Z[((int64_t)pair * p.A + (a0 + a)) * p.L + g];
                reinterpret_cast<float2 *>(&seg[a][k])[pp] = v;
            }
            __syncthreads();
            for (int a = 0; a < na; ++a) {
                const FbpTap tap = fbp_tap(fbp_u(dj, ndi, scos[a], ssin[a], p.center));
                const float w0 = tap.w0, w1 = tap.w1;
                int k = (int)tap.fl - sbase[a];
                k = k < 0 ? 0 : k > FBP_SEG - 2 ? FBP_SEG - 2 : k;     // never taken inside the tile; keeps an overhanging thread's read inside the segment
                const float4 q0 = seg[a][k], q1 = seg[a][k + 1];
                acc[0] = fmaf(w1, q1.x, fmaf(w0, q0.x, acc[0]));
                acc[1] = fmaf(w1, q1.y, fmaf(w0, q0.y, acc[1]));
                acc[2] = fmaf(w1, q1.z, fmaf(w0, q0.z, acc[2]));
                acc[3] = fmaf(w1, q1.w, fmaf(w0, q0.w, acc[3]));
            }
            __syncthreads();
        }
    }
    if (!voxel) return;
#pragma unroll
    for (int r = 0; r < FBP_ROWS; ++r)
        if (rb + r < p.n) p.vol[((int64_t)(rb + r) * p.m + i) * p.m + j] = lit ? acc[r] * p.scale : 0.f;
}

// ---- FDK: the filtered lines of every row, resident, and the divergent back-projector ------------------------------------
constexpr int FDK_TILE = 16;     // a thread per voxel column (i, j) of a 16 x 16 tile
constexpr int FDK_SLICES = 8;    // slices a thread walks down: t, w, U, u and the column tap are formed once per angle for them

// Q[a][r0 + 2 rp (+ 1)][k] = Z[rp][a][k].x (.y): the filtered row pairs of a block into the plan's sinogram of all rows
__global__ __launch_bounds__(256) void k_fdk_unpack(const float2 *__restrict__ Z, float *__restrict__ Q, int A, int n, int m, int L,
                                                    int r0, int npairs) {
    const int64_t N = (int64_t)npairs * A * m;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(p % m);
        const int64_t la = p / m;
        const int a = (int)(la % A), rp = (int)(la / A);
        const float2 z = Z[((int64_t)rp * A + a) * L + k];
        const int r = r0 + 2 * rp;
        const int64_t q = ((int64_t)a * n + r) * m + k;
        Q[q] = z.x;
        if (r + 1 < n) Q[q + m] = z.y;
    }
}

struct FdkArgs {
    const float *Q;           // [A][n][m]: the weighted, filtered sinogram
    const double *cs;         // [A] cos, then [A] sin
    float *vol;               // [n][m][m]
    double center, vcenter, dso;
    float scale;              // pi / (2A)
    int A, n, m, circle;
};

// One thread per voxel column (i, j) and block of FDK_SLICES slices; the angles in ascending order, no atomics.  The four
// taps are read from global memory: neighbouring threads in j read neighbouring columns of the same detector rows.
__global__ __launch_bounds__(256) void k_fdk_backproject(FdkArgs p) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int h = p.m / 2;
    const int j = blockIdx.x * FDK_TILE + (tid & (FDK_TILE - 1)), i = blockIdx.y * FDK_TILE + (tid >> 4);
    const int Z0 = blockIdx.z * FDK_SLICES;
    if (i >= p.m || j >= p.m) return;
    const int nz = min(FDK_SLICES, p.n - Z0);
    float *out = p.vol + ((int64_t)Z0 * p.m + i) * p.m + j;
    const int64_t zstride = (int64_t)p.m * p.m;
    if (!fbp_lit<int64_t>(i, j, h, p.circle)) {
        for (int z = 0; z < nz; ++z) out[z * zstride] = 0.f;
        return;
    }
    float acc[FDK_SLICES];
#pragma unroll
    for (int z = 0; z < FDK_SLICES; ++z) acc[z] = 0.f;
    const double dj = (double)(j - h), di = (double)(i - h);
    const int m = p.m, n = p.n;
    for (int a = 0; a < p.A; ++a) {
        const double c = p.cs[a], s = p.cs[p.A + a];
        const double t = dj * c - di * s, w = dj * s + di * c;
        const double U = p.dso / (p.dso + w);                       // dso + w > 0: |w| <= sqrt(2) h < m <= dso
        const double u = t * U + p.center;
        if (!(u > -1.0 && u < (double)m)) continue;                 // off the detector for every slice
        const FbpTap tu = fbp_tap(u);
        const int ku = (int)tu.fl;                                  // in [-1, m - 1]
        const bool c0 = ku >= 0, c1 = ku + 1 < m;
        const float U2 = (float)(U * U);
        const float *qa = p.Q + (int64_t)a * n * m;                 // the angle's rows; every tap below is indexed inside them
#pragma unroll
        for (int z = 0; z < FDK_SLICES; ++z) {
            if (z >= nz) break;
            const double v = ((double)(Z0 + z) - p.vcenter) * U + p.vcenter;
            if (!(v > -1.0 && v < (double)n)) continue;
            const FbpTap tv = fbp_tap(v);
            const int kv = (int)tv.fl;                              // in [-1, n - 1]
            const bool r0 = kv >= 0, r1 = kv + 1 < n;
            const int64_t o0 = (int64_t)kv * m + ku, o1 = o0 + m;   // (kv, ku) and (kv + 1, ku): read only where on the detector
            const float q00 = r0 && c0 ? qa[o0] : 0.f, q01 = r0 && c1 ? qa[o0 + 1] : 0.f;
            const float q10 = r1 && c0 ? qa[o1] : 0.f, q11 = r1 && c1 ? qa[o1 + 1] : 0.f;
            const float lo = fmaf(tu.w1, q01, tu.w0 * q00), hi = fmaf(tu.w1, q11, tu.w0 * q10);
            acc[z] = fmaf(U2, fmaf(tv.w1, hi, tv.w0 * lo), acc[z]);
        }
    }
#pragma unroll
    for (int z = 0; z < FDK_SLICES; ++z)
        if (z < nz) out[z * zstride] = acc[z] * p.scale;
}

// ---- forward projection: sino = B^T vol, the gather form ---------------------------------------------------------------
// Per angle the slice is walked along its major axis: lines of constant i when |cos| >= |sin| (u moves by cos per step of
// the minor index j), lines of constant j otherwise (u moves by -sin per step of i).  |g| = |du/dq| >= 1/sqrt(2), so on
// one line the voxels with a weight on sample k -- those with |u - k| < 1 -- lie in the open interval
// (lo, lo + 2/|g|) of the minor index, lo = q* - 1/|g|, at most 2 sqrt(2) long: at most 3 integers.  lo comes from the
// inverted coordinate, affine in the line index and good to ~2e-9 (|center| <= 2^20, m <= 8192); the candidates are
// floor(lo - 1e-6) + {1, 2, 3}: every integer above lo - 1e-6 and below lo + 2.8285 is among them (1e-6 to spare below,
// 0.17 above).  Each candidate's u, floor and weights are the back-projector's: fbp_u and fbp_tap on (i, j); a candidate outside
// the interval gets the weight 0.  The inverted coordinate only chooses where to look.
constexpr int PRJ_KS = 64;       // samples per workgroup: one per lane
constexpr int PRJ_LINES = 16;    // major-axis lines staged per piece: four per wave
constexpr int PRJ_PARTS = 4;     // partial sums per sample: line L goes to partial L & 3, one wave each
constexpr int PRJ_CAND = 3;      // candidates per line and sample
// Minor indices one staged line holds: floor(lo - 1e-6) of the 64 samples spans at most ceil(63/|g|) + 1 values from the
// base (the smallest) on, the first candidate is one above it and two more follow: ceil(63/|g|) + 4 <= 94.  97 keeps the
// lines of a piece on different LDS banks when they are filled line-fastest; a fill takes 6 rounds of 16 or 32 indices.
constexpr int PRJ_W = 97;

struct PrjArgs {
    const float *vol;         // [n][m][m]
    const double *cs;         // [A] cos, then [A] sin
    float *sino;              // [A][n][m]
    double center;
    int A, n, m, r0, circle, runs;
};

__global__ __launch_bounds__(256) void k_fbp_project(PrjArgs p) {
    __shared__ float4 seg[PRJ_LINES][PRJ_W];         // seg[l][x] = the four rows' voxel (line L0 + l, minor sbase[l] + x), 0 if unlit
    __shared__ float4 part[PRJ_PARTS][PRJ_KS];
    __shared__ int sbase[2][PRJ_LINES];

    const int tid = threadIdx.x;
    const int ks = tid & (PRJ_KS - 1), wv = tid >> 6;
    const int a = blockIdx.x / p.runs, k0 = (blockIdx.x % p.runs) * PRJ_KS;
    const int rb = p.r0 + blockIdx.y * FBP_ROWS;
    const int m = p.m, h = m / 2;
    const double c = p.cs[a], s = p.cs[p.A + a];
    const bool alongj = fabs(c) >= fabs(s);          // the minor index is j (lines of constant i); 45 degrees goes here
    // lo(k, L) = h + (k - center + (L - h) s)/c - 1/|c| along j, h + (k - center - (L - h) c)/(-s) - 1/|s| along i
    const double inv = 1.0 / (alongj ? c : -s), reach = fabs(inv), slope = (alongj ? s : -c) * inv;
    const double off = (double)h - (double)h * slope - reach - 1e-6 - p.center * inv;
    const double kd = (double)(k0 + ks);
    const double lo_k = fma(kd, inv, off);                                          // the thread's lo at L = 0
    const double lo_a = fma((double)k0, inv, off), lo_b = fma((double)(k0 + PRJ_KS - 1), inv, off);
    const int wneed = (int)ceil((double)(PRJ_KS - 1) * reach) + 4;                  // <= 94
    const int64_t mm = (int64_t)m * m;
    // rows of the block that exist: the others are read from row 0 and zeroed
    const int nr = p.n - rb;
    const float *const vol0 = p.vol + (int64_t)rb * mm;
    const int64_t o1 = nr > 1 ? mm : 0, o2 = nr > 2 ? 2 * mm : 0, o3 = nr > 3 ? 3 * mm : 0;

    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int piece = 0;
    for (int L0 = 0; L0 < m; L0 += PRJ_LINES, ++piece) {
        int *const base = sbase[piece & 1];
        int live = 0;
        if (tid < PRJ_LINES) {
            const int L = L0 + tid;
            const double Ld = (double)L;
            const int b = (int)floor(fmin(fma(Ld, slope, lo_a), fma(Ld, slope, lo_b)));
            base[tid] = b;
            if (L < m) {
                // the lit voxels of the line: |q - h| <= sqrt(h^2 - (L - h)^2), one more on either side for the root's rounding
                const double dl = (double)(L - h);
                const double half = p.circle ? sqrt(fmax((double)h * h - dl * dl, 0.0)) + 1.0 : (double)m;
                const double lo = fmax(0.0, (double)h - half), hi = fmin((double)(m - 1), (double)h + half);
                live = (double)(b + wneed) > lo && (double)b <= hi;
            }
        }
        if (!__syncthreads_or(live)) continue;       // no voxel of these lines can reach the samples: the same for the whole workgroup

        // fill: six rounds, the slice's j fastest whichever axis is major; every load is in bounds (clamped) and
        // unconditional, so that the 24 of a thread are in flight together, and what is outside or unlit is zeroed after
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int l = alongj ? (tid >> 5) + 8 * (it & 1) : tid & 15;
            const int x = alongj ? (tid & 31) + 32 * (it >> 1) : (tid >> 4) + 16 * it;
            const int L = L0 + l, q = base[l] + x;
            const int Lc = L < m ? L : m - 1, qc = q < 0 ? 0 : q < m ? q : m - 1;
            const bool ok = L < m && q >= 0 && q < m && fbp_lit<int>(Lc, qc, h, p.circle);   // inside the slice: int is exact
            const float *src = vol0 + (alongj ? (int64_t)Lc * m + qc : (int64_t)qc * m + Lc);
            float4 v = make_float4(src[0], src[o1], src[o2], src[o3]);
            if (nr < 4) {
                if (nr < 2) v.y = 0.f;
                if (nr < 3) v.z = 0.f;
                v.w = 0.f;
            }
            if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (x < wneed) seg[l][x] = v;
        }
        __syncthreads();

#pragma unroll
        for (int t = 0; t < PRJ_LINES / PRJ_PARTS; ++t) {
            const int l = wv + PRJ_PARTS * t, L = L0 + l;
            const double dl = (double)(L - h);
            int x = (int)floor(fma((double)L, slope, lo_k)) + 1 - base[l];
            x = x < 0 ? 0 : x > wneed - PRJ_CAND ? wneed - PRJ_CAND : x;   // never taken: keeps the reads inside the filled line whatever the arithmetic did
            const int q = base[l] + x;
#pragma unroll
            for (int e = 0; e < PRJ_CAND; ++e) {
                const double dq = (double)(q + e - h);
                // (i, j) = (L, q + e) along j, (q + e, L) along i: the orientation only chooses u's arguments
                const FbpTap tap = fbp_tap(alongj ? fbp_u(dq, -dl, c, s, p.center) : fbp_u(dl, -dq, c, s, p.center));
                const float wt = tap.fl == kd ? tap.w0 : tap.fl + 1.0 == kd ? tap.w1 : 0.f;
                const float4 v = seg[l][x + e];
                acc.x = fmaf(wt, v.x, acc.x);
                acc.y = fmaf(wt, v.y, acc.y);
                acc.z = fmaf(wt, v.z, acc.z);
                acc.w = fmaf(wt, v.w, acc.w);
            }
        }
    }
    part[wv][ks] = acc;
    __syncthreads();
    const int k = k0 + ks;
    if (wv != 0 || k >= m) return;
    const float4 p0 = part[0][ks], p1 = part[1][ks], p2 = part[2][ks], p3 = part[3][ks];
    float *const dst = p.sino + ((int64_t)a * p.n + rb) * m + k;
    dst[0] = (p0.x + p1.x) + (p2.x + p3.x);
    if (nr > 1) dst[m] = (p0.y + p1.y) + (p2.y + p3.y);
    if (nr > 2) dst[2 * (int64_t)m] = (p0.z + p1.z) + (p2.z + p3.z);
    if (nr > 3) dst[3 * (int64_t)m] = (p0.w + p1.w) + (p2.w + p3.w);
}

// ---- the total-variation step of the primal-dual solver (psx_fbp_tv_step_f32; the contract is in include/paresis_hip.h) --
// One workgroup per 8 x 32 tile of one slice, one voxel per thread.  xbar is staged with a one-voxel halo; the projected
// dual p' is then formed for the tile plus the row above and the column to the left -- the two neighbours whose p' enter a
// voxel's divergence -- by ONE loop, so a value a neighbouring workgroup also forms comes from the same instructions on the
// same inputs: the same bits.  Each voxel then reads u, c, x, xbar, px, py once (the halo comes from cache) and writes x,
// xbar, px, py: 40 bytes.
constexpr int TV_TW = 32;        // tile width (slice columns j): a wave covers two rows of 128 bytes
constexpr int TV_TH = 8;         // tile height (slice rows i)

struct TvArgs {
    const float *u, *c;       // [n][m][m]: B y, and C = B 1
    float *x;                 // in place
    const float *xbar_in, *px_in, *py_in;
    float *xbar_out, *px_out, *py_out;
    float lambda;
    int m, r0, circle, nonneg;
};

__global__ __launch_bounds__(256) void k_fbp_tv_step(TvArgs p) {
    __shared__ float sx[TV_TH + 2][TV_TW + 2];       // xbar of (i0 - 1 + li, j0 - 1 + lj), 0 outside the slice
    __shared__ float spx[TV_TH + 1][TV_TW + 1];      // p' of (i0 - 1 + li, j0 - 1 + lj)
    __shared__ float spy[TV_TH + 1][TV_TW + 1];
    __shared__ unsigned char sact[TV_TH + 1][TV_TW + 1];   // bit 0: the difference along i is active, bit 1: along j

    const int tid = threadIdx.x;
    const int m = p.m, h = m / 2;
    const int j0 = blockIdx.x * TV_TW, i0 = blockIdx.y * TV_TH;
    const int64_t slice = (int64_t)(p.r0 + (int)blockIdx.z) * m * m;
    const int circle = p.circle;
    auto lit = [m, h, circle](int i, int j) {
        return i >= 0 && i < m && j >= 0 && j < m && fbp_lit<int64_t>(i, j, h, circle);
    };

    // every global load of the workgroup is issued before the first barrier, so that all of them are in flight together:
    // two elements of the staged xbar and of the p' region per thread (340 and 297 elements), then the thread's own voxel
    constexpr int NX = (TV_TH + 2) * (TV_TW + 2), NP = (TV_TH + 1) * (TV_TW + 1);
    float xb_ld[2], px_ld[2], py_ld[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int e = tid + 256 * r;
        const int xi = i0 - 1 + e / (TV_TW + 2), xj = j0 - 1 + e % (TV_TW + 2);
        const bool xin = e < NX && xi >= 0 && xi < m && xj >= 0 && xj < m;
        xb_ld[r] = xin ? p.xbar_in[slice + (int64_t)xi * m + xj] : 0.f;
        const int pi = i0 - 1 + e / (TV_TW + 1), pj = j0 - 1 + e % (TV_TW + 1);
        const bool pin = e < NP && pi >= 0 && pi < m && pj >= 0 && pj < m;
        px_ld[r] = pin ? p.px_in[slice + (int64_t)pi * m + pj] : 0.f;
        py_ld[r] = pin ? p.py_in[slice + (int64_t)pi * m + pj] : 0.f;
    }
    const int li = tid / TV_TW, lj = tid % TV_TW;
    const int i = i0 + li, j = j0 + lj;
    const bool own = i < m && j < m;
    const int64_t q = slice + (int64_t)(own ? i : 0) * m + (own ? j : 0);
    const float u = own ? p.u[q] : 0.f, c = own ? p.c[q] : 0.f, x = own ? p.x[q] : 0.f;

#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int e = tid + 256 * r;
        if (e < NX) sx[e / (TV_TW + 2)][e % (TV_TW + 2)] = xb_ld[r];
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int e = tid + 256 * r;
        if (e >= NP) break;
        const int pl = e / (TV_TW + 1), pc = e % (TV_TW + 1);
        const int pi = i0 - 1 + pl, pj = j0 - 1 + pc;
        float px = 0.f, py = 0.f;
        unsigned act = 0;
        if (pi >= 0 && pi < m && pj >= 0 && pj < m) {
            const bool here = lit(pi, pj);
            const bool ax = here && lit(pi + 1, pj), ay = here && lit(pi, pj + 1);
            act = (ax ? 1u : 0u) | (ay ? 2u : 0u);
            const float xb = sx[pl][pc];
            const float gx = ax ? sx[pl + 1][pc] - xb : 0.f, gy = ay ? sx[pl][pc + 1] - xb : 0.f;
            px = fmaf(0.5f, gx, px_ld[r]);
            py = fmaf(0.5f, gy, py_ld[r]);
            const float nr = sqrtf(fmaf(px, px, __fmul_rn(py, py)));
            if (nr > p.lambda) {                     // nr > lambda >= 0: no division by zero
                const float s = p.lambda / nr;
                px = __fmul_rn(px, s);
                py = __fmul_rn(py, s);
            }
        }
        spx[pl][pc] = px;
        spy[pl][pc] = py;
        sact[pl][pc] = (unsigned char)act;
    }
    __syncthreads();

    if (!own) return;
    const unsigned here = sact[li + 1][lj + 1], up = sact[li][lj + 1] & 1u, left = sact[li + 1][lj] & 2u;
    const float pxc = spx[li + 1][lj + 1], pyc = spy[li + 1][lj + 1];
    p.px_out[q] = pxc;
    p.py_out[q] = pyc;
    // d = px'[i-1][j] - px'[i][j] + py'[i][j-1] - py'[i][j], the inactive differences' terms 0, summed left to right
    float d = (up ? spx[li][lj + 1] : 0.f) - ((here & 1u) ? pxc : 0.f);
    d = __fadd_rn(d, left ? spy[li + 1][lj] : 0.f);
    d = __fsub_rn(d, (here & 2u) ? pyc : 0.f);
    const int deg = (int)(here & 1u) + (int)(here >> 1) + (int)up + (int)(left >> 1);
    const float cd = c + (float)deg;
    const float tau = cd > 1e-6f ? 1.0f / cd : 0.f;
    float xn = fmaf(-tau, __fadd_rn(u, d), x);
    if (p.nonneg) xn = fmaxf(xn, 0.f);
    p.x[q] = xn;
    p.xbar_out[q] = fmaf(2.0f, xn, -x);
}

// in-place radix-2 transform of a power-of-two length in float64 (the filter table: once per plan)
void fft_f64(std::vector<std::complex<double>> &x) {
    const size_t n = x.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(x[i], x[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const double ang = -PSX_TWO_PI * (double)k / (double)len;
                const std::complex<double> w(std::cos(ang), std::sin(ang));
                const std::complex<double> u = x[i + k], v = x[i + k + len / 2] * w;
                x[i + k] = u + v;
                x[i + k + len / 2] = u - v;
            }
    }
}

// The table the filter kernel multiplies by, the inverse transform's 1/P folded in.  Ramp filters: He[k]/P, the even part of
// H = 2 Re FFT(f).  Hilbert filters (PSX_FBP_DIFFERENTIAL): Ho[k]/P, the odd part of H = Im FFT(g) with H[0] = H[P/2] = 0,
// g[j] = 2/(pi^2 s) for odd signed lag s.  Either H is first multiplied by the shifted Hann window if the filter has one.
std::vector<double> filter_table(int P, int filter) {
    const bool differential = (filter & PSX_FBP_DIFFERENTIAL) != 0;
    const bool hann = (filter & ~PSX_FBP_DIFFERENTIAL) == PSX_FBP_HANN;
    std::vector<std::complex<double>> f((size_t)P);
    for (int jx = 0; jx < P; ++jx) {
        const int jj = jx < P - jx ? jx : P - jx;
        const double pj = M_PI * (double)jj;
        if (differential)
            f[jx] = (jj & 1) ? (jx < P / 2 ? 2.0 : -2.0) / (M_PI * pj) : 0.0;
        else
            f[jx] = jx == 0 ? 0.25 : (jj & 1) ? -1.0 / (pj * pj) : 0.0;
    }
    fft_f64(f);
    std::vector<double> H((size_t)P), T((size_t)P);
    for (int k = 0; k < P; ++k) {
        H[k] = differential ? (k == 0 || k == P / 2 ? 0.0 : f[k].imag()) : 2.0 * f[k].real();
        if (hann) {
            const int nn = (k + P / 2) % P;                       // fftshift of an even length
            H[k] *= 0.5 - 0.5 * std::cos(PSX_TWO_PI * (double)nn / (double)(P - 1));
        }
    }
    const double sign = differential ? -1.0 : 1.0;
    for (int k = 0; k < P; ++k) T[k] = 0.5 * (H[k] + sign * H[(P - k) % P]) / (double)P;
    return T;
}

}  // namespace

struct psx_fbp_plan {
    int A = 0, m = 0, P = 0, L = 0, filter = 0, circle = 0, max_rows = 0;
    double center = 0.0;
    size_t bytes = 0;
    FftPlan fft;              // forward + inverse, P points, A lines (one row pair)
    DevBuf<float2> Z;         // [max_rows / 2][A][L]
    DevBuf<double> cs;        // [A] cos, [A] sin
    DevBuf<double> table;     // [P]: filter_table's
};

// What the plan's three operators ask of (plan, the two arrays, n).  NAME and WHAT are literals: each message is the
// entry point's own text.
#define FBP_REQUIRE_RANGE(NAME, WHAT, plan, a, b, n)                                                                           \
    PSX_REQUIRE(plan != nullptr, NAME ": null plan");                                                                          \
    PSX_REQUIRE(a != nullptr && b != nullptr, NAME ": null " WHAT);                                                            \
    PSX_REQUIRE(n >= 1 && (int64_t)n * plan->A * plan->m <= (int64_t)1 << 40 && (int64_t)n * plan->m * plan->m <= (int64_t)1 << 40, \
                NAME ": n=%d detector rows outside [1, 2^40 elements]", n)

// Z = the filtered lines (the packed ones, unless `filtered`) of the row pairs [r0, r0 + 2 npairs) of sino, each sample
// times wt's weight: the first half of psx_fbp_f32 and of psx_fdk_f32.  Inlined into its callers, so that the library's
// symbols stay what they were.
template <typename Weight>
__attribute__((always_inline)) static inline int fbp_filter_rows(psx_fbp_plan *plan, const float *sino, int n, int r0, int npairs,
                                                                 bool filtered, Weight wt, hipStream_t st) {
    const int A = plan->A, m = plan->m, L = plan->L;
    float2 *const Z = plan->Z.get();
    const int64_t N = (int64_t)npairs * A * L;
    PSX_TIMED("k_fbp_pack", st, k_fbp_pack<<<ew_grid(N, 256), 256, 0, st>>>(sino, Z, A, n, m, L, r0, npairs, wt));
    if (int rc = launch_check("k_fbp_pack")) return rc;
    if (filtered) {
        for (int rp = 0; rp < npairs; ++rp)
            if (int rc = plan->fft.execute(FftPlan::FWD, Z + (size_t)rp * A * L, st, "rocfft_fbp_forward")) return rc;
        if (plan->filter & PSX_FBP_DIFFERENTIAL)
            PSX_TIMED("k_fbp_filter_hilbert", st, k_fbp_filter<true><<<ew_grid(N, 256), 256, 0, st>>>(Z, plan->table.get(), plan->P, N));
        else
            PSX_TIMED("k_fbp_filter", st, k_fbp_filter<false><<<ew_grid(N, 256), 256, 0, st>>>(Z, plan->table.get(), plan->P, N));
        if (int rc = launch_check("k_fbp_filter")) return rc;
        for (int rp = 0; rp < npairs; ++rp)
            if (int rc = plan->fft.execute(FftPlan::INV, Z + (size_t)rp * A * L, st, "rocfft_fbp_inverse")) return rc;
    }
    return 0;
}

// vol = scale * B sino, by row blocks of the plan's max_rows: pack, with `filtered` the plan's filter, back-projection.
// Inlined into its two entry points, so that the library's symbols stay what they were.
__attribute__((always_inline)) static inline int fbp_backproject(psx_fbp_plan *plan, const float *sino, int n, float *vol,
                                                                 bool filtered, float scale, hipStream_t st) {
    const int A = plan->A, m = plan->m, L = plan->L;
    float2 *const Z = plan->Z.get();
    const int tiles = (int)cdiv(m, FBP_TILE);
    for (int r0 = 0; r0 < n; r0 += plan->max_rows) {
        const int rows = n - r0 < plan->max_rows ? n - r0 : plan->max_rows;
        const int npairs = (rows + 1) / 2;
        if (int rc = fbp_filter_rows(plan, sino, n, r0, npairs, filtered, NoWeight{}, st)) return rc;
        FbpArgs a;
        a.Z = Z; a.cs = plan->cs.get(); a.vol = vol; a.center = plan->center; a.scale = scale;
        a.A = A; a.n = n; a.m = m; a.L = L; a.r0 = r0; a.npairs = npairs; a.circle = plan->circle;
        const dim3 grid((unsigned)tiles, (unsigned)tiles, (unsigned)cdiv(rows, FBP_ROWS));
        PSX_TIMED("k_fbp_backproject", st, k_fbp_backproject<<<grid, 256, 0, st>>>(a));
        if (int rc = launch_check("k_fbp_backproject")) return rc;
    }
    return 0;
}

// FDK's plan: a parallel plan for the tables, the transform and the row-block buffer, and the filtered sinogram of all rows
struct psx_fdk_plan {
    int n = 0;
    double vcenter = 0.0, dso = 0.0;
    psx_fbp_plan *base = nullptr;
    DevBuf<float> Q;          // [A][n][m]
    ~psx_fdk_plan() { delete base; }
};

extern "C" {

int psx_fbp_plan_create(int A, int m, const double *theta_deg, double center, int filter, int circle, int max_rows,
                        psx_fbp_plan **plan) {
    PSX_REQUIRE(plan != nullptr, "psx_fbp_plan_create: null plan pointer");
    *plan = nullptr;
    PSX_REQUIRE(A >= 1 && A <= PSX_FBP_MAX_ANGLES, "psx_fbp_plan_create: A=%d angles outside [1,%d]", A, PSX_FBP_MAX_ANGLES);
    PSX_REQUIRE(m >= 2 && m <= PSX_FBP_MAX_M, "psx_fbp_plan_create: m=%d detector columns outside [2,%d]", m, PSX_FBP_MAX_M);
    PSX_REQUIRE(theta_deg != nullptr, "psx_fbp_plan_create: null theta array");
    for (int a = 0; a < A; ++a)
        PSX_REQUIRE(std::isfinite(theta_deg[a]), "psx_fbp_plan_create: theta[%d]=%g is not finite", a, theta_deg[a]);
    PSX_REQUIRE(std::isfinite(center) && std::fabs(center) <= 1048576.0, "psx_fbp_plan_create: center=%g is not a finite column within 2^20", center);
    PSX_REQUIRE(filter == PSX_FBP_RAMP || filter == PSX_FBP_HANN || filter == PSX_FBP_NONE || filter == PSX_FBP_HILBERT ||
                filter == PSX_FBP_HILBERT_HANN, "psx_fbp_plan_create: unknown filter %d", filter);
    PSX_REQUIRE(circle == 0 || circle == 1, "psx_fbp_plan_create: circle=%d is not 0 or 1", circle);
    PSX_REQUIRE(max_rows >= 0 && max_rows <= 4096, "psx_fbp_plan_create: max_rows=%d outside [0,4096]", max_rows);

    std::unique_ptr<psx_fbp_plan> p(new psx_fbp_plan());
    p->A = A; p->m = m; p->filter = filter; p->circle = circle; p->center = center;
    int P = 64;
    while (P < 2 * m) P <<= 1;
    p->P = P;
    p->L = filter == PSX_FBP_NONE ? m : P;
    if (max_rows == 0) {
        const int64_t fit = ((int64_t)256 << 20) / ((int64_t)A * p->L * (int64_t)sizeof(float2));   // row pairs in 256 MiB
        max_rows = (int)(fit < 1 ? 2 : fit > 32 ? 64 : 2 * fit);
    }
    p->max_rows = max_rows + (max_rows & 1);

    std::vector<double> cs(2 * (size_t)A);
    for (int a = 0; a < A; ++a) {
        const double th = theta_deg[a] * (M_PI / 180.0);
        cs[a] = std::cos(th);
        cs[(size_t)A + a] = std::sin(th);
    }
    if (int rc = p->cs.upload(cs.data(), cs.size())) return rc;
    if (filter != PSX_FBP_NONE) {
        const std::vector<double> table = filter_table(P, filter);
        if (int rc = p->table.upload(table.data(), table.size())) return rc;
        const size_t lengths[1] = {(size_t)P};
        if (int rc = p->fft.create(FftPlan::BOTH, rocfft_precision_single, 1, lengths, (size_t)A)) return rc;
    }
    if (int rc = p->Z.alloc((size_t)(p->max_rows / 2) * A * p->L)) return rc;
    p->bytes = p->Z.bytes() + p->cs.bytes() + p->table.bytes() + p->fft.work_bytes();
    *plan = p.release();
    return 0;
}

int psx_fbp_plan_destroy(psx_fbp_plan *plan) {
    delete plan;
    return 0;
}

size_t psx_fbp_plan_bytes(const psx_fbp_plan *plan) { return plan ? plan->bytes : 0; }

int psx_fbp_f32(psx_fbp_plan *plan, const float *sino, int n, float *vol, void *stream) {
    FBP_REQUIRE_RANGE("psx_fbp_f32", "sinogram or volume", plan, sino, vol, n);
    return fbp_backproject(plan, sino, n, vol, plan->filter != PSX_FBP_NONE, (float)(M_PI / (2.0 * (double)plan->A)),
                           (hipStream_t)stream);
}

int psx_fbp_project_f32(psx_fbp_plan *plan, const float *vol, int n, float *sino, void *stream) {
    FBP_REQUIRE_RANGE("psx_fbp_project_f32", "volume or sinogram", plan, vol, sino, n);
    hipStream_t st = (hipStream_t)stream;
    PrjArgs a;
    a.vol = vol; a.cs = plan->cs.get(); a.sino = sino; a.center = plan->center;
    a.A = plan->A; a.n = n; a.m = plan->m; a.circle = plan->circle; a.runs = (int)cdiv(plan->m, PRJ_KS);
    const int step = FBP_ROWS * 32768;               // rows per launch: grid.y stays below 65536
    for (int r0 = 0; r0 < n; r0 += step) {
        const int rows = n - r0 < step ? n - r0 : step;
        a.r0 = r0;
        // x: the sample runs of one angle, then the angles; y: the blocks of four rows -- every angle of a block runs
        // before the next block starts, so its four slices are read from cache
        const dim3 grid((unsigned)(a.runs * a.A), (unsigned)cdiv(rows, FBP_ROWS));
        PSX_TIMED("k_fbp_project", st, k_fbp_project<<<grid, 256, 0, st>>>(a));
        if (int rc = launch_check("k_fbp_project")) return rc;
    }
    return 0;
}

int psx_fbp_adjoint_f32(psx_fbp_plan *plan, const float *sino, int n, float *vol, void *stream) {
    FBP_REQUIRE_RANGE("psx_fbp_adjoint_f32", "sinogram or volume", plan, sino, vol, n);
    return fbp_backproject(plan, sino, n, vol, false, 1.0f, (hipStream_t)stream);
}

int psx_fbp_tv_step_f32(psx_fbp_plan *plan, int n, double lambda, int nonneg, const float *u, const float *c, float *x,
                        const float *xbar_in, float *xbar_out, const float *px_in, const float *py_in, float *px_out,
                        float *py_out, void *stream) {
    PSX_REQUIRE(plan != nullptr, "psx_fbp_tv_step_f32: null plan");
    PSX_REQUIRE(u != nullptr && c != nullptr && x != nullptr && xbar_in != nullptr && xbar_out != nullptr && px_in != nullptr &&
                py_in != nullptr && px_out != nullptr && py_out != nullptr, "psx_fbp_tv_step_f32: null volume pointer");
    PSX_REQUIRE(n >= 1, "psx_fbp_tv_step_f32: n=%d slices, at least 1", n);
    PSX_REQUIRE(std::isfinite(lambda) && lambda >= 0.0, "psx_fbp_tv_step_f32: lambda=%g is not a finite weight >= 0", lambda);
    PSX_REQUIRE(xbar_out != xbar_in && px_out != px_in && py_out != py_in,
                "psx_fbp_tv_step_f32: xbar_out, px_out and py_out must not be their own inputs (neighbouring tiles read them)");
    PSX_REQUIRE(xbar_out != x, "psx_fbp_tv_step_f32: xbar_out must not be x");
    PSX_REQUIRE((int64_t)n * plan->m * plan->m <= (int64_t)1 << 40, "psx_fbp_tv_step_f32: n=%d slices outside [1, 2^40 elements]", n);
    hipStream_t st = (hipStream_t)stream;
    TvArgs a;
    a.u = u; a.c = c; a.x = x; a.xbar_in = xbar_in; a.px_in = px_in; a.py_in = py_in;
    a.xbar_out = xbar_out; a.px_out = px_out; a.py_out = py_out;
    a.lambda = (float)lambda; a.m = plan->m; a.circle = plan->circle; a.nonneg = nonneg != 0;
    const int step = 32768;                          // slices per launch: grid.z stays below 65536
    for (int r0 = 0; r0 < n; r0 += step) {
        a.r0 = r0;
        const dim3 grid((unsigned)cdiv(plan->m, TV_TW), (unsigned)cdiv(plan->m, TV_TH), (unsigned)(n - r0 < step ? n - r0 : step));
        PSX_TIMED("k_fbp_tv_step", st, k_fbp_tv_step<<<grid, 256, 0, st>>>(a));
        if (int rc = launch_check("k_fbp_tv_step")) return rc;
    }
    return 0;
}

int psx_fdk_plan_create(int A, int n, int m, const double *theta_deg, double center, double vcenter, double dso, int filter,
                        int circle, psx_fdk_plan **plan) {
    PSX_REQUIRE(plan != nullptr, "psx_fdk_plan_create: null plan pointer");
    *plan = nullptr;
    PSX_REQUIRE(filter == PSX_FBP_RAMP || filter == PSX_FBP_HANN || filter == PSX_FBP_NONE,
                "psx_fdk_plan_create: filter %d is not PSX_FBP_RAMP, _HANN or _NONE (FDK has no differential form)", filter);
    PSX_REQUIRE(n >= 1 && n <= 65535, "psx_fdk_plan_create: n=%d detector rows outside [1,65535]", n);
    PSX_REQUIRE(A >= 1 && A <= PSX_FBP_MAX_ANGLES && m >= 2 && m <= PSX_FBP_MAX_M,
                "psx_fdk_plan_create: A=%d angles outside [1,%d] or m=%d detector columns outside [2,%d]", A, PSX_FBP_MAX_ANGLES, m,
                PSX_FBP_MAX_M);
    PSX_REQUIRE((int64_t)A * n * m <= PSX_FDK_MAX_SAMPLES,
                "psx_fdk_plan_create: the filtered sinogram of %d x %d x %d samples is outside [1, 2^31]", A, n, m);
    PSX_REQUIRE(std::isfinite(vcenter) && std::fabs(vcenter) <= 1048576.0,
                "psx_fdk_plan_create: vcenter=%g is not a finite row within 2^20", vcenter);
    PSX_REQUIRE(dso >= (double)m && dso <= 1e30, "psx_fdk_plan_create: dso=%g outside [m=%d, 1e30] voxels", dso, m);
    std::unique_ptr<psx_fdk_plan> p(new psx_fdk_plan());
    if (int rc = psx_fbp_plan_create(A, m, theta_deg, center, filter, circle, 0, &p->base)) return rc;
    p->n = n; p->vcenter = vcenter; p->dso = dso;
    if (int rc = p->Q.alloc((size_t)A * n * m)) return rc;
    *plan = p.release();
    return 0;
}

int psx_fdk_plan_destroy(psx_fdk_plan *plan) {
    delete plan;
    return 0;
}

size_t psx_fdk_plan_bytes(const psx_fdk_plan *plan) { return plan ? plan->base->bytes + plan->Q.bytes() : 0; }

int psx_fdk_f32(psx_fdk_plan *plan, const float *sino, float *vol, void *stream) {
    PSX_REQUIRE(plan != nullptr, "psx_fdk_f32: null plan");
    PSX_REQUIRE(sino != nullptr && vol != nullptr, "psx_fdk_f32: null sinogram or volume");
    hipStream_t st = (hipStream_t)stream;
    psx_fbp_plan *base = plan->base;
    const int A = base->A, m = base->m, n = plan->n;
    PSX_REQUIRE((int64_t)n * m * m <= (int64_t)1 << 40, "psx_fdk_f32: a volume of %d x %d x %d voxels is outside 2^40", n, m, m);
    const ConeWeight wt{plan->dso, base->center, plan->vcenter};
    for (int r0 = 0; r0 < n; r0 += base->max_rows) {
        const int rows = n - r0 < base->max_rows ? n - r0 : base->max_rows;
        const int npairs = (rows + 1) / 2;
        if (int rc = fbp_filter_rows(base, sino, n, r0, npairs, base->filter != PSX_FBP_NONE, wt, st)) return rc;
        PSX_TIMED("k_fdk_unpack", st, k_fdk_unpack<<<ew_grid((int64_t)npairs * A * m, 256), 256, 0, st>>>(
                      base->Z.get(), plan->Q.get(), A, n, m, base->L, r0, npairs));
        if (int rc = launch_check("k_fdk_unpack")) return rc;
    }
    FdkArgs a;
    a.Q = plan->Q.get(); a.cs = base->cs.get(); a.vol = vol; a.center = base->center; a.vcenter = plan->vcenter; a.dso = plan->dso;
    a.scale = (float)(M_PI / (2.0 * (double)A)); a.A = A; a.n = n; a.m = m; a.circle = base->circle;
    const int tiles = (int)cdiv(m, FDK_TILE);
    const dim3 grid((unsigned)tiles, (unsigned)tiles, (unsigned)cdiv(n, FDK_SLICES));
    PSX_TIMED("k_fdk_backproject", st, k_fdk_backproject<<<grid, 256, 0, st>>>(a));
    return launch_check("k_fdk_backproject");
}

}  // extern "C"
