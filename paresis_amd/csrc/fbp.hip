// fbp.hip -- filtered back-projection of a stack of projections (psx_fbp_*; the contract is in include/paresis_hip.h).
//   k_fbp_pack     Z[rp][a][k] = (sino[a][r0+2rp][k], sino[a][r0+2rp+1][k]) for k < m, 0 up to the line's length L: two
//                  detector rows per complex line (L = P with a filter, m without)
//   rocFFT         P-point forward transforms, A lines per row pair and launch
//   k_fbp_filter   Z *= He/P, He the even part of the real filter H (float64 table): the pair stays separable
//   rocFFT         inverse; Z.x / Z.y are now the filtered lines of the two rows
//   k_fbp_backproject   one workgroup per 16 x 16 tile of the slice and block of 4 detector rows (two row pairs)
// The filtered sinogram is never cropped or copied: the back-projector reads the float2 lines of Z as they are, and a row
// pair of Z is the (row, row + 1) interleave its LDS image wants.
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

__global__ __launch_bounds__(256) void k_fbp_pack(const float *__restrict__ sino, float2 *__restrict__ Z, int A, int n, int m,
                                                  int L, int r0, int npairs) {
    const int64_t N = (int64_t)npairs * A * L;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(p % L);
        const int64_t la = p / L;
        const int a = (int)(la % A), rp = (int)(la / A);
        float2 z = make_float2(0.f, 0.f);
        if (k < m) {
            const int r = r0 + 2 * rp;
            const int64_t q = ((int64_t)a * n + r) * m + k;
            z.x = sino[q];
            if (r + 1 < n) z.y = sino[q + m];
        }
        Z[p] = z;
    }
}

__global__ __launch_bounds__(256) void k_fbp_filter(float2 *__restrict__ Z, const double *__restrict__ He, int P, int64_t N) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const double w = He[p & (P - 1)];
        const float2 z = Z[p];
        Z[p] = make_float2((float)((double)z.x * w), (float)((double)z.y * w));
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
    const bool lit = voxel && (!p.circle || (int64_t)(i - h) * (i - h) + (int64_t)(j - h) * (j - h) <= (int64_t)h * h);

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
                const double u00 = fma(cj0, c, fma(ci0, s, p.center)), u01 = fma(cj1, c, fma(ci0, s, p.center));
                const double u10 = fma(cj0, c, fma(ci1, s, p.center)), u11 = fma(cj1, c, fma(ci1, s, p.center));
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
                const double u = fma(dj, scos[a], fma(ndi, ssin[a], p.center));
                const double fl = floor(u);
                const float w1 = (float)(u - fl), w0 = 1.0f - w1;
                int k = (int)fl - sbase[a];
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

// He[k]/P: the even part of H = 2 Re FFT(f) (times the shifted Hann window), the inverse transform's 1/P folded in
std::vector<double> filter_table(int P, int filter) {
    std::vector<std::complex<double>> f((size_t)P);
    for (int jx = 0; jx < P; ++jx) {
        const int jj = jx < P - jx ? jx : P - jx;
        const double pj = M_PI * (double)jj;
        f[jx] = jx == 0 ? 0.25 : (jj & 1) ? -1.0 / (pj * pj) : 0.0;
    }
    fft_f64(f);
    std::vector<double> H((size_t)P), He((size_t)P);
    for (int k = 0; k < P; ++k) {
        H[k] = 2.0 * f[k].real();
        if (filter == PSX_FBP_HANN) {
            const int nn = (k + P / 2) % P;                       // fftshift of an even length
            H[k] *= 0.5 - 0.5 * std::cos(PSX_TWO_PI * (double)nn / (double)(P - 1));
        }
    }
    for (int k = 0; k < P; ++k) He[k] = 0.5 * (H[k] + H[(P - k) % P]) / (double)P;
    return He;
}

}  // namespace

struct psx_fbp_plan {
    int A = 0, m = 0, P = 0, L = 0, filter = 0, circle = 0, max_rows = 0;
    double center = 0.0;
    size_t bytes = 0;
    FftPlan fft;              // forward + inverse, P points, A lines (one row pair)
    DevBuf<float2> Z;         // [max_rows / 2][A][L]
    DevBuf<double> cs;        // [A] cos, [A] sin
    DevBuf<double> He;        // [P]
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
    PSX_REQUIRE(filter == PSX_FBP_RAMP || filter == PSX_FBP_HANN || filter == PSX_FBP_NONE, "psx_fbp_plan_create: unknown filter %d", filter);
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
        const std::vector<double> He = filter_table(P, filter);
        if (int rc = p->He.upload(He.data(), He.size())) return rc;
        const size_t lengths[1] = {(size_t)P};
        if (int rc = p->fft.create(FftPlan::BOTH, rocfft_precision_single, 1, lengths, (size_t)A)) return rc;
    }
    if (int rc = p->Z.alloc((size_t)(p->max_rows / 2) * A * p->L)) return rc;
    p->bytes = p->Z.bytes() + p->cs.bytes() + p->He.bytes() + p->fft.work_bytes();
    *plan = p.release();
    return 0;
}

int psx_fbp_plan_destroy(psx_fbp_plan *plan) {
    delete plan;
    return 0;
}

size_t psx_fbp_plan_bytes(const psx_fbp_plan *plan) { return plan ? plan->bytes : 0; }

int psx_fbp_f32(psx_fbp_plan *plan, const float *sino, int n, float *vol, void *stream) {
    PSX_REQUIRE(plan != nullptr, "psx_fbp_f32: null plan");
    PSX_REQUIRE(sino != nullptr && vol != nullptr, "psx_fbp_f32: null sinogram or volume");
    PSX_REQUIRE(n >= 1 && (int64_t)n * plan->A * plan->m <= (int64_t)1 << 40 && (int64_t)n * plan->m * plan->m <= (int64_t)1 << 40,
                "psx_fbp_f32: n=%d detector rows outside [1, 2^40 elements]", n);
    hipStream_t st = (hipStream_t)stream;
    const int A = plan->A, m = plan->m, L = plan->L;
    float2 *const Z = plan->Z.get();
    const int tiles = (int)cdiv(m, FBP_TILE);
    for (int r0 = 0; r0 < n; r0 += plan->max_rows) {
        const int rows = n - r0 < plan->max_rows ? n - r0 : plan->max_rows;
        const int npairs = (rows + 1) / 2;
        const int64_t N = (int64_t)npairs * A * L;
        PSX_TIMED("k_fbp_pack", st, k_fbp_pack<<<ew_grid(N, 256), 256, 0, st>>>(sino, Z, A, n, m, L, r0, npairs));
        if (int rc = launch_check("k_fbp_pack")) return rc;
        if (plan->filter != PSX_FBP_NONE) {
            for (int rp = 0; rp < npairs; ++rp)
                if (int rc = plan->fft.execute(FftPlan::FWD, Z + (size_t)rp * A * L, st, "rocfft_fbp_forward")) return rc;
            PSX_TIMED("k_fbp_filter", st, k_fbp_filter<<<ew_grid(N, 256), 256, 0, st>>>(Z, plan->He.get(), plan->P, N));
            if (int rc = launch_check("k_fbp_filter")) return rc;
            for (int rp = 0; rp < npairs; ++rp)
                if (int rc = plan->fft.execute(FftPlan::INV, Z + (size_t)rp * A * L, st, "rocfft_fbp_inverse")) return rc;
        }
        FbpArgs a;
        a.Z = Z; a.cs = plan->cs.get(); a.vol = vol; a.center = plan->center;
        a.scale = (float)(M_PI / (2.0 * (double)A));
        a.A = A; a.n = n; a.m = m; a.L = L; a.r0 = r0; a.npairs = npairs; a.circle = plan->circle;
        const dim3 grid((unsigned)tiles, (unsigned)tiles, (unsigned)cdiv(rows, FBP_ROWS));
        PSX_TIMED("k_fbp_backproject", st, k_fbp_backproject<<<grid, 256, 0, st>>>(a));
        if (int rc = launch_check("k_fbp_backproject")) return rc;
    }
    return 0;
}

}  // extern "C"
