// retrieve.hip -- speckle-tracking phase retrieval of simulated image stacks: LCS (psx_lcs_f32) and Frankot-Chellappa
// integration (psx_integrate_*).
//
// LCS ("Low Coherence System", Quenot et al., Optica 8, 1412, 2021), per detector pixel, over K positions:
//   R_k ~ x0*S_k + x1*g0_k + x2*g1_k,   (g0, g1) = np.gradient(R_k) (unit spacing, edge_order=1),
//   M = sum_k a_k a_k^T, v = sum_k a_k R_k with a_k = (S_k, g0_k, g1_k), in float64;  M x = v;
//   transmission = 1/x0, (dx, dy) = (x1, x2);  x = (1, 0, 0) when det M <= 1e-12 M00 M11 M22 or x0 <= 0, and where a sample
//   the pixel reads is not finite (det or x0 is then NaN or infinite, and every test refuses those).
// LCS-DF (psx_lcs_df_f32; the diffusion term of the X-ray Fokker-Planck model, Morgan & Paganin, Sci. Rep. 9, 17465, 2019):
//   R_k ~ x0*S_k + x1*g0_k + x2*g1_k + x3*L_k, L_k the edge-replicated 5-point Laplacian of R_k in float64;
//   4x4 LDL^T without pivoting; x = (1, 0, 0, 0) when a pivot <= 0, prod d_i <= 1e-12 M00 M11 M22 M33, or x0 <= 0;
//   df = -x3 (detector px^2: a Gaussian blur of per-axis variance s^2 gives df = s^2/2).
// k_lcs, k_lcs_df: one thread per pixel, all K positions in one launch; the gradient's neighbours come from L1/L2 (the rows above
// and below are the neighbouring wavefronts' own rows), so HBM sees every input image about once.
//
// Frankot-Chellappa (IEEE PAMI 10, 1988) with mirror extension, 2n x 2m complex64 grid:
//   k_integ_pack    Z = s*(Gx + i*Gy), Gx odd in axis 0 / even in axis 1, Gy even / odd: both gradients, one transform
//   rocFFT forward, in place
//   k_integ_filter  Gx^(k) = (Z(k) + conj Z(-k))/2, Gy^(k) = (Z(k) - conj Z(-k))/(2i),
//                   P = (-i kx Gx^ - i ky Gy^)/(kx^2 + ky^2), P(0) = 0; one thread owns the pair (k, -k)
//   rocFFT inverse, in place
//   k_integ_crop    phi = Re(.)/(4nm) on the n x m corner
//
// Paganin (J. Microsc. 206, 33, 2002; psx_paganin_f32) on the same plan, two images per transform pair:
//   k_pag_pack      Z = xA + i*xB, x = float32(I/I0 - 1) (1 -> 0 at guarded pixels), mirrored evenly: one thread per source pixel
//   rocFFT forward, in place
//   k_pag_filter    A^(k) = (Z(k) + conj Z(-k))/2, B^(k) = (Z(k) - conj Z(-k))/(2i), Y = fA A^ + i fB B^, f = 1/(1 + alpha k^2)
//   rocFFT inverse, in place
//   k_pag_crop      y = Re / Im (.)/(4nm) on the n x m corner; contact = 1 + y, thickness = -log1p(y)/mu
#include "fresnel_plan.hpp"

using namespace psx;

namespace {

constexpr int LCS_BX = 64, LCS_BY = 4;

// one thread per pixel (i, j) of the n x m images; no barrier, so out-of-range threads leave at once
__global__ __launch_bounds__(LCS_BX * LCS_BY) void k_lcs(SpecklePtrs p, int K, int n, int m, float max_shift,
                                                         float *__restrict__ trans, float *__restrict__ dx,
                                                         float *__restrict__ dy) {
    const int j = blockIdx.x * LCS_BX + threadIdx.x;
    const int i = blockIdx.y * LCS_BY + threadIdx.y;
    if (i >= n || j >= m) return;
    // np.gradient, edge_order=1: central differences inside, one-sided first differences on the border (n, m >= 3)
    const int ip = i + 1 < n ? i + 1 : n - 1, im = i > 0 ? i - 1 : 0;
    const int jp = j + 1 < m ? j + 1 : m - 1, jm = j > 0 ? j - 1 : 0;
    const float h0 = ip - im == 2 ? 0.5f : 1.0f, h1 = jp - jm == 2 ? 0.5f : 1.0f;
    const int64_t c = (int64_t)i * m + j;
    const int64_t up = (int64_t)ip * m + j, dn = (int64_t)im * m + j;
    const int64_t rt = (int64_t)i * m + jp, lt = (int64_t)i * m + jm;
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0;
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
        const float *R = p.R[k];
        const float s = p.S[k][c], r = R[c], ru = R[up], rd = R[dn], rr = R[rt], rl = R[lt];
        const double a0 = s, a1 = (ru - rd) * h0, a2 = (rr - rl) * h1, b = r;   // float32 differences, as numpy forms them
        m00 = fma(a0, a0, m00);
        m01 = fma(a0, a1, m01);
        m02 = fma(a0, a2, m02);
        m11 = fma(a1, a1, m11);
        m12 = fma(a1, a2, m12);
        m22 = fma(a2, a2, m22);
        v0 = fma(a0, b, v0);
        v1 = fma(a1, b, v1);
        v2 = fma(a2, b, v2);
    }
    // cofactors of the symmetric M; det by the first row
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double det = m00 * c00 + m01 * c01 + m02 * c02;
    float t = 1.0f, x = 0.0f, y = 0.0f;
    if (!(det <= 1e-12 * m00 * m11 * m22)) {
        const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const double inv = 1.0 / det;
        const double x0 = (c00 * v0 + c01 * v1 + c02 * v2) * inv;
        // x0 = +inf: an interior pixel whose own R_k is +inf has finite M and an infinite v, so only this test sees it
        if (x0 > 0.0 && x0 < INFINITY) {
            t = (float)(1.0 / x0);
            x = (float)((c01 * v0 + c11 * v1 + c12 * v2) * inv);
            y = (float)((c02 * v0 + c12 * v1 + c22 * v2) * inv);
        }
    }
    if (max_shift > 0.0f) {
        x = fminf(fmaxf(x, -max_shift), max_shift);
        y = fminf(fmaxf(y, -max_shift), max_shift);
    }
    trans[c] = t;
    dx[c] = x;
    dy[c] = y;
}

// LCS-DF: k_lcs with a fourth column, the 5-point Laplacian of R_k with edge-replicated neighbours (the same clamped indices
// as the gradients, so the same six loads), formed in float64 from the float32 samples: exact for image data.  The 4x4
// system is solved by LDL^T without pivoting; fallback x = (1, 0, 0, 0) when a pivot is <= 0, when prod d_i (= det M) <=
// 1e-12*M00*M11*M22*M33, or when x0 <= 0.  df = -x3 is not clamped.
__global__ __launch_bounds__(LCS_BX * LCS_BY) void k_lcs_df(SpecklePtrs p, int K, int n, int m, float max_shift,
                                                            float *__restrict__ trans, float *__restrict__ dx,
                                                            float *__restrict__ dy, float *__restrict__ df) {
    const int j = blockIdx.x * LCS_BX + threadIdx.x;
    const int i = blockIdx.y * LCS_BY + threadIdx.y;
    if (i >= n || j >= m) return;
    const int ip = i + 1 < n ? i + 1 : n - 1, im = i > 0 ? i - 1 : 0;
    const int jp = j + 1 < m ? j + 1 : m - 1, jm = j > 0 ? j - 1 : 0;
    const float h0 = ip - im == 2 ? 0.5f : 1.0f, h1 = jp - jm == 2 ? 0.5f : 1.0f;
    const int64_t c = (int64_t)i * m + j;
    const int64_t up = (int64_t)ip * m + j, dn = (int64_t)im * m + j;
    const int64_t rt = (int64_t)i * m + jp, lt = (int64_t)i * m + jm;
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m03 = 0.0, m11 = 0.0, m12 = 0.0, m13 = 0.0, m22 = 0.0, m23 = 0.0, m33 = 0.0;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
        const float *R = p.R[k];
        const float s = p.S[k][c], r = R[c], ru = R[up], rd = R[dn], rr = R[rt], rl = R[lt];
        const double b = r;
        const double a0 = s, a1 = (ru - rd) * h0, a2 = (rr - rl) * h1;
        const double a3 = (((double)ru + (double)rd) + ((double)rr + (double)rl)) - 4.0 * b;   // exact in float64
        m00 = fma(a0, a0, m00);
        m01 = fma(a0, a1, m01);
        m02 = fma(a0, a2, m02);
        m03 = fma(a0, a3, m03);
        m11 = fma(a1, a1, m11);
        m12 = fma(a1, a2, m12);
        m13 = fma(a1, a3, m13);
        m22 = fma(a2, a2, m22);
        m23 = fma(a2, a3, m23);
        m33 = fma(a3, a3, m33);
        v0 = fma(a0, b, v0);
        v1 = fma(a1, b, v1);
        v2 = fma(a2, b, v2);
        v3 = fma(a3, b, v3);
    }
    float t = 1.0f, x = 0.0f, y = 0.0f, w = 0.0f;
    // M = L D L^T, column by column; e_ij = L_ij*d_j
    const double d0 = m00;
    if (d0 > 0.0) {
        const double r0 = 1.0 / d0;
        const double l10 = m01 * r0, l20 = m02 * r0, l30 = m03 * r0;
        const double d1 = m11 - l10 * m01;
        if (d1 > 0.0) {
            const double r1 = 1.0 / d1;
            const double e21 = m12 - l20 * m01, e31 = m13 - l30 * m01;
            const double l21 = e21 * r1, l31 = e31 * r1;
            const double d2 = m22 - l20 * m02 - l21 * e21;
            if (d2 > 0.0) {
                const double r2 = 1.0 / d2;
                const double e32 = m23 - l30 * m02 - l31 * e21;
                const double l32 = e32 * r2;
                const double d3 = m33 - l30 * m03 - l31 * e31 - l32 * e32;
                if (d3 > 0.0 && !(d0 * d1 * d2 * d3 <= 1e-12 * m00 * m11 * m22 * m33)) {
                    const double y1 = v1 - l10 * v0;
                    const double y2 = v2 - l20 * v0 - l21 * y1;
                    const double y3 = v3 - l30 * v0 - l31 * y1 - l32 * y2;
                    const double x3 = y3 / d3;
                    const double x2 = y2 * r2 - l32 * x3;
                    const double x1 = y1 * r1 - l21 * x2 - l31 * x3;
                    const double x0 = v0 * r0 - l10 * x1 - l20 * x2 - l30 * x3;
                    if (x0 > 0.0) {
                        t = (float)(1.0 / x0);
                        x = (float)x1;
                        y = (float)x2;
                        w = (float)(-x3);
                    }
                }
            }
        }
    }
    if (max_shift > 0.0f) {
        x = fminf(fmaxf(x, -max_shift), max_shift);
        y = fminf(fmaxf(y, -max_shift), max_shift);
    }
    trans[c] = t;
    dx[c] = x;
    dy[c] = y;
    df[c] = w;
}

// Z[a][b] on the 2n x 2m extension: Gx = +-gx (minus on the mirrored rows), Gy = +-gy (minus on the mirrored columns)
__global__ __launch_bounds__(256) void k_integ_pack(const float *__restrict__ gx, const float *__restrict__ gy, double scale,
                                                    float2 *__restrict__ Z, int n, int m) {
    const int64_t W = 2 * (int64_t)m, N = 2 * (int64_t)n * W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(q / W), b = (int)(q - (int64_t)a * W);
        const bool ra = a >= n, rb = b >= m;
        const int64_t src = (int64_t)(ra ? 2 * n - 1 - a : a) * m + (rb ? 2 * m - 1 - b : b);
        const double x = scale * (double)gx[src], y = scale * (double)gy[src];
        Z[q] = make_float2((float)(ra ? -x : x), (float)(rb ? -y : y));
    }
}

// P(k) from Z(k) and Z(-k) at the angular frequency (kx, ky)
__device__ __forceinline__ float2 fc_filter(float2 zk, float2 zm, double kx, double ky) {
    // Gx^ = (zk + conj zm)/2;  Gy^ = (zk - conj zm)/(2i) = (-i)(zk - conj zm)/2
    const float gxr = 0.5f * (zk.x + zm.x), gxi = 0.5f * (zk.y - zm.y);
    const float dr = zk.x - zm.x, di = zk.y + zm.y;
    const float gyr = 0.5f * di, gyi = -0.5f * dr;
    const double den = kx * kx + ky * ky;
    const float fx = (float)(kx / den), fy = (float)(ky / den);
    // -i*(fx*Gx^ + fy*Gy^)
    const float sr = fx * gxr + fy * gyr, si = fx * gxi + fy * gyi;
    return make_float2(si, -sr);
}

__global__ __launch_bounds__(256) void k_integ_filter(float2 *__restrict__ Z, int n, int m) {
    const int H = 2 * n, W = 2 * m;
    const int64_t N = (int64_t)H * W;
    const double wx = PSX_TWO_PI / (double)H, wy = PSX_TWO_PI / (double)W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(q / W), b = (int)(q - (int64_t)a * W);
        const int a2 = a ? H - a : 0, b2 = b ? W - b : 0;
        const int64_t q2 = (int64_t)a2 * W + b2;
        if (q2 < q) continue;   // the pair belongs to the thread of its smaller index
        // np.fft.fftfreq: index f < H/2 -> f, else f - H (the Nyquist row is -H/2)
        const double kx = wx * (a < n ? a : a - H), ky = wy * (b < m ? b : b - W);
        const double kx2 = wx * (a2 < n ? a2 : a2 - H), ky2 = wy * (b2 < m ? b2 : b2 - W);
        const float2 z1 = Z[q], z2 = Z[q2];
        const float2 p1 = q == 0 ? make_float2(0.f, 0.f) : fc_filter(z1, z2, kx, ky);
        if (q2 != q) Z[q2] = fc_filter(z2, z1, kx2, ky2);
        Z[q] = p1;
    }
}

__global__ __launch_bounds__(256) void k_integ_crop(const float2 *__restrict__ Z, float *__restrict__ phi, int n, int m,
                                                    float norm) {
    const int64_t N = (int64_t)n * m;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(p / m), j = (int)(p - (int64_t)i * m);
        phi[p] = Z[(int64_t)i * 2 * m + j].x * norm;
    }
}

// The two images of one Paganin transform (psx_paganin_f32): B's pointers are null and its numbers unused for a last odd image
struct PagPair {
    const float *I[2], *W[2];
    float *contact[2], *thickness[2];
    double alpha[2], mu[2];
};

// x = float32(I/I0 - 1) of pixel p of image s of the pair; 0 for an absent image and at a guarded pixel
__device__ __forceinline__ float pag_contrast(const PagPair &pp, int s, int64_t p) {
    if (!pp.I[s]) return 0.0f;
    const float v = pp.I[s][p];
    if (!isfinite(v)) return 0.0f;
    if (!pp.W[s]) return (float)((double)v - 1.0);
    const float w = pp.W[s][p];
    if (!(isfinite(w) && w > 0.0f)) return 0.0f;
    return (float)((double)v / (double)w - 1.0);
}

// one thread per source pixel (i, j): its value goes to the four mirror images (i | 2n-1-i, j | 2m-1-j) of the extension
__global__ __launch_bounds__(256) void k_pag_pack(PagPair pp, float2 *__restrict__ Z, int n, int m) {
    const int64_t N = (int64_t)n * m, W = 2 * (int64_t)m;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(p / m), j = (int)(p - (int64_t)i * m);
        const float2 z = make_float2(pag_contrast(pp, 0, p), pag_contrast(pp, 1, p));
        const int64_t r0 = (int64_t)i * W, r1 = (int64_t)(2 * n - 1 - i) * W;
        const int j1 = 2 * m - 1 - j;
        Z[r0 + j] = z;
        Z[r0 + j1] = z;
        Z[r1 + j] = z;
        Z[r1 + j1] = z;
    }
}

// Y(k) from Z(k) and Z(-k): the two real images' spectra, each times its own factor, recombined
__device__ __forceinline__ float2 pag_filter(float2 zk, float2 zm, float fa, float fb) {
    // A^ = (zk + conj zm)/2;  B^ = (-i)(zk - conj zm)/2
    const float ar = 0.5f * (zk.x + zm.x), ai = 0.5f * (zk.y - zm.y);
    const float br = 0.5f * (zk.y + zm.y), bi = -0.5f * (zk.x - zm.x);
    // fa*A^ + i*fb*B^
    return make_float2(fa * ar - fb * bi, fa * ai + fb * br);
}

// k_integ_filter's pairing: the thread of the smaller index owns (k, -k); k^2 is the same for both
__global__ __launch_bounds__(256) void k_pag_filter(float2 *__restrict__ Z, int n, int m, double alpha_a, double alpha_b) {
    const int H = 2 * n, W = 2 * m;
    const int64_t N = (int64_t)H * W;
    const double wx = PSX_TWO_PI / (double)H, wy = PSX_TWO_PI / (double)W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(q / W), b = (int)(q - (int64_t)a * W);
        const int a2 = a ? H - a : 0, b2 = b ? W - b : 0;
        const int64_t q2 = (int64_t)a2 * W + b2;
        if (q2 < q) continue;
        const double kx = wx * (a < n ? a : a - H), ky = wy * (b < m ? b : b - W);
        const double k2 = kx * kx + ky * ky;
        const float fa = (float)(1.0 / (1.0 + alpha_a * k2)), fb = (float)(1.0 / (1.0 + alpha_b * k2));
        const float2 z1 = Z[q], z2 = Z[q2];
        if (q2 != q) Z[q2] = pag_filter(z2, z1, fa, fb);
        Z[q] = pag_filter(z1, z2, fa, fb);
    }
}

__global__ __launch_bounds__(256) void k_pag_crop(PagPair pp, const float2 *__restrict__ Z, int n, int m, double norm) {
    const int64_t N = (int64_t)n * m;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
        const int i = (int)(p / m), j = (int)(p - (int64_t)i * m);
        const float2 z = Z[(int64_t)i * 2 * m + j];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double y = (double)(s ? z.y : z.x) * norm;
            const double c = 1.0 + y;
            if (pp.contact[s]) pp.contact[s][p] = (float)c;
            if (pp.thickness[s]) pp.thickness[s][p] = (float)((c > 0.0 ? -log1p(y) : 87.33654475055310898657) / pp.mu[s]);
        }
    }
}

}  // namespace

struct psx_integrate_plan {
    int n = 0, m = 0;
    size_t bytes = 0;
    FftPlan fft;         // forward + inverse, [2n][2m]
    DevBuf<float2> Z;    // [2n][2m]
};

namespace {

// The argument checks, pointer packing (pack_speckle) and grid shared by psx_lcs_f32 and psx_lcs_df_f32.  fn: the entry point's
// name in the error texts; Kmin: its smallest K; outputs_ok: all its output maps are there.
int lcs_prepare(const char *fn, int Kmin, const float *const *S, const float *const *R, int K, int n, int m, float max_shift,
                bool outputs_ok, SpecklePtrs &p, dim3 &grid) {
    if (int rc = pack_speckle(p, fn, Kmin, S, R, K)) return rc;
    PSX_REQUIRE(n >= 3 && m >= 3, "%s: images %dx%d smaller than 3x3", fn, n, m);
    PSX_REQUIRE(outputs_ok, "%s: null output map", fn);
    PSX_REQUIRE(max_shift >= 0.0f, "%s: max_shift=%g < 0", fn, (double)max_shift);
    grid = dim3((unsigned)cdiv(m, LCS_BX), (unsigned)cdiv(n, LCS_BY));
    return 0;
}

}  // namespace

extern "C" {

int psx_lcs_f32(const float *const *S, const float *const *R, int K, int n, int m, float max_shift, float *transmission,
                float *dx, float *dy, void *stream) {
    SpecklePtrs p;
    dim3 grid;
    if (int rc = lcs_prepare("psx_lcs_f32", 3, S, R, K, n, m, max_shift, transmission && dx && dy, p, grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    PSX_TIMED("k_lcs", st, k_lcs<<<grid, dim3(LCS_BX, LCS_BY), 0, st>>>(p, K, n, m, max_shift, transmission, dx, dy));
    return launch_check("k_lcs");
}

int psx_lcs_df_f32(const float *const *S, const float *const *R, int K, int n, int m, float max_shift, float *transmission,
                   float *dx, float *dy, float *df, void *stream) {
    SpecklePtrs p;
    dim3 grid;
    if (int rc = lcs_prepare("psx_lcs_df_f32", 4, S, R, K, n, m, max_shift, transmission && dx && dy && df, p, grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    PSX_TIMED("k_lcs_df", st, k_lcs_df<<<grid, dim3(LCS_BX, LCS_BY), 0, st>>>(p, K, n, m, max_shift, transmission, dx, dy, df));
    return launch_check("k_lcs_df");
}

int psx_integrate_plan_create(int n, int m, psx_integrate_plan **plan) {
    PSX_REQUIRE(plan != nullptr, "psx_integrate_plan_create: null plan pointer");
    *plan = nullptr;
    PSX_REQUIRE(n >= 2 && m >= 2, "psx_integrate_plan_create: grid %dx%d too small", n, m);
    PSX_REQUIRE((int64_t)n * m <= (int64_t)1 << 28, "psx_integrate_plan_create: grid %dx%d too large", n, m);
    std::unique_ptr<psx_integrate_plan> p(new psx_integrate_plan());
    p->n = n; p->m = m;
    const size_t lengths[2] = {2 * (size_t)m, 2 * (size_t)n};   // fastest first
    if (int rc = p->fft.create(FftPlan::BOTH, rocfft_precision_single, 2, lengths)) return rc;
    if (int rc = p->Z.alloc(4 * (size_t)n * (size_t)m)) return rc;
    p->bytes = p->Z.bytes() + p->fft.work_bytes();
    *plan = p.release();
    return 0;
}

int psx_integrate_plan_destroy(psx_integrate_plan *plan) {
    delete plan;
    return 0;
}

size_t psx_integrate_plan_bytes(const psx_integrate_plan *plan) { return plan ? plan->bytes : 0; }

int psx_integrate_f32(psx_integrate_plan *plan, const float *gx, const float *gy, double scale, float *phi, void *stream) {
    PSX_REQUIRE(plan != nullptr, "psx_integrate_f32: null plan");
    PSX_REQUIRE(gx && gy && phi, "psx_integrate_f32: null image");
    hipStream_t st = (hipStream_t)stream;
    const int n = plan->n, m = plan->m;
    const int64_t N = 4 * (int64_t)n * m;
    float2 *const Z = plan->Z.get();
    PSX_TIMED("k_integ_pack", st, k_integ_pack<<<ew_grid(N, 256), 256, 0, st>>>(gx, gy, scale, Z, n, m));
    if (int rc = launch_check("k_integ_pack")) return rc;
    if (int rc = plan->fft.execute(FftPlan::FWD, Z, st, "rocfft_integrate_forward")) return rc;
    PSX_TIMED("k_integ_filter", st, k_integ_filter<<<ew_grid(N, 256), 256, 0, st>>>(Z, n, m));
    if (int rc = launch_check("k_integ_filter")) return rc;
    if (int rc = plan->fft.execute(FftPlan::INV, Z, st, "rocfft_integrate_inverse")) return rc;
    const float norm = (float)(1.0 / (double)N);
    PSX_TIMED("k_integ_crop", st, k_integ_crop<<<ew_grid((int64_t)n * m, 256), 256, 0, st>>>(Z, phi, n, m, norm));
    return launch_check("k_integ_crop");
}

int psx_paganin_f32(psx_integrate_plan *plan, int B, const float *const *image, const float *const *white,
                    const double *alpha, const double *mu, float *const *contact, float *const *thickness, void *stream) {
    PSX_REQUIRE(plan != nullptr, "psx_paganin_f32: null plan");
    PSX_REQUIRE(B >= 1 && B <= PSX_MAX_PAGANIN, "psx_paganin_f32: B=%d images outside [1,%d]", B, PSX_MAX_PAGANIN);
    PSX_REQUIRE(image && alpha && mu, "psx_paganin_f32: null image, alpha or mu array");
    PSX_REQUIRE(contact || thickness, "psx_paganin_f32: neither contact nor thickness asked for");
    for (int b = 0; b < B; ++b) {
        PSX_REQUIRE(image[b] != nullptr, "psx_paganin_f32: image %d is null", b);
        PSX_REQUIRE(std::isfinite(alpha[b]) && alpha[b] >= 0.0, "psx_paganin_f32: alpha[%d]=%g is not a finite value >= 0", b, alpha[b]);
        PSX_REQUIRE(std::isfinite(mu[b]) && mu[b] > 0.0, "psx_paganin_f32: mu[%d]=%g is not a finite value > 0", b, mu[b]);
        PSX_REQUIRE((contact && contact[b]) || (thickness && thickness[b]), "psx_paganin_f32: image %d has neither output", b);
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = plan->n, m = plan->m;
    const int64_t N = 4 * (int64_t)n * m;
    float2 *const Z = plan->Z.get();
    const double norm = 1.0 / (double)N;
    for (int b0 = 0; b0 < B; b0 += 2) {
        PagPair pp = {};
        for (int s = 0; s < 2; ++s) {
            const int b = b0 + s;
            const bool on = b < B;
            pp.I[s] = on ? image[b] : nullptr;
            pp.W[s] = on && white ? white[b] : nullptr;
            pp.contact[s] = on && contact ? contact[b] : nullptr;
            pp.thickness[s] = on && thickness ? thickness[b] : nullptr;
            pp.alpha[s] = on ? alpha[b] : 0.0;
            pp.mu[s] = on ? mu[b] : 1.0;
        }
        PSX_TIMED("k_pag_pack", st, k_pag_pack<<<ew_grid((int64_t)n * m, 256), 256, 0, st>>>(pp, Z, n, m));
        if (int rc = launch_check("k_pag_pack")) return rc;
        if (int rc = plan->fft.execute(FftPlan::FWD, Z, st, "rocfft_paganin_forward")) return rc;
        PSX_TIMED("k_pag_filter", st, k_pag_filter<<<ew_grid(N, 256), 256, 0, st>>>(Z, n, m, pp.alpha[0], pp.alpha[1]));
        if (int rc = launch_check("k_pag_filter")) return rc;
        if (int rc = plan->fft.execute(FftPlan::INV, Z, st, "rocfft_paganin_inverse")) return rc;
        PSX_TIMED("k_pag_crop", st, k_pag_crop<<<ew_grid((int64_t)n * m, 256), 256, 0, st>>>(pp, Z, n, m, norm));
        if (int rc = launch_check("k_pag_crop")) return rc;
    }
    return 0;
}

}  // extern "C"
