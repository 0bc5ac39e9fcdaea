// decompose.hip -- projection-domain material decomposition of energy-binned scans (psx_decompose_f32).
//
// Per pixel, from the B per-bin log-transmissions L_b = -ln(transmission of bin b), the thicknesses x_m of M materials under
// the polychromatic model  T_b(x) = sum_e w_be exp(-sum_m a_mbe x_m)  (w: the flat field's per-energy share of bin b, summing
// to 1; a: the materials' linear attenuation coefficients, 1/m), beam hardening included: weighted Gauss-Newton on
// r_b = L_b + ln T_b(x) from the linearised start x = G L, everything in float64 (the contract is in include/paresis_hip.h).
//
// k_decompose<M>: one thread per pixel, templated on M so that the normal matrix, its factor and the step live in registers.
// The spectral tables (at most 256*5 + 44 doubles) are staged once per workgroup in LDS, one (w, a_0 .. a_M-1) record per
// energy, and read at wave-uniform addresses (broadcasts).  The cost is the float64 exp: one per energy, iteration and pixel,
// plus one log per bin.  The B x M Jacobian is never kept: a bin's row g_b goes into N and rhs as soon as it is known.  A
// pixel stops on its own step alone (no wave vote), so its result does not depend on its neighbours; a lane that is done
// idles until the last lane of its wave is.
#include "common.hpp"

#include <vector>

using namespace psx;

namespace {

constexpr int DEC_BLOCK = 256;
constexpr int DEC_TAB_MAX = PSX_DECOMP_MAX_ENERGIES * (PSX_DECOMP_MAX_MAT + 1) + PSX_DECOMP_MAX_BINS +
                            PSX_DECOMP_MAX_MAT * PSX_DECOMP_MAX_BINS + PSX_DECOMP_MAX_MAT;

struct DecompArgs {
    const float *L[PSX_DECOMP_MAX_BINS];
    float *X[PSX_DECOMP_MAX_MAT];
    float *residual, *steps;
    const double *tab;     // [E][M+1] records (w, a_0 ..), then v[B], G[M][B], abar[M]
    int bin_size[PSX_DECOMP_MAX_BINS];
    int B, E, iterations;
    double tol;
    int64_t n;
};

// r_b = L_b + ln T_b(x) of one bin whose records start at `rec`; u = sum_e a_e s_e (not yet divided by T)
template <int M>
__device__ __forceinline__ double bin_eval(const double *rec, int ne, const double (&x)[M], double Lb, double (&u)[M], double &T) {
    T = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) u[m] = 0.0;
    for (int e = 0; e < ne; ++e, rec += M + 1) {
        double t = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) t = fma(rec[1 + m], x[m], t);
        const double s = rec[0] * exp(-t);
        T += s;
#pragma unroll
        for (int m = 0; m < M; ++m) u[m] = fma(rec[1 + m], s, u[m]);
    }
    return Lb + log(T);
}

// N d = rhs by LDL^T without pivoting (N: lower triangle, overwritten by the factor); false when a pivot is <= 0 or not finite
template <int M>
__device__ __forceinline__ bool ldl_solve(double (&N)[M][M], const double (&rhs)[M], double (&d)[M]) {
    double D[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double dj = N[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= N[j][k] * N[j][k] * D[k];
        if (!(dj > 0.0) || !isfinite(dj)) return false;
        D[j] = dj;
        const double rj = 1.0 / dj;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double lij = N[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) lij -= N[i][k] * N[j][k] * D[k];
            N[i][j] = lij * rj;
        }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double y = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) y -= N[i][k] * d[k];
        d[i] = y;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) d[i] /= D[i];
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
#pragma unroll
        for (int k = i + 1; k < M; ++k) d[i] -= N[k][i] * d[k];
    }
    return true;
}

template <int M>
__global__ __launch_bounds__(DEC_BLOCK) void k_decompose(DecompArgs p) {
    __shared__ double sh[DEC_TAB_MAX];
    const int B = p.B;
    const int ntab = p.E * (M + 1) + B + M * B + M;
    for (int q = threadIdx.x; q < ntab; q += DEC_BLOCK) sh[q] = p.tab[q];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * DEC_BLOCK + threadIdx.x;
    if (i >= p.n) return;                      // after the only barrier
    const double *v = sh + p.E * (M + 1), *G = v + B, *abar = G + M * B;

    double x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = 0.0;
    bool finite = true;
    for (int b = 0; b < B; ++b) {
        const double Lb = (double)p.L[b][i];
        finite = finite && isfinite(Lb);
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = fma(G[m * B + b], Lb, x[m]);
    }
    if (!finite) {
#pragma unroll
        for (int m = 0; m < M; ++m) p.X[m][i] = 0.0f;
        if (p.residual) p.residual[i] = INFINITY;
        if (p.steps) p.steps[i] = -1.0f;
        return;
    }

    int steps = 0;
    for (int k = 1; k <= p.iterations; ++k) {
        double N[M][M], rhs[M];
#pragma unroll
        for (int a = 0; a < M; ++a) {
            rhs[a] = 0.0;
#pragma unroll
            for (int c = 0; c <= a; ++c) N[a][c] = 0.0;
        }
        const double *rec = sh;
        for (int b = 0; b < B; ++b) {
            double u[M], T;
            const double r = bin_eval<M>(rec, p.bin_size[b], x, (double)p.L[b][i], u, T);
            rec += p.bin_size[b] * (M + 1);
            const double rT = 1.0 / T, vb = v[b];
#pragma unroll
            for (int a = 0; a < M; ++a) u[a] *= rT;                     // g_b
#pragma unroll
            for (int a = 0; a < M; ++a) {
                const double vg = vb * u[a];
                rhs[a] = fma(vg, r, rhs[a]);
#pragma unroll
                for (int c = 0; c <= a; ++c) N[a][c] = fma(vg, u[c], N[a][c]);
            }
        }
        double d[M];
        bool ok = ldl_solve<M>(N, rhs, d);
        double big = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            ok = ok && isfinite(d[m]);
            big = fmax(big, fabs(d[m]) * abar[m]);
        }
        if (!ok) {
            steps = -2;
            break;
        }
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] += d[m];
        steps = k;
        if (big <= p.tol) break;
    }

#pragma unroll
    for (int m = 0; m < M; ++m) p.X[m][i] = (float)x[m];
    if (p.steps) p.steps[i] = (float)steps;
    if (p.residual) {
        double sum = 0.0;
        const double *rec = sh;
        for (int b = 0; b < B; ++b) {
            double u[M], T;
            const double r = bin_eval<M>(rec, p.bin_size[b], x, (double)p.L[b][i], u, T);
            rec += p.bin_size[b] * (M + 1);
            sum = fma(v[b] * r, r, sum);
        }
        p.residual[i] = (float)sqrt(sum);
    }
}

}  // namespace

extern "C" int psx_decompose_f32(const float *const *logT, int B, const int *bin_size, const double *w, const double *a, int M,
                                 const double *v, const double *G, int iterations, double tol, int64_t n,
                                 float *const *thickness, float *residual, float *steps, void *stream) {
    const char *fn = "psx_decompose_f32";
    PSX_REQUIRE(B >= 1 && B <= PSX_DECOMP_MAX_BINS, "%s: B=%d bins outside [1,%d]", fn, B, PSX_DECOMP_MAX_BINS);
    PSX_REQUIRE(M >= 1 && M <= PSX_DECOMP_MAX_MAT, "%s: M=%d materials outside [1,%d]", fn, M, PSX_DECOMP_MAX_MAT);
    PSX_REQUIRE(M <= B, "%s: M=%d materials from B=%d bins: M must not exceed B", fn, M, B);
    PSX_REQUIRE(logT != nullptr, "%s: null logT pointer array", fn);
    PSX_REQUIRE(bin_size != nullptr, "%s: null bin_size", fn);
    PSX_REQUIRE(w != nullptr, "%s: null w", fn);
    PSX_REQUIRE(a != nullptr, "%s: null a", fn);
    PSX_REQUIRE(v != nullptr, "%s: null v", fn);
    PSX_REQUIRE(G != nullptr, "%s: null G", fn);
    PSX_REQUIRE(thickness != nullptr, "%s: null thickness pointer array", fn);
    int E = 0;
    for (int b = 0; b < B; ++b) {
        PSX_REQUIRE(logT[b] != nullptr, "%s: logT[%d] is null", fn, b);
        PSX_REQUIRE(bin_size[b] >= 1, "%s: bin_size[%d]=%d < 1", fn, b, bin_size[b]);
        PSX_REQUIRE(bin_size[b] <= PSX_DECOMP_MAX_ENERGIES - E, "%s: bin_size sums to more than %d energies", fn,
                    PSX_DECOMP_MAX_ENERGIES);
        E += bin_size[b];
        PSX_REQUIRE(std::isfinite(v[b]) && v[b] > 0.0, "%s: v[%d]=%g is not a finite value > 0", fn, b, v[b]);
    }
    for (int m = 0; m < M; ++m) PSX_REQUIRE(thickness[m] != nullptr, "%s: thickness[%d] is null", fn, m);
    PSX_REQUIRE(iterations >= 1, "%s: iterations=%d < 1", fn, iterations);
    PSX_REQUIRE(std::isfinite(tol) && tol >= 0.0, "%s: tol=%g is not a finite value >= 0", fn, tol);
    PSX_REQUIRE(n >= 1, "%s: n=%lld < 1", fn, (long long)n);
    PSX_REQUIRE(n <= (int64_t)0x7fffffff * DEC_BLOCK, "%s: n=%lld pixels exceed one launch", fn, (long long)n);

    // the kernel's table: one (w, a_0 .. a_M-1) record per energy, then v, G and abar_m = max_b sum_e w_be a_mbe
    std::vector<double> tab((size_t)E * (M + 1) + B + (size_t)M * B + M);
    double *tv = tab.data() + (size_t)E * (M + 1), *tG = tv + B, *tA = tG + (size_t)M * B;
    for (int e = 0; e < E; ++e) {
        tab[(size_t)e * (M + 1)] = w[e];
        for (int m = 0; m < M; ++m) tab[(size_t)e * (M + 1) + 1 + m] = a[(size_t)m * E + e];
    }
    for (int b = 0; b < B; ++b) tv[b] = v[b];
    for (int q = 0; q < M * B; ++q) tG[q] = G[q];
    for (int m = 0; m < M; ++m) {
        tA[m] = 0.0;
        for (int b = 0, e0 = 0; b < B; e0 += bin_size[b], ++b) {
            double s = 0.0;
            for (int e = e0; e < e0 + bin_size[b]; ++e) s += w[e] * a[(size_t)m * E + e];
            if (b == 0 || s > tA[m]) tA[m] = s;
        }
    }

    DecompArgs p = {};
    for (int b = 0; b < B; ++b) {
        p.L[b] = logT[b];
        p.bin_size[b] = bin_size[b];
    }
    for (int m = 0; m < M; ++m) p.X[m] = thickness[m];
    p.residual = residual;
    p.steps = steps;
    p.B = B; p.E = E; p.iterations = iterations; p.tol = tol; p.n = n;
    hipStream_t st = (hipStream_t)stream;
    // a stream-ordered temporary, declared after the host vector it is filled from: it waits for the stream and goes back to
    // its pool before the vector does
    DevBuf<double> d_tab;
    if (int rc = d_tab.upload_async(tab.data(), tab.size(), st)) return rc;
    p.tab = d_tab.get();
    const unsigned grid = (unsigned)cdiv(n, DEC_BLOCK);
    switch (M) {
        case 1: PSX_TIMED("k_decompose", st, k_decompose<1><<<grid, DEC_BLOCK, 0, st>>>(p)); break;
        case 2: PSX_TIMED("k_decompose", st, k_decompose<2><<<grid, DEC_BLOCK, 0, st>>>(p)); break;
        case 3: PSX_TIMED("k_decompose", st, k_decompose<3><<<grid, DEC_BLOCK, 0, st>>>(p)); break;
        default: PSX_TIMED("k_decompose", st, k_decompose<4><<<grid, DEC_BLOCK, 0, st>>>(p)); break;
    }
    return launch_check("k_decompose");
}
