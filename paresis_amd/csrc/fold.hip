// fold.hip -- a stack of more than PSX_MAX_MAT thickness maps folded into three (psx_fold_materials_f32).
// Elementwise, HBM-bound: every input map is read once, three maps are written, in one launch.
#include "common.hpp"

using namespace psx;

namespace {

constexpr int FOLD_GROUP = 8;   // maps loaded together: unconditional, independent loads, one wait per group

struct FoldMats {
    const float *T[PSX_MAX_FOLD];   // padded to a multiple of FOLD_GROUP with T[0] and zero coefficients
    double cphase[PSX_MAX_FOLD];
    double catt[PSX_MAX_FOLD];
    int ngroups;
};

// P and A by the consumers' own recurrence (mats_eval, common.hpp): ph = fma(cphase[m], T[m], ph) from 0, m in order.
// A padded slot adds fma(0, t, ph) = ph.
__global__ __launch_bounds__(256) void k_fold_materials(FoldMats f, float *__restrict__ P_hi, float *__restrict__ P_lo,
                                                        float *__restrict__ A_out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        double ph = 0.0, la = 0.0;
        for (int g = 0; g < f.ngroups; ++g) {
            float t[FOLD_GROUP];
#pragma unroll
            for (int i = 0; i < FOLD_GROUP; ++i) t[i] = f.T[g * FOLD_GROUP + i][p];
#pragma unroll
            for (int i = 0; i < FOLD_GROUP; ++i) {
                ph = fma(f.cphase[g * FOLD_GROUP + i], (double)t[i], ph);
                la = fma(f.catt[g * FOLD_GROUP + i], (double)t[i], la);
            }
        }
        const float hi = (float)ph;
        P_hi[p] = hi;
        P_lo[p] = (float)(ph - (double)hi);
        A_out[p] = (float)la;
    }
}

}  // namespace

extern "C" int psx_fold_materials_f32(const float *const *T, const double *cphase, const double *catt, int nmat, float *P_hi,
                                      float *P_lo, float *A_out, int64_t n, void *stream) {
    PSX_REQUIRE(nmat >= 1 && nmat <= PSX_MAX_FOLD, "nmat=%d outside [1,%d]", nmat, PSX_MAX_FOLD);
    PSX_REQUIRE(T != nullptr && cphase != nullptr && catt != nullptr, "T, cphase and catt must not be null");
    PSX_REQUIRE(P_hi && P_lo && A_out, "null output map");
    PSX_REQUIRE(n >= 0, "n=%lld < 0", (long long)n);
    FoldMats f;
    const int ng = (nmat + FOLD_GROUP - 1) / FOLD_GROUP;
    for (int i = 0; i < PSX_MAX_FOLD; ++i) {
        f.T[i] = nullptr;
        f.cphase[i] = 0.0;
        f.catt[i] = 0.0;
    }
    for (int i = 0; i < nmat; ++i) {
        PSX_REQUIRE(T[i] != nullptr, "T[%d] is null", i);
        f.T[i] = T[i];
        f.cphase[i] = cphase[i];
        f.catt[i] = catt[i];
    }
    for (int i = nmat; i < ng * FOLD_GROUP; ++i) f.T[i] = T[0];
    f.ngroups = ng;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    PSX_TIMED("k_fold_materials", st, k_fold_materials<<<ew_grid(n, 256), 256, 0, st>>>(f, P_hi, P_lo, A_out, n));
    return launch_check("k_fold_materials");
}
