// fresnel_plan.hpp -- the plan object behind psx_fresnel_*: grid geometry + engine-specific state.
#pragma once
#include <rocfft/rocfft.h>

#include "common.hpp"

#define PSX_ROCFFT(expr)                                                                          \
    do {                                                                                          \
        rocfft_status s__ = (expr);                                                               \
        if (s__ != rocfft_status_success)                                                         \
            return psx::fail(1000 + (int)s__, "%s:%d: %s -> rocfft_status %d", __FILE__, __LINE__, #expr, (int)s__); \
    } while (0)

namespace psx {

int rocfft_ensure_setup();   // rocfft_setup() once per process (fresnel.hip)

// Owner of rocFFT plans of one geometry with their execution info and work buffer: a single transform (FWD or INV), or BOTH
// directions of the same lengths sharing one execution info and one work buffer of the larger size.  Like DevBuf: no
// copy, never at namespace scope, allocates in create() only.
class FftPlan {
    rocfft_plan plan_[2] = {nullptr, nullptr};   // [FWD], [INV]
    rocfft_execution_info info_ = nullptr;
    DevBuf<char> work_;

  public:
    enum Dir { FWD = 0, INV = 1, BOTH = 2 };
    FftPlan() = default;
    FftPlan(const FftPlan &) = delete;
    FftPlan &operator=(const FftPlan &) = delete;
    ~FftPlan() {
        for (rocfft_plan pl : plan_)
            if (pl) rocfft_plan_destroy(pl);
        if (info_) rocfft_execution_info_destroy(info_);
    }

    // in-place complex transforms; lengths are fastest-first
    int create(Dir dir, rocfft_precision prec, size_t dims, const size_t *lengths, size_t batch = 1) {
        if (int rc = rocfft_ensure_setup()) return rc;
        size_t work = 0;
        for (int d = FWD; d <= INV; ++d) {
            if (dir != BOTH && dir != d) continue;
            PSX_ROCFFT(rocfft_plan_create(&plan_[d], rocfft_placement_inplace,
                                          d == FWD ? rocfft_transform_type_complex_forward : rocfft_transform_type_complex_inverse,
                                          prec, dims, lengths, batch, nullptr));
            size_t w = 0;
            PSX_ROCFFT(rocfft_plan_get_work_buffer_size(plan_[d], &w));
            work = w > work ? w : work;
        }
        PSX_ROCFFT(rocfft_execution_info_create(&info_));
        if (work) {
            if (int rc = work_.alloc(work)) return rc;
            PSX_ROCFFT(rocfft_execution_info_set_work_buffer(info_, work_.get(), work));
        }
        return 0;
    }
    size_t work_bytes() const { return work_.bytes(); }

    // one transform of buf in place on st, timed under `name` (psx_profile_*)
    int execute(Dir dir, void *buf, hipStream_t st, const char *name) {
        PSX_ROCFFT(rocfft_execution_info_set_stream(info_, st));
        ProfScope ps(name, st);
        PSX_ROCFFT(rocfft_execute(plan_[dir], &buf, nullptr, info_));
        return 0;
    }
};

struct LdsEngine;   // fresnel_lds.hip

struct RocfftEngine {
    FftPlan fft;              // forward + inverse, [Px][Py]
    DevBuf<float2> spec;      // [Px][Py] padded wave, transformed in place
    DevBuf<float2> prod;      // [Px][Py] spectrum x chirp, inverse-transformed in place (one distance at a time)
    DevBuf<float2> cx;        // [Px] chirp along axis 0 (FFT order), carries the global phase and 1/(Px*Py)
    DevBuf<float2> cy;        // [Py]
};

}  // namespace psx

struct psx_fresnel_plan {
    int Nx = 0, Ny = 0, margin = 0, Px = 0, Py = 0, max_dist = 0, engine = 0;
    size_t bytes = 0;
    std::unique_ptr<psx::RocfftEngine> rf;
    std::unique_ptr<psx::LdsEngine> lds;
    psx_fresnel_plan();    // both in fresnel_lds.hip, where LdsEngine is complete
    ~psx_fresnel_plan();
};

namespace psx {

// engine entry points (same contract as psx_fresnel_propagate, arguments already validated and packed)
struct PropArgs {
    const float2 *wave_in;
    float amp;
    Mats m;
    int n_dist;
    const double *a, *gphase;
    double du_x, du_y;
    float2 *const *wave_out;
    float *const *inten_out;
    const float *inten_scale;
    int accumulate;
    hipStream_t stream;
};

// a batch of source waves over the same thickness maps (psx_fresnel_propagate_sources); arrays indexed [source] or
// [source * n_dist + distance], coefficients [source * maps.n + material]
struct SourcesArgs {
    int n_src, n_dist;
    const float2 *const *wave_in;   // may be NULL (unit waves), entries may be NULL
    const float *amp;
    Mats maps;                      // T and n; its coefficients are not used
    const double *cphase, *catt;
    const double *a, *gphase;
    double du_x, du_y;
    float2 *const *wave_out;
    float *const *inten_out;
    const float *inten_scale;
    hipStream_t stream;
};

// source s of a batch as a call of its own
inline PropArgs slice_source(const SourcesArgs &a, int s) {
    PropArgs pa;
    pa.wave_in = a.wave_in ? a.wave_in[s] : nullptr;
    pa.amp = a.amp[s];
    pa.m = a.maps;
    for (int i = 0; i < a.maps.n; ++i) {
        pa.m.cphase[i] = a.cphase ? a.cphase[(size_t)s * a.maps.n + i] : 0.0;
        pa.m.catt[i] = a.catt ? a.catt[(size_t)s * a.maps.n + i] : 0.0;
    }
    pa.n_dist = a.n_dist; pa.a = a.a + (size_t)s * a.n_dist; pa.gphase = a.gphase ? a.gphase + (size_t)s * a.n_dist : nullptr;
    pa.du_x = a.du_x; pa.du_y = a.du_y;
    pa.wave_out = a.wave_out ? a.wave_out + (size_t)s * a.n_dist : nullptr;
    pa.inten_out = a.inten_out ? a.inten_out + (size_t)s * a.n_dist : nullptr;
    pa.inten_scale = a.inten_scale ? a.inten_scale + (size_t)s * a.n_dist : nullptr;
    pa.accumulate = 0; pa.stream = a.stream;
    return pa;
}

int rocfft_engine_create(psx_fresnel_plan *p);
int rocfft_engine_propagate(psx_fresnel_plan *p, const PropArgs &a);

bool lds_engine_supported(int Nx, int Ny, int margin);
int lds_engine_create(psx_fresnel_plan *p);
int lds_engine_propagate(psx_fresnel_plan *p, const PropArgs &a);
void lds_engine_work_queue(psx_fresnel_plan *p, int on);
int lds_engine_propagate_sources(psx_fresnel_plan *p, const SourcesArgs &a);

// psi(p) = amp * wave_in * transmission at UN-padded pixel p
template <int NM>
__device__ __forceinline__ float2 source_wave(const float2 *__restrict__ wave_in, float amp, const Mats &m, int64_t p) {
    float2 w = wave_in ? wave_in[p] : make_float2(1.f, 0.f);
    float a = amp;
    if (NM > 0) {
        double ph, la;
        mats_eval<NM>(m, p, ph, la);
        float c, s;
        cis_f64(ph, c, s);
        a *= exp_att(la);
        w = make_float2(w.x * c - w.y * s, w.x * s + w.y * c);
    }
    return make_float2(a * w.x, a * w.y);
}

// np.pad(..., mode='reflect') index: mirror without repeating the edge sample (EXP:237, DET:93)
__host__ __device__ __forceinline__ int reflect_index(int q, int n) {
    if (q < 0) q = -q;
    if (q >= n) q = 2 * (n - 1) - q;
    return q;
}

}  // namespace psx
