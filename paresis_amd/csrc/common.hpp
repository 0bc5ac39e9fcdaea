// common.hpp -- shared host/device helpers of libparesis_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <memory>

#include "paresis_hip.h"

namespace psx {

// ---- thread-local error text behind psx_last_error() --------------------------------------------------------
char *err_buf();
int fail(int code, const char *fmt, ...);

#define PSX_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return psx::fail((int)e__, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
    } while (0)

#define PSX_REQUIRE(cond, ...)                         \
    do {                                               \
        if (!(cond)) return psx::fail(PSX_E_ARG, __VA_ARGS__); \
    } while (0)

inline int launch_check(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, "launch of %s failed: %s", what, hipGetErrorString(e));
    return 0;
}

// ---- the owner of a device allocation ------------------------------------------------------------------------------
// Move-only; every hipMalloc / hipFree of the library is in here.  It allocates only where alloc / upload is called, and
// never lives at namespace scope or in a static (its destructor must not run after the HIP runtime is gone): plans are
// heap objects destroyed through the ABI, per-call temporaries are locals.  Kernel argument blocks take get().
// Stream-ordered mode (the *_async calls, per-call temporaries): the memory comes from the stream's pool, and reset()
// waits for the stream before it hands it back, so the host arrays of an upload_async may go once the buffer is gone.
template <class T>
class DevBuf {
    T *p_ = nullptr;
    size_t n_ = 0;
    hipStream_t st_ = nullptr;
    bool async_ = false;

  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { *this = static_cast<DevBuf &&>(o); }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_; st_ = o.st_; async_ = o.async_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }

    int alloc(size_t n) {
        reset();
        PSX_HIP(hipMalloc((void **)&p_, sizeof(T) * n));
        n_ = n; async_ = false;
        return 0;
    }
    int upload(const T *host, size_t n) {
        if (int rc = alloc(n)) return rc;
        PSX_HIP(hipMemcpy(p_, host, sizeof(T) * n, hipMemcpyHostToDevice));
        return 0;
    }
    int upload_async(const T *host, size_t n, hipStream_t st) {
        reset();
        PSX_HIP(hipMallocAsync((void **)&p_, sizeof(T) * n, st));
        n_ = n; st_ = st; async_ = true;
        PSX_HIP(hipMemcpyAsync(p_, host, sizeof(T) * n, hipMemcpyHostToDevice, st));
        return 0;
    }
    void reset() {
        if (p_ && async_) {
            (void)hipStreamSynchronize(st_);
            (void)hipFreeAsync(p_, st_);
        } else if (p_) {
            (void)hipFree(p_);
        }
        p_ = nullptr; n_ = 0;
    }
    T *get() const { return p_; }
    size_t elems() const { return n_; }
    size_t bytes() const { return sizeof(T) * n_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// ---- a stack of thickness maps with per-map coefficients, passed to kernels by value ---------------------------
struct Mats {
    const float *T[PSX_MAX_MAT];
    double cphase[PSX_MAX_MAT];
    double catt[PSX_MAX_MAT];
    int n;
};

// Validates (T, cphase, catt, nmat) and packs them.  Null coefficient arrays mean zeros.
int pack_mats(Mats &m, const float *const *T, const double *cphase, const double *catt, int nmat);

// ---- the K sample / reference image pairs of a speckle tracker (retrieve.hip, umpa.hip), passed to kernels by value ----
struct SpecklePtrs {
    const float *S[PSX_MAX_LCS];
    const float *R[PSX_MAX_LCS];
};

// Validates (S, R, K) for the entry point `fn`, whose smallest K is Kmin, and packs them; the unused slots are null.
inline int pack_speckle(SpecklePtrs &p, const char *fn, int Kmin, const float *const *S, const float *const *R, int K) {
    PSX_REQUIRE(K >= Kmin && K <= PSX_MAX_LCS, "%s: K=%d positions outside [%d,%d]", fn, K, Kmin, PSX_MAX_LCS);
    PSX_REQUIRE(S != nullptr && R != nullptr, "%s: null pointer array", fn);
    for (int k = 0; k < PSX_MAX_LCS; ++k) {
        PSX_REQUIRE(k >= K || (S[k] != nullptr && R[k] != nullptr), "%s: position %d has a null image", fn, k);
        p.S[k] = k < K ? S[k] : nullptr;
        p.R[k] = k < K ? R[k] : nullptr;
    }
    return 0;
}

// ---- device math ---------------------------------------------------------------------------------------------
#define PSX_TWO_PI 6.283185307179586476925286766559
#define PSX_INV_TWO_PI 0.15915494309189533576888376337251

// exp(i*ph) for a float64 phase of any magnitude: the phase in REVOLUTIONS is reduced to [-0.5, 0.5] in float64 and goes
// through the hardware's v_sin_f32 / v_cos_f32, which take revolutions: two quarter-rate instructions instead of the ~50 of
// sincosf (round 4; the transposing pre-pass of the Fresnel engine was bound by this arithmetic: 49 us of a 135 us step at
// 2048^2).  Measured on gfx950 over 2^26 points of [-0.5, 0.5) (tools/sincos_accuracy.hip): max |error| 1.25e-7 for either
// function, against 0.6-0.7e-7 for sincosf -- both below the 1.9e-7 rad that rounding the reduced angle to float32 costs.
__device__ __forceinline__ void cis_f64(double ph, float &c, float &s) {
    const double t = ph * PSX_INV_TWO_PI;
    const float rev = (float)(t - rint(t));
    s = __builtin_amdgcn_sinf(rev);
    c = __builtin_amdgcn_cosf(rev);
}

// exp(x) for a float64 log-attenuation of a few units at most: 2^(x log2 e) through v_exp_f32 (1 ulp); the product is formed
// in float64 and rounded once (half an ulp of a number of a few units: <= 2e-7 relative in the result)
__device__ __forceinline__ float exp_att(double la) { return __builtin_amdgcn_exp2f((float)(la * 1.4426950408889634)); }

// sum_m cphase[m]*T[m][p] and sum_m catt[m]*T[m][p] in float64.
// NM is the compile-time material count the kernel was instantiated for (pack_mats pads unused slots with T[0] and zero
// coefficients), so the NM loads are unconditional and independent: the compiler issues them together and waits once.
// (A run-time `if (i < n)` around each load makes hipcc wait vmcnt(0) per material -- guide, "register or load" trap.)
template <int NM>
__device__ __forceinline__ void mats_eval(const Mats &m, int64_t p, double &ph, double &la) {
    float t[NM > 0 ? NM : 1];
#pragma unroll
    for (int i = 0; i < NM; ++i) t[i] = m.T[i][p];
    ph = 0.0;
    la = 0.0;
#pragma unroll
    for (int i = 0; i < NM; ++i) {
        ph = fma(m.cphase[i], (double)t[i], ph);
        la = fma(m.catt[i], (double)t[i], la);
    }
}

// smallest instantiated count >= n
inline int mats_variant(int n) { return n <= 4 ? n : 8; }

// The map pointers of a kernel that takes them apart from a packed Mats (its coefficients come per image or per source):
// every slot the instantiated variant loads, pack_mats' padding included.  The ONE place such a table is built.
inline void map_table(const float *(&T)[PSX_MAX_MAT], const Mats &m) {
    for (int i = 0; i < PSX_MAX_MAT; ++i) T[i] = i < mats_variant(m.n) ? m.T[i] : nullptr;
}

// instantiate the statement for the variant matching n; NM is the compile-time count inside it
#define PSX_DISPATCH_NMAT(n, ...)                    \
    switch (psx::mats_variant(n)) {                  \
        case 0: { constexpr int NM = 0; __VA_ARGS__; } break; \
        case 1: { constexpr int NM = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int NM = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int NM = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int NM = 4; __VA_ARGS__; } break; \
        default: { constexpr int NM = 8; __VA_ARGS__; } break; \
    }

// ---- the rows of a projected line that can reach a window (phantom.hip, volume.hip) ------------------------------------
// Rows r of [0, dimY) where lo - 1 < a + b r < hi + 1 may hold, widened by 2 rows; r0 <= r1, both in [0, dimY].  The
// sample points of the rows outside are more than a pixel outside (lo, hi), which no rounding of the loop's own
// (a' + b r) + off (a few ulps of a value of ~1e4) can close: their four neighbours lie outside the window, and the terms
// skipped are exact zeros.  A slope of ~1e-16 (a multiple of 90 degrees) gives bounds of ~1e17: clamped before any cast.
__device__ inline void row_span(double a, double b, double lo, double hi, double dimY, double &r0, double &r1) {
    lo -= 1.0;
    hi += 1.0;
    if (b == 0.0) {
        if (lo < a && a < hi) {
            r0 = 0.0;
            r1 = dimY;
        } else {
            r0 = r1 = 0.0;
        }
        return;
    }
    double u = (lo - a) / b, v = (hi - a) / b;
    if (u > v) {
        const double w = u;
        u = v;
        v = w;
    }
    r0 = fmin(fmax(0.0, floor(u) - 2.0), dimY);
    r1 = fmax(fmin(dimY, ceil(v) + 3.0), 0.0);
}

// diagnostic phase-timestamp buffer (psx_debug_stamps); null in every timed run
extern unsigned long long *g_stamps;

// Diagnostic A/B switches (psx_debug_switch): process-wide, all 0 by default (stamp_round: 1), never read from the
// environment -- a stray variable must not change what a product run computes.  The host code reads them per call.
enum DebugSwitch {
    DBG_STAMP_PASS1 = 0,   // psx_debug_stamps records pass 1 instead of pass 2
    DBG_STAMP_ROUND,       // which round of a unit the stamps are taken in
    DBG_DETECT_4PASS,      // detector stages as four passes instead of fused pairs
    DBG_NO_P2,             // Fresnel LDS engine: lines through the 576 R3-point transforms even where a power of two serves (read when a plan is created)
    DBG_COUNT
};
int debug_switch(DebugSwitch s);

// ---- optional per-kernel timing with HIP events on the launch stream (psx_profile_*) ---------------------------------
// Off by default: a ProfScope then costs one branch.  When on, every kernel launch of the library is bracketed by two
// events recorded on the stream it is launched on; psx_profile_summary() resolves them after the work has drained.
bool prof_enabled();
int prof_begin(const char *name, hipStream_t st);
void prof_end(int handle, hipStream_t st);

struct ProfScope {
    int h;
    hipStream_t st;
    ProfScope(const char *name, hipStream_t s) : h(prof_enabled() ? prof_begin(name, s) : -1), st(s) {}
    ~ProfScope() {
        if (h >= 0) prof_end(h, st);
    }
};

// launch statement(s) bracketed by a timing scope:  PSX_TIMED("k_name", stream, k_name<<<g, b, 0, stream>>>(args));
#define PSX_TIMED(name, st, ...)        \
    do {                                \
        psx::ProfScope ps__(name, st);  \
        __VA_ARGS__;                    \
    } while (0)

// Per-device one-time set-up (function attributes such as the dynamic LDS limit belong to the device's copy of the code
// object): true the first time it is called for `mask` on the CURRENT device.  Nothing in the library caches a device
// property in a process-wide static, so one process may drive several GPUs (one host thread per GPU).
inline bool first_on_device(std::atomic<unsigned long long> &mask) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    return !(mask.fetch_or(bit) & bit);
}

// The dynamic-LDS limit of a kernel that launches with more than the default allows, set once per device: one mask per
// kernel instantiation.  if (int rc = allow_dynamic_lds<k_name<...>>(bytes)) return rc;
template <auto Kernel>
int allow_dynamic_lds(int bytes) {
    static std::atomic<unsigned long long> mask{0};
    if (first_on_device(mask))
        PSX_HIP(hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return 0;
}

// compute units of the current device (queried per call: ~0.1 us, no cache to go stale when the device changes)
inline int current_cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 8;
    return n < 8 ? 8 : n;
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// grid for a grid-stride elementwise kernel: enough blocks to fill 256 CUs x 8, capped (guide G11)
inline int ew_grid(int64_t n, int block, int per_thread = 1) {
    int64_t g = cdiv(n, (int64_t)block * per_thread);
    if (g > 2048 * 8) g = 2048 * 8;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace psx
