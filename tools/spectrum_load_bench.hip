// Microbenchmark (diagnostic): what the engine waves' kernel-spectrum loads of the power-of-two line kernels (fresnel_p2.hip) cost
// by the cache lines a wave instruction touches.  Per round every lane of 8 waves takes 128 bytes of an L2-resident 64 KiB table
// (four tables in turn, as four distances) in eight 16-byte loads:
//   pattern (a), slab order:  a lane reads its own 128-byte slab, lanes permuted as the middle stage's slab_of_lane -- neighbouring
//                             lanes 256 bytes apart, every wave instruction touches 64 different 128-byte lines
//   pattern (b), lane order:  instruction q of a wave reads one aligned 1 KiB block, lane l at byte 16 l -- 8 lines
// alone, and beside four more waves that issue pass 2's loader fetch (16-byte loads at a 64-byte stride from a 134 MB buffer, 16
// per thread and round) just behind the spectrum loads, as the kernel does at barrier (1).
// 256 persistent workgroups; a round is: spectrum loads issued | barrier | fetch issued, everything waited for | barrier.
// Prints microseconds per round (kernel time / rounds), the time from issue to arrival of the spectrum loads (wave 0), and the
// time the fetch takes to ISSUE (loader wave 0), each as min / mean / max over REPS launches of the same process.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
constexpr int NWG = 256, TE = 512, TLD = 256, ROUNDS = 2000, REPS = 6;
constexpr size_t TABLE = 64 * 1024, NTAB = 4, FETCH_BYTES = 128u << 20, CHUNK = 256 * 1024;
__device__ __forceinline__ int slab_of_lane(int ln) { return (ln & 32) + ((ln & 31) < 16 ? 2 * (ln & 31) : 2 * ((ln & 31) - 16) + 1); }
// PAT 0: (a), 1: (b), 2: no spectrum loads (the fetch alone)
template <int PAT, bool FETCH>
__global__ __launch_bounds__(TE + (FETCH ? TLD : 0)) void k(const char *tab, const char *big, float *sink, long long *clk) {
    const int tid = threadIdx.x;
    float acc = 0.f;
    long long t_spec = 0, t_issue = 0;
    if (tid < TE) {
        const int w = tid >> 6, ln = tid & 63;
        const size_t lane_off = PAT == 0 ? (size_t)(64 * w + slab_of_lane(ln)) * 128 : (size_t)(8 * w) * 1024 + 16 * ln;
        constexpr int QS = PAT == 0 ? 1 : 64;            // float4 elements between a lane's eight loads
        for (int r = 0; r < ROUNDS; ++r) {
            float4 hh[8];
            long long t0 = 0;
            if constexpr (PAT != 2) {
                const float4 *h4 = reinterpret_cast<const float4 *>(tab + (size_t)(r & 3) * TABLE + lane_off);
                t0 = wall_clock64();
#pragma unroll
                for (int q = 0; q < 8; ++q) hh[q] = h4[q * QS];
            }
            __syncthreads();
            if constexpr (PAT != 2) {
#pragma unroll
                for (int q = 0; q < 8; ++q) acc += hh[q].x + hh[q].y + hh[q].z + hh[q].w;
                asm volatile("" : "+v"(acc));
                t_spec += wall_clock64() - t0;
            }
            __syncthreads();
        }
        if (tid == 0) clk[2 * blockIdx.x] = t_spec;
    } else {
        const int lt = tid - TE;
        for (int r = 0; r < ROUNDS; ++r) {
            const size_t chunk = ((size_t)blockIdx.x * 131 + r) % (FETCH_BYTES / CHUNK);
            const float4 *src = reinterpret_cast<const float4 *>(big + chunk * CHUNK + (size_t)lt * 64);
            float4 xv[16];
            __syncthreads();
            const long long t0 = wall_clock64();
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) xv[kk] = src[(size_t)kk * TLD * 4];     // 64-byte stride between lanes, 16 KiB between loads
            asm volatile("" ::: "memory");
            t_issue += wall_clock64() - t0;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) acc += xv[kk].x + xv[kk].w;
            asm volatile("" : "+v"(acc));
            __syncthreads();
        }
        if (lt == 0) clk[2 * blockIdx.x + 1] = t_issue;
    }
    if (acc == 12345.678f) sink[blockIdx.x] = acc;
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
int main() {
    char *tab, *big; float *sink; long long *clk, hclk[2 * NWG];
    CK(hipMalloc(&tab, NTAB * TABLE)); CK(hipMalloc(&big, FETCH_BYTES)); CK(hipMalloc(&sink, NWG * sizeof(float))); CK(hipMalloc(&clk, sizeof(hclk)));
    CK(hipMemset(tab, 0, NTAB * TABLE)); CK(hipMemset(big, 0, FETCH_BYTES));
    int khz = 0;
    CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto run = [&](const char *nm, auto f) {
        double us[REPS], sp[REPS], is[REPS];
        f(); (void)hipDeviceSynchronize();
        for (int rep = 0; rep < REPS; ++rep) {
            (void)hipMemset(clk, 0, sizeof(hclk));
            (void)hipEventRecord(e0); f(); (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
            float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
            (void)hipMemcpy(hclk, clk, sizeof(hclk), hipMemcpyDeviceToHost);
            double a = 0, b = 0;
            for (int i = 0; i < NWG; ++i) { a += (double)hclk[2 * i]; b += (double)hclk[2 * i + 1]; }
            us[rep] = ms * 1e3 / ROUNDS; sp[rep] = a / NWG / ROUNDS / (khz * 1e-3); is[rep] = b / NWG / ROUNDS / (khz * 1e-3);
        }
        auto st = [&](const double *v, char *out) {
            double mn = v[0], mx = v[0], s = 0;
            for (int i = 0; i < REPS; ++i) { mn = v[i] < mn ? v[i] : mn; mx = v[i] > mx ? v[i] : mx; s += v[i]; }
            sprintf(out, "%6.3f / %6.3f / %6.3f", mn, s / REPS, mx);
        };
        char b0[64], b1[64], b2[64]; st(us, b0); st(sp, b1); st(is, b2);
        printf("%-44s round %s us   spectrum issue->arrival %s us   fetch issue %s us\n", nm, b0, b1, b2);
    };
    printf("min / mean / max of %d launches, %d rounds each, %d workgroups; wall clock %d kHz\n", REPS, ROUNDS, NWG, khz);
    for (int pass = 0; pass < 2; ++pass) {          // the whole table twice: (a) is repeated inside ONE process, interleaved with (b)
        run("(a) slab order, alone", [&] { k<0, false><<<NWG, TE>>>(tab, big, sink, clk); });
        run("(b) lane order, alone", [&] { k<1, false><<<NWG, TE>>>(tab, big, sink, clk); });
        run("fetch alone (no spectrum loads)", [&] { k<2, true><<<NWG, TE + TLD>>>(tab, big, sink, clk); });
        run("(a) slab order, beside the fetch", [&] { k<0, true><<<NWG, TE + TLD>>>(tab, big, sink, clk); });
        run("(b) lane order, beside the fetch", [&] { k<1, true><<<NWG, TE + TLD>>>(tab, big, sink, clk); });
    }
    CK(hipDeviceSynchronize());
    return 0;
}
