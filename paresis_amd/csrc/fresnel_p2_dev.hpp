// fresnel_p2_dev.hpp -- device helpers shared by the power-of-two line kernels of the LDS Fresnel engine (fresnel_p2.hip: lines that
// fit ONE M-point transform; fresnel_p2x.hip: lines of 4 M points' worth, two coupled rounds): stage A's twiddles from binary
// powers, the stage-B butterflies on registers, the window stores of inverse stage A.
#pragma once
#include "fresnel_stages.hpp"

namespace psx {
namespace p2dev {

using namespace psx::lines;

constexpr int BSTR = 256 + 8;  // padded stride of a block of 256 points (one pad slot per 32)

// ---- Memory order of the kernel-spectrum tables.  In the middle stage lane ln of a wave holds slab slab_of_lane(ln) of the wave's
// 64 slabs: within each half-wave the first 16 lanes take the even slabs and the last 16 the odd ones (one pad slot per TWO slabs:
// 16 different bank pairs per ds_write_b64 group).  The table is stored so that ONE load instruction of a wave reads ONE aligned
// 1 KiB block, lane ln at byte 16 ln (8 cache lines, where a slab-major table cost 64):
//     [group of 64 slabs][unit q of the slab][lane][16 bytes],
// a unit being the 16 bytes a lane takes with one load: UPS = 8 units of two points per slab in fresnel_p2.hip, 16 units of one
// (bin, bin + M) pair in fresnel_p2x.hip.  The table builders (k_p2_perm, k_p2x_perm) and the readers use the functions below and
// nothing else.
namespace spectrum {
__host__ __device__ constexpr int slab_of_lane(int ln) { return (ln & 32) + ((ln & 31) < 16 ? 2 * (ln & 31) : 2 * ((ln & 31) - 16) + 1); }
__host__ __device__ constexpr int lane_of_slab(int s) { return (s & 32) + ((s & 1) ? 16 : 0) + ((s & 31) >> 1); }
// 16-byte unit index of unit q of lane ln's slab in group g (the reader's form: g and q are uniform, ln is the lane itself)
template <int UPS>
__host__ __device__ constexpr int unit_of_lane(int g, int q, int ln) { return (g * UPS + q) * 64 + ln; }
// ... and of unit q of slab s of the transformed line (the builder's form)
template <int UPS>
__host__ __device__ constexpr int unit_of_slab(int s, int q) { return unit_of_lane<UPS>(s >> 6, q, lane_of_slab(s & 63)); }
// fresnel_p2.hip: float2 index of position p = 16 slab + k3 of the transformed line (points 2q, 2q + 1 of a slab share a unit)
__host__ __device__ constexpr int point_index(int p) { return 2 * unit_of_slab<8>(p >> 4, (p & 15) >> 1) + (p & 1); }
// fresnel_p2x.hip: float4 index of the pair at position p of a round's LDS lines
__host__ __device__ constexpr int pair_index(int p) { return unit_of_slab<16>(p >> 4, p & 15); }

constexpr bool lanes_invert() {
    for (int ln = 0; ln < 64; ++ln)
        if (lane_of_slab(slab_of_lane(ln)) != ln || slab_of_lane(lane_of_slab(ln)) != ln) return false;
    return true;
}
// is f a bijection of [0, m)?  (m <= 8192)
template <typename F>
constexpr bool is_bijection(F f, int m) {
    bool seen[8192] = {};
    for (int p = 0; p < m; ++p) {
        const int i = f(p);
        if (i < 0 || i >= m || seen[i]) return false;
        seen[i] = true;
    }
    return true;
}
// what the reader finds: unit q of lane ln of group g holds positions 16 slab + 2q, + 1 of slab 64 g + slab_of_lane(ln)
constexpr bool reader_meets_builder(int m) {
    for (int g = 0; g < m / 1024; ++g)
        for (int q = 0; q < 8; ++q)
            for (int ln = 0; ln < 64; ++ln) {
                const int p = 16 * (64 * g + slab_of_lane(ln)) + 2 * q;
                if (point_index(p) != 2 * unit_of_lane<8>(g, q, ln) || point_index(p + 1) != 2 * unit_of_lane<8>(g, q, ln) + 1) return false;
                if (q == 0 && (pair_index(p) != unit_of_lane<16>(g, 0, ln) || pair_index(p + 15) != unit_of_lane<16>(g, 15, ln))) return false;
            }
    return true;
}
static_assert(lanes_invert(), "slab_of_lane and lane_of_slab are inverse permutations of the 64 lanes");
static_assert(is_bijection(point_index, 256 * 4) && is_bijection(point_index, 256 * 8) && is_bijection(point_index, 256 * 16) &&
                  is_bijection(point_index, 256 * 32) && is_bijection(pair_index, 256 * 32),
              "the table order is a bijection of the M positions for R1 = 4, 8, 16, 32");
static_assert(reader_meets_builder(256 * 4) && reader_meets_builder(256 * 32), "a lane's loads find its own slab");
}  // namespace spectrum

// ---- One round of k_fresnel_p2 as the engine waves AND the loader waves see it: which of its phases run and which workgroup
// barriers it executes, by (DUAL, index of the round among the rounds of its line group, their number).  Both branches of the kernel
// take every barrier through round_barrier() with the plan of round_plan() and nothing else: a barrier one side executes and the
// other does not is a hang, so there is no second place to state it.
//   plain rounds and the first round of a DUAL line group: forward stage A, barrier FWD_A behind it.
//   DUAL, first round of several: the loaders copy the first half of the LDS lines -- the line after forward stage A, which forward
//     stage B reads and no longer overwrites -- into registers.  No barrier for it: the loaders count themselves in an LDS flag
//     once their reads have returned and an engine wave tests the flag before its middle stage's first write into that half.
//   DUAL, every round but the last: behind barrier REGS the loaders write the snapshot back (restore) where they otherwise spread
//     the next group's samples; the next round then starts at forward stage B: no forward stage A, no barrier FWD_A.
enum RoundBarrier { RB_FWD_A = 0, RB_PRIVATE, RB_REGS, RB_NEXT, RB_COUNT };
struct RoundPlan {
    bool forward_a, snapshot, restore;
    constexpr bool has(RoundBarrier b) const { return b == RB_FWD_A ? forward_a : true; }
};
__host__ __device__ constexpr RoundPlan round_plan(bool dual, int sub, int nsub) {
    return RoundPlan{!dual || sub == 0, dual && sub == 0 && nsub > 1, dual && sub + 1 < nsub};
}
__device__ __forceinline__ void round_barrier(const RoundPlan &rp, RoundBarrier b) {
    if (rp.has(b)) lds_barrier();
}
// a line group's rounds hang together: a round starts from the snapshot exactly when the round before it restored one, a
// snapshot is taken exactly when one will be restored, and plain rounds are what they were
constexpr bool rounds_consistent() {
    for (int nsub = 1; nsub <= 16; ++nsub) {
        bool held = false;
        for (int s = 0; s < nsub; ++s) {
            const RoundPlan rp = round_plan(true, s, nsub), pl = round_plan(false, s, nsub);
            if (!pl.forward_a || pl.snapshot || pl.restore) return false;
            if (rp.forward_a != (s == 0) || (s > 0 && !held)) return false;
            if (rp.snapshot) held = true;
            if (rp.snapshot && !rp.forward_a) return false;
            if (rp.restore && !held) return false;
            if (s > 0 && !round_plan(true, s - 1, nsub).restore) return false;
        }
        if (round_plan(true, nsub - 1, nsub).restore || held != (nsub > 1)) return false;
    }
    return true;
}
static_assert(rounds_consistent(), "the rounds of a DUAL line group");

// Stage A's twiddles w_M^{n q}, q < R, from the LB = log2(R) powers w^(n 2^b) of the thread's row: w^(n q) is the product of the
// powers of q's set bits, at most four multiplications deep -- 26 products for R = 32 where two factor tables cost 31 and 62 LDS
// reads (fresnel_lds.hip, twiddle_A); 5 reads here.  The lower half is applied as it is built, the upper half takes w^(16 n) first.
template <int R, bool CONJ>
__device__ __forceinline__ v2f tw_apply(v2f x, v2f w) {
    return CONJ ? pk_cmulc(x, w) : pk_cmul(x, w);
}
template <int R>
__device__ __forceinline__ void tw_powers(v2f (&pw)[5], const v2f *row) {
    pw[0] = lds_read(row);
    if constexpr (R >= 4) pw[1] = lds_read(row + 1);
    if constexpr (R >= 8) pw[2] = lds_read(row + 2);
    if constexpr (R >= 16) pw[3] = lds_read(row + 3);
    if constexpr (R == 32) pw[4] = lds_read(row + 4);
}
template <int R, bool CONJ>
__device__ __forceinline__ void twiddle_A2(v2f (&v)[R], const v2f (&pw)[5]) {
    constexpr int H = R >= 16 ? 16 : R;          // twiddles built explicitly: q < H
    v2f t[H];
    t[1] = pw[0];
    if constexpr (R >= 4) t[2] = pw[1];
    if constexpr (R >= 8) t[4] = pw[2];
    if constexpr (R >= 16) t[8] = pw[3];
    v2f t16 = (v2f){1.f, 0.f};
    if constexpr (R == 32) t16 = pw[4];
    if constexpr (R >= 4) t[3] = pk_cmul(t[1], t[2]);
    if constexpr (R >= 8) {
#pragma unroll
        for (int r = 1; r < 4; ++r) t[4 + r] = pk_cmul(t[4], t[r]);
    }
    if constexpr (R >= 16) {
#pragma unroll
        for (int r = 1; r < 8; ++r) t[8 + r] = pk_cmul(t[8], t[r]);
    }
#pragma unroll
    for (int q = 1; q < H; ++q) v[q] = tw_apply<R, CONJ>(v[q], t[q]);
    if constexpr (R == 32) {
#pragma unroll
        for (int q = 16; q < 32; ++q) v[q] = tw_apply<R, CONJ>(v[q], t16);
#pragma unroll
        for (int q = 17; q < 32; ++q) v[q] = tw_apply<R, CONJ>(v[q], t[q - 16]);
    }
}

// leg q of a stage-B butterfly / point q of a slab
__device__ __forceinline__ int offB(int q) { return 16 * q + (q >> 1); }

// forward stage B on registers: radix 16, then twiddle w_256^{n3 k2} on the outputs
__device__ __forceinline__ void fwdB_regs(v2f (&v)[16], const v2f (&w)[16]) {
    DftPk<16, false>::run(v);
#pragma unroll
    for (int q = 1; q < 16; ++q) v[q] = pk_cmul(v[q], w[q]);
}
// inverse stage B: conjugate twiddle on the inputs, then the inverse butterfly
__device__ __forceinline__ void invB_regs(v2f (&v)[16], const v2f (&w)[16]) {
#pragma unroll
    for (int q = 1; q < 16; ++q) v[q] = pk_cmulc(v[q], w[q]);
    DftPk<16, true>::run(v);
}

// Legs Q0 .. R-1 + the wrapped leg of one inverse stage-A butterfly through a buffer descriptor whose range is the window the
// line may touch (fresnel_stages.hpp, store_window: the hardware drops what falls outside).  Leg q goes to element e0 + q *
// estep, the wrapped leg vw (leg 0 + its fix-up) to e0 + R * estep.
// Q0 = R / 2: the caller knows that the lower half of the legs lies before sample 0 for EVERY butterfly of the line (leg q of
// butterfly n is sample n + 256 q - (P - 1); so whenever P - 1 >= M / 2, i.e. on every power-of-two grid) -- their stores, and
// the |.|^2 or global phase in front of them, are not issued at all.  (A per-leg uniform test instead of the two compiled forms
// cost pass 2 what it saved: gpurun_out/r6s9.)
template <int R, int Q0>
__device__ __forceinline__ void store_legs(const v2f (&v)[R], v2f vw, v2f *wo, float *io, int64_t wbase, int welems, int e0, int estep,
                                           v2f gp, float sc, int accumulate) {
    // byte offsets in UNSIGNED arithmetic: an element index below the window wraps to a huge offset (dropped), and the window of a
    // 16384^2 intermediate is 2^31 bytes long
    if (wo) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(wo + wbase, 0, (int)((unsigned)welems * 8u), 0x00020000);
        const bool plain = gp.x == 1.f && gp.y == 0.f;     // pass 1: no global phase
        unsigned off = ((unsigned)e0 + (unsigned)Q0 * (unsigned)estep) * 8u;
#pragma unroll
        for (int q = Q0; q <= R; ++q) {
            const v2f x = q < R ? v[q < R ? q : 0] : vw;
            const v2f r = plain ? x : pk_cmul_s(x, gp);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, r), rs, (int)off, 0, 0);
            off += (unsigned)estep * 8u;
        }
    }
    if (io) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(io + wbase, 0, (int)((unsigned)welems * 4u), 0x00020000);
        unsigned off = ((unsigned)e0 + (unsigned)Q0 * (unsigned)estep) * 4u;
#pragma unroll
        for (int q = Q0; q <= R; ++q) {
            const v2f x = q < R ? v[q < R ? q : 0] : vw;
            float I = sc * (x.x * x.x + x.y * x.y);
            if (accumulate) I += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0));
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, I), rs, (int)off, 0, 0);
            off += (unsigned)estep * 4u;
        }
    }
}

// CNT consecutive legs, the first of them leg q0, of a butterfly whose leg q goes to element e0 + q * estep of the window (the
// two-round kernel stores a butterfly in two halves, each as soon as its data is there)
template <int CNT>
__device__ __forceinline__ void store_legs_range(const v2f (&v)[CNT], int q0, v2f *wo, float *io, int64_t wbase, int welems, int e0, int estep,
                                                 v2f gp, float sc, int accumulate) {
    if (wo) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(wo + wbase, 0, (int)((unsigned)welems * 8u), 0x00020000);
        const bool plain = gp.x == 1.f && gp.y == 0.f;
        unsigned off = ((unsigned)e0 + (unsigned)q0 * (unsigned)estep) * 8u;
#pragma unroll
        for (int q = 0; q < CNT; ++q) {
            const v2f r = plain ? v[q] : pk_cmul_s(v[q], gp);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, r), rs, (int)off, 0, 0);
            off += (unsigned)estep * 8u;
        }
    }
    if (io) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(io + wbase, 0, (int)((unsigned)welems * 4u), 0x00020000);
        unsigned off = ((unsigned)e0 + (unsigned)q0 * (unsigned)estep) * 4u;
#pragma unroll
        for (int q = 0; q < CNT; ++q) {
            float I = sc * (v[q].x * v[q].x + v[q].y * v[q].y);
            if (accumulate) I += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0));
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, I), rs, (int)off, 0, 0);
            off += (unsigned)estep * 4u;
        }
    }
}

}  // namespace p2dev
}  // namespace psx
