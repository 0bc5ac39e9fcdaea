// umpa.hip -- UMPA windowed speckle tracking (psx_umpa_f32): integer search over (2s+1)^2 shifts of a uniform (2w+1)^2 window
// and a per-axis parabola, for displacements beyond the one pixel that LCS (retrieve.hip) is valid for.
//
// UMPA ("Unified Modulated Pattern Analysis", Zdora et al., PRL 118, 203903, 2017) in the separable form of De Marco et al.,
// Opt. Express 31, 635 (2023), with a UNIFORM window (no Hamming taper: that is what makes the window sums box filters).
// Model S_k(q) ~ T*R_k(q - u).  Per interior pixel r (at least w+s from every border), sums over k and the window around r:
//   E = sum S_k(q)^2,  B(u) = sum S_k(q) R_k(q-u),  C(u) = sum R_k(q-u)^2,  L(u) = E - B*B/C,  T(u) = B/C  (float64);
//   a candidate with C(u) == 0 is skipped; u* = the first strict minimum of L, a outer, b inner, ascending.
// The sums are box filters of per-pixel maps: B(u)(r) = box_w[sum_k S_k(q) R_k(q-u)](r), C(u)(r) = box_w[sum_k R_k^2](r-u)
// (once per tile), E = box_w[sum_k S_k^2]: K FMAs and 2(2w+1) adds per pixel and candidate, not K(2w+1)^2.
//
// k_umpa<TW, S>: one workgroup of 256 threads per 16 x TW output tile (TW = 32 up to w = 4, 16 beyond).
//   "region": the tile grown by w, Hr x Wr = (16+2w) x (TW+2w): where the product maps are needed.  A thread owns two "units" of two
//   adjacent region pixels and keeps their float64 product sums for one chunk of NB candidates (one row a, NB consecutive b).
//   prologue  sum_k R_k^2 on the region grown by s -> LDS -> separable box -> Cb, the tile grown by s (float64, LDS);
//             sum_k S_k^2 on the region -> box -> E (registers)
//   per row a, per chunk: for every k, the R_k rows of this a (region grown by s along axis 1) are staged as float32 in LDS,
//             double-buffered (position k+1 is in flight while k is used: one barrier per position); S_k comes straight from
//             L2 into the owning thread.  Then, candidate by candidate: product map -> LDS (float64) -> row sums -> column
//             sums -> B at the thread's output pixels -> cost, running minimum and its four parabola neighbours.
//   The images are read again from L2 for every chunk; no cost volume exists anywhere.  The previous row's costs stay in
//   registers (statically indexed: the chunk loop is unrolled), which is why the search half-width is a template parameter.
// Nothing outside the images is ever read: staged pixels outside are 0 and belong to border-band windows only, whose pixels
// get (1, 0, 0, 0) by the border rule.
//
// Dark field (psx_umpa_df_f32, k_umpa<TW, S, true>): the model S_k(q) ~ alpha*R_k(q - u) + beta*mu_k, mu_k the mean of reference
// frame k, T = alpha + beta, visibility V = alpha/T.  The same kernel under `if constexpr (DF)`, with
//   F = box_w[sum_k mu_k S_k] beside E (registers), G(u)(r) = box_w[sum_k mu_k R_k](r - u) beside C (a second LDS map Gb laid
//   out like Cb, from the loads prologue 1 makes anyway), H = (2w+1)^2 sum_k mu_k^2 (host), mu and H in the argument block;
//   per candidate the 2 x 2 normal equations (umpa_df_solve, every operation rounded on its own) instead of E - B*B/C.
// The search loop's staging and product FMAs are the same code.
#include "common.hpp"

using namespace psx;

namespace {

// The dark-field kernel's own arguments, last in the argument block (empty without: k_umpa<TW, S, false> is then the kernel it
// was): the reference frames' means, H = (2w+1)^2 sum_k mu_k^2 and the fifth map.
template <bool DF>
struct UmpaDf {};
template <>
struct UmpaDf<true> {
    double mu[PSX_MAX_LCS];
    double H;
    float *vis;
};

constexpr int UMPA_TH = 16, UMPA_NT = 256, UMPA_NU = 2;
// The tile is UMPA_TH x TW, TW = 32 up to w = 4 and 16 beyond, so that the region's (16+2w)(TW/2+w) units never exceed
// UMPA_NU = 2 per thread (480 at w = 4, 512 at w = 8) and the accumulators, the previous cost row and the running minimum stay
// inside the register file at every (w, s).  A thread has TH*TW/256 output pixels: rows ty, ty + 256/TW, column tx.
// The dark-field kernel takes the narrow tile at s = 8 for every w: its TW = 32, s = 8 instantiation (256 VGPRs + 56 AGPRs)
// spilled 12 VGPRs, with a shorter chunk 20, and is not compiled (umpa_launch); <16, 8> has 235 and none.
inline int umpa_tw(int w, int s, bool df) { return w > 4 || (df && s == 8) ? 16 : 32; }

// candidates per chunk / chunks per row for the search half-width s: NB*NCH >= 2s+1 with at most one surplus candidate
__host__ __device__ constexpr int umpa_nb(int s) { return s <= 3 ? 2 * s + 1 : s == 4 || s == 7 ? 5 : s == 6 ? 7 : 6; }
__host__ __device__ constexpr int umpa_nch(int s) { return (2 * s + 1 + umpa_nb(s) - 1) / umpa_nb(s); }

struct UmpaLds {   // byte offsets into the dynamic LDS
    int cb, rbuf0, rbuf1, pmap, hmap, tmp, total;
};

// Cb | 16 B | R buffer 0 | 16 B | R buffer 1 | P | H, the prologue's sum R^2 map overlaying everything behind Cb.  The 16 bytes
// before each R buffer take the one read at column -1 that a surplus candidate (b = s+1, dropped) makes in region row 0.
// Dark field: Gb follows Cb at once (cb then spans both), at most 2 * 11 KB; the largest total is 46304 bytes at (4, 7).
inline UmpaLds umpa_lds(int w, int s, bool df) {
    const int UMPA_TW = umpa_tw(w, s, df);
    const int Hr = UMPA_TH + 2 * w, Wr = UMPA_TW + 2 * w, Wrr = Wr + 2 * s;
    UmpaLds l;
    l.cb = 0;
    const int cb_bytes = (UMPA_TH + 2 * s) * (UMPA_TW + 2 * s) * 8 * (df ? 2 : 1);
    l.tmp = cb_bytes;
    l.rbuf0 = cb_bytes + 16;
    const int rb = (Hr * Wrr * 4 + 15) & ~15;
    l.rbuf1 = l.rbuf0 + rb + 16;
    l.pmap = l.rbuf1 + rb;
    l.hmap = l.pmap + Hr * Wr * 8;
    const int main_end = l.hmap + Hr * UMPA_TW * 8;
    const int tmp_end = l.tmp + (Hr + 2 * s) * Wrr * 8;
    l.total = main_end > tmp_end ? main_end : tmp_end;
    return l;
}

// Separable box sum of one region map: vals (this thread's NU units) -> P -> row sums H -> column sums at the thread's
// output pixels.  Two barriers; the caller's next P write may follow at once (it is behind the second barrier, and
// the next H write is behind the next call's first).
template <int UMPA_TW, int NU = UMPA_NU, int UMPA_PX = UMPA_TH * UMPA_TW / UMPA_NT>
__device__ __forceinline__ void umpa_box(const double (&v0)[NU], const double (&v1)[NU], const bool (&uok)[NU], const int (&upos)[NU],
                                         double *__restrict__ P, double *__restrict__ H, int w, int Hr, int Wr, int tx, int ty,
                                         double (&out)[UMPA_PX]) {
    constexpr int RS = UMPA_NT / UMPA_TW;
#pragma unroll
    for (int u = 0; u < NU; ++u)
        if (uok[u]) *reinterpret_cast<double2 *>(P + upos[u]) = make_double2(v0[u], v1[u]);
    __syncthreads();
    for (int row = ty; row < Hr; row += RS) {
        const double *p = P + row * Wr + tx;
        double acc = p[0];
        for (int d = 1; d <= 2 * w; ++d) acc += p[d];
        H[row * UMPA_TW + tx] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < UMPA_PX; ++t) {
        const double *h = H + (ty + RS * t) * UMPA_TW + tx;
        double acc = h[0];
        for (int d = 1; d <= 2 * w; ++d) acc += h[d * UMPA_TW];
        out[t] = acc;
    }
}

// The dark-field candidate: the 2 x 2 normal equations of S ~ alpha*R(q-u) + beta*mu, every operation rounded on its own (the
// contract fixes the sequence, and the tests compare bit for bit).  false: the candidate is skipped.
__device__ __forceinline__ bool umpa_df_solve(double E, double B, double C, double F, double G, double H, double &Lc, double &al,
                                              double &Tc) {
#pragma clang fp contract(off)
    const double pp = C * H, qq = G * G, det = pp - qq;
    if (!(det > 1e-12 * pp)) return false;
    const double bh = B * H, fg = F * G, cf = C * F, gb = G * B;
    al = (bh - fg) / det;
    const double be = (cf - gb) / det;
    const double ab = al * B, bf = be * F;
    Lc = E - (ab + bf);
    Tc = al + be;
    return true;
}

template <int UMPA_TW, int S, bool DF = false>
__global__ __launch_bounds__(UMPA_NT) void k_umpa(SpecklePtrs p, int K, int n, int m, int w, UmpaLds L, float *__restrict__ trans,
                                                  float *__restrict__ dx, float *__restrict__ dy, float *__restrict__ resid,
                                                  UmpaDf<DF> mu) {
    constexpr int NU = UMPA_NU, UMPA_PX = UMPA_TH * UMPA_TW / UMPA_NT, RS = UMPA_NT / UMPA_TW;
    constexpr int NB = umpa_nb(S), NCH = umpa_nch(S), ROW = NB * NCH;
    constexpr int W2 = UMPA_TW + 2 * S, H2 = UMPA_TH + 2 * S;        // the tile grown by s: where C is needed
    extern __shared__ __attribute__((aligned(16))) unsigned char umpa_smem[];
    double *const Cb = reinterpret_cast<double *>(umpa_smem + L.cb);
    double *const Gb = Cb + H2 * W2;                                 // dark field only
    float *const Rb0 = reinterpret_cast<float *>(umpa_smem + L.rbuf0);
    float *const Rb1 = reinterpret_cast<float *>(umpa_smem + L.rbuf1);
    double *const P = reinterpret_cast<double *>(umpa_smem + L.pmap);
    double *const H = reinterpret_cast<double *>(umpa_smem + L.hmap);
    double *const tmp = reinterpret_cast<double *>(umpa_smem + L.tmp);

    const int tid = threadIdx.x, tx = tid & (UMPA_TW - 1), ty = tid / UMPA_TW;
    const int lane = tid & 63, wv = tid >> 6;
    const int i0 = blockIdx.y * UMPA_TH, j0 = blockIdx.x * UMPA_TW;
    const int Hr = UMPA_TH + 2 * w, Wr = UMPA_TW + 2 * w, Wrr = Wr + 2 * S;
    const double NaN = __builtin_nan("");

    // ---- prologue 1: sum_k R_k^2 on (Hr+2s) x Wrr (lane = column, wave = rows wv, wv+4, ...) -> tmp -> box -> Cb ----------
    // (dark field: sum_k mu_k R_k from the same loads, through the same box -> Gb)
    {
        constexpr int RMAX = (UMPA_TH + 2 * PSX_MAX_UMPA_WINDOW + 2 * S + 3) / 4;
        const int Hc = Hr + 2 * S;
        const int gj = j0 - w - S + lane;
        const bool cok = lane < Wrr && gj >= 0 && gj < m;
        double acc[RMAX], accg[DF ? RMAX : 1];
#pragma unroll
        for (int t = 0; t < RMAX; ++t) acc[t] = 0.0;
        if constexpr (DF) {
#pragma unroll
            for (int t = 0; t < RMAX; ++t) accg[t] = 0.0;
        }
        for (int k = 0; k < K; ++k) {
            const float *Rk = p.R[k];
            double muk = 0.0;
            if constexpr (DF) muk = mu.mu[k];
#pragma unroll
            for (int t = 0; t < RMAX; ++t) {
                const int row = wv + 4 * t, gi = i0 - w - S + row;
                if (row < Hc && cok && gi >= 0 && gi < n) {
                    const double r = Rk[gi * m + gj];
                    acc[t] = fma(r, r, acc[t]);
                    if constexpr (DF) accg[t] = fma(muk, r, accg[t]);
                }
            }
        }
        auto box = [&](const double *src, double *dst) {
#pragma unroll
        for (int t = 0; t < RMAX; ++t) {
            const int row = wv + 4 * t;
            if (row < Hc && lane < Wrr) tmp[row * Wrr + lane] = src[t];
        }
        __syncthreads();
        // row sums: Hc x W2, kept in registers until every thread has read, then written over the map
        constexpr int HMAX = ((UMPA_TH + 2 * PSX_MAX_UMPA_WINDOW + 2 * S) * W2 + UMPA_NT - 1) / UMPA_NT;
        double hs[HMAX];
#pragma unroll
        for (int t = 0; t < HMAX; ++t) {
            const int e = tid + UMPA_NT * t;
            hs[t] = 0.0;
            if (e < Hc * W2) {
                const double *q = tmp + (e / W2) * Wrr + (e % W2);
                double a = q[0];
                for (int d = 1; d <= 2 * w; ++d) a += q[d];
                hs[t] = a;
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < HMAX; ++t) {
            const int e = tid + UMPA_NT * t;
            if (e < Hc * W2) tmp[e] = hs[t];                         // [Hc][W2]
        }
        __syncthreads();
        for (int e = tid; e < H2 * W2; e += UMPA_NT) {
            const double *q = tmp + e;                               // row e / W2 is the window's first row
            double a = q[0];
            for (int d = 1; d <= 2 * w; ++d) a += q[d * W2];
            dst[e] = a;                                              // Cb[y][x]: pixel (i0 - s + y, j0 - s + x)
        }
        __syncthreads();
        };
        box(acc, Cb);
        if constexpr (DF) box(accg, Gb);
    }

    // ---- the thread's units: region pixels (ri, rj) and (ri, rj+1), rj even --------------------------------------------
    const int nunits = Hr * (Wr / 2);
    bool uok[NU];
    int upos[NU], urow[NU], soff0[NU], soff1[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int e = tid + UMPA_NT * u;
        uok[u] = e < nunits;
        const int ee = uok[u] ? e : 0;
        const int ri = ee / (Wr / 2), rj = 2 * (ee % (Wr / 2));
        upos[u] = ri * Wr + rj;
        urow[u] = ri * Wrr + rj;                                     // R buffer: column rj + s - b of row ri
        const int gi = i0 - w + ri, gj = j0 - w + rj;
        const bool rok = uok[u] && gi >= 0 && gi < n;
        soff0[u] = rok && gj >= 0 && gj < m ? gi * m + gj : -1;
        soff1[u] = rok && gj + 1 >= 0 && gj + 1 < m ? gi * m + gj + 1 : -1;
    }

    // ---- prologue 2: E = box[sum_k S_k^2] --------------------------------------------------------------------------------
    double E[UMPA_PX], F[UMPA_PX];                                   // F = box[sum_k mu_k S_k]: dark field only
    {
        double e0[NU], e1[NU], f0[NU], f1[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) e0[u] = e1[u] = f0[u] = f1[u] = 0.0;
        for (int k = 0; k < K; ++k) {
            const float *Sk = p.S[k];
            double muk = 0.0;
            if constexpr (DF) muk = mu.mu[k];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const double a = soff0[u] >= 0 ? Sk[soff0[u]] : 0.f, b = soff1[u] >= 0 ? Sk[soff1[u]] : 0.f;
                e0[u] = fma(a, a, e0[u]);
                e1[u] = fma(b, b, e1[u]);
                if constexpr (DF) {
                    f0[u] = fma(muk, a, f0[u]);
                    f1[u] = fma(muk, b, f1[u]);
                }
            }
        }
        umpa_box<UMPA_TW>(e0, e1, uok, upos, P, H, w, Hr, Wr, tx, ty, E);
        if constexpr (DF) umpa_box<UMPA_TW>(f0, f1, uok, upos, P, H, w, Hr, Wr, tx, ty, F);
    }

    // ---- the search ----------------------------------------------------------------------------------------------------------
    // staging of the R rows: lane = column of the Wrr-wide buffer, wave = region rows wv, wv+4, ...
    constexpr int SMAX = (UMPA_TH + 2 * PSX_MAX_UMPA_WINDOW + 3) / 4;
    const int sgj = j0 - w - S + lane;
    const bool scok = lane < Wrr && sgj >= 0 && sgj < m;

    double bestL[UMPA_PX], bestT[UMPA_PX], bestA[UMPA_PX], Lam[UMPA_PX], Lap[UMPA_PX], Lbm[UMPA_PX], Lbp[UMPA_PX], last[UMPA_PX];
    double prev[UMPA_PX][ROW];
    int ba[UMPA_PX], bb[UMPA_PX];
#pragma unroll
    for (int t = 0; t < UMPA_PX; ++t) {
        bestL[t] = __builtin_inf();
        bestT[t] = bestA[t] = 0.0;                                   // bestA: alpha at the minimum, dark field only
        Lam[t] = Lap[t] = Lbm[t] = Lbp[t] = last[t] = NaN;
        ba[t] = bb[t] = -100;                                        // no minimum yet
#pragma unroll
        for (int c = 0; c < ROW; ++c) prev[t][c] = NaN;              // NaN: no such candidate, or skipped
    }

    for (int a = -S; a <= S; ++a) {
#pragma unroll
        for (int t = 0; t < UMPA_PX; ++t) last[t] = NaN;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const int b0 = -S + ch * NB;
            double acc0[NU][NB], acc1[NU][NB];
#pragma unroll
            for (int u = 0; u < NU; ++u)
#pragma unroll
                for (int c = 0; c < NB; ++c) acc0[u][c] = acc1[u][c] = 0.0;

            float rpre[SMAX], s0[NU], s1[NU];
            auto fetch = [&](int k) {
                const float *Rk = p.R[k], *Sk = p.S[k];
#pragma unroll
                for (int t = 0; t < SMAX; ++t) {
                    const int row = wv + 4 * t, gi = i0 - w + row - a;
                    rpre[t] = row < Hr && scok && gi >= 0 && gi < n ? Rk[gi * m + sgj] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    s0[u] = soff0[u] >= 0 ? Sk[soff0[u]] : 0.f;
                    s1[u] = soff1[u] >= 0 ? Sk[soff1[u]] : 0.f;
                }
            };
            auto stash = [&](float *Rb) {
#pragma unroll
                for (int t = 0; t < SMAX; ++t) {
                    const int row = wv + 4 * t;
                    if (row < Hr && lane < Wrr) Rb[row * Wrr + lane] = rpre[t];
                }
            };
            fetch(0);
            stash(Rb0);
            __syncthreads();
            for (int k = 0; k < K; ++k) {
                const float *Rb = (k & 1) ? Rb1 : Rb0;
                double c0[NU], c1[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    c0[u] = s0[u];
                    c1[u] = s1[u];
                }
                if (k + 1 < K) fetch(k + 1);                         // in flight during the FMAs below
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    // candidate c = b0 + c of pixel rj + q reads column rj + q + s - b0 - c: NB + 1 neighbours in all
                    const float *r = Rb + urow[u] + (S - b0 - (NB - 1));
                    double rv[NB + 1];
#pragma unroll
                    for (int x = 0; x <= NB; ++x) rv[x] = r[x];
#pragma unroll
                    for (int c = 0; c < NB; ++c) {
                        acc0[u][c] = fma(c0[u], rv[NB - 1 - c], acc0[u][c]);
                        acc1[u][c] = fma(c1[u], rv[NB - c], acc1[u][c]);
                    }
                }
                if (k + 1 < K) stash((k & 1) ? Rb0 : Rb1);           // last read before the previous barrier
                __syncthreads();
            }

#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const int b = b0 + c;
                if (b > S) continue;                                 // the surplus candidate of the last chunk
                double v0[NU], v1[NU], B[UMPA_PX];
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    v0[u] = acc0[u][c];
                    v1[u] = acc1[u][c];
                }
                umpa_box<UMPA_TW>(v0, v1, uok, upos, P, H, w, Hr, Wr, tx, ty, B);
#pragma unroll
                for (int t = 0; t < UMPA_PX; ++t) {
                    const double Cv = Cb[(ty + RS * t - a + S) * W2 + (tx - b + S)];
                    double Lc = NaN, Tc = 0.0, Ac = 0.0;
                    if constexpr (DF) {
                        const double Gv = Gb[(ty + RS * t - a + S) * W2 + (tx - b + S)];
                        double Ls, As, Ts;
                        if (umpa_df_solve(E[t], B[t], Cv, F[t], Gv, mu.H, Ls, As, Ts)) {
                            Lc = Ls;
                            Ac = As;
                            Tc = Ts;
                        }
                    } else if (Cv != 0.0) {
                        Lc = E[t] - B[t] * B[t] / Cv;
                        Tc = B[t] / Cv;
                    }
                    if (ba[t] == a - 1 && bb[t] == b) Lap[t] = Lc;
                    if (ba[t] == a && bb[t] == b - 1) Lbp[t] = Lc;
                    if (Lc < bestL[t]) {                             // false for NaN: strict, first in scan order
                        bestL[t] = Lc;
                        bestT[t] = Tc;
                        if constexpr (DF) bestA[t] = Ac;
                        ba[t] = a;
                        bb[t] = b;
                        Lam[t] = prev[t][ch * NB + c];
                        Lbm[t] = last[t];
                        Lap[t] = Lbp[t] = NaN;
                    }
                    prev[t][ch * NB + c] = Lc;
                    last[t] = Lc;
                }
            }
        }
    }

    // ---- sub-pixel refinement and the outputs ----------------------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < UMPA_PX; ++t) {
        const int i = i0 + ty + RS * t, j = j0 + tx;
        if (i >= n || j >= m) continue;
        const int band = w + S;
        float ot = 1.f, ox = 0.f, oy = 0.f, ov = 1.f, orr = 0.f;
        const bool interior = i >= band && i < n - band && j >= band && j < m - band;
        if (interior && ba[t] != -100 && bestT[t] > 0.0) {
            double da = 0.0, db = 0.0;
            if (Lam[t] == Lam[t] && Lap[t] == Lap[t]) {              // both neighbours exist
                const double den = Lam[t] - 2.0 * bestL[t] + Lap[t];
                if (den > 0.0) da = fmin(fmax(0.5 * (Lam[t] - Lap[t]) / den, -0.5), 0.5);
            }
            if (Lbm[t] == Lbm[t] && Lbp[t] == Lbp[t]) {
                const double den = Lbm[t] - 2.0 * bestL[t] + Lbp[t];
                if (den > 0.0) db = fmin(fmax(0.5 * (Lbm[t] - Lbp[t]) / den, -0.5), 0.5);
            }
            ot = (float)bestT[t];
            ox = (float)((double)ba[t] + da);
            oy = (float)((double)bb[t] + db);
            orr = (float)(fmax(bestL[t], 0.0) / E[t]);
            if constexpr (DF) ov = (float)(bestA[t] / bestT[t]);
        }
        const int64_t o = (int64_t)i * m + j;
        trans[o] = ot;
        dx[o] = ox;
        dy[o] = oy;
        if constexpr (DF) mu.vis[o] = ov;
        resid[o] = orr;
    }
}

// The launch of k_umpa<UMPA_TW, s, DF>, s in [1, PSX_MAX_UMPA_SEARCH] (umpa_args has checked it).
template <int UMPA_TW, bool DF>
void umpa_launch(int s, dim3 grid, const UmpaLds &L, hipStream_t st, const SpecklePtrs &p, int K, int n, int m, int w, float *t,
                 float *dx, float *dy, float *res, const UmpaDf<DF> &mu) {
#define PSX_UMPA_GO(SV)                        \
    PSX_TIMED(DF ? "k_umpa_df" : "k_umpa", st, \
              k_umpa<UMPA_TW, SV, DF><<<grid, UMPA_NT, L.total, st>>>(p, K, n, m, w, L, t, dx, dy, res, mu))
    switch (s) {
        case 1: PSX_UMPA_GO(1); break;
        case 2: PSX_UMPA_GO(2); break;
        case 3: PSX_UMPA_GO(3); break;
        case 4: PSX_UMPA_GO(4); break;
        case 5: PSX_UMPA_GO(5); break;
        case 6: PSX_UMPA_GO(6); break;
        case 7: PSX_UMPA_GO(7); break;
        case 8:
            // k_umpa<32, 8, true> spills and must not be instantiated, not even in dead code; umpa_tw never sends s = 8 to it
            if constexpr (!DF || UMPA_TW == 16) PSX_UMPA_GO(8);
            break;
    }
#undef PSX_UMPA_GO
}

// The argument checks of psx_umpa_f32 and psx_umpa_df_f32 beyond pack_speckle's.
int umpa_args(const char *fn, int n, int m, int window, int search) {
    PSX_REQUIRE(window >= 1 && window <= PSX_MAX_UMPA_WINDOW, "%s: window=%d outside [1,%d]", fn, window, PSX_MAX_UMPA_WINDOW);
    PSX_REQUIRE(search >= 1 && search <= PSX_MAX_UMPA_SEARCH, "%s: search=%d outside [1,%d]", fn, search, PSX_MAX_UMPA_SEARCH);
    const int least = 2 * (window + search) + 1;
    PSX_REQUIRE(n >= least && m >= least, "%s: images %dx%d smaller than %dx%d = 2(window+search)+1", fn, n, m, least, least);
    PSX_REQUIRE((int64_t)n * m <= (int64_t)1 << 30, "%s: images %dx%d too large", fn, n, m);
    return 0;
}

// The host side of both entry points.  DF: mean and visibility are psx_umpa_df_f32's, null otherwise.
template <bool DF>
int umpa_run(const char *fn, const float *const *S, const float *const *R, const double *mean, int K, int n, int m, int window,
             int search, float *transmission, float *dx, float *dy, float *visibility, float *residual, void *stream) {
    SpecklePtrs p;
    if (int rc = pack_speckle(p, fn, 1, S, R, K)) return rc;
    if (int rc = umpa_args(fn, n, m, window, search)) return rc;
    PSX_REQUIRE(!DF || mean != nullptr, "%s: null mean array", fn);
    PSX_REQUIRE(transmission && dx && dy && (!DF || visibility) && residual, "%s: null output map", fn);
    UmpaDf<DF> mu;
    if constexpr (DF) {
        mu.vis = visibility;
        double sq = 0.0;
        for (int k = 0; k < PSX_MAX_LCS; ++k) mu.mu[k] = 0.0;
        for (int k = 0; k < K; ++k) {
            PSX_REQUIRE(std::isfinite(mean[k]), "%s: mean[%d] is not finite", fn, k);
            mu.mu[k] = mean[k];
            sq += mean[k] * mean[k];
        }
        const double side = 2 * window + 1;
        mu.H = side * side * sq;
    }
    const UmpaLds L = umpa_lds(window, search, DF);
    const int tw = umpa_tw(window, search, DF);
    const dim3 grid((unsigned)cdiv(m, tw), (unsigned)cdiv(n, UMPA_TH));
    hipStream_t st = (hipStream_t)stream;
    if (tw == 32)
        umpa_launch<32, DF>(search, grid, L, st, p, K, n, m, window, transmission, dx, dy, residual, mu);
    else
        umpa_launch<16, DF>(search, grid, L, st, p, K, n, m, window, transmission, dx, dy, residual, mu);
    return launch_check(DF ? "k_umpa_df" : "k_umpa");
}

}  // namespace

extern "C" int psx_umpa_f32(const float *const *S, const float *const *R, int K, int n, int m, int window, int search,
                            float *transmission, float *dx, float *dy, float *residual, void *stream) {
    return umpa_run<false>("psx_umpa_f32", S, R, nullptr, K, n, m, window, search, transmission, dx, dy, nullptr, residual, stream);
}

extern "C" int psx_umpa_df_f32(const float *const *S, const float *const *R, const double *mean, int K, int n, int m, int window,
                               int search, float *transmission, float *dx, float *dy, float *visibility, float *residual,
                               void *stream) {
    return umpa_run<true>("psx_umpa_df_f32", S, R, mean, K, n, m, window, search, transmission, dx, dy, visibility, residual, stream);
}
