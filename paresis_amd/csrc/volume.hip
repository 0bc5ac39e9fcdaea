// volume.hip -- a stored volume of material labels projected at one angle: the contrast phantom's model (phantom.hip,
// skimage radon of a slice: bilinear samples along the rotated rays, summed in row order) fed from memory instead of from 13
// analytic discs.  The contract is in include/paresis_hip.h ("labelled voxel volume").  k_volume_project walks parallel rays,
// k_volume_project_cone the rays that diverge from a point source ("the same volume under a point source").
#include "common.hpp"

using namespace psx;

namespace {

constexpr int BLOCK = 64;     // one wave: a thread per study column, its PSX_VOLUME_MAX_MAT sums in LDS
constexpr int CHUNK = 32;     // steps of the rays between two stagings of the labels
constexpr int STAGE = 8;      // rows of the staged box loaded together
constexpr int TILE = 8192;    // bytes of labels staged per chunk: the bounding box of 64 columns x 32 steps up to s ~ 1.4

// The slice of study row x: n / 2 + floor((x - dimX / 2) s + 0.5), or -1 outside [0, n).  Non-decreasing in x.
__device__ __forceinline__ int slice_of(const psx_volume_desc &d, int x) {
#pragma clang fp contract(off)
    const double z = (double)(d.n / 2) + floor((double)(x - d.dimX / 2) * d.s + 0.5);   // |.| <= 2^30 + 2^15: exact
    return (z < 0.0 || z >= (double)d.n) ? -1 : (int)z;
}

__device__ __forceinline__ int wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

// One block (one wave) per (study row x, tile of 64 study columns); one thread per column y.  Several rows share a slice
// when s < 1: only the first row of a run of equal z works -- it forms the line of every material in one walk over the
// slice's labels and writes it to every row of the run; the others leave at once.  A row outside the volume writes its own
// zeros.
//
// The label is a run-time index, so the per-thread sums live in LDS as acc[k][thread] (a thread only ever touches its own
// column).  A step reads four labels and adds to the at most four materials among them; a material that is absent from the
// four corners would add (1 - dr)*(+0) + dr*(+0) = +0.0 to a sum that is never negative: skipping it changes no bit.  Each
// thread walks r in ascending order, which is the contract's order of summation.
//
// The 64 sample points of a step lie on a line across the slice, a voxel or so apart: read from global memory they touch
// some 40 cache lines per load at 30 degrees (measured: 13.5 ms for 512 slices of 2048^2 on a 2048-column grid, 7.3 ms
// staged).  So the wave walks CHUNK steps at a time and first copies the bounding box of their
// sample points into LDS, consecutive lanes on consecutive bytes, STAGE rows' loads in flight together.  A point outside the staged box (a box too large for TILE: s above ~1.4; or, never observed, a
// rounding that the box's margin of one voxel does not cover) is read from global memory: the box decides speed only.
__global__ __launch_bounds__(BLOCK) void k_volume_project(psx_volume_desc d, const uint8_t *__restrict__ labels,
                                                          double *__restrict__ lines, float *__restrict__ geom) {
#pragma clang fp contract(off)
    extern __shared__ double acc[];                     // [nmat][BLOCK]
    __shared__ uint8_t tile[TILE];
    const int x = blockIdx.x, tid = threadIdx.x;
    const int y0 = blockIdx.y * BLOCK, y = y0 + tid;
    const int z = slice_of(d, x);
    if (z >= 0 && x > 0 && slice_of(d, x - 1) == z) return;          // a follower of its run (the whole block)
    const bool live = y < d.dimY;
    const int64_t plane = (int64_t)d.dimX * d.dimY;
    if (z < 0) {
        for (int k = 0; live && k < d.nmat; ++k) {
            const int64_t o = k * plane + (int64_t)x * d.dimY + y;
            geom[o] = 0.f;
            if (lines) lines[o] = 0.0;
        }
        return;
    }
    for (int k = 0; k < d.nmat; ++k) acc[k * BLOCK + tid] = 0.0;

    const int m = d.m;
    int row0 = 0, row1 = m, col0 = 0, col1 = m;
    if (d.box) {
        const int32_t *b = d.box + 4 * (int64_t)z;
        row0 = b[0], row1 = b[1], col0 = b[2], col1 = b[3];
    }
    int r0 = 0, r1 = 0;
    const double cpos = (double)(y - d.dimY / 2) * d.s + (double)(m / 2);
    const double ax = d.cos_a * cpos, ay = -d.sin_a * cpos;
    if (live && row1 > row0 && col1 > col0) {
        double rx0, rx1, ry0, ry1;
        row_span(ax + d.off_x, d.sin_a, col0 - 1.0, (double)col1, (double)m, rx0, rx1);
        row_span(ay + d.off_y, d.cos_a, row0 - 1.0, (double)row1, (double)m, ry0, ry1);
        r0 = (int)fmax(rx0, ry0), r1 = (int)fmin(rx1, ry1);           // both in [0, m] (row_span)
    }
    const int w0 = wave_min(r1 > r0 ? r0 : m), w1 = -wave_min(r1 > r0 ? -r1 : 0);      // the wave's steps: [w0, w1)
    const uint8_t *__restrict__ sl = labels + (int64_t)z * m * m;
    // the columns at the two ends of the wave: the sample points of a chunk lie in the quadrilateral they span
    const double cposA = (double)(y0 - d.dimY / 2) * d.s + (double)(m / 2);
    const double cposB = (double)(y0 + BLOCK - 1 - d.dimY / 2) * d.s + (double)(m / 2);

    for (int rb = w0; rb < w1; rb += CHUNK) {
        // ---- stage rows [tr0, tr0 + H) x columns [tc0, tc0 + W) of the slice: the chunk's sample points, a voxel of margin
        const int re = min(rb + CHUNK, w1) - 1;
        double Xlo = INFINITY, Xhi = -INFINITY, Ylo = INFINITY, Yhi = -INFINITY;
        for (int c = 0; c < 4; ++c) {
            const double cp = (c & 1) ? cposB : cposA, rr = (double)((c & 2) ? re : rb);
            const double X = d.cos_a * cp + d.sin_a * rr + d.off_x, Y = -d.sin_a * cp + d.cos_a * rr + d.off_y;
            Xlo = fmin(Xlo, X), Xhi = fmax(Xhi, X), Ylo = fmin(Ylo, Y), Yhi = fmax(Yhi, Y);
        }
        const int tc0 = max((int)floor(Xlo) - 1, 0), tc1 = min((int)ceil(Xhi) + 1, m - 1);
        const int tr0 = max((int)floor(Ylo) - 1, 0), tr1 = min((int)ceil(Yhi) + 1, m - 1);
        int W = tc1 - tc0 + 1, H = tr1 - tr0 + 1;
        if (W <= 0 || H <= 0 || (int64_t)W * H > TILE) W = H = 0;
        __syncthreads();                                              // the previous chunk's reads are done
        // STAGE rows at a time, their loads issued together (a row past the last repeats it: no branch between the loads)
        const uint8_t *__restrict__ src = sl + tr0 * m + tc0;
        for (int i0 = 0; i0 < H; i0 += STAGE) {
            for (int j = tid; j < W; j += BLOCK) {
                uint8_t v[STAGE];
#pragma unroll
                for (int u = 0; u < STAGE; ++u) v[u] = src[min(i0 + u, H - 1) * m + j];
#pragma unroll
                for (int u = 0; u < STAGE; ++u) tile[min(i0 + u, H - 1) * W + j] = v[u];
            }
        }
        __syncthreads();

        auto label_at = [&](int i, int j) -> int {                    // 0 outside the slice (warp's mode='constant', cval=0)
            const int ti = i - tr0, tj = j - tc0;                    // the staged box lies inside the slice
            if ((unsigned)ti < (unsigned)H && (unsigned)tj < (unsigned)W) return tile[ti * W + tj];
            if ((unsigned)i >= (unsigned)m || (unsigned)j >= (unsigned)m) return 0;
            return sl[i * m + j];
        };
        const int ra = max(rb, r0), rz = min(re + 1, r1);
        double rd = (double)ra;                                       // r as a double: integers, so rd + 1.0 is exact
        for (int r = ra; r < rz; ++r, rd += 1.0) {
            const double X = ax + d.sin_a * rd + d.off_x;
            const double Y = ay + d.cos_a * rd + d.off_y;
            // |X|, |Y| < 2^28 (|cpos| <= 2^26 + 2^13, m <= 2^13): the floors fit an int; Y - (double)minr is Y - floor(Y), and
            // ceil(Y) is floor(Y) + (Y > floor(Y)).  (Conversions between doubles and 64-bit integers are long instruction
            // sequences on gfx950, and floor, ceil and the conversions run at a quarter of the rate of an addition.)
            const double fY = floor(Y), fX = floor(X);
            const int minr = (int)fY, minc = (int)fX, maxr = minr + (Y > fY ? 1 : 0), maxc = minc + (X > fX ? 1 : 0);
            const int l0 = label_at(minr, minc), l1 = label_at(minr, maxc);
            const int l2 = label_at(maxr, minc), l3 = label_at(maxr, maxc);
            if ((l0 | l1 | l2 | l3) == 0) continue;
            const double dr = Y - fY, dc = X - fX;
            const double wr = 1.0 - dr, wc = 1.0 - dc;
            // the term of material L - 1, with its indicator at each corner: k_phantom_lines' expression
            auto add = [&](int L) {
                if (L == 0 || L > d.nmat) return;
                const double tl = l0 == L ? 1.0 : 0.0, tr = l1 == L ? 1.0 : 0.0, bl = l2 == L ? 1.0 : 0.0, br = l3 == L ? 1.0 : 0.0;
                const double top = wc * tl + dc * tr;
                const double bottom = wc * bl + dc * br;
                acc[(L - 1) * BLOCK + tid] += wr * top + dr * bottom;
            };
            add(l0);
            if (l1 != l0) add(l1);
            if (l2 != l0 && l2 != l1) add(l2);
            if (l3 != l0 && l3 != l1 && l3 != l2) add(l3);
        }
    }
    if (!live) return;
    for (int k = 0; k < d.nmat; ++k) {
        const double a = acc[k * BLOCK + tid];
        const float g = (float)(a * d.voxel_m);
        for (int xx = x; xx < d.dimX && slice_of(d, xx) == z; ++xx) {
            const int64_t o = k * plane + (int64_t)xx * d.dimY + y;
            geom[o] = g;
            if (lines) lines[o] = a;
        }
    }
}

// The divergent projection of the same volume (psx_volume_project_cone_u8): the source at depth -dso on the optical axis, the
// study grid on the plane through the rotation axis.  One block (one wave) per (study row x, 64 study columns), a thread
// per column y, the per-material sums in LDS as above.  A ray crosses slices and every row has its own rays, so nothing of
// k_volume_project's sharing carries over: no run of rows on one slice, no staged box -- the labels are read from global
// memory.  The step's magnification g and its slice z depend on (x, r) alone: they are the same for the whole wave, and so
// is the branch on the slice's occupied box, which spares only steps whose four labels are empty (exact zeros).
__global__ __launch_bounds__(BLOCK) void k_volume_project_cone(psx_volume_desc d, double dso, const uint8_t *__restrict__ labels,
                                                               double *__restrict__ lines, float *__restrict__ geom) {
#pragma clang fp contract(off)
    extern __shared__ double acc[];                     // [nmat][BLOCK]
    const int x = blockIdx.x, tid = threadIdx.x;
    const int y = blockIdx.y * BLOCK + tid;
    if (y >= d.dimY) return;                            // no barrier below: a thread only touches its own column of acc
    for (int k = 0; k < d.nmat; ++k) acc[k * BLOCK + tid] = 0.0;

    const int m = d.m, c0 = m / 2;
    const double dc0 = (double)c0;
    const double t0 = (double)(y - d.dimY / 2) * d.s, z0 = (double)(x - d.dimX / 2) * d.s;
    for (int r = 0; r < m; ++r) {
        const double rd = (double)r;
        const double g = (dso + (double)(r - c0)) / dso;               // in (0, 2]: dso >= m
        const double zd = (double)(d.n / 2) + floor(z0 * g + 0.5);     // |.| <= 2^31 + 2^15: compared as a double
        if (zd < 0.0 || zd >= (double)d.n) continue;
        const int z = (int)zd;
        int row0 = 0, row1 = m, col0 = 0, col1 = m;
        if (d.box) {
            const int32_t *b = d.box + 4 * (int64_t)z;
            row0 = b[0], row1 = b[1], col0 = b[2], col1 = b[3];
            if (row1 <= row0) continue;
        }
        const uint8_t *__restrict__ sl = labels + (int64_t)z * m * m;
        const double cpos = t0 * g + dc0;
        const double X = d.cos_a * cpos + d.sin_a * rd + d.off_x;
        const double Y = (-d.sin_a * cpos) + d.cos_a * rd + d.off_y;
        // |X|, |Y| < 2^29 (|cpos| <= 2^27 + 2^13, m <= 2^13): the floors fit an int
        const double fY = floor(Y), fX = floor(X);
        const int minr = (int)fY, minc = (int)fX, maxr = minr + (Y > fY ? 1 : 0), maxc = minc + (X > fX ? 1 : 0);
        if (maxr < row0 || minr >= row1 || maxc < col0 || minc >= col1) continue;
        auto label_at = [&](int i, int j) -> int {                    // 0 outside the slice
            if ((unsigned)i >= (unsigned)m || (unsigned)j >= (unsigned)m) return 0;
            return sl[i * m + j];
        };
        const int l0 = label_at(minr, minc), l1 = label_at(minr, maxc);
        const int l2 = label_at(maxr, minc), l3 = label_at(maxr, maxc);
        if ((l0 | l1 | l2 | l3) == 0) continue;
        const double dr = Y - fY, dc = X - fX;
        const double wr = 1.0 - dr, wc = 1.0 - dc;
        auto add = [&](int L) {                                       // k_volume_project's term
            if (L == 0 || L > d.nmat) return;
            const double tl = l0 == L ? 1.0 : 0.0, tr = l1 == L ? 1.0 : 0.0, bl = l2 == L ? 1.0 : 0.0, br = l3 == L ? 1.0 : 0.0;
            const double top = wc * tl + dc * tr;
            const double bottom = wc * bl + dc * br;
            acc[(L - 1) * BLOCK + tid] += wr * top + dr * bottom;
        };
        add(l0);
        if (l1 != l0) add(l1);
        if (l2 != l0 && l2 != l1) add(l2);
        if (l3 != l0 && l3 != l1 && l3 != l2) add(l3);
    }
    const double L = sqrt(1.0 + (t0 * t0 + z0 * z0) / (dso * dso));   // the path of a unit step in depth
    const int64_t plane = (int64_t)d.dimX * d.dimY;
    for (int k = 0; k < d.nmat; ++k) {
        const double a = acc[k * BLOCK + tid] * L;
        const int64_t o = k * plane + (int64_t)x * d.dimY + y;
        geom[o] = (float)(a * d.voxel_m);
        if (lines) lines[o] = a;
    }
}

// What both entry points ask of (descriptor, labels, geometry buffer); fn is the entry point's name in the messages.
int volume_check(const char *fn, const psx_volume_desc *desc, const uint8_t *labels, const float *geom) {
    PSX_REQUIRE(desc != nullptr, "%s: null descriptor", fn);
    PSX_REQUIRE(labels != nullptr && geom != nullptr, "%s: null labels or geometry buffer", fn);
    const psx_volume_desc d = *desc;
    PSX_REQUIRE(d.nmat >= 1 && d.nmat <= PSX_VOLUME_MAX_MAT, "%s: nmat=%d outside [1,%d]", fn, d.nmat, PSX_VOLUME_MAX_MAT);
    PSX_REQUIRE(d.m >= 1 && d.m <= 8192, "%s: m=%d outside [1,8192]", fn, d.m);
    PSX_REQUIRE(d.n >= 1 && d.n <= 65535, "%s: n=%d outside [1,65535]", fn, d.n);
    PSX_REQUIRE(d.dimY >= 1 && d.dimY <= (1 << 20) && d.dimX >= 1 && d.dimX <= (1 << 24), "%s: study grid %d x %d", fn, d.dimX,
                d.dimY);
    PSX_REQUIRE((int64_t)d.nmat * d.dimX * d.dimY <= ((int64_t)1 << 40), "%s: %d maps of %d x %d too large", fn, d.nmat, d.dimX,
                d.dimY);
    PSX_REQUIRE(std::isfinite(d.s) && d.s >= 1.0 / 64 && d.s <= 64.0, "%s: s=%g outside [1/64,64]", fn, d.s);
    PSX_REQUIRE(std::isfinite(d.voxel_m), "%s: voxel_m=%g", fn, d.voxel_m);
    PSX_REQUIRE(std::isfinite(d.cos_a) && std::isfinite(d.sin_a) && std::isfinite(d.off_x) && std::isfinite(d.off_y),
                "%s: non-finite angle scalars", fn);
    return 0;
}

}  // namespace

extern "C" int psx_volume_project_u8(const psx_volume_desc *desc, const uint8_t *labels, double *lines, float *geom,
                                     void *stream) {
    if (int rc = volume_check("psx_volume_project_u8", desc, labels, geom)) return rc;
    const psx_volume_desc d = *desc;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d.dimX, (unsigned)cdiv(d.dimY, BLOCK));
    PSX_TIMED("k_volume_project", st,
              k_volume_project<<<grid, BLOCK, sizeof(double) * BLOCK * d.nmat, st>>>(d, labels, lines, geom));
    return launch_check("k_volume_project");
}

extern "C" int psx_volume_project_cone_u8(const psx_volume_desc *desc, double dso, const uint8_t *labels, double *lines,
                                          float *geom, void *stream) {
    if (int rc = volume_check("psx_volume_project_cone_u8", desc, labels, geom)) return rc;
    const psx_volume_desc d = *desc;
    PSX_REQUIRE(dso >= (double)d.m && dso <= 1e30, "psx_volume_project_cone_u8: dso=%g outside [m=%d, 1e30] voxels", dso, d.m);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d.dimX, (unsigned)cdiv(d.dimY, BLOCK));
    PSX_TIMED("k_volume_project_cone", st,
              k_volume_project_cone<<<grid, BLOCK, sizeof(double) * BLOCK * d.nmat, st>>>(d, dso, labels, lines, geom));
    return launch_check("k_volume_project_cone");
}
