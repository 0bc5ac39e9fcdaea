// phantom.hip -- the contrast phantom (Samples/generateContrastPhantom.py:50-106): 12 material tubes in a solid-water
// support, rasterised on a dimY x dimY slice and projected at one angle (skimage radon), one line per material.
// The slices are never stored (13 dimY^2 values: 936 MB as float64 at 3000 pixels): the projection evaluates the indicator at
// the four bilinear neighbours of each sample point.  The host (paresis_amd/Samples/generateContrastPhantom.py) derives every
// scalar by the reference's own expressions; the kernels do the per-pixel work.
#include "common.hpp"

using namespace psx;

namespace {

constexpr int NSLICE = PSX_PHANTOM_TUBES + 1;   // 12 tubes, then the support
constexpr int SUPPORT = PSX_PHANTOM_TUBES;

// Inside the half-open window of slice m and (i - ci)^2 + (j - cj)^2 < rad2, in float64 with every product and sum rounded
// on its own (generateContrastPhantom.py:57-59, 73-76): one boundary pixel that flips moves a whole column's sum by up to a pixel.
__device__ bool in_disc(const psx_phantom_desc &d, int m, int64_t i, int64_t j) {
#pragma clang fp contract(off)
    if (i < d.row0[m] || i >= d.row1[m] || j < d.col0[m] || j >= d.col1[m]) return false;
    const double di = (double)i - d.ci[m];
    const double dj = (double)j - d.cj[m];
    return di * di + dj * dj < d.rad2[m];
}

// Slice m at integer pixel (i, j): 0 outside the image (warp's mode='constant', cval=0); the support excludes every tube
// pixel (sliceTotMat == 0, generateContrastPhantom.py:73).
__device__ double slice_value(const psx_phantom_desc &d, int m, int64_t i, int64_t j) {
    if (i < 0 || i >= d.dimY || j < 0 || j >= d.dimY) return 0.0;
    if (!in_disc(d, m, i, j)) return 0.0;
    if (m == SUPPORT) {
        for (int t = 0; t < PSX_PHANTOM_TUBES; ++t)
            if (in_disc(d, t, i, j)) return 0.0;
    }
    return 1.0;
}

// One thread per (slice m, output column c): lines[m][c] = sum over rows r in order of the bilinear sample of slice m at
// column x = cos c + sin r + off_x, row y = -sin c + cos r + off_y -- skimage 0.18 radon: warp(..., order=1, mode='constant',
// clip=False) of the slice, then sum(0).  Only the rows whose sample points can reach slice m's window are visited.
__global__ __launch_bounds__(64) void k_phantom_lines(psx_phantom_desc d, double *__restrict__ lines) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = blockIdx.y;
    if (c >= d.dimY) return;
    const double ax = d.cos_a * (double)c, ay = -d.sin_a * (double)c;
    double rx0, rx1, ry0, ry1;
    row_span(ax + d.off_x, d.sin_a, d.col0[m] - 1.0, (double)d.col1[m], (double)d.dimY, rx0, rx1);
    row_span(ay + d.off_y, d.cos_a, d.row0[m] - 1.0, (double)d.row1[m], (double)d.dimY, ry0, ry1);
    const int r0 = (int)fmax(rx0, ry0), r1 = (int)fmin(rx1, ry1);    // both in [0, dimY] (row_span)
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) {
        const double x = ax + d.sin_a * (double)r + d.off_x;     // _transform_affine: H0 x + H1 y + H2
        const double y = ay + d.cos_a * (double)r + d.off_y;
        const double fr = floor(y), fc = floor(x);
        const int64_t minr = (int64_t)fr, minc = (int64_t)fc, maxr = (int64_t)ceil(y), maxc = (int64_t)ceil(x);
        const double dr = y - (double)minr, dc = x - (double)minc;
        const double tl = slice_value(d, m, minr, minc), tr = slice_value(d, m, minr, maxc);
        const double bl = slice_value(d, m, maxr, minc), br = slice_value(d, m, maxr, maxc);
        const double top = (1.0 - dc) * tl + dc * tr;
        const double bottom = (1.0 - dc) * bl + dc * br;
        acc += (1.0 - dr) * top + dr * bottom;
    }
    lines[(int64_t)m * d.dimY + c] = acc;
}

// geom[m][row][c] = (float)(lines[m][c] * pix_mm * 1e-3) on slice m's output rows, 0 elsewhere (generateContrastPhantom.py:98-104)
__global__ __launch_bounds__(256) void k_phantom_maps(psx_phantom_desc d, const double *__restrict__ lines,
                                                      float *__restrict__ geom) {
#pragma clang fp contract(off)
    const int64_t plane = (int64_t)d.dimX * d.dimY, n = NSLICE * plane;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const int m = (int)(p / plane);
        const int64_t q = p - (int64_t)m * plane;
        const int row = (int)(q / d.dimY), c = (int)(q - (int64_t)row * d.dimY);
        const bool on = m == SUPPORT ? (row >= d.support_row0 && row < d.support_row1)
                                     : (row >= d.tube_row0 && row < d.tube_row1);
        geom[p] = on ? (float)(lines[(int64_t)m * d.dimY + c] * d.pix_mm * 1e-3) : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_phantom_slices(psx_phantom_desc d, uint8_t *__restrict__ out) {
    const int64_t plane = (int64_t)d.dimY * d.dimY, n = NSLICE * plane;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const int m = (int)(p / plane);
        const int64_t q = p - (int64_t)m * plane;
        out[p] = slice_value(d, m, q / d.dimY, q % d.dimY) != 0.0 ? 1 : 0;
    }
}

int check_desc(const psx_phantom_desc *d) {
    PSX_REQUIRE(d != nullptr, "null phantom descriptor");
    PSX_REQUIRE(d->dimX >= 1 && d->dimY >= 1 && d->dimY <= (1 << 20), "phantom grid %d x %d", d->dimX, d->dimY);
    PSX_REQUIRE((int64_t)d->dimX * d->dimY <= ((int64_t)1 << 40) / NSLICE, "phantom grid %d x %d too large", d->dimX, d->dimY);
    for (int m = 0; m < NSLICE; ++m)
        PSX_REQUIRE(d->row0[m] >= 0 && d->row1[m] <= d->dimY && d->col0[m] >= 0 && d->col1[m] <= d->dimY,
                    "window of slice %d [%d,%d) x [%d,%d) outside the %d-pixel slice", m, d->row0[m], d->row1[m], d->col0[m],
                    d->col1[m], d->dimY);
    PSX_REQUIRE(d->tube_row0 >= 0 && d->tube_row1 <= d->dimX && d->support_row0 >= 0 && d->support_row1 <= d->dimX,
                "output rows outside [0,%d)", d->dimX);
    return 0;
}

}  // namespace

extern "C" int psx_contrast_phantom_f32(const psx_phantom_desc *desc, double *lines, float *geom, void *stream) {
    if (int rc = check_desc(desc)) return rc;
    PSX_REQUIRE(lines != nullptr && geom != nullptr, "null lines or geometry buffer");
    hipStream_t st = (hipStream_t)stream;
    const psx_phantom_desc d = *desc;
    PSX_TIMED("k_phantom_lines", st,
              k_phantom_lines<<<dim3((unsigned)cdiv(d.dimY, 64), NSLICE), 64, 0, st>>>(d, lines));
    if (int rc = launch_check("k_phantom_lines")) return rc;
    const int64_t n = NSLICE * (int64_t)d.dimX * d.dimY;
    PSX_TIMED("k_phantom_maps", st, k_phantom_maps<<<ew_grid(n, 256), 256, 0, st>>>(d, lines, geom));
    return launch_check("k_phantom_maps");
}

extern "C" int psx_contrast_phantom_slices_u8(const psx_phantom_desc *desc, uint8_t *slices, void *stream) {
    if (int rc = check_desc(desc)) return rc;
    PSX_REQUIRE(slices != nullptr, "null slice buffer");
    PSX_REQUIRE(desc->dimY <= 4096, "slices are a debug output: dimY %d > 4096", desc->dimY);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = NSLICE * (int64_t)desc->dimY * desc->dimY;
    PSX_TIMED("k_phantom_slices", st, k_phantom_slices<<<ew_grid(n, 256), 256, 0, st>>>(*desc, slices));
    return launch_check("k_phantom_slices");
}
