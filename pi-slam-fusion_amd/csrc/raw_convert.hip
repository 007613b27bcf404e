// raw_convert.hip -- gfx950 kernels of the raw-frame front end (raw_convert.hpp): NV12 / NV21 / I420, grey and Bayer to packed BGR8.
//
// Memory-bound element-wise work: a thread owns kRun = 8 consecutive pixels of one row (YUV: of two adjacent rows, so that every chroma
// sample is read once for its 2 x 2 block), loads them with 8-byte loads and stores the 24 bytes of a row as three 8-byte or six 4-byte
// stores.  A wave is 512 consecutive pixels of a row.  Whatever does not fit that shape -- the last partial run of a row, a pointer or a
// pitch that is not aligned, the border columns of a Bayer frame -- goes byte by byte, and never past the end of a row.  Integer
// arithmetic only (raw_convert.hpp), no LDS: the three source rows of a Bayer run are shared between neighbouring rows through L2.
#include "raw_convert.hpp"

namespace pf {

namespace {

constexpr int kRun = 8;                  // pixels of one row a thread owns
constexpr int kBX = 64, kBY = 4;         // a block: 4 waves, one row (YUV: one row pair) each

// the block's place in the frame from a 1-D grid (the y extent of a grid is too small for a frame of many short rows)
__device__ __forceinline__ void run_origin(unsigned nbx, int& x0, int& row)
{
    const unsigned by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    x0 = (int)(bx * kBX + threadIdx.x) * kRun;
    row = (int)(by * kBY + threadIdx.y);
}

struct Run { uint32_t w[6]; };           // 8 BGR pixels as they lie in memory

__device__ __forceinline__ void put(Run& r, int k, uint8_t v) { r.w[k >> 2] |= (uint32_t)v << (8 * (k & 3)); }      // k: a constant after unrolling

// n <= 8 pixels of r to out
__device__ __forceinline__ void store_run(uint8_t* out, const Run& r, int n)
{
    if (n == kRun && ((uintptr_t)out & 7) == 0) {
        uint2* o = (uint2*)out;
        o[0] = make_uint2(r.w[0], r.w[1]); o[1] = make_uint2(r.w[2], r.w[3]); o[2] = make_uint2(r.w[4], r.w[5]);
    } else if (n == kRun && ((uintptr_t)out & 3) == 0) {
        uint32_t* o = (uint32_t*)out;
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = r.w[k];
    } else {
#pragma unroll
        for (int k = 0; k < 3 * kRun; k++)
            if (k < 3 * n) out[k] = (uint8_t)(r.w[k >> 2] >> (8 * (k & 3)));
    }
}

// n <= 8 bytes at p, one 8-byte load where the run is whole and aligned; bytes past n are 0
__device__ __forceinline__ void load_run(const uint8_t* p, int n, uint8_t v[kRun])
{
    if (n == kRun && ((uintptr_t)p & 7) == 0) {
        const uint2 q = *(const uint2*)p;
#pragma unroll
        for (int i = 0; i < 4; i++) { v[i] = (uint8_t)(q.x >> (8 * i)); v[4 + i] = (uint8_t)(q.y >> (8 * i)); }
    } else {
#pragma unroll
        for (int i = 0; i < kRun; i++) v[i] = i < n ? p[i] : 0;
    }
}
// n <= 4 bytes at p, one 4-byte load where whole and aligned
__device__ __forceinline__ void load_half(const uint8_t* p, int n, uint8_t v[4])
{
    if (n == 4 && ((uintptr_t)p & 3) == 0) {
        const uint32_t q = *(const uint32_t*)p;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (uint8_t)(q >> (8 * i));
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = i < n ? p[i] : 0;
    }
}

// FORMAT: PF_RAW_NV12, _NV21 (pu: the interleaved plane, pv unused) or _I420.  rows, cols even
template <int FORMAT>
__global__ __launch_bounds__(kBX * kBY) void k_yuv420(const uint8_t* __restrict__ py, size_t sy, const uint8_t* __restrict__ pu, size_t su,
                                                      const uint8_t* __restrict__ pv, size_t sv, int rows, int cols, unsigned nbx,
                                                      uint8_t* __restrict__ dst, size_t dst_step)
{
    int x0, pair;
    run_origin(nbx, x0, pair);
    const int y = 2 * pair;
    if (y >= rows || x0 >= cols) return;
    const int n = min(kRun, cols - x0);          // even
    uint8_t Y0[kRun], Y1[kRun], U[4], V[4];
    load_run(py + (size_t)y * sy + x0, n, Y0);
    load_run(py + (size_t)(y + 1) * sy + x0, n, Y1);
    if (FORMAT == PF_RAW_I420) {
        load_half(pu + (size_t)pair * su + x0 / 2, n / 2, U);
        load_half(pv + (size_t)pair * sv + x0 / 2, n / 2, V);
    } else {
        uint8_t uv[kRun];
        load_run(pu + (size_t)pair * su + x0, n, uv);
#pragma unroll
        for (int i = 0; i < 4; i++) { U[i] = uv[2 * i + (FORMAT == PF_RAW_NV21 ? 1 : 0)]; V[i] = uv[2 * i + (FORMAT == PF_RAW_NV21 ? 0 : 1)]; }
    }
    Run r0{}, r1{};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const raw::Chroma c = raw::yuv_chroma(U[i], V[i]);
#pragma unroll
        for (int j = 0; j < 2; j++) {
            uint8_t b, g, r;
            raw::yuv_pixel(Y0[2 * i + j], c, b, g, r);
            put(r0, 6 * i + 3 * j, b); put(r0, 6 * i + 3 * j + 1, g); put(r0, 6 * i + 3 * j + 2, r);
            raw::yuv_pixel(Y1[2 * i + j], c, b, g, r);
            put(r1, 6 * i + 3 * j, b); put(r1, 6 * i + 3 * j + 1, g); put(r1, 6 * i + 3 * j + 2, r);
        }
    }
    store_run(dst + (size_t)y * dst_step + (size_t)x0 * 3, r0, n);
    store_run(dst + (size_t)(y + 1) * dst_step + (size_t)x0 * 3, r1, n);
}

__global__ __launch_bounds__(kBX * kBY) void k_grey(const uint8_t* __restrict__ src, size_t step, int rows, int cols, unsigned nbx,
                                                    uint8_t* __restrict__ dst, size_t dst_step)
{
    int x0, y;
    run_origin(nbx, x0, y);
    if (y >= rows || x0 >= cols) return;
    const int n = min(kRun, cols - x0);
    uint8_t v[kRun];
    load_run(src + (size_t)y * step + x0, n, v);
    Run r{};
#pragma unroll
    for (int i = 0; i < kRun; i++) { put(r, 3 * i, v[i]); put(r, 3 * i + 1, v[i]); put(r, 3 * i + 2, v[i]); }
    store_run(dst + (size_t)y * dst_step + (size_t)x0 * 3, r, n);
}

// rows, cols >= 3.  A run whose pixels are all interior columns (1 <= x <= cols - 2) and whose source rows are 8-byte aligned at x0 reads
// 10 bytes of each of the three rows around it: the aligned 8 and the byte on either side.  The row clamp moves the three rows, never a
// load: cy - 1 .. cy + 1 lie inside the image.  Every other run asks raw::bayer_pixel, which clamps the coordinates.
template <int FORMAT>
__global__ __launch_bounds__(kBX * kBY) void k_bayer(const uint8_t* __restrict__ src, size_t step, int rows, int cols, unsigned nbx,
                                                     uint8_t* __restrict__ dst, size_t dst_step)
{
    int x0, y;
    run_origin(nbx, x0, y);
    if (y >= rows || x0 >= cols) return;
    const int n = min(kRun, cols - x0);
    uint8_t* out = dst + (size_t)y * dst_step + (size_t)x0 * 3;
    const int cy = raw::clampi(y, 1, rows - 2);
    const uint8_t* r1 = src + (size_t)cy * step + x0;
    Run r{};
    if (x0 >= 1 && x0 + kRun <= cols - 1 && (((uintptr_t)r1 | (uintptr_t)step) & 7) == 0) {
        uint8_t a[3][kRun + 2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint8_t* p = k == 0 ? r1 - step : k == 1 ? r1 : r1 + step;
            const uint2 q = *(const uint2*)p;
            a[k][0] = p[-1]; a[k][kRun + 1] = p[kRun];
#pragma unroll
            for (int i = 0; i < 4; i++) { a[k][1 + i] = (uint8_t)(q.x >> (8 * i)); a[k][5 + i] = (uint8_t)(q.y >> (8 * i)); }
        }
        // x0 is even: the sites of the run alternate between those of columns 0 and 1 of row cy
        const int s0 = raw::bayer_site(FORMAT, cy, 0), s1 = raw::bayer_site(FORMAT, cy, 1);
#pragma unroll
        for (int i = 0; i < kRun; i++) {
            uint8_t px[3];
            raw::bayer_window((i & 1) ? s1 : s0, (i & 1) ? s0 : s1, a[0][i], a[0][i + 1], a[0][i + 2], a[1][i], a[1][i + 1], a[1][i + 2],
                              a[2][i], a[2][i + 1], a[2][i + 2], px);
            put(r, 3 * i, px[0]); put(r, 3 * i + 1, px[1]); put(r, 3 * i + 2, px[2]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < kRun; i++) {
            if (i < n) {
                uint8_t px[3];
                raw::bayer_pixel(FORMAT, src, step, rows, cols, y, x0 + i, px);
                put(r, 3 * i, px[0]); put(r, 3 * i + 1, px[1]); put(r, 3 * i + 2, px[2]);
            }
        }
    }
    store_run(out, r, n);
}

}  // namespace

void launch_raw_convert(hipStream_t s, const pf_raw_frame& f, uint8_t* dst, size_t dst_step)
{
    const int units = raw::is_yuv(f.format) ? f.rows / 2 : f.rows;          // rows, or row pairs
    const unsigned nbx = (unsigned)((f.cols + kBX * kRun - 1) / (kBX * kRun)), nby = (unsigned)((units + kBY - 1) / kBY);
    if (!nbx || !nby) return;
    const dim3 block(kBX, kBY), grid(nbx * nby);          // below 2^31: a plane has fewer bytes than that
    const uint8_t* p0 = (const uint8_t*)f.plane[0];
    const uint8_t* p1 = (const uint8_t*)f.plane[1];
    const uint8_t* p2 = (const uint8_t*)f.plane[2];
    const size_t s0 = raw::plane_step(f, 0);
    switch (f.format) {
    case PF_RAW_GREY: k_grey<<<grid, block, 0, s>>>(p0, s0, f.rows, f.cols, nbx, dst, dst_step); break;
    case PF_RAW_NV12: k_yuv420<PF_RAW_NV12><<<grid, block, 0, s>>>(p0, s0, p1, raw::plane_step(f, 1), nullptr, 0, f.rows, f.cols, nbx, dst, dst_step); break;
    case PF_RAW_NV21: k_yuv420<PF_RAW_NV21><<<grid, block, 0, s>>>(p0, s0, p1, raw::plane_step(f, 1), nullptr, 0, f.rows, f.cols, nbx, dst, dst_step); break;
    case PF_RAW_I420: k_yuv420<PF_RAW_I420><<<grid, block, 0, s>>>(p0, s0, p1, raw::plane_step(f, 1), p2, raw::plane_step(f, 2), f.rows, f.cols, nbx, dst, dst_step); break;
    case PF_RAW_BAYER_RGGB: k_bayer<PF_RAW_BAYER_RGGB><<<grid, block, 0, s>>>(p0, s0, f.rows, f.cols, nbx, dst, dst_step); break;
    case PF_RAW_BAYER_BGGR: k_bayer<PF_RAW_BAYER_BGGR><<<grid, block, 0, s>>>(p0, s0, f.rows, f.cols, nbx, dst, dst_step); break;
    case PF_RAW_BAYER_GRBG: k_bayer<PF_RAW_BAYER_GRBG><<<grid, block, 0, s>>>(p0, s0, f.rows, f.cols, nbx, dst, dst_step); break;
    case PF_RAW_BAYER_GBRG: k_bayer<PF_RAW_BAYER_GBRG><<<grid, block, 0, s>>>(p0, s0, f.rows, f.cols, nbx, dst, dst_step); break;
    default: break;
    }
}

}  // namespace pf
