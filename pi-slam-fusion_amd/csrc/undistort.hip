// undistort.hip -- gfx950 kernel of keyframe undistortion (undistort.hpp): an output-centred gather through the remap table.
//
// A thread owns kUndistortRun = 4 consecutive output pixels of one row: their table entries are two aligned 16-byte loads and their twelve
// BGR bytes three dword stores (byte stores where the row does not start on a dword, and in the tail of a row whose width is not a multiple
// of the run).  A wave is 256 consecutive pixels of one output row, so its taps lie on a few neighbouring source rows and the byte gathers of
// neighbouring lanes share cache lines.  Per output pixel: 8 bytes of table, 3 bytes out, and at least 3 bytes of source.
// Compiled with -ffp-contract=off like the rest of the library: the sums below are rounded product by product, in the order written.
#include "undistort.hpp"

namespace pf {

namespace {

constexpr int kUX = 64, kUY = 4;        // a block: 4 waves, one output row each

template <int CN>
__device__ __forceinline__ void undistort_pixel(const uint8_t* __restrict__ src, size_t src_step, int w_in, int h_in, float X, float Y, uint8_t bgr[3])
{
    if (X < 0.f) { bgr[0] = bgr[1] = bgr[2] = 0; return; }
    const int xi = (int)X, yi = (int)Y;
    const float xx = X - (float)xi, yy = Y - (float)yi;
    const float xy = xx * yy;
    const float c0 = ((1.f - xx) - yy) + xy, c1 = xx - xy, c2 = yy - xy, c3 = xy;
    const int x0 = min(max(xi, 0), w_in - 1), x1 = min(max(xi + 1, 0), w_in - 1);
    const int y0 = min(max(yi, 0), h_in - 1), y1 = min(max(yi + 1, 0), h_in - 1);
    const uint8_t* r0 = src + (size_t)y0 * src_step;
    const uint8_t* r1 = src + (size_t)y1 * src_step;
    const uint8_t* p0 = r0 + (size_t)x0 * CN; const uint8_t* p1 = r0 + (size_t)x1 * CN;
    const uint8_t* p2 = r1 + (size_t)x0 * CN; const uint8_t* p3 = r1 + (size_t)x1 * CN;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float v = (float)p0[j] * c0 + (float)p1[j] * c1 + (float)p2[j] * c2 + (float)p3[j] * c3;
        bgr[j] = (uint8_t)(int)v;       // truncation, then the low byte: what x86-64 makes of (uchar)float
    }
}

template <int CN>
__global__ __launch_bounds__(kUX * kUY) void k_undistort(const uint8_t* __restrict__ src, size_t src_step, int w_in, int h_in,
                                                         const float2* __restrict__ table, size_t pitch,
                                                         uint8_t* __restrict__ dst, size_t dst_step, int w_out, int h_out)
{
    const int x0 = (blockIdx.x * kUX + threadIdx.x) * kUndistortRun;
    const int y = blockIdx.y * kUY + threadIdx.y;
    if (y >= h_out || x0 >= w_out) return;
    const float4* t = (const float4*)(table + (size_t)y * pitch + x0);     // pitch and x0 are multiples of the run: 32-byte aligned
    const float4 a = t[0], b = t[1];
    const float X[kUndistortRun] = { a.x, a.z, b.x, b.z }, Y[kUndistortRun] = { a.y, a.w, b.y, b.w };
    uint8_t* out = dst + (size_t)y * dst_step + (size_t)x0 * 3;
    if (x0 + kUndistortRun <= w_out && ((uintptr_t)out & 3) == 0) {
        uint8_t px[kUndistortRun][3];
#pragma unroll
        for (int i = 0; i < kUndistortRun; i++) undistort_pixel<CN>(src, src_step, w_in, h_in, X[i], Y[i], px[i]);
        uint32_t* o = (uint32_t*)out;
        o[0] = (uint32_t)px[0][0] | (uint32_t)px[0][1] << 8 | (uint32_t)px[0][2] << 16 | (uint32_t)px[1][0] << 24;
        o[1] = (uint32_t)px[1][1] | (uint32_t)px[1][2] << 8 | (uint32_t)px[2][0] << 16 | (uint32_t)px[2][1] << 24;
        o[2] = (uint32_t)px[2][2] | (uint32_t)px[3][0] << 8 | (uint32_t)px[3][1] << 16 | (uint32_t)px[3][2] << 24;
        return;
    }
#pragma unroll
    for (int i = 0; i < kUndistortRun; i++) {
        if (x0 + i >= w_out) break;
        uint8_t px[3];
        undistort_pixel<CN>(src, src_step, w_in, h_in, X[i], Y[i], px);
        out[3 * i] = px[0]; out[3 * i + 1] = px[1]; out[3 * i + 2] = px[2];
    }
}

}  // namespace

void launch_undistort(hipStream_t s, const uint8_t* src, size_t src_step, int w_in, int h_in, int cn, const float2* table,
                      uint8_t* dst, size_t dst_step, int w_out, int h_out)
{
    if (w_out <= 0 || h_out <= 0) return;
    const dim3 block(kUX, kUY), grid((unsigned)((w_out + kUX * kUndistortRun - 1) / (kUX * kUndistortRun)), (unsigned)((h_out + kUY - 1) / kUY));
    const size_t pitch = undistort_pitch(w_out);
    if (cn == 4) k_undistort<4><<<grid, block, 0, s>>>(src, src_step, w_in, h_in, table, pitch, dst, dst_step, w_out, h_out);
    else         k_undistort<3><<<grid, block, 0, s>>>(src, src_step, w_in, h_in, table, pitch, dst, dst_step, w_out, h_out);
}

}  // namespace pf
