// view.hip -- a view of the mosaic at any pan, zoom, rotation or camera pose (view.hpp, view_plan.hpp, DESIGN.md "Views"):
// cv::warpPerspective(INTER_LINEAR, BORDER_CONSTANT 0) of the 4-channel image B G R C -- the collapsed rectangle of tiles and its
// coverage -- with OpenCV 2.4.9's arithmetic, byte for byte what oracle.c's orc_warp_linear_const_8u computes.
//
//   k_view_cover   the coverage of the rectangle at the view's level, a byte a pixel, from the level's fp32 weights through the
//                  rectangle's tile table: one thread a pixel, a wave reads 256 contiguous bytes of a tile row.
//   k_view_warp    one thread a view pixel, a wave = 64 pixels of a row.  The fp64 coordinates keep warpPerspective's block-origin
//                  rule: every pixel carries the origin xb of its run of bw0 = min(1024 / min(16, height), width) pixels and adds
//                  M0 x1 to the run's (M0 xb + M1 y + M2), with no contraction into FMA (the file is built with -ffp-contract=off).
//                  W ? 32. / W : 0 in IEEE fp64, the convert that rounds to even and saturates (== clamp + cvRound), then plain
//                  integer code: the taps, their weights and the bytes they load are view_index.hpp's, which a host program checks.
//                  Pixels whose warped coverage is 0 get the background colour; 3 or 4 bytes a pixel leave with a row step.
//   k_view_fill    a view that misses the content: the background colour, coverage 0.
// Algorithmic bytes: the weights of the rectangle read once (4 a pixel) and a byte a pixel written; per view pixel four taps of 4
// bytes, neighbours in the source for neighbouring lanes, and 3 or 4 bytes written.
#include "view.hpp"
#include "view_index.hpp"
#include "plan_limits.hpp"

namespace pf {

namespace {

__global__ __launch_bounds__(256) void k_view_cover(const uint64_t* __restrict__ table, int wx, int level, uint32_t w_off, int cols, uint8_t* __restrict__ cover)
{
    const int x = (int)blockIdx.x * 256 + (int)threadIdx.x, y = (int)blockIdx.y;
    if (x >= cols) return;
    const int sh = 8 - level, ts = kElePixels >> level;
    const uint64_t ent = table[(size_t)(y >> sh) * wx + (x >> sh)];
    uint8_t c = 0;
    if (ent) c = ((const float*)(ent + w_off))[(y & (ts - 1)) * ts + (x & (ts - 1))] != 0.f ? 255 : 0;
    cover[(size_t)y * cols + x] = c;
}

struct ViewArgs {
    double M[9];
    int srows, scols, width, height, channels, bw0;
    uint32_t bg;              // the background colour in the three colour channels, coverage 0
    size_t step;
};

__device__ __forceinline__ void view_store(uint8_t* __restrict__ out, const ViewArgs& a, int x, int y, uint32_t v, bool words)
{
    uint8_t* d = out + (size_t)y * a.step + (size_t)x * a.channels;
    if (words) { *(uint32_t*)d = v; return; }
    d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16);
    if (a.channels == 4) d[3] = (uint8_t)(v >> 24);
}

__global__ __launch_bounds__(256) void k_view_warp(const uint8_t* __restrict__ bgr, const uint8_t* __restrict__ cover, ViewArgs a, uint8_t* __restrict__ out, int words)
{
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const int xb = x / a.bw0 * a.bw0, x1 = x - xb;
    const double X0 = a.M[0] * xb + a.M[1] * y + a.M[2];
    const double Y0 = a.M[3] * xb + a.M[4] * y + a.M[5];
    const double W0 = a.M[6] * xb + a.M[7] * y + a.M[8];
    double W = W0 + a.M[6] * x1;
    W = W ? 32. / W : 0;
    const int X = __double2int_rn((X0 + a.M[0] * x1) * W);          // the convert saturates: clamp to int + cvRound
    const int Y = __double2int_rn((Y0 + a.M[3] * x1) * W);
    uint32_t v = view_sample(bgr, cover, X, Y, a.srows, a.scols);
    if (!(v >> 24)) v = a.bg;
    view_store(out, a, x, y, v, words != 0);
}

__global__ __launch_bounds__(256) void k_view_fill(ViewArgs a, uint8_t* __restrict__ out, int words)
{
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    view_store(out, a, x, y, a.bg, words != 0);
}

ViewArgs view_args(int srows, int scols, const double Minv[9], int width, int height, int channels, int bg, size_t step)
{
    ViewArgs a{};
    if (Minv) for (int i = 0; i < 9; i++) a.M[i] = Minv[i];
    a.srows = srows; a.scols = scols; a.width = width; a.height = height; a.channels = channels;
    const int bh0 = height < 16 ? height : 16, bw = 1024 / bh0;
    a.bw0 = bw < width ? bw : width;
    const uint32_t b = (uint32_t)(bg < 0 ? 0 : (bg > 255 ? 255 : bg));
    a.bg = b | (b << 8) | (b << 16);
    a.step = step;
    return a;
}

// four-byte pixels leave as one store where every one of them is aligned
int word_stores(const uint8_t* out, size_t step, int channels) { return channels == 4 && (((uintptr_t)out | step) & 3) == 0; }

}  // namespace

void launch_view_cover(hipStream_t s, const uint64_t* table_dev, int wx, int wy, int level, uint32_t w_off, uint8_t* cover)
{
    const int e = kElePixels >> level, cols = wx * e, rows = wy * e;
    if (cols <= 0 || rows <= 0) return;
    hipLaunchKernelGGL(k_view_cover, dim3((unsigned)((cols + 255) / 256), (unsigned)rows), dim3(256), 0, s, table_dev, wx, level, w_off, cols, cover);
}

void launch_view_warp(hipStream_t s, const uint8_t* bgr, const uint8_t* cover, int srows, int scols, const double Minv[9], int width, int height, int channels, int bg,
                      uint8_t* out, size_t step)
{
    if (width <= 0 || height <= 0) return;
    const ViewArgs a = view_args(srows, scols, Minv, width, height, channels, bg, step);
    hipLaunchKernelGGL(k_view_warp, dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4)), dim3(256), 0, s, bgr, cover, a, out, word_stores(out, step, channels));
}

void launch_view_fill(hipStream_t s, int width, int height, int channels, int bg, uint8_t* out, size_t step)
{
    if (width <= 0 || height <= 0) return;
    const ViewArgs a = view_args(0, 0, nullptr, width, height, channels, bg, step);
    hipLaunchKernelGGL(k_view_fill, dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4)), dim3(256), 0, s, a, out, word_stores(out, step, channels));
}

}  // namespace pf
