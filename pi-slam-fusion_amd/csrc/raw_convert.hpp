// raw_convert.hpp -- raw frames (pf_raw_frame, include/pifusion.h) to packed BGR8: the formats, their per-pixel arithmetic, the checks and
// the host converter.  Pure: no HIP call, no allocation; what a kernel needs is marked PF_RAW_HD.  Three users: image_io.cpp (pf_raw_to_bgr:
// the host converter below), raw_convert.hip (its kernels call the same per-pixel functions) and tests/cpp/san_raw_convert.cpp.
// DESIGN.md "Raw frames" is the specification; tests/raw_model.py is written from it, not from this file.
//
// YUV 4:2:0 (NV12, NV21, I420): cv::cvtColor(CV_YUV2BGR_NV12 / _NV21 / _I420) of OpenCV 2.4.9 -- BT.601 studio range in 20-bit fixed
// point, one (U, V) per 2 x 2 block, no chroma interpolation.  Grey: CV_GRAY2BGR.  Bayer: bilinear, the one-pixel frame taking the value
// of the nearest interior pixel; specified by this project, not claimed byte-equal to OpenCV.
#pragma once
#include "../../include/pifusion.h"
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PF_RAW_HD __host__ __device__ __forceinline__
#else
#define PF_RAW_HD inline
#endif

namespace pf {
namespace raw {

constexpr int kCY = 1220542, kCUB = 2116026, kCUG = -409993, kCVG = -852492, kCVR = 1673527, kShift = 20;

PF_RAW_HD bool is_yuv(int format) { return format == PF_RAW_NV12 || format == PF_RAW_NV21 || format == PF_RAW_I420; }
PF_RAW_HD bool is_bayer(int format) { return format >= PF_RAW_BAYER_RGGB && format <= PF_RAW_BAYER_GBRG; }
PF_RAW_HD int  planes_of(int format) { return format == PF_RAW_I420 ? 3 : (format == PF_RAW_NV12 || format == PF_RAW_NV21) ? 2 : 1; }

// the chroma part of a 2 x 2 block, then each of its four pixels
struct Chroma { int ruv, guv, buv; };
PF_RAW_HD Chroma yuv_chroma(int U, int V)
{
    const int u = U - 128, v = V - 128;
    return Chroma{ (1 << (kShift - 1)) + kCVR * v, (1 << (kShift - 1)) + kCVG * v + kCUG * u, (1 << (kShift - 1)) + kCUB * u };
}
// sat8(v >> kShift) with the clamp done first, which is the same value (the shift is monotonic; (256 << kShift) - 1 is the largest v that
// gives 255).  In the written order hipcc fuses shift and saturation of two pixels into one v_ashr_pk_u8_i32 and ORs further bytes into the
// result as if the upper half of that register were zero; on gfx950 it is not, and neighbouring bytes of the kernel's output picked up
// stray bits.  Clamp, then shift, compiles to v_med3_i32 and a plain shift.
PF_RAW_HD uint8_t sat8_shifted(int v)
{
    const int top = (256 << kShift) - 1;
    return (uint8_t)((v < 0 ? 0 : v > top ? top : v) >> kShift);
}
PF_RAW_HD void yuv_pixel(int Y, const Chroma& c, uint8_t& b, uint8_t& g, uint8_t& r)
{
    const int y = (Y > 16 ? Y - 16 : 0) * kCY;
    b = sat8_shifted(y + c.buv);
    g = sat8_shifted(y + c.guv);
    r = sat8_shifted(y + c.ruv);
}

// Bayer.  The colour of the site (y, x), as its index in a BGR pixel: 0 blue, 1 green, 2 red.  Formats are named by row 0's first two pixels.
PF_RAW_HD int bayer_site(int format, int y, int x)
{
    const int k = (y & 1) * 2 + (x & 1);
    // RGGB: R G / G B     BGGR: B G / G R     GRBG: G R / B G     GBRG: G B / R G
    const int packed = format == PF_RAW_BAYER_RGGB ? 0x0112 : format == PF_RAW_BAYER_BGGR ? 0x2110 : format == PF_RAW_BAYER_GRBG ? 0x1021 : 0x1201;
    return (packed >> (4 * k)) & 3;
}
// One interior pixel from its 3 x 3 neighbourhood.  site: its own colour; row_colour: on a green site, the colour of its row neighbours
PF_RAW_HD void bayer_window(int site, int row_colour, int nw, int n, int ne, int w, int c, int e, int sw, int s, int se, uint8_t bgr[3])
{
    if (site != 1) {
        bgr[site] = (uint8_t)c;
        bgr[1] = (uint8_t)((n + s + w + e + 2) >> 2);
        bgr[2 - site] = (uint8_t)((nw + ne + sw + se + 2) >> 2);
    } else {
        bgr[1] = (uint8_t)c;
        bgr[row_colour] = (uint8_t)((w + e + 1) >> 1);
        bgr[2 - row_colour] = (uint8_t)((n + s + 1) >> 1);
    }
}
PF_RAW_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
// Any pixel (y, x) of a rows x cols mosaic (both >= 3): the interior pixel at the clamped position.  p: rows of `step` bytes
PF_RAW_HD void bayer_pixel(int format, const uint8_t* p, size_t step, int rows, int cols, int y, int x, uint8_t bgr[3])
{
    const int cy = clampi(y, 1, rows - 2), cx = clampi(x, 1, cols - 2);
    const uint8_t* r0 = p + (size_t)(cy - 1) * step + (cx - 1);
    const uint8_t* r1 = r0 + step;
    const uint8_t* r2 = r1 + step;
    bayer_window(bayer_site(format, cy, cx), bayer_site(format, cy, cx + 1), r0[0], r0[1], r0[2], r1[0], r1[1], r1[2], r2[0], r2[1], r2[2], bgr);
}

// ---- the descriptor
// bytes of a row and number of rows of plane k
inline size_t plane_row(const pf_raw_frame& f, int k)
{
    if (k == 0) return (size_t)f.cols;
    return f.format == PF_RAW_I420 ? (size_t)f.cols / 2 : (size_t)f.cols;          // NV12 / NV21: cols / 2 pairs
}
inline int    plane_rows(const pf_raw_frame& f, int k) { return k == 0 ? f.rows : f.rows / 2; }
inline size_t plane_step(const pf_raw_frame& f, int k) { return f.step[k] ? f.step[k] : plane_row(f, k); }
// what a reader of plane k may touch: (rows - 1) * step + row
inline size_t plane_bytes(const pf_raw_frame& f, int k) { return (size_t)(plane_rows(f, k) - 1) * plane_step(f, k) + plane_row(f, k); }

// the refusals of pf_raw_to_bgr and its kin: false with the reason in `why`
inline bool check(const pf_raw_frame& f, std::string& why)
{
    if (f.format != PF_RAW_GREY && !is_yuv(f.format) && !is_bayer(f.format)) { why = "unknown raw format " + std::to_string(f.format); return false; }
    if (f.rows < 1 || f.cols < 1) { why = "rows and cols must be at least 1"; return false; }
    if (is_yuv(f.format) && ((f.rows | f.cols) & 1)) { why = "a YUV 4:2:0 frame needs even rows and cols"; return false; }
    if (is_bayer(f.format) && (f.rows < 3 || f.cols < 3)) { why = "a Bayer frame needs at least 3 x 3 pixels"; return false; }
    for (int k = 0; k < planes_of(f.format); k++) {
        if (!f.plane[k]) { why = "plane " + std::to_string(k) + " is missing"; return false; }
        if (f.step[k] && f.step[k] < plane_row(f, k)) { why = "step of plane " + std::to_string(k) + " is smaller than its row"; return false; }
        if (plane_step(f, k) >= (1ull << 31) || (unsigned long long)plane_step(f, k) * (unsigned long long)plane_rows(f, k) >= (1ull << 31)) {
            why = "plane " + std::to_string(k) + " has 2 GiB or more"; return false;
        }
    }
    return true;
}
// the destination: `step` bytes per row, 0 = packed; false for a step below the row or an image of 2 GiB or more
inline bool check_bgr(const pf_raw_frame& f, size_t& step, std::string& why)
{
    const size_t row = (size_t)f.cols * 3;
    if (!step) step = row;
    if (step < row) { why = "bgr_step is smaller than a row"; return false; }
    if (step >= (1ull << 31) || (unsigned long long)step * (unsigned long long)f.rows >= (1ull << 31)) { why = "the BGR image has 2 GiB or more"; return false; }
    return true;
}

// ---- the host converter: f checked, planes in host memory, step resolved by check_bgr.  Touches 3 * cols bytes of each destination row
inline void to_bgr_host(const pf_raw_frame& f, uint8_t* bgr, size_t step)
{
    const uint8_t* p0 = (const uint8_t*)f.plane[0];
    const size_t s0 = plane_step(f, 0);
    if (f.format == PF_RAW_GREY) {
        for (int y = 0; y < f.rows; y++) {
            const uint8_t* s = p0 + (size_t)y * s0;
            uint8_t* d = bgr + (size_t)y * step;
            for (int x = 0; x < f.cols; x++) d[3 * x] = d[3 * x + 1] = d[3 * x + 2] = s[x];
        }
    } else if (is_yuv(f.format)) {
        const bool planar = f.format == PF_RAW_I420;
        const uint8_t* pu = (const uint8_t*)f.plane[1];
        const uint8_t* pv = planar ? (const uint8_t*)f.plane[2] : pu;
        const size_t su = plane_step(f, 1), sv = planar ? plane_step(f, 2) : su;
        const int uo = planar ? 0 : (f.format == PF_RAW_NV21 ? 1 : 0), vo = planar ? 0 : 1 - uo, cs = planar ? 1 : 2;
        for (int y = 0; y < f.rows; y += 2) {
            const uint8_t* y0 = p0 + (size_t)y * s0;
            const uint8_t* y1 = y0 + s0;
            const uint8_t* u = pu + (size_t)(y / 2) * su + uo;
            const uint8_t* v = pv + (size_t)(y / 2) * sv + vo;
            uint8_t* d0 = bgr + (size_t)y * step;
            uint8_t* d1 = d0 + step;
            for (int x = 0; x < f.cols; x += 2) {
                const Chroma c = yuv_chroma(u[(x / 2) * cs], v[(x / 2) * cs]);
                yuv_pixel(y0[x], c, d0[3 * x], d0[3 * x + 1], d0[3 * x + 2]);
                yuv_pixel(y0[x + 1], c, d0[3 * x + 3], d0[3 * x + 4], d0[3 * x + 5]);
                yuv_pixel(y1[x], c, d1[3 * x], d1[3 * x + 1], d1[3 * x + 2]);
                yuv_pixel(y1[x + 1], c, d1[3 * x + 3], d1[3 * x + 4], d1[3 * x + 5]);
            }
        }
    } else {
        for (int y = 0; y < f.rows; y++) {
            uint8_t* d = bgr + (size_t)y * step;
            for (int x = 0; x < f.cols; x++) bayer_pixel(f.format, p0, s0, f.rows, f.cols, y, x, d + 3 * x);
        }
    }
}

}  // namespace raw

#if defined(__HIPCC__)
// raw_convert.hip: the conversion of a checked frame whose planes lie in device memory, queued on s; dst rows dst_step bytes apart (resolved
// by check_bgr).  Allocates nothing and does not wait.  Reads stay inside plane_bytes() of each plane, writes inside 3 * cols bytes of each
// destination row.
void launch_raw_convert(hipStream_t s, const pf_raw_frame& f, uint8_t* dst, size_t dst_step);
#endif

}  // namespace pf
