// view_index.hpp -- source addressing of the view warp (view.hip: cv::warpPerspective INTER_LINEAR + BORDER_CONSTANT 0 on 8UC4,
// remapBilinear's 15-bit fixed-point taps): which pixels the four taps of a warped pixel are, which of them lie in the image, which
// bytes they load and how the taps are weighed.  Plain integer code shared by the kernel and by the host-side check
// tests/cpp/view_index_check.cpp, which proves under AddressSanitizer for every source coordinate around small images that no byte
// outside the two buffers is loaded and that the taps are the pixels OpenCV's in-range flags name.
//
// The source is the collapsed rectangle where the collapse left it -- srows x scols packed BGR8 -- and its coverage, a byte a
// pixel; together the 4-channel image B G R C of the specification.  A tap outside the image contributes 0 and loads nothing.
#pragma once
#include "warp_index.hpp"          // PF_HD, sat_short
#include <cstddef>

namespace pf {

// the four taps (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1): in[k] says whether tap k lies in the image, px[k] is its
// pixel index sy * scols + sx (0 where it does not: an index that is always valid).  false: all four lie outside
struct ViewTaps { bool in[4]; uint32_t px[4]; };

PF_HD bool view_taps(int sx, int sy, int srows, int scols, ViewTaps& t)
{
    if (sx >= scols || sx + 1 < 0 || sy >= srows || sy + 1 < 0) return false;
    const bool x0 = sx >= 0, x1 = sx + 1 < scols, y0 = sy >= 0, y1 = sy + 1 < srows;
    t.in[0] = x0 && y0; t.in[1] = x1 && y0; t.in[2] = x0 && y1; t.in[3] = x1 && y1;
    const uint32_t base = (uint32_t)(y0 ? sy : 0) * (uint32_t)scols, next = (uint32_t)(sy + 1) * (uint32_t)scols;      // srows, scols <= 32767: no wrap
    t.px[0] = t.in[0] ? base + (uint32_t)sx : 0u;
    t.px[1] = t.in[1] ? base + (uint32_t)(sx + 1) : 0u;
    t.px[2] = t.in[2] ? next + (uint32_t)sx : 0u;
    t.px[3] = t.in[3] ? next + (uint32_t)(sx + 1) : 0u;
    return true;
}

// B | G << 8 | R << 16 | C << 24 of pixel p: three bytes of the mosaic, one of the coverage
PF_HD uint32_t view_load(const uint8_t* bgr, const uint8_t* cover, uint32_t p)
{
    const uint8_t* s = bgr + (size_t)p * 3;
    return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)cover[p] << 24);
}

// initInterTab2D's integer weights of the sub-pixel phase (a, b) = (X & 31, Y & 31): saturate_cast<short>(w * 32768) of the float
// products (1 - fy)(1 - fx), (1 - fy) fx, fy (1 - fx), fy fx with fx = a / 32, fy = b / 32.  On the 1 / 32 grid those products and
// their scaling are exact, so the weights are the integers below; they sum to 32768 except at (0, 0), where 32768 saturates to 32767
// and the table's fix-up hands the missing 1 to the last tap
PF_HD void view_weights(int a, int b, int w[4])
{
    w[0] = (32 - a) * (32 - b) * 32; w[1] = a * (32 - b) * 32; w[2] = (32 - a) * b * 32; w[3] = a * b * 32;
    if (w[0] > 32767) { w[0] = 32767; w[3] += 1; }
}

PF_HD uint32_t view_sat_u8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// the warped pixel at fixed-point source position (X, Y) (1 / 32 pixel): FixedPtCast<int, uchar, 15> of the four taps, four channels
PF_HD uint32_t view_sample(const uint8_t* bgr, const uint8_t* cover, int X, int Y, int srows, int scols)
{
    ViewTaps t;
    if (!view_taps(sat_short(X >> 5), sat_short(Y >> 5), srows, scols, t)) return 0u;
    int w[4];
    view_weights(X & 31, Y & 31, w);
    int acc[4] = { 1 << 14, 1 << 14, 1 << 14, 1 << 14 };
    for (int k = 0; k < 4; k++) {
        if (!t.in[k]) continue;
        const uint32_t v = view_load(bgr, cover, t.px[k]);
        for (int c = 0; c < 4; c++) acc[c] += (int)((v >> (8 * c)) & 0xffu) * w[k];
    }
    uint32_t c0 = view_sat_u8(acc[0] >> 15), c1 = view_sat_u8(acc[1] >> 15), c2 = view_sat_u8(acc[2] >> 15), c3 = view_sat_u8(acc[3] >> 15);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));          // each component through an asm operand before the OR: see pack_bgra (single_band.hip)
#endif
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

}  // namespace pf
