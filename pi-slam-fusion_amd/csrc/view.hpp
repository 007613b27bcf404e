// view.hpp -- the launchers of view.hip: a view of the mosaic at any pan, zoom, rotation or camera pose (view_plan.hpp, DESIGN.md
// "Views"), warped on the GPU from a collapsed rectangle of tiles and its coverage where both lie in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace pf {

// the coverage of a rectangle of wx x wy tile slots at pyramid level `level`, a byte a pixel (255 where the fp32 weight at w_off
// inside the slot is not 0, else 0; a slot without a tile: zeros): (wy E) rows of (wx E) bytes, E = 256 >> level
void launch_view_cover(hipStream_t s, const uint64_t* table_dev, int wx, int wy, int level, uint32_t w_off, uint8_t* cover);

// cv::warpPerspective(B G R C, M0, Size(width, height), INTER_LINEAR, BORDER_CONSTANT 0) with OpenCV 2.4.9's arithmetic, Minv =
// invert3x3(M0) handed over; bgr: srows x scols packed BGR8, cover: srows x scols bytes.  Pixels whose warped coverage is 0 get bg in
// their colour channels.  out: height rows of width pixels of `channels` (3 or 4) bytes, `step` bytes apart, in device memory
void launch_view_warp(hipStream_t s, const uint8_t* bgr, const uint8_t* cover, int srows, int scols, const double Minv[9], int width, int height, int channels, int bg,
                      uint8_t* out, size_t step);
// a view without content: bg in the colour channels, coverage 0
void launch_view_fill(hipStream_t s, int width, int height, int channels, int bg, uint8_t* out, size_t step);

}  // namespace pf
