// undistort.hpp -- launch wrapper of the undistortion kernel (undistort.hip): a frame of a distorted camera remapped into the map's pinhole
// camera through the table of undistort_plan.hpp.  The pixel is UndistorterImpl::undistort's colour branch (GSLAM/core/Undistorter.h:141-164,
// :296-309) in float, no fused multiply-add, summed left to right:
//   xi = (int)X, yi = (int)Y, xx = X - xi, yy = Y - yi, xy = xx * yy
//   c0 = ((1 - xx) - yy) + xy, c1 = xx - xy, c2 = yy - xy, c3 = xy     on the taps (xi, yi), (xi+1, yi), (xi, yi+1), (xi+1, yi+1)
//   channel = (uchar)(p0 c0 + p1 c1 + p2 c2 + p3 c3), truncated
// with tap indices clamped into the source and an entry with X < 0 giving a black pixel ("Undistortion").
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace pf {

constexpr int kUndistortRun = 4;        // consecutive output pixels of one row that a thread owns

// entries of a table row as the kernel reads it: the width rounded up to whole runs, so that a run's entries are two aligned 16-byte loads
inline size_t undistort_pitch(int w_out) { return ((size_t)w_out + kUndistortRun - 1) / kUndistortRun * kUndistortRun; }

// table: h_out rows of undistort_pitch(w_out) (x, y) pairs, 16-byte aligned (entries past w_out are not used).  src: h_in rows of w_in pixels
// of cn (3: BGR8, 4: BGRA8, alpha ignored) bytes, src_step bytes apart.  dst: h_out rows of w_out packed BGR8 pixels, dst_step bytes apart.
// Reads of src stay inside (h_in - 1) * src_step + w_in * cn bytes, writes inside (h_out - 1) * dst_step + 3 * w_out.
void launch_undistort(hipStream_t s, const uint8_t* src, size_t src_step, int w_in, int h_in, int cn, const float2* table,
                      uint8_t* dst, size_t dst_step, int w_out, int h_out);

}  // namespace pf
