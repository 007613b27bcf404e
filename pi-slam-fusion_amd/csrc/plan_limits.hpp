// plan_limits.hpp -- the plain limits the kernels' launch arguments and the host's keyframe plan (frame_plan.hpp) share; no HIP header.
#pragma once

namespace pf {

constexpr int kElePixels = 256;
constexpr int kMaxLevels = 9;
constexpr int kArgTable = 256;      // tile-table entries that can travel inside the kernel arguments of a launch
constexpr int kMaxRects = 8;        // need rectangles of a level-0 job (tile-sharded canvases, the cull): what LevelLaunch can hold
constexpr int kMaxRectsUpper = 4;   // ... of an upper-level job (their need bitmaps took the room in the kernel arguments; they are the fallback there)
constexpr int kNeedWords = 100;     // 32-bit words of need bitmaps a launch can carry for its upper-level jobs (kernel arguments are 4 KB)
struct BlockRect { short x0, y0, x1, y1; };      // [x0,x1) x [y0,y1) in blocks of the job's block grid

}  // namespace pf
