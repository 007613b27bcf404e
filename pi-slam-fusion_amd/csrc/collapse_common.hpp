// collapse_common.hpp -- device helpers shared by the collapse kernels (collapse_fused.hip: level 0; collapse_level.hip: the views of
// level k): pyrUp_'s arithmetic for the four parities of a destination pixel, the 16S / 32F pixel types, and the addressing of a
// Laplacian pixel in a tile's padded square (Ele::blend) or in the pasted mosaic (save).
#pragma once
#include "kernels.hpp"
#include "warp_index.hpp"

namespace pf {
namespace cf {

#define PF_GLOBAL __attribute__((address_space(1)))

template <bool F32> struct Px;
template <> struct Px<false> { using T = short; using WT = int; };
template <> struct Px<true>  { using T = float; using WT = float; };

// pyrUp_'s vertical step + cast for the four parities of a destination pixel.  E = even-column horizontal sum, O = odd-column sum / 4
// (see the header); rows 0 / 1 / 2 = source rows sy-1 / sy / sy+1.
__device__ __forceinline__ int   up_ee(int e0, int e1, int e2)       { return (int)(short)((e0 + e1 * 6 + e2 + 32) >> 6); }   // (short) C cast: wraps
__device__ __forceinline__ int   up_eo(int o0, int o1, int o2)       { return (int)(short)((o0 + o1 * 6 + o2 + 8) >> 4); }
__device__ __forceinline__ int   up_oe(int e1, int e2)               { return (int)(short)((e1 + e2 + 8) >> 4); }
__device__ __forceinline__ int   up_oo(int o1, int o2)               { return (int)(short)((o1 + o2 + 2) >> 2); }
__device__ __forceinline__ float up_ee(float e0, float e1, float e2) { return (e0 + e1 * 6 + e2) * (1.f / 64); }
__device__ __forceinline__ float up_eo(float o0, float o1, float o2) { return (o0 + o1 * 6 + o2) * (1.f / 16); }
__device__ __forceinline__ float up_oe(float e1, float e2)           { return (e1 + e2) * (1.f / 16); }
__device__ __forceinline__ float up_oo(float o1, float o2)           { return (o1 + o2) * (1.f / 4); }
__device__ __forceinline__ int   add_sat(int up, int lap)     { return sat_short(up + lap); }  // cv::add on 16S saturates
__device__ __forceinline__ float add_sat(float up, float lap) { return up + lap; }
__device__ __forceinline__ uint32_t sat_u8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// idx / w for 0 <= idx < 4096, 1 <= w <= 128, rcp = 1.f / w: (idx + 0.5) / w is at least 1 / 256 away from an integer, the float error is below 2^-10
__device__ __forceinline__ int div_small(int idx, float rcp) { return (int)(((float)idx + 0.5f) * rcp); }

// three components of a pixel.  int16 pixels (6 bytes, 2-byte aligned) of a TILE SLOT are read as one 8-byte load: the two bytes behind a
// pixel are the next pixel's or the level's alignment padding inside the slot (levels are 256-byte aligned, the weights follow the last one).
// Packed halo strips keep three 2-byte loads: their last pixel may be the last bytes of the exchange buffer.
template <bool F32, bool SLOT>
__device__ __forceinline__ void load_px(const PF_GLOBAL typename Px<F32>::T* s, typename Px<F32>::WT out[3])
{
    using WT = typename Px<F32>::WT;
    if constexpr (!F32 && SLOT) {
        typedef uint32_t u2u __attribute__((ext_vector_type(2), aligned(1)));
        const u2u v = *(const PF_GLOBAL u2u*)s;
        out[0] = (int)(short)(v.x & 0xffffu); out[1] = (int)v.x >> 16; out[2] = (int)(short)(v.y & 0xffffu);
    } else { out[0] = (WT)s[0]; out[1] = (WT)s[1]; out[2] = (WT)s[2]; }
}

__device__ __forceinline__ void strip_dims_d(int nlev, int level, int dx, int dy, int& w, int& h)
{
    const int ts = kElePixels >> level, b = 1 << (nlev - 1 - level);
    w = dx == 0 ? ts : b; h = dy == 0 ? ts : b;
}

// Laplacian pixel (py, px) of level `level` of a tile's padded square (Ele::blend's assembly, .cpp:93-117)
template <bool F32>
__device__ __forceinline__ void fetch_blend(const BlendJob& job, int nlev, int level, int lap_off, int py, int px, typename Px<F32>::WT out[3])
{
    using T = typename Px<F32>::T;
    const int ts = kElePixels >> level, b = job.border ? 1 << (nlev - 1 - level) : 0;
    int rx = 1, sx = px - b, ry = 1, sy = py - b;
    if (sx < 0) { rx = 0; sx += ts; } else if (sx >= ts) { rx = 2; sx -= ts; }
    if (sy < 0) { ry = 0; sy += ts; } else if (sy >= ts) { ry = 2; sy -= ts; }
    const int j = ry * 3 + rx;
    const PF_GLOBAL T* s;
    if (!((job.strip_mask >> j) & 1)) {
        s = (const PF_GLOBAL T*)((const PF_GLOBAL char*)job.src[j] + lap_off) + (sy * ts + sx) * 3;
        load_px<F32, true>(s, out);
        return;
    } else {                                              // packed strips: levels concatenated, each h x w row-major from the strip's corner
        const int dx = rx - 1, dy = ry - 1;
        int off = 0;
        for (int i = 0; i < level; i++) { int w, h; strip_dims_d(nlev, i, dx, dy, w, h); off += w * h; }
        int w, h; strip_dims_d(nlev, level, dx, dy, w, h);
        const int lx = rx == 0 ? sx - (ts - b) : sx, ly = ry == 0 ? sy - (ts - b) : sy;
        s = (const PF_GLOBAL T*)job.src[j] + (off + ly * w + lx) * 3;
    }
    load_px<F32, false>(s, out);
}

// ... of the pasted mosaic (save, .cpp:806-834): absent tiles are zero
template <bool F32>
__device__ __forceinline__ void fetch_mosaic(const uint64_t* __restrict__ table, int wx, int level, int lap_off, int py, int px, typename Px<F32>::WT out[3])
{
    using T = typename Px<F32>::T; using WT = typename Px<F32>::WT;
    const int sh = 8 - level, ts = kElePixels >> level;
    const uint64_t ent = table[(py >> sh) * wx + (px >> sh)];
    if (!ent) { out[0] = out[1] = out[2] = (WT)0; return; }
    const PF_GLOBAL T* s = (const PF_GLOBAL T*)((const PF_GLOBAL char*)ent + lap_off) + ((py & (ts - 1)) * ts + (px & (ts - 1))) * 3;
    load_px<F32, true>(s, out);
}

}  // namespace cf
}  // namespace pf
