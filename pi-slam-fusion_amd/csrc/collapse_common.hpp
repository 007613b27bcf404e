// collapse_common.hpp -- the steps shared by the collapse kernels (collapse_fused.hip: level 0; collapse_level.hip: the views of
// level k): the block geometry and the recurrence of the regions a block depends on, pyrUp_'s arithmetic for the four parities of a
// destination pixel with its edge forms, the in-LDS restore of the levels above the result's, the 16S / 32F pixel types and the 8U
// view, and the addressing of a Laplacian pixel in a tile's padded square (Ele::blend) or in the pasted mosaic (save).  The two
// kernels differ in how they load the regions (phase 1) and in how they emit the result's level (phase 3).
#pragma once
#include "kernels.hpp"
#include "warp_index.hpp"
#include "level_step.hpp"

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
// the 8U view (updateTexture's / save's convertTo CV_8UC3)
template <bool F32> __device__ __forceinline__ uint32_t view_8u(typename Px<F32>::WT v)
{
    if constexpr (F32) return sat_u8(__float2int_rn(v * 255.f));
    else return sat_u8(v);
}

// idx / w for 0 <= idx < 4096, 1 <= w <= 128, rcp = 1.f / w: (idx + 0.5) / w is at least 1 / 256 away from an integer, the float error is below 2^-10
__device__ __forceinline__ int div_small(int idx, float rcp) { return (int)(((float)idx + 0.5f) * rcp); }

// ---- block geometry: a workgroup owns a block of the result's level, at most kBW x kBH pixels (level 0: always that)
constexpr int kBW = 128, kBH = 32;
constexpr int kCT = 256;                              // threads
constexpr int region_edge(int s, int up) { for (int i = 0; i < up; i++) s = ((s + 1) >> 1) + 2; return s; }
constexpr int region_px(int up) { return region_edge(kBW, up) * region_edge(kBH, up); }
constexpr int region_px_total(int from) { int n = 0; for (int i = from; i < kMaxLevels; i++) n += region_px(i); return n; }
constexpr int kLdsPx = region_px_total(1);            // 1925 pixels = 23 100 B of 3 x 4-byte components: the regions of a full block with 8 levels above it
static_assert(region_edge(128, 1) == 66 && region_edge(32, 1) == 18 && region_edge(66, 1) == 35, "pyrUp dependence regions");
static_assert(kLdsPx == 1925 && kBW * kBH <= 4096 && kBW <= 128, "div_small: idx < 4096, w <= 128");

// region of a level held in LDS: rows [y0, y0 + h) x cols [x0, x0 + w) of the level's image (rows x cols); the regions of levels
// k+1, k+2, ... lie back to back, pixel p of the flat list at lds[3 p]
struct Reg {
    int y0, x0, h, w;
    int poff, rows, cols;                // first pixel in the flat list; extent of the level's image
};

// what the level-k block rows [Y0, Y0 + bh) x cols [X0, X0 + bw) needs of level `level` > k: pyrUp is a 3-tap filter, so rows
// [lo, hi] of level i-1 need rows [(lo-1)>>1, (hi>>1)+1] of level i.  rowsk x colsk: the level-k image.  Every input is
// workgroup-uniform, so this is scalar code.
__device__ __forceinline__ Reg level_region(int k, int level, int Y0, int X0, int bh, int bw, int rowsk, int colsk)
{
    int ylo = Y0, yhi = Y0 + bh - 1, xlo = X0, xhi = X0 + bw - 1, poff = 0;
    Reg r{};
    for (int i = k + 1; i <= level; i++) {
        const int rows = rowsk >> (i - k), cols = colsk >> (i - k);
        level_step(ylo, yhi, rows);
        level_step(xlo, xhi, cols);
        r.y0 = ylo; r.x0 = xlo; r.h = yhi - ylo + 1; r.w = xhi - xlo + 1; r.poff = poff; r.rows = rows; r.cols = cols;
        poff += r.h * r.w;
    }
    return r;
}

// pyrUp_'s horizontal sums for the 2 x 2 destination quad under source pixel (sy, sx) of the level whose region rs lies at `src`
// ([(y * w + x) * 3] = source pixel (y, x)): E = even-column sum, O = odd-column sum / 4, for source rows sy-1 / sy / sy+1 under
// pyrUp's row rule (-1 -> 1, rows -> rows - 1).  Rows and columns are clamped into the region: one the region lacks is only ever
// asked for by a destination pixel outside the destination region, which is not stored.  The interior / edge test stands outside
// the row x component loops.  The sums come back by value: as array out-parameters they changed the level-0 kernel's instruction
// stream more, and its int16 blend was 0.6 % slower than with the sums written in place (profiles/output_side_refactor.md).
template <class WT> struct QuadSums { WT E[3][3], O[3][3]; };
template <class WT>
__device__ __forceinline__ QuadSums<WT> quad_sums(const WT* src, const Reg& rs, int sy, int sx)
{
    QuadSums<WT> q;
    auto& E = q.E; auto& O = q.O;
    const int ylo = rs.y0, yhi = rs.y0 + rs.h - 1, xlo = rs.x0, xhi = rs.x0 + rs.w - 1;
    int r0 = sy - 1; if (r0 < 0) r0 = rs.rows > 1 ? 1 : 0;
    int r2 = sy + 1; if (r2 > rs.rows - 1) r2 = rs.rows - 1;
    r0 = r0 < ylo ? ylo : (r0 > yhi ? yhi : r0); r2 = r2 > yhi ? yhi : r2;
    const int r1 = sy > yhi ? yhi : sy;
    int ca = sx - 1; ca = ca < xlo ? xlo : ca;
    int cc = sx + 1; cc = cc > xhi ? xhi : cc;
    const int cb = sx > xhi ? xhi : sx;
    const int rowo[3] = { r0 * rs.w * 3, r1 * rs.w * 3, r2 * rs.w * 3 };
    if (sx > 0 && sx < rs.cols - 1) {
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const WT a = src[rowo[rr] + ca * 3 + k], b = src[rowo[rr] + cb * 3 + k], c = src[rowo[rr] + cc * 3 + k];
                E[rr][k] = a + b * 6 + c; O[rr][k] = b + c;
            }
    } else {
        const bool single = rs.cols == 1, left = sx == 0;
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const WT a = src[rowo[rr] + ca * 3 + k], b = src[rowo[rr] + cb * 3 + k], c = src[rowo[rr] + cc * 3 + k];
                if (single)    { E[rr][k] = b * 8; O[rr][k] = b * 2; }
                else if (left) { E[rr][k] = b * 6 + c * 2; O[rr][k] = b + c; }
                else           { E[rr][k] = a + b * 7; O[rr][k] = b * 2; }      // right edge
            }
    }
    return q;
}

// restore levels top-1 .. k+1 in place in LDS: pyr[i-1] = pyrUp(pyr[i]) + pyr[i-1] for i = top .. k+2, thread t of CT one 2 x 2
// destination quad at a time (quads aligned to even coordinates; a quad on the rim of the region has pixels outside it, which are
// not stored).  pyrUp + add in the reference's operation order, with its C cast and saturation.  Ends on a barrier.
template <class WT, int CT>
__device__ __forceinline__ void restore_levels(WT* lds, int k, int top, int Y0, int X0, int bh, int bw, int rowsk, int colsk, int t)
{
    for (int i = top; i >= k + 2; i--) {
        const Reg rs = level_region(k, i, Y0, X0, bh, bw, rowsk, colsk), rd = level_region(k, i - 1, Y0, X0, bh, bw, rowsk, colsk);
        const WT* src = lds + rs.poff * 3 - (rs.y0 * rs.w + rs.x0) * 3;          // [(y * w + x) * 3] = source pixel (y, x)
        WT* dst = lds + rd.poff * 3 - (rd.y0 * rd.w + rd.x0) * 3;
        const int qy0 = rd.y0 >> 1, qx0 = rd.x0 >> 1, qw = ((rd.x0 + rd.w - 1) >> 1) - qx0 + 1, nq = (((rd.y0 + rd.h - 1) >> 1) - qy0 + 1) * qw;
        const float rcp_qw = 1.f / (float)qw;
        for (int qi = t; qi < nq; qi += CT) {
            const int qy = div_small(qi, rcp_qw), qx = qi - qy * qw;
            const int sy = qy0 + qy, sx = qx0 + qx;
            const QuadSums<WT> q = quad_sums<WT>(src, rs, sy, sx);
            const auto& E = q.E; const auto& O = q.O;
            const int y = 2 * sy, x = 2 * sx;
            const bool vy0 = y >= rd.y0, vy1 = y + 1 < rd.y0 + rd.h, vx0 = x >= rd.x0, vx1 = x + 1 < rd.x0 + rd.w;
            WT* d0 = dst + (y * rd.w + x) * 3;
            WT* d1 = d0 + rd.w * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (vy0 && vx0) d0[c] = add_sat(up_ee(E[0][c], E[1][c], E[2][c]), d0[c]);
                if (vy0 && vx1) d0[3 + c] = add_sat(up_eo(O[0][c], O[1][c], O[2][c]), d0[3 + c]);
                if (vy1 && vx0) d1[c] = add_sat(up_oe(E[1][c], E[2][c]), d1[c]);
                if (vy1 && vx1) d1[3 + c] = add_sat(up_oo(O[1][c], O[2][c]), d1[3 + c]);
            }
        }
        __syncthreads();
    }
}

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
