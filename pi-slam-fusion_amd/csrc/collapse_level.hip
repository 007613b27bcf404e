// collapse_level.hip -- reduced-resolution views: the pyramid collapsed from the top and STOPPED at level k (gfx950, wave64).
//
// Collapsing a Laplacian pyramid down to level k gives the blended Gaussian level k: a low-passed 1 / 2^k view with the same seam
// blending.  The blending rule is self-similar -- Ele::blend's halo at level i is 1 << (L - i) -- so the level-k view is Ele::blend
// (MultiBandMap2DCPU.cpp:77-146) / save (:806-840) of a map whose tiles are E_k = 256 >> k pixels wide with levels k .. L: the
// reference's own operations, truncated.  Level 0 is collapse_fused.hip's and never comes here.
//
// One launch per request.  A workgroup owns a block of the level-k result, at most 128 x 32 pixels:
//   tile views (MOSAIC = false): the block is clipped to the tile, E_k x E_k.  4 blocks a tile at k = 1, 2 at k = 2, and from
//     k = 3 on (E_k <= 32) one workgroup takes a whole tile;
//   mosaic view (MOSAIC = true): the block grid covers the wy E_k x wx E_k image, the last row / column of blocks clipped to it.
//   1. the regions of levels k+1 .. L the block depends on (one pixel of halo per level: cf::level_region, the recurrence
//      started at level k) go from the tile slots straight into LDS -- at most the 1925 pixels = 23 100 B of the level-0 kernel;
//   2. levels L-1 .. k+1 are restored in place, one thread per 2 x 2 destination quad, with pyrUp_'s edge forms at the borders of
//      the padded square / the mosaic;
//   3. level k: a thread takes a 2 x 2 quad, forms pyrUp of level k+1 from LDS, adds the tile's own level-k Laplacian, masks by
//      the LEVEL-k weights (0 in a tile view, the background colour in the mosaic) and stores raw and / or 8U.  k = L has no
//      pyrUp: the masked top level, pixel by pixel.
// Nothing of a level > k returns to HBM, level k is read once and the result written once.
//
// Phase 2 and every sum are collapse_common.hpp's, shared with collapse_fused.hip; this file is the simple loads (1) and the 2 x 2 emit (3).
// Bit-exactness: -ffp-contract=off and the sums of collapse_common.hpp, in the association order of OpenCV 2.4.9's pyrUp_.
#include "collapse_common.hpp"

namespace pf {
namespace {

using namespace cf;

// One workgroup = one block of a level-k result (k >= 1; see the header).
//   MOSAIC = false: block (blockIdx % per_tile) of tile job[blockIdx / per_tile]; results to raw / bgr at tile index job.out
//   MOSAIC = true : block of the block grid of the pasted mosaic's level k; result to bgr (wy E_k x wx E_k x 3)
template <bool F32, bool MOSAIC>
__global__ __launch_bounds__(kCT) void k_collapse_level(TileLayout lay, int k, const BlendJob* __restrict__ jobs, const uint64_t* __restrict__ table,
                                                        int wx, int wy, int bg, char* __restrict__ raw, uint8_t* __restrict__ bgr)
{
    using T = typename Px<F32>::T; using WT = typename Px<F32>::WT;
    __shared__ WT lds[kLdsPx * 3];
    __shared__ BlendJob job;
    const int tid = threadIdx.x, L = lay.nlev - 1, wg = blockIdx.x;
    const int E = kElePixels >> k, sh = 8 - k;        // tile edge at level k

    int Y0, X0, bh, bw, rowsk, colsk;                 // the block and the extent of the (padded) level-k image
    int b = 0;                                        // border of the padded square at level k
    const PF_GLOBAL char* self = nullptr;             // tile views: the tile itself
    size_t out_base = 0;                              // ... and its first pixel in the outputs
    if constexpr (MOSAIC) {
        rowsk = wy * E; colsk = wx * E;
        const int nbx = (colsk + kBW - 1) / kBW;
        const int by = wg / nbx, bx = wg - by * nbx;
        Y0 = by * kBH; X0 = bx * kBW;
        bh = rowsk - Y0 < kBH ? rowsk - Y0 : kBH; bw = colsk - X0 < kBW ? colsk - X0 : kBW;
    } else {
        bw = E < kBW ? E : kBW; bh = E < kBH ? E : kBH;
        const int nbx = E / bw, per_tile = nbx * (E / bh);
        const int z = wg / per_tile, blk = wg - z * per_tile;
        if (tid < (int)(sizeof(BlendJob) / 4)) ((uint32_t*)&job)[tid] = ((const uint32_t*)(jobs + z))[tid];
        b = jobs[z].border ? 1 << (L - k) : 0;
        Y0 = b + (blk / nbx) * bh; X0 = b + (blk % nbx) * bw; rowsk = colsk = E + 2 * b;
        self = (const PF_GLOBAL char*)jobs[z].src[4];
        out_base = (size_t)jobs[z].out * E * E;
    }
    __syncthreads();

    // ---- 1. Laplacian regions of levels k+1 .. L -> LDS
    for (int i = k + 1; i <= L; i++) {
        const Reg r = level_region(k, i, Y0, X0, bh, bw, rowsk, colsk);
        const int n = r.h * r.w, lap_off = (int)lay.lap_off[i];
        const float rcp_w = 1.f / (float)r.w;
        for (int p = tid; p < n; p += kCT) {
            const int ry = div_small(p, rcp_w), rx = p - ry * r.w;
            WT v[3];
            if constexpr (MOSAIC) fetch_mosaic<F32>(table, wx, i, lap_off, r.y0 + ry, r.x0 + rx, v);
            else fetch_blend<F32>(job, lay.nlev, i, lap_off, r.y0 + ry, r.x0 + rx, v);
            WT* d = lds + (r.poff + p) * 3;
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2];
        }
    }
    __syncthreads();

    // ---- 2. restore levels L-1 .. k+1 in place (collapse_common.hpp)
    restore_levels<WT, kCT>(lds, k, L, Y0, X0, bh, bw, rowsk, colsk, tid);

    // ---- 3. level k.  A pixel's own Laplacian and weight: (ty, tx) inside the tile at `tile` (0: no tile there, mosaic only)
    const uint32_t lapk = lay.lap_off[k], wk = lay.w_off[k];
    const uint32_t bg8 = sat_u8(bg);
    auto emit = [&](const PF_GLOBAL char* tile, int ty, int tx, size_t o, const WT up[3], bool has_up) {
        WT v[3] = { (WT)0, (WT)0, (WT)0 };
        bool zero = true;
        if (tile) {
            load_px<F32, true>((const PF_GLOBAL T*)(tile + lapk) + (ty * E + tx) * 3, v);
            zero = ((const PF_GLOBAL float*)(tile + wk))[ty * E + tx] == 0.f;
            if (has_up) { v[0] = add_sat(up[0], v[0]); v[1] = add_sat(up[1], v[1]); v[2] = add_sat(up[2], v[2]); }
        }
        if constexpr (MOSAIC) {
            uint8_t* d = bgr + o * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) d[c] = (uint8_t)(zero ? bg8 : view_8u<F32>(v[c]));
        } else {
            if (zero) v[0] = v[1] = v[2] = (WT)0;
            if (bgr) {
                uint8_t* d = bgr + o * 3;
#pragma unroll
                for (int c = 0; c < 3; c++) d[c] = (uint8_t)view_8u<F32>(v[c]);
            }
            if (raw) {
                T* d = (T*)raw + o * 3;
#pragma unroll
                for (int c = 0; c < 3; c++) d[c] = (T)v[c];
            }
        }
    };
    // the tile under level-k pixel (y, x) and the pixel's place in it and in the output
    auto place = [&](int y, int x, const PF_GLOBAL char*& tile, int& ty, int& tx, size_t& o) {
        if constexpr (MOSAIC) {
            tile = (const PF_GLOBAL char*)table[(y >> sh) * wx + (x >> sh)];
            ty = y & (E - 1); tx = x & (E - 1); o = (size_t)y * colsk + x;
        } else { tile = self; ty = y - b; tx = x - b; o = out_base + (size_t)ty * E + tx; }
    };

    if (k == L) {                                      // the masked top level: no pyrUp
        const float rcp_bw = 1.f / (float)bw;
        const WT none[3] = { (WT)0, (WT)0, (WT)0 };
        for (int p = tid; p < bh * bw; p += kCT) {
            const int py = div_small(p, rcp_bw), px = p - py * bw;
            const PF_GLOBAL char* tile; int ty, tx; size_t o;
            place(Y0 + py, X0 + px, tile, ty, tx, o);
            emit(tile, ty, tx, o, none, false);
        }
        return;
    }
    // k < L: E_k, the border and the block origin are even, so the block is whole 2 x 2 quads, each inside one tile
    const Reg r1 = level_region(k, k + 1, Y0, X0, bh, bw, rowsk, colsk);
    const WT* src1 = lds - (r1.y0 * r1.w + r1.x0) * 3;
    const int qw = bw >> 1, nq = (bh >> 1) * qw;
    const float rcp_qw = 1.f / (float)qw;
    for (int qi = tid; qi < nq; qi += kCT) {
        const int qy = div_small(qi, rcp_qw), qx = qi - qy * qw;
        const int y = Y0 + 2 * qy, x = X0 + 2 * qx;
        const PF_GLOBAL char* tile; int ty, tx; size_t o;
        place(y, x, tile, ty, tx, o);
        WT up[4][3];
        if (tile) {
            const QuadSums<WT> q = quad_sums<WT>(src1, r1, y >> 1, x >> 1);
            const auto& Es = q.E; const auto& Os = q.O;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                up[0][c] = up_ee(Es[0][c], Es[1][c], Es[2][c]);
                up[1][c] = up_eo(Os[0][c], Os[1][c], Os[2][c]);
                up[2][c] = up_oe(Es[1][c], Es[2][c]);
                up[3][c] = up_oo(Os[1][c], Os[2][c]);
            }
        }
        const size_t orow = MOSAIC ? (size_t)colsk : (size_t)E;
        emit(tile, ty, tx, o, up[0], true);
        emit(tile, ty, tx + 1, o + 1, up[1], true);
        emit(tile, ty + 1, tx, o + orow, up[2], true);
        emit(tile, ty + 1, tx + 1, o + orow + 1, up[3], true);
    }
}

}  // namespace

// Ele::blend truncated at level k >= 1 (+ the 8U view) for n tiles in one launch; jobs in device memory (strip sources are not used here)
void launch_blend_level(hipStream_t s, const TileLayout& lay, int level, const BlendJob* jobs_dev, int n, void* raw_out, uint8_t* bgr_out)
{
    if (n <= 0) return;
    const int E = kElePixels >> level, bw = E < kBW ? E : kBW, bh = E < kBH ? E : kBH;
    const int nblocks = n * (E / bw) * (E / bh);
    if (lay.f32) hipLaunchKernelGGL((k_collapse_level<true, false>), dim3(nblocks), dim3(kCT), 0, s, lay, level, jobs_dev, (const uint64_t*)nullptr, 0, 0, 0, (char*)raw_out, bgr_out);
    else         hipLaunchKernelGGL((k_collapse_level<false, false>), dim3(nblocks), dim3(kCT), 0, s, lay, level, jobs_dev, (const uint64_t*)nullptr, 0, 0, 0, (char*)raw_out, bgr_out);
}

// save() truncated at level k >= 1: levels k .. L of the wx x wy mosaic pasted and collapsed, 8U, background where no level-k weight
void launch_save_level(hipStream_t s, const TileLayout& lay, int level, const uint64_t* table_dev, int wx, int wy, int bg, uint8_t* bgr_out)
{
    const int E = kElePixels >> level;
    const int nblocks = ((wx * E + kBW - 1) / kBW) * ((wy * E + kBH - 1) / kBH);
    if (nblocks <= 0) return;
    if (lay.f32) hipLaunchKernelGGL((k_collapse_level<true, true>), dim3(nblocks), dim3(kCT), 0, s, lay, level, (const BlendJob*)nullptr, table_dev, wx, wy, bg, (char*)nullptr, bgr_out);
    else         hipLaunchKernelGGL((k_collapse_level<false, true>), dim3(nblocks), dim3(kCT), 0, s, lay, level, (const BlendJob*)nullptr, table_dev, wx, wy, bg, (char*)nullptr, bgr_out);
}

}  // namespace pf
