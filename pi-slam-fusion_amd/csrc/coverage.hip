// coverage.hip -- the GPU side of the masked pyramid TIFF's masks (tiff_pyramid.hpp, coverage.hpp): where the mosaic has content,
// as bit planes, straight from what lies in HBM.  All of it is bandwidth-bound word arithmetic: plain vector loads and stores, no
// atomics, no LDS beyond the workgroup vote behind the flags.
//
//   k_coverage_tiles   one workgroup of 256 lanes per tile slot of the mosaic.  A wave takes 8 rows of the slot's level-0 weight
//                      plane per step: every lane loads the 16 bytes of four weights of each row (8 loads in flight, each one
//                      a contiguous kilobyte across the wave), turns them into four "!= 0" bits, the 8 lanes of a word OR
//                      their nibbles together, and every lane stores ONE 32-bit word: lane (8 g + j) the word g of row j.
//                      A slot without a tile gives zeros.
//   k_coverage_bytes   the same plane from a byte per pixel of any size and step; zeroes the bits past the image.
//   k_mask_overview    one workgroup per tile of image k + 1: OR of the two rows, OR of neighbouring bits, the even bits squeezed
//                      together -- 64 pixels of image k per lane and step, no per-pixel work.
//   k_mask_gather      the tiles that are neither all zero nor all one, of all levels, back to back: what crosses to the host.
//   k_coverage_expand  bits to 0 / 255 bytes (pf_save_to_memory_mask).
// The three makers clear the per-tile flags "all zero" / "all one" of what they write: bytes preset to 1 by the caller, cleared
// with a plain store by one lane of the workgroup that owns the tile (k_coverage_bytes: by up to eight workgroups, all storing 0).
// Algorithmic bytes: 4 per pixel read (the weights), 1/8 written; every further level reads 1/8 and writes 1/32 of a byte per pixel
// of the level above.
#include "coverage.hpp"

namespace pf {

namespace {

// a plane's bytes hold column 0 in bit 7 of byte 0: a word read little-endian is byte-swapped, then bit 31 is its first column
__device__ inline uint32_t msb_first(uint32_t v) { return __builtin_bswap32(v); }

// four bytes (byte 0 = the first column) -> four "non-zero" bits, the first column highest
__device__ inline uint32_t nonzero4(uint32_t w)
{
    const uint32_t t = (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
    return ((t >> 4) & 8u) | ((t >> 13) & 4u) | ((t >> 22) & 2u) | (t >> 31);
}

// 32 columns (bit 31 first) -> 16: every pair ORed, the results in bits 15 ... 0
__device__ inline uint32_t or_pairs(uint32_t v)
{
    v = ((v | (v << 1)) >> 1) & 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0F0F0F0Fu;
    v = (v | (v >> 4)) & 0x00FF00FFu;
    v = (v | (v >> 8)) & 0x0000FFFFu;
    return v;
}

// one lane of the workgroup clears the flags of the tile the workgroup wrote words of
__device__ inline void clear_flags(bool any, bool all, uint8_t* fzero, uint8_t* fone, size_t tile)
{
    const int a = __syncthreads_or(any ? 1 : 0), b = __syncthreads_and(all ? 1 : 0);
    if (threadIdx.x == 0) {
        if (a && fzero) fzero[tile] = 0;
        if (!b && fone) fone[tile] = 0;
    }
}

__global__ __launch_bounds__(256) void k_coverage_tiles(const uint64_t* __restrict__ table, int wx, uint32_t w_off, uint8_t* __restrict__ plane,
                                                        uint8_t* __restrict__ fzero, uint8_t* __restrict__ fone)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t slot = (size_t)blockIdx.y * wx + blockIdx.x, pstep = (size_t)wx * 32;
    uint8_t* out = plane + (size_t)blockIdx.y * 256 * pstep + (size_t)blockIdx.x * 32;
    const uint64_t ent = table[slot];
    bool any = false, all = true;
    if (!ent) {          // no tile: a row of 32 zero bytes per lane
        uint4* d = (uint4*)(out + (size_t)t * pstep);
        d[0] = uint4{ 0, 0, 0, 0 }; d[1] = uint4{ 0, 0, 0, 0 };
        all = false;
    } else {
        const float* w = (const float*)(ent + w_off);
        const int j = lane & 7, g = lane >> 3;
#pragma unroll 1
        for (int step = 0; step < 8; step++) {
            const int row0 = 32 * step + 8 * wave;
            float4 v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = *(const float4*)(w + (size_t)(row0 + i) * 256 + 4 * lane);
            uint32_t mine = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                uint32_t x = ((v[i].x != 0.f ? 8u : 0u) | (v[i].y != 0.f ? 4u : 0u) | (v[i].z != 0.f ? 2u : 0u) | (v[i].w != 0.f ? 1u : 0u)) << (28 - 4 * j);
                x |= __shfl_xor(x, 1); x |= __shfl_xor(x, 2); x |= __shfl_xor(x, 4);
                if (i == j) mine = x;
            }
            *(uint32_t*)(out + (size_t)(row0 + j) * pstep + 4 * g) = msb_first(mine);
            any = any || mine != 0; all = all && mine == 0xFFFFFFFFu;
        }
    }
    clear_flags(any, all, fzero, fone, slot);
}

// a workgroup per 32 rows of a tile: lane = (row, word), 32 bytes of the mask per lane
__global__ __launch_bounds__(256) void k_coverage_bytes(const uint8_t* __restrict__ mask, int rows, int cols, size_t step, uint8_t* __restrict__ plane, size_t pstep, int tx,
                                                        uint8_t* __restrict__ fzero, uint8_t* __restrict__ fone)
{
    const int t = threadIdx.x, word = t & 7;
    const int y = 32 * (int)blockIdx.y + (t >> 3), x0 = 256 * (int)blockIdx.x + 32 * word;          // inside the padded plane
    uint32_t bits = 0;
    if (y < rows && x0 < cols) {
        const uint8_t* p = mask + (size_t)y * step + x0;
        if (x0 + 32 <= cols && ((size_t)p & 3) == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) bits |= nonzero4(((const uint32_t*)p)[i]) << (28 - 4 * i);
        } else {
            const int n = min(32, cols - x0);
            for (int i = 0; i < n; i++) bits |= (p[i] ? 1u : 0u) << (31 - i);
        }
    }
    *(uint32_t*)(plane + (size_t)y * pstep + (size_t)x0 / 8) = msb_first(bits);
    clear_flags(bits != 0, bits == 0xFFFFFFFFu, fzero, fone, (size_t)(blockIdx.y >> 3) * tx + blockIdx.x);
}

// a workgroup per tile of the level it writes: 8 steps of 32 rows, lane = (row, word); the two words above each half of the word
// come as one 8-byte load per row.  What lies past the source plane counts as 0, as what lies past the image inside it is 0.
__global__ __launch_bounds__(256) void k_mask_overview(const uint8_t* __restrict__ src, int srows, size_t sstep, uint8_t* __restrict__ dst, size_t dstep, int tx,
                                                       uint8_t* __restrict__ fzero, uint8_t* __restrict__ fone)
{
    const int t = threadIdx.x, word = t & 7;
    const size_t w = 8 * (size_t)blockIdx.x + word;          // word of the destination row; its source: words 2 w and 2 w + 1
    bool any = false, all = true;
#pragma unroll 1
    for (int it = 0; it < 8; it++) {
        const int y = 256 * (int)blockIdx.y + 32 * it + (t >> 3);
        uint32_t a = 0, b = 0;
        if (8 * w + 8 <= sstep) {
            if (2 * y < srows) { const uint2 v = *(const uint2*)(src + (size_t)(2 * y) * sstep + 8 * w); a = msb_first(v.x); b = msb_first(v.y); }
            if (2 * y + 1 < srows) { const uint2 v = *(const uint2*)(src + (size_t)(2 * y + 1) * sstep + 8 * w); a |= msb_first(v.x); b |= msb_first(v.y); }
        }
        const uint32_t o = (or_pairs(a) << 16) | or_pairs(b);
        *(uint32_t*)(dst + (size_t)y * dstep + 4 * w) = msb_first(o);
        any = any || o != 0; all = all && o == 0xFFFFFFFFu;
    }
    clear_flags(any, all, fzero, fone, (size_t)blockIdx.y * tx + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_mask_gather(const uint8_t* __restrict__ base, const uint64_t* __restrict__ where, uint8_t* __restrict__ dst)
{
    const size_t i = blockIdx.x;
    const uint4* s = (const uint4*)(base + where[2 * i] + (size_t)threadIdx.x * where[2 * i + 1]);
    uint4* d = (uint4*)(dst + i * 8192 + (size_t)threadIdx.x * 32);
    d[0] = s[0]; d[1] = s[1];
}

// 16 pixels per lane: two bytes of the plane in, 16 bytes out
__global__ __launch_bounds__(256) void k_coverage_expand(const uint8_t* __restrict__ plane, size_t pstep, int rows, int cols, uint8_t* __restrict__ bytes)
{
    const size_t per_row = (size_t)cols / 16, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_row * rows) return;
    const size_t y = i / per_row, g = i - y * per_row;
    const uint32_t v = *(const uint16_t*)(plane + y * pstep + 2 * g);          // byte 0: columns 0 ... 7, its bit 7 first
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t b = (v >> (8 * (q >> 1))) >> (4 * (1 - (q & 1)));          // the nibble of columns 4 q ... 4 q + 3, its bit 3 first
        o[q] = ((b & 8u) ? 0xFFu : 0u) | ((b & 4u) ? 0xFF00u : 0u) | ((b & 2u) ? 0xFF0000u : 0u) | ((b & 1u) ? 0xFF000000u : 0u);
    }
    *(uint4*)(bytes + y * cols + 16 * g) = uint4{ o[0], o[1], o[2], o[3] };
}

}  // namespace

void launch_coverage_tiles(hipStream_t s, const uint64_t* table_dev, int wx, int wy, uint32_t w_off, uint8_t* plane, uint8_t* fzero, uint8_t* fone)
{
    if (wx <= 0 || wy <= 0) return;
    hipLaunchKernelGGL(k_coverage_tiles, dim3((unsigned)wx, (unsigned)wy), dim3(256), 0, s, table_dev, wx, w_off, plane, fzero, fone);
}

void launch_coverage_bytes(hipStream_t s, const uint8_t* mask_dev, int rows, int cols, size_t step, uint8_t* plane, uint8_t* fzero, uint8_t* fone)
{
    if (rows <= 0 || cols <= 0) return;
    const int tx = (cols + 255) / 256;
    hipLaunchKernelGGL(k_coverage_bytes, dim3((unsigned)tx, (unsigned)(coverage_plane_rows(rows) / 32)), dim3(256), 0, s, mask_dev, rows, cols, step, plane, coverage_plane_step(cols), tx, fzero, fone);
}

void launch_mask_overview(hipStream_t s, const uint8_t* src_plane, int rows, int cols, uint8_t* dst_plane, uint8_t* fzero, uint8_t* fone)
{
    const int r2 = (rows + 1) / 2, c2 = (cols + 1) / 2, tx = (c2 + 255) / 256, ty = (r2 + 255) / 256;
    hipLaunchKernelGGL(k_mask_overview, dim3((unsigned)tx, (unsigned)ty), dim3(256), 0, s, src_plane, (int)coverage_plane_rows(rows), coverage_plane_step(cols), dst_plane,
                       coverage_plane_step(c2), tx, fzero, fone);
}

void launch_mask_gather(hipStream_t s, const uint8_t* base, const uint64_t* where_dev, int n, uint8_t* dst)
{
    if (n > 0) hipLaunchKernelGGL(k_mask_gather, dim3((unsigned)n), dim3(256), 0, s, base, where_dev, dst);
}

void launch_coverage_expand(hipStream_t s, const uint8_t* plane, int rows, int cols, uint8_t* bytes)
{
    const size_t n = (size_t)rows * (cols / 16);
    if (n) hipLaunchKernelGGL(k_coverage_expand, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, plane, coverage_plane_step(cols), rows, cols, bytes);
}

}  // namespace pf
