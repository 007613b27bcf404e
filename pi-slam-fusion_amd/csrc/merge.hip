// merge.hip -- gfx950 kernels of the map merge (merge.hpp): src tile slots selected into dst tile slots, or copied whole where dst was fresh.
//
// A streaming kernel: per pair it reads src's weights, dst's weights, src's Laplacians where some pixel of the group wins, and writes what
// src won.  dst's Laplacians are never read.  An item is one 16-byte vector of fp32 weights (4 pixels: 3 x 16 bytes of Laplacian) or two of
// them for int16 pyramids (8 pixels: again 3 x 16 bytes of Laplacian); a group src wins whole is stored with 16-byte stores, a group it
// wins in part pixel by pixel, a group it loses not at all -- so a wave without a winning lane issues no store.  Levels smaller than one
// group (int16: 2 x 2; both types: 1 x 1) are items of one pixel.
// Grid: (chunk of the slot, pair) -- a block never looks past its own pair's two slots, and the table has exactly gridDim.y entries.
#include "merge.hpp"

namespace pf {

namespace {

constexpr int kMT = 256;            // threads of a block: 4 waves
constexpr int kItemsPerThread = 4;  // items a thread handles, kMT apart: a wave's loads of one step are contiguous
constexpr int kChunk = kMT * kItemsPerThread;

// the items of one multi-band slot, level by level
struct MergePlan {
    int      nlev;
    uint32_t item0[kMaxLevels + 1];     // first item of level i; [nlev .. kMaxLevels]: items of a slot
    uint32_t nvec;                      // 16-byte vectors of a slot image
};

__device__ __forceinline__ void copy_slot_chunk(char* dst, const char* src, uint32_t nvec)
{
    const uint32_t per = (nvec + gridDim.x - 1) / gridDim.x;
    const uint32_t v0 = blockIdx.x * per, v1 = min(v0 + per, nvec);
    for (uint32_t v = v0 + threadIdx.x; v < v1; v += kMT) ((uint4*)dst)[v] = ((const uint4*)src)[v];
}

template <bool F32>
__global__ __launch_bounds__(kMT) void k_merge(TileLayout lay, MergePlan plan, const MergePair* __restrict__ pairs, unsigned long long* won)
{
    using T = typename std::conditional<F32, uint32_t, uint16_t>::type;      // Laplacian channels move as bits
    constexpr uint32_t GPX = F32 ? 4 : 8;
    const MergePair pr = pairs[blockIdx.y];
    char* dst = (char*)(uintptr_t)pr.dst;
    const char* src = (const char*)(uintptr_t)pr.src;
    if (pr.dst_was_fresh) { copy_slot_chunk(dst, src, plan.nvec); return; }
    unsigned nwon = 0;
#pragma unroll
    for (int k = 0; k < kItemsPerThread; k++) {
        const uint32_t it = blockIdx.x * kChunk + k * kMT + threadIdx.x;
        if (it >= plan.item0[kMaxLevels]) break;
        // the item's level: constant indices into the kernel arguments, selected
        uint32_t lo = lay.lap_off[0], wo = lay.w_off[0], first = 0; int lv = 0;
#pragma unroll
        for (int i = 1; i < kMaxLevels; i++)
            if (it >= plan.item0[i]) { lo = lay.lap_off[i]; wo = lay.w_off[i]; first = plan.item0[i]; lv = i; }
        const uint32_t j = it - first, side = (uint32_t)kElePixels >> lv;
        if (side * side < GPX) {
            // scalar tail: item j is pixel j
            const float sw = ((const float*)(src + wo))[j], dw = ((const float*)(dst + wo))[j];
            if (sw >= dw) {
                const T* sl = (const T*)(src + lo) + 3 * j; T* dl = (T*)(dst + lo) + 3 * j;
                dl[0] = sl[0]; dl[1] = sl[1]; dl[2] = sl[2];
                ((float*)(dst + wo))[j] = sw;
                nwon++;
            }
            continue;
        }
        float sw[GPX], dw[GPX];
        {
            const float4* s4 = (const float4*)(src + wo) + j * (GPX / 4); const float4* d4 = (const float4*)(dst + wo) + j * (GPX / 4);
#pragma unroll
            for (uint32_t q = 0; q < GPX / 4; q++) {
                const float4 a = s4[q], b = d4[q];
                sw[4 * q] = a.x; sw[4 * q + 1] = a.y; sw[4 * q + 2] = a.z; sw[4 * q + 3] = a.w;
                dw[4 * q] = b.x; dw[4 * q + 1] = b.y; dw[4 * q + 2] = b.z; dw[4 * q + 3] = b.w;
            }
        }
        unsigned win = 0;
#pragma unroll
        for (uint32_t p = 0; p < GPX; p++) win |= (sw[p] >= dw[p] ? 1u : 0u) << p;
        if (!win) continue;
        nwon += __popc(win);
        const uint4* sl = (const uint4*)(src + lo) + 3 * j;
        const uint4 a = sl[0], b = sl[1], c = sl[2];
        uint4* dl = (uint4*)(dst + lo) + 3 * j;
        if (win == (1u << GPX) - 1) {
            dl[0] = a; dl[1] = b; dl[2] = c;
            float4* d4 = (float4*)(dst + wo) + j * (GPX / 4);
#pragma unroll
            for (uint32_t q = 0; q < GPX / 4; q++) d4[q] = make_float4(sw[4 * q], sw[4 * q + 1], sw[4 * q + 2], sw[4 * q + 3]);
            continue;
        }
        const uint32_t L[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
        float* dwp = (float*)(dst + wo) + j * GPX;
#pragma unroll
        for (uint32_t p = 0; p < GPX; p++) {
            if (!(win >> p & 1)) continue;
            T* d = (T*)dl + 3 * p;
#pragma unroll
            for (uint32_t ch = 0; ch < 3; ch++) {
                const uint32_t e = 3 * p + ch;                                  // element of the group's 12 words / 24 halves
                d[ch] = F32 ? (T)L[e] : (T)(L[e / 2] >> (16 * (e & 1)));
            }
            dwp[p] = sw[p];
        }
    }
    if (won && nwon) atomicAdd(won, (unsigned long long)nwon);
}

// single band: a slot is 256 x 256 BGRA words, alpha (the weight byte) on top; an item is four pixels
__global__ __launch_bounds__(kMT) void k_merge_bgra(const MergePair* __restrict__ pairs, unsigned long long* won)
{
    constexpr uint32_t nvec = kElePixels * kElePixels / 4;
    const MergePair pr = pairs[blockIdx.y];
    uint4* dst = (uint4*)(uintptr_t)pr.dst;
    const uint4* src = (const uint4*)(uintptr_t)pr.src;
    if (pr.dst_was_fresh) { copy_slot_chunk((char*)dst, (const char*)src, nvec); return; }
    unsigned nwon = 0;
#pragma unroll
    for (int k = 0; k < kItemsPerThread; k++) {
        const uint32_t it = blockIdx.x * kChunk + k * kMT + threadIdx.x;
        if (it >= nvec) break;
        const uint4 s = src[it], d = dst[it];
        const bool w0 = (d.x >> 24) < (s.x >> 24), w1 = (d.y >> 24) < (s.y >> 24), w2 = (d.z >> 24) < (s.z >> 24), w3 = (d.w >> 24) < (s.w >> 24);
        if (!(w0 | w1 | w2 | w3)) continue;
        nwon += (unsigned)w0 + w1 + w2 + w3;
        if (w0 & w1 & w2 & w3) { dst[it] = s; continue; }
        uint32_t* p = (uint32_t*)(dst + it);
        if (w0) p[0] = s.x;
        if (w1) p[1] = s.y;
        if (w2) p[2] = s.z;
        if (w3) p[3] = s.w;
    }
    if (won && nwon) atomicAdd(won, (unsigned long long)nwon);
}

}  // namespace

void launch_merge(hipStream_t s, const TileLayout& lay, bool single_band, const MergePair* pairs_dev, int n, unsigned long long* won)
{
    if (n <= 0) return;
    if (single_band) {
        const uint32_t nvec = kElePixels * kElePixels / 4;
        hipLaunchKernelGGL(k_merge_bgra, dim3((nvec + kChunk - 1) / kChunk, (unsigned)n), dim3(kMT), 0, s, pairs_dev, won);
        return;
    }
    MergePlan plan{};
    plan.nlev = lay.nlev; plan.nvec = lay.slot_bytes / 16;
    const uint32_t gpx = lay.f32 ? 4 : 8;
    uint32_t items = 0;
    for (int i = 0; i < lay.nlev; i++) {
        const uint32_t npx = (uint32_t)(kElePixels >> i) * (kElePixels >> i);
        plan.item0[i] = items;
        items += npx >= gpx ? npx / gpx : npx;
    }
    for (int i = lay.nlev; i <= kMaxLevels; i++) plan.item0[i] = items;
    const dim3 grid((items + kChunk - 1) / kChunk, (unsigned)n);
    if (lay.f32) hipLaunchKernelGGL(k_merge<true>, grid, dim3(kMT), 0, s, lay, plan, pairs_dev, won);
    else         hipLaunchKernelGGL(k_merge<false>, grid, dim3(kMT), 0, s, lay, plan, pairs_dev, won);
}

}  // namespace pf
