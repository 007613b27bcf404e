// merge.hpp -- launch wrapper of the map-merge kernels (merge.hip): tile slots of one map selected into the slots of another.
//
// The rule is the render's own select with src in the place of the newer keyframe (MultiBandMap2DCPU.cpp:521,542; Map2DCPU.cpp:326):
//   multi-band, per pixel and level:  if (srcW >= dstW) { dstL = srcL; dstW = srcW; }
//   single band, per BGRA pixel:      if (dst.a < src.a) dst = src;
// and a dst slot that was fresh (no pyramid yet) takes src's slot image whole, padding included.
#pragma once
#include "kernels.hpp"

namespace pf {

// one pair of a merge launch; both addresses are 16-byte aligned slot images of TileLayout::slot_bytes bytes
struct MergePair {
    uint64_t dst, src;
    uint32_t dst_was_fresh;     // 1: copy the slot image, the select is not run against what the slot holds
    uint32_t pad_;
};
static_assert(sizeof(MergePair) == 24, "MergePair is read by the kernel as three words");

constexpr int kMergeBatch = 512;        // pairs per launch (FusionMap::launch_merge)

// pairs_dev[0..n): every pair's dst slot ends as the merge of the two.  single_band: slots are 256 x 256 BGRA words.
// won (may be null; measurement only): incremented by the pixel-levels src won, fresh slots not counted.
void launch_merge(hipStream_t s, const TileLayout& lay, bool single_band, const MergePair* pairs_dev, int n, unsigned long long* won);

}  // namespace pf
