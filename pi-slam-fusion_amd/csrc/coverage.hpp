// coverage.hpp -- the launchers of coverage.hip: the transparency masks of the masked pyramid TIFF (tiff_pyramid.hpp) as bit planes
// in HBM.  A plane of an image of r x c pixels is round256(r) rows of round256(c) / 8 bytes: bit 7 of byte 0 is column 0, every
// bit past the image is 0, so mask tile (ty, tx) is the window of 256 rows x 32 bytes at row 256 ty, byte 32 tx.
// Flags: a byte per tile, preset to 1 by the caller; fzero stays 1 where every bit of the tile is 0, fone where all 65 536 are 1.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace pf {

inline size_t coverage_plane_step(int cols) { return (size_t)((cols + 255) / 256) * 32; }
inline size_t coverage_plane_rows(int rows) { return (size_t)((rows + 255) / 256) * 256; }

// level 0 from a mosaic's tile table: wx x wy slots of 256 x 256 pixels (0 = no tile: zeros), covered = the fp32 weight at
// w_off inside the slot is not 0.  fzero / fone may be null
void launch_coverage_tiles(hipStream_t s, const uint64_t* table_dev, int wx, int wy, uint32_t w_off, uint8_t* plane, uint8_t* fzero, uint8_t* fone);
// level 0 from a byte per pixel (non-zero = covered), any size, rows of `step` bytes
void launch_coverage_bytes(hipStream_t s, const uint8_t* mask_dev, int rows, int cols, size_t step, uint8_t* plane, uint8_t* fzero, uint8_t* fone);
// the plane of image k + 1 (ceil(rows / 2) x ceil(cols / 2)) from that of image k (rows x cols): the OR of every 2 x 2 block
void launch_mask_overview(hipStream_t s, const uint8_t* src_plane, int rows, int cols, uint8_t* dst_plane, uint8_t* fzero, uint8_t* fone);
// n mask tiles (8192 bytes each), back to back into dst: tile i is the window at base + where[2 i] with rows of where[2 i + 1] bytes
void launch_mask_gather(hipStream_t s, const uint8_t* base, const uint64_t* where_dev, int n, uint8_t* dst);
// a plane whose image is whole tiles (cols a multiple of 256) as rows x cols bytes, 255 = covered, 0 = not
void launch_coverage_expand(hipStream_t s, const uint8_t* plane, int rows, int cols, uint8_t* bytes);

}  // namespace pf
