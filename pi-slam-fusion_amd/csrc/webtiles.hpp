// webtiles.hpp -- the launchers of webtiles.hip and the pyramid driver above them: north-up Web-Mercator map tiles (EPSG:3857, z/x/y
// of 256 x 256 pixels) resampled on the GPU from a mosaic and its coverage where they lie in HBM (pf_webtiles_device, pf_webtiles,
// pf_save_webtiles).  The georeference and the tables the sampler reads are webtiles_plan.hpp's.
//
// A tile in HBM is 256 x 256 x 3 bytes of BGR8 in a slot of a pixel buffer, 8192 bytes of mask in the slot of the same number of a
// mask buffer (the TIFF's mask-tile format: 32 bytes a row, bit 7 of byte 0 = column 0, 1 = covered), and two flag bytes, preset to 1
// by the caller as coverage.hpp's: fzero stays 1 where no pixel of the tile is covered, fone where all are.
#pragma once
#include "jpeg_encode.hpp"
#include "../../include/pifusion.h"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace pf {

constexpr size_t kWebTilePixels = (size_t)256 * 256 * 3, kWebTileMask = 8192;

// what the sampler reads: the mosaic (BGR8, `step` bytes a row), its coverage (a byte per pixel, non-zero = covered, `mask_step`
// bytes a row) and the four tables of webtiles_plan.hpp, ux / uy from the global column c0 on, vx / vy from the global row r0 on
struct WebSampleSource {
    const uint8_t* bgr; size_t step;
    const uint8_t* mask; size_t mask_step;
    int rows, cols;
    const double *ux, *uy, *vx, *vy;
    long long c0, r0;
    int bg;                   // the background colour, already saturated to 0 .. 255
};

// gw x gh tiles of the sampling zoom, tile (gx0 + i, gy0 + j) into slot slot0 + j * pitch + i.  Every column and row of them lies inside the tables
void launch_webtile_sample(hipStream_t s, const WebSampleSource& src, int gx0, int gy0, int gw, int gh, int slot0, int pitch, uint8_t* px, uint8_t* mask, uint8_t* fzero, uint8_t* fone);

// n parent tiles from their children: desc holds five ints a parent -- the slots of the children (2X, 2Y), (2X + 1, 2Y), (2X, 2Y + 1),
// (2X + 1, 2Y + 1) in the source buffers (-1: no such tile) and the parent's slot in the destination buffers.  A child whose fzero
// flag is still 1 counts as absent
void launch_webtile_reduce(hipStream_t s, const int* desc_dev, int n, const uint8_t* src_px, const uint8_t* src_mask, const uint8_t* src_fzero,
                           uint8_t* dst_px, uint8_t* dst_mask, uint8_t* dst_fzero, uint8_t* dst_fone, int bg);

// tiles of 2^k x 2^k sampling-zoom tiles go through HBM at a time (k = 3 unless pf_debug_webtiles_batch says otherwise)
void webtiles_set_batch(int edge);
int  webtiles_batch();

// The whole export: tiles of zmax sampled, every zoom above reduced from the one below down to zmin, every tile that has a covered pixel
// encoded with `enc` and handed to the sink.  Everything is queued on `stream`; returns when the last tile was handed over.
// zmax < 0: the native zoom; zmin < 0: the first zoom at which the range is one tile.  False with the reason in last_error()
bool webtiles_export(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, const double px2ll[6], int zmin, int zmax,
                     int quality, int bg, bool want_pixels, pf_webtile_sink sink, void* user, JpegEncoder& enc, hipStream_t stream);

// milliseconds the three parts of the most recent webtiles_export of this thread's process took on the GPU, by HIP events around
// their launches -- sample kernel, reduce kernel, encoder (its host waits included) -- and the tiles it sampled; measured only while
// webtiles_set_timing(true)
void webtiles_set_timing(bool on);
void webtiles_last_timing(double out[4]);

}  // namespace pf
