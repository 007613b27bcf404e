/*
 * pifusion.h -- C ABI of libpifusion.so, the MI355X-native drop-in for the
 * Map2DFusion multi-band hot path of Immortalqx/pi-slam-fusion.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the reference tree).  Plain pointers and sizes only; no C++/torch types.
 * All int-returning calls follow the reference's bool convention: 1 = ok,
 * 0 = failed (message on stderr), never throw, never abort.
 *
 * Poses are 7 doubles in the reference's SE3 stream order
 * `x y z qx qy qz qw` (GSLAM/GSLAM/core/SE3.h:112-117); a pose is
 * camera-to-world exactly as handed to Map2D::feed (Map2DFusion/Map2D.h:91).
 */
#ifndef PIFUSION_H
#define PIFUSION_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ELE_PIXELS 256            /* Map2DFusion/Map2D.h:35 ELE_PIXELS */

/* Map2D::Map2DType, Map2DFusion/Map2D.h:83 */
enum { PF_TYPE_NONE = 0, PF_TYPE_CPU = 1, PF_TYPE_GPU = 2, PF_TYPE_MULTIBAND = 3, PF_TYPE_RENDER = 4 };

/* OpenCV / GImage type codes (GSLAM/GSLAM/core/GImage.h:27-36,97) */
enum { PF_8UC1 = 0, PF_8UC3 = 16, PF_8UC4 = 24, PF_16SC3 = 19, PF_32FC1 = 5, PF_32FC3 = 21 };

/* Image view, layout-compatible with cv::Mat / GSLAM::GImage headers
 * (rows, cols, type, data; GImage.h:387-389).  step = bytes per row
 * (0 = packed).  data may be a host pointer (pf_feed) or a device pointer
 * (pf_feed_device). */
typedef struct pf_image {
    int         rows, cols, type;
    const void* data;
    size_t      step;
} pf_image;

/* The svar keys read on the path, as one struct. */
typedef struct pf_options {
    int    band_number;      /* MultiBandMap2DCPU.BandNumber   (5)  .cpp:260 */
    int    force_float;      /* MultiBandMap2DCPU.ForceFloat   (0)  .cpp:444 */
    int    high_quality_show;/* MultiBandMap2DCPU.HighQualityShow (1) .cpp:261 */
    int    weight_type;      /* Map2D.WeightType               (0)  .cpp:407 */
    int    bg_color;         /* Result.BackGroundColor         (0)  .cpp:840 */
    double resolution;       /* Map2D.Resolution (0 = auto)         .cpp:228 */
    double scale;            /* Map2D.Scale                    (1)  .cpp:235 */
    int    device;           /* HIP device ordinal (-1 = current)            */
    int    shard_rank;       /* tile sharding: this rank ...                 */
    int    shard_count;      /* ... of shard_count (1 = own every tile)      */
    int    shard_block;      /* spatial-hash cell edge in tiles (default 8)  */
    int    max_queue;        /* feed queue cap, drop-oldest (20)    .cpp:302 */
    int    fused;            /* fused level kernels.  1 (default): one launch per keyframe,
                                levels pipelined across frames; 3: one launch and stream
                                per level; 2: as 3 in the 4-stage 64x16-block shape;
                                0: one kernel per reference op (warp / pyrDown /
                                Laplacian+select)                                    */
    int    lookahead;        /* keyframes that wait, fed but not rendered, so that the cull can leave a keyframe out of the cells
                                in which one of the NEXT `lookahead` keyframes is bound to overwrite it (default 48; 0: every
                                keyframe is rendered inside its own feed call).  The select keeps the largest weight, the newest
                                keyframe among equals, whatever the order, and every call that reads tiles, flags or counters
                                (pf_sync, blend, save, tile access, statistics) renders what waits first (the window then fills
                                again at two keyframes per three feeds, so the GPU is not left idle): what a caller can observe
                                is the map after the keyframes fed so far, exactly as without it.  Multi-band maps with
                                fused = 1 and Map2DCPU maps (a shard looks ahead among its own tiles); elsewhere the value is ignored.  A pf_feed_device frame must stay valid until
                                pf_sync in either case.                                                                      */
} pf_options;

typedef struct pf_map pf_map;

/* --- lifecycle --------------------------------------------------------- */
void    pf_default_options(pf_options* o);
/* key=value setter accepting the reference's svar key names
 * ("MultiBandMap2DCPU.BandNumber", "Map2D.Scale", ...); 1 if the key is known */
int     pf_options_set(pf_options* o, const char* key, const char* value);
/* Map2D::create(type, thread), Map2DFusion/Map2D.cpp:51-66.  MULTIBAND -> the multi-band
 * engine; CPU -> Map2DCPU semantics (single 8-bit band); GPU -> the same, as the reference
 * itself falls back ("CUDA is not enabled, switch to CPU"); NONE/RENDER -> NULL.        */
pf_map* pf_create(int type, int thread, const pf_options* opt);
void    pf_destroy(pf_map* m);
const char* pf_last_error(void);

/* --- Map2D virtuals ---------------------------------------------------- */
/* Map2D::prepare(plane, camera, frames), MultiBandMap2DCPU.cpp:266-286.
 * cam = {w,h,fx,fy,cx,cy} (PinHoleParameters, Map2D.h:37-43).  imgs may be
 * NULL (only the poses size the grid when thread=0; with thread=1 frames
 * that carry an image are queued and rendered first, Map2D.cpp:42).        */
int     pf_prepare(pf_map* m, const double plane[7], const double cam[6],
                   int n, const pf_image* imgs, const double* poses7);
/* Map2D::feed(img, pose), MultiBandMap2DCPU.cpp:288-309.  Host BGR8 (or BGRA8) frame; the
 * rows are copied to HBM as they lie (img->step is kept) by one blocking linear H2D copy, so
 * the caller may release its pixels when feed returns (the reference keeps a refcounted
 * cv::Mat instead).
 * When HBM runs out (a tile slab, the frame workspace or a frame slot cannot be allocated) the feed that meets it
 * returns 0 with the reason in pf_last_error() and costs that keyframe alone: nothing of it is in the map or in the
 * cull's bounds, the tiles it created before the failure stay as tiles without pyramid, keyframes fed before and
 * after it are fused exactly as if it had never been fed, and the same keyframe may be fed again once memory is back.
 * With a lookahead the tiles and the workspace of a keyframe are allocated when it is admitted, inside its own feed
 * call, so this holds there as well.  What can still fail when a waiting keyframe is rendered later (a launch, the
 * one-off weight plane) is met by the call that renders it: a pf_feed returns 0 although its own keyframe is in (to
 * feed it again is harmless: the select is idempotent), a reader returns its data.  Every keyframe lost either way is
 * counted (pf_stats_failed) and reported by the next pf_sync; a frame that never got its slot in HBM was not
 * accepted and is not.                                                                                           */
int     pf_feed(pf_map* m, const pf_image* img, const double pose[7]);
/* Same, frame already resident in HBM (img->data is a device pointer that
 * must stay valid -- and unchanged -- until pf_sync: the frame is read when its keyframe is rendered, which with
 * pf_options.lookahead = n may be n feeds later; a caller that cycles through a ring of device buffers without
 * pf_sync needs more than n + 1 of them, or sets lookahead to 0).  thread=0 maps only.                          */
int     pf_feed_device(pf_map* m, const pf_image* img, const double pose[7]);
/* Test hook (no reference counterpart): the bytes of the host frame most recently copied by pf_feed / pf_prepare,
 * read back from HBM -- (rows-1)*step + cols*channels of them.  Returns the byte count (out may be NULL to query it),
 * -1 when there is none.  Lets a test prove that a row-padded frame arrived byte for byte.                        */
long    pf_debug_read_last_frame(pf_map* m, void* out, size_t cap);
/* Diagnostics (PF_STAMP=1 selects a stamped instantiation of the level kernel; tools/stamp_phases.py): in-kernel clock
 * stamps of the most recent launch, 8 uint64 per workgroup.  Returns the workgroup count.                            */
int     pf_debug_phase_stamps(unsigned long long* out, int cap_blocks);
/* PF_STAMP=1 builds only: per pyramid level, pixels the max-weight select looked at (out[2*level]) and pixels that won
 * (out[2*level+1]) since the last reset; out holds 18 values.  Counts the useful tile bytes of a launch. */
int     pf_debug_select_counts(unsigned long long* out, int reset);
/* Map2D::queueSize(), MultiBandMap2DCPU.h:110-113: frames in the feed queue (cap 20, drop-oldest).  Keyframes the render thread has
 * taken out of it and holds for the cull's lookahead are not counted: they no longer occupy a place in the queue and cannot be dropped. */
unsigned pf_queue_size(pf_map* m);
/* drain the feed queue, render the keyframes that wait for the cull's lookahead (pf_options.lookahead) and wait for the
 * device stream (no reference counterpart: the reference is synchronous on the CPU).
 * Returns 0 ONCE, with the message of the newest failure in pf_last_error() of the calling thread, when an accepted keyframe was
 * lost to a failure (an allocation, a launch) since the previous pf_sync -- inside a pf_feed (which returned 0 then), while a
 * reader rendered what waited, or on the render thread of a thread=1 map, whose pf_feed cannot know.  The queue is drained and
 * the device waited for all the same, so the next pf_sync returns 1 unless more was lost; pf_stats_failed counts the keyframes
 * and pf_debug_render_log names the ones that are in.
 * The rule behind it: a keyframe enters the bounds that later keyframes are culled against only when nothing that needs memory
 * is left of its render -- its tiles exist and the workspace holds its canvas -- so an allocation failure never leaves cells that
 * were skipped for a keyframe that is not there.  A failure of the render itself after that (a launch error) loses the keyframe
 * as well, and cells of its canvas may then lack pixels of keyframes admitted after it: that is never silent -- this call
 * returns 0 and the count moves -- and the caller should rebuild the map.
 * The readers (tile access, blend, save, statistics, pf_debug_*) render what waits, ignore such a failure and return their data
 * of the map as it is; the failure stays pending for pf_sync.                                                                  */
int     pf_sync(pf_map* m);
/* Map2D::save(filename), MultiBandMap2DCPU.cpp:779-847.  Writes PNG (.png),
 * JPEG (.jpg / .jpeg, either case: quality 95, 4:2:0, cv::imwrite's default;
 * the collapsed mosaic is encoded on the GPU and only the stream comes back;
 * a mosaic of more than 65535 pixels a side returns 0 and writes no file),
 * a tiled pyramid TIFF (.tif / .tiff, either case: pf_save_tiff at quality
 * 95, classic unless the file needs BigTIFF; no limit on the mosaic's side),
 * else binary PPM.                                                         */
int     pf_save(pf_map* m, const char* filename);
/* save("x.tif") with what pf_save cannot carry: the tiles' JPEG quality and a flag that forces BigTIFF.  The file is
 * pf_tiff_write_bgr(filename, <the mosaic pf_save_to_memory returns>, quality, Result.BackGroundColor, T, force_bigtiff) with
 * T = the affine pixel (column, row) -> plane coordinates in metres: x = min.x + (tile_x0 - off_x) * eleSize + column *
 * lengthPixel, y = min.y + (tile_y0 - off_y) * eleSize + row * lengthPixel (pf_grid's geo and dims, pf_save_to_memory's origin
 * tile; row-major 4 x 4, z = 0).  Multi-band maps: overview chain, empty test and tile encode run on the GPU on the mosaic where the
 * collapse left it (csrc/overview.hip, jpeg_encode.hip); only flags, offsets and streams cross to the host.  Any file name.  */
int     pf_save_tiff(pf_map* m, const char* filename, int quality, int force_bigtiff);
/* pf_save_tiff with a transparency mask behind every image: the file is pf_tiff_write_bgr_masked(filename, bgr, ..., mask, ...,
 * quality, Result.BackGroundColor, T, force_bigtiff) of the bgr and mask pf_save_to_memory_mask returns and pf_save_tiff's T.
 * Covered = the level-0 weight of the pixel is not 0 (exactly where save() does not paint the background); tile slots of the
 * bounding box without a map tile are not covered.  Multi-band maps: the masks come from the weights where they lie in HBM
 * (csrc/coverage.hip, k_coverage_tiles, on the table the collapse uses) under the same hold of the map as the collapse.
 * Single-band maps: the host writer, covered = the tile's alpha byte (the winning weight) is not 0.  A map without content
 * returns 0.  pf_save never writes this file: ".tif" stays unmasked.                                                     */
int     pf_save_tiff_masked(pf_map* m, const char* filename, int quality, int force_bigtiff);
/* The file leg of save() alone: cv::imwrite(filename, result), MultiBandMap2DCPU.cpp:841.  8-bit BGR in,
 * PNG (8-bit RGB, deflate) when the name ends in .png/.PNG, JPEG (pf_jpeg_encode_bgr at quality 95) when it ends in
 * .jpg/.jpeg in either case, the pyramid TIFF (pf_tiff_write_bgr at quality 95, background 0, no geo tags) when it ends in
 * .tif/.tiff in either case, binary PPM (P6) otherwise.  No device needed. */
int     pf_write_image(const char* filename, const uint8_t* bgr, int rows, int cols);
/* The tiled pyramid TIFF of an orthomosaic (no reference counterpart: the reference writes one big .jpg / .png).  One
 * little-endian file, a pure function of (pixels, quality, bg, model_transform, force_bigtiff):
 *   images   image 0 = the rows x cols BGR picture (any size >= 1, `step` bytes per row, 0 = packed); image k >= 1 = the 2 x 2
 *            mean of image k - 1: ceil(r/2) x ceil(c/2), every channel (p00 + p01 + p10 + p11 + 2) >> 2, a missing last row or
 *            column repeating the one before it; the chain ends with the first image of at most 256 x 256.  NewSubfileType 0
 *            for image 0, 1 (reduced resolution) for the others; IFDs chained in that order.
 *   tiles    256 x 256, row-major; past the image its last column, then its last row, repeated.  Every tile is a complete
 *            baseline JPEG stream, the bytes of pf_jpeg_encode_bgr(tile, 256, 256, 0, quality): Compression 7, Photometric 6
 *            (YCbCr), YCbCrSubSampling 2 2, BitsPerSample 8 8 8, SamplesPerPixel 3, PlanarConfiguration 1, no JPEGTables.
 *   empty    a tile whose 256 x 256 filled pixels all equal the background colour (bg saturated to 8 bits, in all channels) is
 *            stored once: every such tile of every image has the same TileOffsets and TileByteCounts value.
 *   geo      model_transform != NULL: image 0 carries ModelTransformationTag (34264, the 16 doubles, row-major 4 x 4: pixel
 *            (column, row, 0, 1) -> model coordinates) and a GeoKeyDirectoryTag (34735) that says user-defined model type
 *            (1024 = 32767) and RasterPixelIsArea (1025 = 1), no CRS.
 *   layout   header; then per image, in order: its IFD (tags sorted), followed by the values that do not fit an entry, in tag
 *            order (BitsPerSample, TileOffsets, TileByteCounts, the doubles, the GeoKeys); then the empty tile's stream, if any
 *            tile is empty; then the streams of the other tiles, image by image, row-major.  Every IFD, value and stream starts
 *            on an even offset.  Classic TIFF (42, 32-bit offsets) when the file ends below 4 GiB, BigTIFF (43, 64-bit offsets,
 *            TileOffsets as LONG8) otherwise or when force_bigtiff is set.  (csrc/tiff_pyramid.hpp, tiff::layout: the one
 *            function both this writer and the GPU path place bytes by.)
 * Host code, no device.  0 + pf_last_error() on failure, and no file is left behind.                                        */
int     pf_tiff_write_bgr(const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, int quality, int bg,
                          const double model_transform[16], int force_bigtiff);
/* The same file, byte for byte, from an image of any size in device memory: the overview chain (csrc/overview.hip: each group of
 * three levels from one read of the level above), the empty test and the tile encode (csrc/jpeg_encode.hip, in bounded batches,
 * empty tiles skipped) run on the GPU in the order of `hip_stream` (a hipStream_t, NULL = the default stream); flags, offsets
 * and streams cross to the host, pixels do not.  The counterpart of pf_jpeg_encode_device; returns when the file is written. */
int     pf_tiff_write_device(const char* filename, const void* dev_bgr, int rows, int cols, size_t step, int quality, int bg,
                             const double model_transform[16], int force_bigtiff, void* hip_stream);
/* The masked pyramid TIFF: the file of pf_tiff_write_bgr for the same pixels, quality, bg, model_transform and force_bigtiff, plus a
 * TIFF 6.0 transparency mask behind every image, so that a reader can tell "no data" from a pixel of the background colour.
 *   masks    mask: a byte per pixel, non-zero = covered, `mask_step` bytes per row (0 = packed).  M_0[y, x] = 1 where the pixel is
 *            covered; M_k+1[y, x] = the OR of the 2 x 2 block of M_k, a missing last row or column repeating the one before it
 *            (the geometry of the colour chain): a pixel of an overview is opaque if any pixel under it is.
 *   IFDs     chained image 0, mask 0, image 1, mask 1, ...; the colour IFDs carry the tags of the unmasked file.  A mask IFD
 *            (tags sorted): NewSubfileType (254) 4 for mask 0 and 5 for the others, ImageWidth / ImageLength of its image,
 *            BitsPerSample 1 (count 1), Compression 1, Photometric 4 (transparency mask), SamplesPerPixel 1,
 *            PlanarConfiguration 1, TileWidth / TileLength 256, TileOffsets, TileByteCounts (every entry 8192).  No FillOrder: the
 *            default, most significant bit first, holds.
 *   tiles    a mask tile is 256 rows of 32 bytes, uncompressed; bit 7 of byte 0 is column 0; bits past the image are 0.
 *   sharing  the mask tiles whose 65 536 bits are all 0 are stored once, those whose bits are all 1 are stored once, every other
 *            mask tile on its own.  The colour streams, the colour empty test and the shared empty stream are the unmasked file's.
 *   layout   header; all IFDs with their out-of-line values, in chain order; the shared empty stream, if any; the shared all-zero
 *            mask tile, if any; the shared all-one mask tile, if any; the colour streams, image by image; the other mask tiles,
 *            image by image, row-major.  Everything starts on an even offset; classic TIFF unless the file needs BigTIFF or
 *            force_bigtiff is set.  (tiff::layout_as again: with no mask it places the bytes of pf_tiff_write_bgr.)
 * Host code, no device.  0 + pf_last_error() on failure (no name, image or mask, a step smaller than a row, a file that cannot be
 * written), and no file is left behind.                                                                                    */
int     pf_tiff_write_bgr_masked(const char* filename, const uint8_t* bgr, int rows, int cols, size_t step,
                                 const uint8_t* mask, size_t mask_step, int quality, int bg,
                                 const double model_transform[16], int force_bigtiff);
/* The same file, byte for byte, from an image and a mask (a byte per pixel) of any size in device memory: pf_tiff_write_device with
 * the masks made beside the colour chain (csrc/coverage.hip: k_coverage_bytes packs level 0, k_mask_overview ORs every further
 * level from the bit plane above, per-tile "all zero" / "all one" flags travel with the colour flags); only the mask tiles that
 * are neither are gathered and cross to the host, no plane does.  Refuses what pf_tiff_write_device refuses. */
int     pf_tiff_write_device_masked(const char* filename, const void* dev_bgr, int rows, int cols, size_t step,
                                    const void* dev_mask, size_t mask_step, int quality, int bg,
                                    const double model_transform[16], int force_bigtiff, void* hip_stream);
/* The lossless tile codec (csrc/deflate_rle.hpp, the format's one definition): a tile of 256 x 256 BGR pixels (`step` bytes per
 * row, 0 = packed) as one complete zlib stream that any inflater reads.
 *   bytes    N = 196 608 predicted bytes: RGB order, 768 a row; TIFF Predictor 2: pixel 0 of a row as it is, every later sample
 *            minus the same channel of the pixel before it, mod 256.
 *   stream   78 01 | 16 deflate blocks, joined bit by bit as RFC 1951 has it | zero bits up to a byte | Adler-32 of the N
 *            predicted bytes, big-endian.
 *   blocks   block b covers rows 16 b .. 16 b + 15 = 12 288 bytes; only block 15 has BFINAL.  A block is dynamic (BTYPE 2) when its
 *            bits (header, tokens, end-of-block) are no more than those of storing it (BTYPE 0) at the bit it begins at: 3 bits,
 *            zero bits up to a byte, LEN, NLEN, the bytes; else it is stored.  No stream is longer than N + 5 * 16 + 6 bytes.
 *   tokens   distance 1 only.  A maximal run of equal bytes inside a block: its first byte is a literal -- unless the run begins
 *            the block, the block is not the tile's first and the last byte of the block before has the run's value: then no
 *            literal is taken.  Of the R bytes that remain: matches of 258 while R >= 258, then one match of the rest if it is
 *            >= 3, else literals.  No token spans two blocks.  Length 258 is code 285.
 *   codes    literal / length code: lengths from the block's counts, end-of-block counted once, by the length builder below with
 *            limit 15.  Distance code: two codes of length 1 (HDIST = 1); distance 1 is code 0, the bit 0.  HLIT = max(257, last
 *            used symbol + 1) - 257.  The HLIT + 257 lengths and the distance code's {1, 1} are run-length coded as ONE sequence,
 *            greedily: a run of r zeros: 18 (up to 138) while r >= 11, then 17 if r >= 3, then single zeros; a run of r equal
 *            lengths v > 0: v, then 16 (up to 6) while what remains is >= 3, then v for each that remains.  The code-length code:
 *            the builder with limit 7 on the counts of those symbols; HCLEN drops trailing zeros of the order 16 17 18 0 8 7 9 6
 *            10 5 11 4 12 3 13 2 14 1 15, never below 4.  Canonical codes as RFC 1951 3.2.2.
 *   builder  pf_deflate_code_lengths(freq, n, max_len, out), 2 <= n <= 288, max_len <= 15, 2^max_len >= n: a count of 0 gives
 *            length 0.  One used symbol: it gets length 1, and so does symbol 0 (symbol 1 if the used one is 0).  Else: the
 *            used symbols sorted by (count, index) ascending; a Huffman tree by two queues (the sorted leaves; the inner nodes in
 *            the order they are made), each step taking twice the lighter head, the leaf when both weigh the same; the leaves'
 *            depths counted per length, depths past max_len counted as max_len; while the Kraft sum (in units of 2^-max_len)
 *            exceeds 1: one code less of length max_len, and the longest length below max_len that has a code gives one up for two
 *            of the next length; then lengths are dealt out in increasing order from the most frequent end of the sorted list.
 * pf_deflate_tile_bgr: host, one tile.  out = NULL: *len = the bound above.  Else *len = the stream's length; 0 if cap is smaller.
 * pf_deflate_tiles_device: n tiles anywhere in one device allocation (tile i begins byte_offsets[i] >= 0 bytes behind dev_base, rows
 * of `step` bytes, all 256 x 256 pixels inside the allocation), encoded on the GPU (csrc/deflate_encode.hip), byte-equal to the
 * host encoder; offsets[0..n] = where stream i begins among the streams laid back to back; out (may be NULL: offsets only) takes
 * them when cap >= offsets[n].  Only streams and offsets cross to the host.                                                    */
int     pf_deflate_tile_bgr(const uint8_t* tile, size_t step, uint8_t* out, size_t cap, size_t* len);
int     pf_deflate_tiles_device(const void* dev_base, int n, const long long* byte_offsets, size_t step, uint8_t* out, size_t cap,
                                size_t* offsets, void* hip_stream);
int     pf_deflate_code_lengths(const uint32_t* freq, int n, int max_len, uint8_t* out);
/* The lossless pyramid TIFF: the file of pf_tiff_write_bgr (mask == NULL) or pf_tiff_write_bgr_masked with every colour tile a
 * stream of the codec above instead of a JPEG one.  The colour IFDs carry Compression 8 (Adobe Deflate), PhotometricInterpretation
 * 2 (RGB), Predictor (317, between 284 and 322) = 2 and no YCbCrSubSampling; the shared empty stream is the codec applied to a tile
 * of the background colour.  Images, overviews, tile order, empty tiles, masks, geo tags, even offsets and the classic / BigTIFF
 * choice are those of the JPEG file (the same tiff::layout_as).  Reading it back gives image k exactly.  Host code, no device. */
int     pf_tiff_write_bgr_lossless(const char* filename, const uint8_t* bgr, int rows, int cols, size_t step,
                                   const uint8_t* mask, size_t mask_step, int bg,
                                   const double model_transform[16], int force_bigtiff);
/* The same file, byte for byte, from an image (and a mask, or NULL) in device memory: pf_tiff_write_device[_masked] with the tiles
 * through csrc/deflate_encode.hip. */
int     pf_tiff_write_device_lossless(const char* filename, const void* dev_bgr, int rows, int cols, size_t step,
                                      const void* dev_mask, size_t mask_step, int bg,
                                      const double model_transform[16], int force_bigtiff, void* hip_stream);
/* A map's mosaic as that file, under any name: pf_tiff_write_bgr_lossless of the pixels (and, masked != 0, the mask)
 * pf_save_to_memory[_mask] returns, Result.BackGroundColor and pf_save_tiff's T.  Multi-band maps encode on the GPU from the mosaic
 * where the collapse left it, under the one hold of the map; single-band maps take the host writer.  pf_save("x.tif") and
 * pf_save_tiff keep writing JPEG tiles. */
int     pf_save_tiff_lossless(pf_map* m, const char* filename, int masked, int force_bigtiff);
/* The PNG of save_png (csrc/png_encode.hpp, the format's one definition): an image of rows x cols BGR pixels (`step` bytes per row,
 * 0 = packed) and, optionally, a mask (a byte per pixel, `mask_step` bytes per row, 0 = packed) as one complete PNG file that any
 * reader takes.
 *   file     signature | IHDR: 8 bits, colour type 2 (RGB), or 6 (RGBA) when a mask is given, compression 0, filter method 0, no
 *            interlace | IDAT chunks | IEND.  No other chunks.
 *   F        the filtered stream: for every row the filter-type byte 1 (Sub), then the samples in R, G, B (, A) order, each minus
 *            the same channel of the pixel to its left, mod 256; the row's first pixel as it is.  A = 255 where the mask byte is not
 *            0, else 0; the colour under A = 0 is the image's.  N = rows * (1 + cols * bpp) bytes, bpp 3 or 4.
 *   blocks   F is cut into deflate blocks of 12 288 stream bytes, row ends ignored; the last is shorter.  Tokens, codes and the
 *            length builder are those of pf_deflate_tile_bgr above, history carrying across blocks (the run that begins a block
 *            which is not the stream's first takes no literal when the byte before the block has its value).  A block is dynamic
 *            when its bits are no more than those of storing it at the bit it begins at -- 3 bits, zero bits up to a byte, LEN,
 *            NLEN, its own bytes -- else it is stored.  Only the stream's last block has BFINAL.
 *   segments sixteen blocks, joined bit by bit.  Every segment but the last ends with an empty stored block (BFINAL 0: three zero
 *            bits, zero bits up to a byte, 00 00 FF FF), so every segment begins on a byte.
 *   chunks   one segment is one IDAT chunk.  The first begins with the zlib header 78 01, the last ends with zero bits up to a byte
 *            and the Adler-32 of F, big-endian.  Chunk CRCs: CRC-32, polynomial 0xEDB88320 reflected, over type and data.
 *   bound    no file is longer than N + 5 per block + (5 + 12) per segment + 51 bytes.  Offsets and lengths that address the stream or
 *            the file are 64-bit; refused before anything is written: a row of F past 2^31 - 1 bytes, more than 2^31 - 1 blocks.
 * pf_png_encode_bgr: host code, no device.  out = NULL: *len = the bound.  Otherwise *len = the file's length, and the file is in
 * `out` if it fits `cap` (0 + pf_last_error() if not; nothing is written then).  0 also for no image, sizes that are not positive and
 * a step smaller than a row (*len = 0 then).
 * pf_png_encode_device: the same file, byte for byte, from an image (and a mask, or NULL) in device memory, made on the GPU
 * (csrc/png_encode.hip), chunk CRCs and the Adler-32 included; the passes run in the order of hip_stream and the call returns when the
 * file is in `out`.  The same conventions.
 * The checksum functions are the format's own (csrc/png_encode.hpp), host code: pf_png_crc32 continues crc (0 at the start) over
 * data; pf_png_crc32_combine gives the CRC of A || B from those of A and B and the length of B (crc_a times x^(8 len_b) mod P, plus
 * crc_b); pf_png_adler32 is built block by block from the sums S = sum x_k and T = sum (n - k) x_k the kernels make;
 * pf_png_adler32_combine gives the Adler-32 of A || B likewise. */
int      pf_png_encode_bgr(const uint8_t* bgr, int rows, int cols, size_t step, const uint8_t* mask, size_t mask_step,
                           uint8_t* out, size_t cap, size_t* len);
int      pf_png_encode_device(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step,
                              uint8_t* out, size_t cap, size_t* len, void* hip_stream);
uint32_t pf_png_crc32(uint32_t crc, const uint8_t* data, size_t len);
uint32_t pf_png_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
uint32_t pf_png_adler32(const uint8_t* data, size_t len);
uint32_t pf_png_adler32_combine(uint32_t adler_a, uint32_t adler_b, uint64_t len_b);
/* A map's mosaic as that file, under any name: pf_png_encode_bgr of the pixels pf_save_to_memory returns, or, masked != 0, of the
 * pixels and the mask pf_save_to_memory_mask returns -- an RGBA file whose alpha is 0 exactly where pf_save paints the background.
 * Multi-band maps encode on the GPU from the mosaic (and the coverage) where the collapse left them, under the one hold of the map;
 * the complete file crosses to the host once.  Single-band maps take the host encoder, covered meaning the tile's alpha byte is not
 * 0.  A map without content returns 0.  pf_save("x.png") keeps its route and its bytes. */
int      pf_save_png(pf_map* m, const char* filename, int masked);
/* cv::imencode(".jpg") / the JPEG leg of cv::imwrite of OpenCV 2.4.9: baseline JPEG, byte for byte what libjpeg writes after
 * jpeg_set_defaults, JCS_RGB input and jpeg_set_quality(quality, TRUE) -- JFIF 1.01, 4:2:0, the Annex K tables, one interleaved
 * scan, integer colour conversion and ISLOW DCT.  bgr: rows x cols 8-bit BGR, `step` bytes per row (0 = packed).  quality is
 * clamped to 1...100.  out = NULL: *len = an upper bound of the stream for any content.  Otherwise *len = the stream's length,
 * and the stream is in `out` if it fits `cap` (0 + pf_last_error() if not; nothing is written then).  Host code, no device. */
int     pf_jpeg_encode_bgr(const uint8_t* bgr, int rows, int cols, size_t step, int quality, uint8_t* out, size_t cap, size_t* len);
/* The same encoder on the GPU (csrc/jpeg_encode.hip), byte-equal to pf_jpeg_encode_bgr, for an image in device memory: the
 * counterpart of pf_jpeg_decode_device.  The passes run in the order of `hip_stream` (a hipStream_t, NULL = the default stream);
 * only the stream crosses to the host, and the call returns when `out` (host memory, pinned or not) holds it. */
int     pf_jpeg_encode_device(const void* dev_bgr, int rows, int cols, size_t step, int quality, uint8_t* out, size_t cap, size_t* len, void* hip_stream);
/* Input side of the file driver: the reference reads each keyframe with cv::imread(imgfile), backup/map2dfusion.cpp:129-132
 * (8-bit BGR, EXIF orientation ignored as OpenCV 2.4.9 does).  JPEG (baseline, extended and progressive Huffman; grey or
 * YCbCr/RGB; libjpeg's default ISLOW IDCT, fancy upsampling and colour tables, byte-equal to libjpeg-turbo), PNG (non-interlaced;
 * grey replicated, palette looked up, alpha dropped, 16-bit samples cut to 8: IMREAD_COLOR's conversion) and binary PPM.
 * pf_image_info fills rows/cols; pf_read_image decodes into rows*cols*3 bytes.  pf_jpeg_* take the stream from memory.
 * Host code; no device needed.  0 + pf_last_error() on anything unsupported or malformed.                              */
int     pf_image_info(const char* filename, int* rows, int* cols);
int     pf_read_image(const char* filename, uint8_t* bgr, int rows, int cols);
int     pf_jpeg_info(const uint8_t* data, size_t len, int* rows, int* cols, int* components);
int     pf_jpeg_decode_bgr(const uint8_t* data, size_t len, uint8_t* bgr, int rows, int cols);
/* The same decode on the GPU (csrc/jpeg_device.hip), byte-equal to pf_jpeg_decode_bgr: the calling thread parses the markers;
 * sequential one-scan streams (with or without restart intervals) are Huffman-decoded on the GPU too (a self-synchronising parallel pass,
 * csrc/jpeg_huff_par.hpp), the others on the calling thread; kernels do libjpeg's dequantise + ISLOW IDCT, fancy upsampling and
 * colour conversion.  dev_bgr: rows*cols*3 bytes of device memory, complete in the order of `hip_stream`
 * (a hipStream_t, NULL = the default stream); the call returns when the work is queued.                               */
int     pf_jpeg_decode_device(const uint8_t* data, size_t len, void* dev_bgr, int rows, int cols, void* hip_stream);
/* Diagnostics: out = { frames whose Huffman pass ran on the GPU, frames that fell back to the host's serial pass after trying,
 * launches the most recent GPU pass took } of the map's decoder (m = NULL: of pf_jpeg_decode_device's).  Sequential one-scan streams,
 * with or without restart intervals, take the GPU pass (csrc/jpeg_huff_par.hpp); PF_JPEG_HOST_HUFFMAN=1 keeps every stream on the host.  */
void    pf_debug_jpeg_huffman(pf_map* m, long long out[3]);
/* Diagnostics of the last pyramid TIFF made on the GPU (JPEG or lossless tiles) by the map m, or, m == NULL, by the process-wide
 * writer behind pf_tiff_write_device* on the current device: out = { tiles of all images, the tiles among them found empty on the
 * GPU (they share one stream and are not encoded), bytes of device memory held for levels and flags }; zeros before the first. */
void    pf_debug_tiff_counts(pf_map* m, long long out[3]);
/* Map2D::feed(cv::imread(imgfile), pose) in one call (backup/map2dfusion.cpp:129-135 + Map2DFusion.cpp:313-327): markers and
 * Huffman on the calling thread, then the frame is finished on the GPU straight into the slot in HBM a host frame would have
 * been uploaded to, and queued (thread=1) or rendered (thread=0) from there.  Returns what pf_feed returns.             */
int     pf_feed_jpeg(pf_map* m, const uint8_t* data, size_t len, const double pose[7]);
/* n keyframes at once: their Huffman passes run side by side on `threads` host threads (0: one per frame; batches of 16), then
 * the frames are uploaded, finished on the GPU and fed in the order given -- the mosaic is the one n pf_feed_jpeg calls build.
 * results[i] (may be NULL) = what pf_feed_jpeg returns for frame i; returns the number of frames fed.                  */
int     pf_feed_jpeg_batch(pf_map* m, int n, const uint8_t* const* data, const size_t* len, const double* poses7, int threads, int* results);
/* --- raw frames: what a hardware video decoder, a machine-vision camera or a thermal camera delivers, converted to BGR8 on the GPU
 * (DESIGN.md "Raw frames"; no reference counterpart: the reference takes CV_8UC3 alone).  8-bit samples.
 *   PF_RAW_GREY        plane 0: a byte per pixel; B = G = R = the byte (CV_GRAY2BGR).
 *   PF_RAW_NV12        plane 0: Y; plane 1: interleaved U, V pairs, one pair per 2 x 2 block of pixels, `cols` bytes a chroma row.
 *   PF_RAW_NV21        the same with V first.
 *   PF_RAW_I420        plane 0: Y, plane 1: U, plane 2: V, cols / 2 bytes a chroma row (YV12: hand the two chroma pointers over swapped).
 *                      The three are cv::cvtColor(CV_YUV2BGR_NV12 / _NV21 / _I420) of OpenCV 2.4.9: BT.601 studio range, 20-bit integer
 *                      arithmetic, no chroma interpolation.  rows and cols even.
 *   PF_RAW_BAYER_xxxx  plane 0: the mosaic, a byte per pixel, named by the first two pixels of row 0 (RGGB: R G / G B).  Bilinear: on a red
 *                      or blue site green = (N + S + W + E + 2) >> 2 and the opposite colour = (NW + NE + SW + SE + 2) >> 2; on a green site
 *                      the colour of its row neighbours = (W + E + 1) >> 1, of its column neighbours = (N + S + 1) >> 1.  The one-pixel
 *                      frame takes the value of the nearest interior pixel, out(y, x) = interior(clamp(y, 1, rows - 2), clamp(x, 1,
 *                      cols - 2)).  At least 3 x 3, odd sizes allowed.  This project's specification: not claimed byte-equal to OpenCV.
 * rows, cols: of the IMAGE.  plane[k]: separate allocations are fine; step[k]: bytes between the rows of plane k, 0 = packed; planes a
 * format does not use are NULL.
 * pf_raw_to_bgr: host to host, no GPU needed.  bgr: rows x cols x 3, bgr_step bytes a row (0 = packed); nothing else is written.
 * pf_raw_to_bgr_device: planes and dev_bgr are device pointers of one device; the kernel is queued on hip_stream (a hipStream_t, NULL =
 * the default stream) and the call returns without waiting.  Byte-equal to pf_raw_to_bgr.
 * Refused (0, the reason in pf_last_error(), nothing written): an unknown format, a missing plane, a step below the row, odd YUV sizes,
 * Bayer below 3 x 3, a plane or a BGR image of 2 GiB or more.
 * pf_feed_raw: pf_feed of the BGR8 frame the conversion yields, from host planes: each plane crosses to HBM as it lies (1 or 1.5 bytes a
 * pixel instead of 3) by one blocking copy and is converted there into the frame's slot, so the planes may be released when the call
 * returns.  Size check (against the input camera, if one is set: the frame is then converted, then undistorted), rejected / dropped
 * counting, queue (thread=1), lookahead, cull and the cost of an allocation failure are pf_feed's.
 * pf_feed_raw_device: the same from planes that already lie in HBM (a decoder's output surface); thread=0 maps only.  The conversion is
 * queued on the map's stream INSIDE the call, not when the keyframe is rendered: the planes must stay valid and unchanged until that
 * kernel has run -- until pf_sync, for a caller without a handle on the map's stream.
 * Not provided: raw frames in pf_prepare's frame list or through pf_dist_feed; BT.709 or full-range matrices; 10 / 12 / 16-bit samples;
 * any demosaic other than bilinear.                                                                                                  */
enum { PF_RAW_GREY = 1, PF_RAW_NV12 = 2, PF_RAW_NV21 = 3, PF_RAW_I420 = 4,
       PF_RAW_BAYER_RGGB = 8, PF_RAW_BAYER_BGGR = 9, PF_RAW_BAYER_GRBG = 10, PF_RAW_BAYER_GBRG = 11 };
typedef struct pf_raw_frame { int format, rows, cols; const void* plane[3]; size_t step[3]; } pf_raw_frame;
int     pf_raw_to_bgr(const pf_raw_frame* src, uint8_t* bgr, size_t bgr_step);
int     pf_raw_to_bgr_device(const pf_raw_frame* src, void* dev_bgr, size_t bgr_step, void* hip_stream);
int     pf_feed_raw(pf_map* m, const pf_raw_frame* src, const double pose[7]);
int     pf_feed_raw_device(pf_map* m, const pf_raw_frame* src, const double pose[7]);
/* save() without the file: whole-mosaic collapse into caller memory.  Call
 * with bgr=NULL to query rows/cols/origin tile.                            */
int     pf_save_to_memory(pf_map* m, uint8_t* bgr, int* rows, int* cols, int* tile_x0, int* tile_y0);
/* The mosaic and its coverage of ONE moment: bgr as pf_save_to_memory gives it, mask rows x cols bytes, 255 where weights[0] != 0,
 * else 0.  bgr == NULL && mask == NULL: the extent alone.  Either of the two may be NULL once the extent is known.       */
int     pf_save_to_memory_mask(pf_map* m, uint8_t* bgr, uint8_t* mask, int* rows, int* cols, int* tile_x0, int* tile_y0);

/* --- MultiBandMap2DCPU::Ele tile surface (MultiBandMap2DCPU.h:32-51) ---- */
int     pf_num_levels(pf_map* m);                        /* bandNum+1          */
int     pf_pyramid_type(pf_map* m);                      /* PF_16SC3 | PF_32FC3 */
/* MultiBandMap2DCPUData geometry (.h:61-69): dims={w,h,off_x,off_y},
 * geo={min.x,min.y,max.x,max.y,eleSize,lengthPixel}.  Tile coordinates in
 * this API are stable: dense grid index + off (they survive spreadMap).    */
int     pf_grid(pf_map* m, int dims[4], double geo[6]);
int     pf_tile_count(pf_map* m);
int     pf_tile_coords(pf_map* m, int* xy, int cap);
/* Ele::pyr_laplace[level] / Ele::weights[level]: D2H copy of one level.    */
int     pf_get_tile_level(pf_map* m, int ix, int iy, int level, void* lap, float* w);
/* Map2DCPU::Map2DCPUEle::img (Map2DFusion/Map2DCPU.h): the 256x256 BGRA tile of a
 * TypeCPU / TypeGPU map (alpha = winning weight byte).                      */
int     pf_get_tile_bgra(pf_map* m, int ix, int iy, uint8_t* bgra256);
/* Ele::blend(neighbors), .cpp:77-146: raw result in the pyramid type.      */
int     pf_blend_tile_raw(pf_map* m, int ix, int iy, void* out);
/* Ele::updateTexture's pixels, .cpp:149-160: blend -> BGR8 256x256.        */
int     pf_blend_tile(pf_map* m, int ix, int iy, uint8_t* bgr256);
/* batch form of the draw() loop (.cpp:705-742): blend every tile whose
 * Ischanged flag is set, clear the flags; xy/bgr sized by cap tiles.       */
int     pf_blend_changed(pf_map* m, int* xy, uint8_t* bgr, int cap);
/* Ele::blend + the 8U view for a caller-chosen list of n tiles (xy = n pairs ix, iy), Ischanged left alone: what a viewer that
 * re-draws a region calls.  bgr: n x 256 x 256 x 3; a tile without pyramid leaves its 196 608 bytes untouched.  One launch
 * per 1024 tiles.  Returns 1 / 0.                                           */
int     pf_blend_tiles(pf_map* m, const int* xy, int n, uint8_t* bgr);
/* pf_blend_tiles whose results leave as n independent JPEG streams (256 x 256 each, what pf_jpeg_encode_bgr gives for the tile),
 * packed back to back: stream i is out[offsets[i] .. offsets[i + 1]), offsets has n + 1 entries.  The tiles stay in HBM; one
 * encode pass per blend launch covers all its tiles.  A tile without pyramid gives an empty range.  0 + pf_last_error() when the
 * streams do not fit `cap` (pf_jpeg_encode_bgr's bound for 256 x 256, times n, always fits). */
int     pf_blend_tiles_jpeg(pf_map* m, const int* xy, int n, int quality, uint8_t* out, size_t cap, size_t* offsets);
/* --- reduced-resolution views: the pyramid collapsed from the top and stopped at level k -------------------------------
 * L = pf_num_levels - 1, E = 256 >> k, 0 <= k <= L.  The blended Gaussian level k: a low-passed 1 / 2^k view with the same seam
 * blending, made from 4^-k of the tile bytes.  It is Ele::blend / save() of a map whose tiles are E pixels wide with levels
 * k .. L: the halo of level i stays 1 << (L - i), the crop is [1 << (L - k), +E), and the mask (0 in a tile, the background
 * colour in the mosaic) comes from the LEVEL-k weights.  k = L is the masked top level.  k = 0 is pf_blend_tiles /
 * pf_blend_tile_raw / pf_blend_changed / pf_save_to_memory, byte for byte.  Each returns 0 with the reason in pf_last_error() and
 * touches no output for k < 0, k > L, k > 0 on a TypeCPU / TypeGPU map (no pyramid) and k > 0 on a sharded map (shard_count > 1).
 *
 * pf_blend_tiles at level k: bgr n x E x E x 3 bytes and / or raw n x E x E x 3 of the pyramid type (pf_pyramid_type; a TypeCPU /
 * TypeGPU map at level 0: four bytes a pixel, pf_get_tile_bgra's); either may be NULL.  A tile without pyramid leaves its range
 * untouched, Ischanged is left alone.                                                                                      */
int     pf_blend_tiles_level(pf_map* m, const int* xy, int n, int level, uint8_t* bgr, void* raw);
/* pf_blend_changed at level k: the same tiles, the same flag clearing and return value; bgr sized by cap x E x E x 3.     */
int     pf_blend_changed_level(pf_map* m, int level, int* xy, uint8_t* bgr, int cap);
/* pf_save_to_memory at level k, the same two calls: rows = tiles_y * E, cols = tiles_x * E, the same origin tile.          */
int     pf_save_to_memory_level(pf_map* m, int level, uint8_t* bgr, int* rows, int* cols, int* tile_x0, int* tile_y0);
/* Page-locked host memory for the output side: results written into such a buffer (pf_blend_changed, pf_blend_tiles,
 * pf_save_to_memory and their _level forms) are copied from HBM straight into it; any other buffer is filled through the library's own pinned
 * staging ring and a host copy (the counterpart of cv::Mat's allocator for the textures updateTexture hands to GL).       */
void*   pf_host_alloc(size_t bytes);
void    pf_host_free(void* p);
/* The text draw() hands to scommand.Call("MapWidget", ...) for a refreshed tile when Fuse2Google is set
 * (MultiBandMap2DCPU.cpp:744-757): "Map2DUpdate LastTexMat <lng lat 0 of the tile's top-left corner> <... bottom-right>".
 * Byte for byte the reference's string: tile corners rounded to float first (.cpp:709-712), plane * corner, then
 * pi::calcLngLatFromDistance around GPS.Origin (PIL/src/hardware/Gps/utils_GPS.cpp:133-160), every field through
 * std::to_string -- six decimals; the call site's setprecision(9) never reaches a number (GSLAM/core/Point.h:166-170).
 * pf_format_map_update: the pure function (grid minimum, tile edge in metres, dense tile index x, y as the draw() loop counts).
 * pf_map_update_command: the same for tile (ix, iy) of a prepared map (stable tile coordinates), with the reference's gate
 * `updated && !inborder`: 0 when the tile holds no pyramid yet, or lies on the rim of the dense grid while
 * HighQualityShow is on (one of its 3x3 neighbours falls outside, .cpp:730-735).  `Fuse2Google` itself is the caller's flag.
 * Both return the length written (without the terminating 0), 0 when nothing is to be sent or cap is too small. */
int     pf_format_map_update(const double plane[7], const double gps_origin[3], double min_x, double min_y, double ele_size,
                             int x, int y, char* out, int cap);
int     pf_map_update_command(pf_map* m, int ix, int iy, const double gps_origin[3], char* out, int cap);
/* pi::calcLngLatFromDistance (utils_GPS.cpp:133-160) alone */
void    pf_lnglat_from_distance(double lng1, double lat1, double dx, double dy, double* lng2, double* lat2);

/* --- north-up Web-Mercator map tiles (EPSG:3857, the XYZ / OSM slippy-map numbering z/x/y, 256 x 256 pixels), resampled on the GPU ---
 * What a web map, QGIS or a ground station loads as it is.  Every other output lives in the fitted ground plane's own frame; these
 * are placed on the globe by the plane pose and GPS.Origin, exactly as pf_format_map_update places a tile's corners.
 *
 * px2ll[6]: the affine from a CONTINUOUS mosaic pixel coordinate (column, row) to degrees, lng = P0 + P1 col + P2 row,
 * lat = P3 + P4 col + P5 row; pixel (i, j) covers [i, i + 1) x [j, j + 1) (RasterPixelIsArea, as the TIFF declares).
 * pf_webtiles_georef: px2ll of the mosaic pf_save_to_memory would report at that moment (its rows and cols are returned too):
 * pf_save_tiff's pixel -> plane metres, the plane pose (East = world x, North = world y), pf_lnglat_from_distance around gps_origin --
 * pf_webtiles_georef_compose is that chain alone, from the 16 doubles of the TIFF's ModelTransformationTag.  0 with the reason in
 * pf_last_error() for a map without content, a sharded map (shard_count > 1: gather with pf_dist_save_to_memory on rank 0 and hand
 * the mosaic to pf_webtiles_device) and a singular affine (a vertical plane).
 *
 * With n = 256 * 2^z, global pixel column c and row r have their centres at lng_c = (c + 0.5) / n * 360 - 180 and
 * lat_r = atan(sinh(pi (1 - 2 (r + 0.5) / n))) * 180 / pi.  pf_webtiles_plan: range = {tx0, ty0, tx1, ty1}, the inclusive range of
 * tiles the bounding box of the four image corners touches at zoom z, and -- A being the inverse of the 2 x 2 part of px2ll -- the tables
 * UX[c] = A00 (lng_c - P0) - 0.5, UY[c] = A10 (lng_c - P0) - 0.5 over the 256 (tx1 - tx0 + 1) columns and VX[r] = A01 (lat_r - P3),
 * VY[r] = A11 (lat_r - P3) over the 256 (ty1 - ty0 + 1) rows of the range: output pixel (c, r) samples the source at pixel-index
 * position (UX[c] + VX[r], UY[c] + VY[r]).  Refuses z outside 0 .. 24, a singular affine, a corner beyond 85.05 degrees of latitude
 * (nothing is written) and tables smaller than needed (cap_cols, cap_rows doubles each: the range alone is written and says what is
 * needed); with all four tables NULL it is asked for the range alone and returns 1.  pf_webtiles_native_zoom: the smallest z at which one source pixel spans at least 1 / sqrt 2 output pixel at the image
 * centre (sqrt |det| of d(global pixel) / d(source pixel)); -1 where pf_webtiles_plan would refuse.
 *
 * The tiles of zmax are sampled from the mosaic and its coverage: x0 = floor(sx), fx = floor((sx - x0) 256) (at most 255), the same
 * for y; four taps with weights (256 - fx, fx) x (256 - fy, fy); a tap counts when it lies inside the image and its mask is not 0;
 * den = the weights that count; 2 den < 65536: the background colour (bg saturated to 0 .. 255), uncovered; otherwise every channel
 * is (sum of w p + den / 2) / den, covered.  A tile of zoom z - 1 is made from its four children: a pixel is (sum + (k >> 1)) / k over
 * the k covered of the 2 x 2 pixels under it, covered when k > 0.  A tile without a covered pixel is not handed over and counts as
 * an absent child.  Every tile handed over carries its JPEG stream (byte-equal to pf_jpeg_encode_bgr(tile, 256, 256, 0, quality)), its
 * cover class (1: partly covered, 2: fully) and, partly covered, its mask: 8192 bytes, 32 a row, bit 7 of byte 0 = column 0, 1 = covered.
 * zmax < 0: the native zoom; zmin < 0: the first zoom, going down, at which the range is a single tile.  The pointers of a pf_webtile
 * are valid during the sink's call; the sink runs on the caller's thread while the library holds the map (pf_webtiles) or its device
 * encoder (pf_webtiles_device), so it must not call back into either; a sink that returns 0 stops the export, which then returns 0.
 * pf_webtiles_device: image (BGR8, step bytes a row, 0 = packed) and mask (a byte per pixel, mask_step a row) in device memory, the
 * work queued on hip_stream.  pf_webtiles: the map's mosaic of that moment -- drain, extent, collapse and coverage under one hold of
 * the map as for every save; a TypeCPU / TypeGPU map goes through its host mosaic and alpha mask.  pf_save_webtiles: dir/z/x/y.jpg, for a
 * partly covered tile dir/z/x/y.pbm beside it (P4, 1 = covered), and dir/tiles.json: bounds in degrees, minzoom, maxzoom and per zoom the
 * tile range and counts.  On failure it returns 0, names the tile in pf_last_error() and leaves what it wrote.
 * Device memory does not grow with the mosaic beyond a fixed batch (8 x 8 tiles of zmax and their three zooms of ancestors) plus the
 * tiles of the zooms <= zmax - 3.  pf_debug_webtiles_batch: test hook, the batch's edge in tiles (8, 4 or 2); returns the edge set. */
typedef struct pf_webtile {
    int z, x, y, cover;
    const uint8_t* jpeg;
    size_t jpeg_len;
    const uint8_t* mask8192;   /* NULL when the tile is fully covered */
    const uint8_t* bgr;        /* NULL unless pixels were asked for   */
} pf_webtile;
typedef int (*pf_webtile_sink)(void* user, const pf_webtile* t);   /* 0 stops the export */
int     pf_webtiles_georef(pf_map* m, const double gps_origin[3], double px2ll[6], int* rows, int* cols);
int     pf_webtiles_georef_compose(const double model_transform[16], const double plane[7], const double gps_origin[3], double px2ll[6]);
int     pf_webtiles_plan(const double px2ll[6], int rows, int cols, int z, int range[4], double* ux, double* uy, double* vx, double* vy,
                         long long cap_cols, long long cap_rows);
int     pf_webtiles_native_zoom(const double px2ll[6], int rows, int cols);
int     pf_webtiles_device(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step,
                           const double px2ll[6], int zmin, int zmax, int quality, int bg,
                           int want_pixels, pf_webtile_sink sink, void* user, void* hip_stream);
int     pf_webtiles(pf_map* m, const double gps_origin[3], int zmin, int zmax, int quality, int want_pixels, pf_webtile_sink sink, void* user);
int     pf_save_webtiles(pf_map* m, const char* dir, const double gps_origin[3], int zmin, int zmax, int quality);
int     pf_debug_webtiles_batch(int edge);
/* test / measurement hook: while on, HIP events bracket the sample kernel, the reduce kernel and the encoder of every export;
 * pf_debug_webtiles_timing_read: their milliseconds in the most recent export and the number of tiles it sampled */
void    pf_debug_webtiles_timing(int on);
void    pf_debug_webtiles_timing_read(double out4[4]);

/* --- views: the mosaic at any pan, zoom, rotation or camera pose, rendered on the GPU at the size of the caller's window (DESIGN.md
 * "Views") ---
 * S_k: the mosaic at pyramid level k as pf_save_to_memory_level(k) gives it; C_k its coverage, 255 where weights[k] != 0, else 0;
 * B G R C stacked as a 4-channel 8-bit image.  A view is cv::warpPerspective(S_k as BGRA, M0, Size(width, height), INTER_LINEAR,
 * BORDER_CONSTANT 0) with OpenCV 2.4.9's arithmetic; after the warp every pixel whose fourth channel is 0 gets bg_color in its three
 * colour channels; a 3-channel view is the first three channels of that.
 *
 * V[9] (row-major) takes plane metres to view pixels, (col, row, 1) ~ V (x, y, 1), in the frame of pf_prepare's plane and pf_grid's
 * geo: it stays valid when the grid grows.  A level-0 pixel index i lies at origin + i lengthPixel, a level-k index j over level-0
 * index 2^k j, so for a region whose first tile is (tx, ty)
 *     A_k = [[lp 2^k, 0, min.x + (tx - off_x) eleSize], [0, lp 2^k, min.y + (ty - off_y) eleSize], [0, 0, 1]],   M0 = V A_k.
 * level = 0 .. L is taken as given; level = -1 chooses k = clamp(floor(log2(max(s, 1))), 0, L), s the square root of |det| of the
 * Jacobian of (view pixel -> level-0 pixel) at the view's centre ((width - 1) / 2, (height - 1) / 2).
 * Only the tiles the view depends on are collapsed (pf_view_info.rect, .tiles): the cost follows the window, not the map; the
 * result is byte-equal to the warp of the whole mosaic.
 *
 * Refused (0, the reason in pf_last_error(), no output touched): a V that is not finite; a singular M0; a denominator that is zero or
 * changes sign over the view's four corners; width or height outside 1 .. 16384; a region of more than 32767 level-k pixels a side
 * (ask for a higher level); a TypeCPU / TypeGPU map; a sharded map (shard_count > 1); a map before pf_prepare.  A map without
 * content, or a view that misses the content, is not an error: bg_color everywhere, coverage 0, info.empty = 1. */
typedef struct pf_view_info {
    int    level;        /* the level the view was taken from */
    int    rect[4];      /* the tiles collapsed: first tile x, y (stable tile coordinates), tiles across, tiles down */
    int    window[4];    /* the level-k pixels the view can reach, inside rect: x0, y0, width, height */
    double M0[9];        /* level-k pixel of rect -> view pixel: what cv::warpPerspective is handed */
    double Minv[9];      /* its inverse by the closed-form adjugate: what the warp runs with */
    int    empty;        /* 1: no content under the view */
    int    tiles;        /* rect[2] * rect[3] */
} pf_view_info;
/* the plan alone, host code without a device or a map: dims[4], geo[6] as pf_grid gives them, num_levels as pf_num_levels,
 * extent = {first tile x, y, tiles across, tiles down} of the content (across or down 0: none). */
int     pf_view_plan(const double V[9], int width, int height, int level, const int dims[4], const double geo[6], int num_levels,
                     const int extent[4], pf_view_info* out);
/* The view of the map after every keyframe fed so far (keyframes that wait for the lookahead are rendered first; Ischanged flags are
 * left alone).  channels: 4 (B G R C) or 3; step: bytes between rows, 0 = packed; info may be NULL.
 * pf_render_view: into host memory (page-locked memory of pf_host_alloc is filled straight from HBM).
 * pf_render_view_device: into device memory of the map's device, left in HBM for a tracker; the work is queued on hip_stream when
 * one is given (the call returns once it is queued), else on the map's stream and complete on return.
 * pf_render_view_jpeg: the 3-channel view as one JPEG stream, encoded on the GPU -- only the stream crosses to the host; byte-equal
 * to pf_jpeg_encode_bgr of the 3-channel view.  out = NULL: *len = an upper bound for any content, nothing is rendered; otherwise
 * *len = the stream's length, and 0 + pf_last_error() when it does not fit cap. */
int     pf_render_view(pf_map* m, const double V[9], int width, int height, int level, int channels, uint8_t* out, size_t step, pf_view_info* info);
int     pf_render_view_device(pf_map* m, const double V[9], int width, int height, int level, int channels, void* dev_out, size_t step,
                              void* hip_stream, pf_view_info* info);
int     pf_render_view_jpeg(pf_map* m, const double V[9], int width, int height, int level, int quality, uint8_t* out, size_t cap, size_t* len,
                            pf_view_info* info);
/* Host-only helpers that make a V.  pf_view_of_extent: the whole content, axes as the map's, aspect kept, centred in width x height
 * (0: no content).  pf_view_from_pose: what a camera at pose_world7 sees -- cam6 = NULL: the camera of pf_prepare, and the view has
 * its size --: pf_footprint's four plane points taken to the image corners (0, 0), (w, 0), (0, h), (w, h) by
 * pf_perspective_transform, as they stand; 0 for a pose pf_feed would reject as oblique.  pf_view_from_lnglat: a north-up window
 * linear in degrees, (lng_w, lat_n) at the view's corner (0, 0) and (lng_e, lat_s) at (width, height) in web tiles' convention that
 * continuous coordinate = index + 0.5, through pf_webtiles_georef's chain inverted: a view and the web tiles of one map put a
 * coordinate on the same mosaic pixel.  (The TIFF's tag calls the extent's corner the corner of pixel 0, half a level-0 pixel from
 * the convention of the views, where it is the centre of pixel 0: DESIGN.md "Views".) */
int     pf_view_of_extent(pf_map* m, int width, int height, double V[9]);
int     pf_view_from_pose(pf_map* m, const double pose_world7[7], const double* cam6_or_null, double V[9]);
int     pf_view_from_lnglat(pf_map* m, const double gps_origin[3], double lng_w, double lat_n, double lng_e, double lat_s, int width, int height, double V[9]);
/* measurement hook (tools/view_rate.py): while on, HIP events bracket the collapse, the coverage pass and the view kernel of every
 * view of m; pf_debug_view_timing_read: their milliseconds in the most recent view and the tiles it collapsed */
void    pf_debug_view_timing(pf_map* m, int on);
void    pf_debug_view_timing_read(pf_map* m, double out4[4]);
/* unused-by-the-reference helpers kept for API completeness (.cpp:57-75)   */
int     pf_normalize_using_weight_map(const float* weight, float* src3, size_t npix);
int     pf_mul_weight_map(const float* weight, float* src3, size_t npix);

/* --- stateless host geometry (no device needed) ---------------------------
 * The fp64 pose algebra the path uses, in the reference's operation order:
 * SE3::inverse / operator* (GSLAM/GSLAM/core/SE3.h:70-90), SO3*Point (SO3.h:445-450),
 * the four-corner ground footprint with the 0.4 gate (.cpp:324-347; pose in plane
 * coordinates, returns 0 when the frame is rejected) and the homography set-up of
 * cv::getPerspectiveTransform (.cpp:441). */
void    pf_se3_inverse(const double a[7], double out[7]);
void    pf_se3_mul(const double a[7], const double b[7], double out[7]);
void    pf_so3_rotate(const double q[4], const double p[3], double out[3]);
int     pf_footprint(const double cam[6], const double pose_plane[7], double pts8[8]);
void    pf_perspective_transform(const float src8[8], const float dst8[8], double M[9]);

/* --- multi-GPU seam exchange (no reference counterpart) ------ */
/* owner rank of a tile under the spatial hash */
int     pf_tile_owner(const pf_options* o, int ix, int iy);
/* Halo strips for Ele::blend across ranks.  A "strip set" of tile (ix,iy)
 * seen from a neighbour at (dx,dy) is the bytes blend() would copy from it
 * (.cpp:101-116), all levels concatenated.  pf_halo_bytes gives its size;
 * pack writes it to a device buffer, blend_tile_halo consumes up to 8 such
 * device buffers (NULL = neighbour absent) in place of local tiles.        */
size_t  pf_halo_bytes(pf_map* m, int dx, int dy);
int     pf_halo_pack(pf_map* m, int ix, int iy, int dx, int dy, void* dev_out);
int     pf_blend_tile_halo(pf_map* m, int ix, int iy, const void* const dev_halo[9], uint8_t* bgr256, void* raw);
/* whole tiles for save()'s gather: bytes of one tile's pyramid + weights   */
size_t  pf_tile_bytes(pf_map* m);
int     pf_tile_export(pf_map* m, int ix, int iy, void* dev_out);
int     pf_tile_import(pf_map* m, int ix, int iy, const void* dev_in);

/* --- merging maps, saving and resuming a map's state (no reference counterpart) --------------------
 * pf_merge: src's tiles merged into dst's on the GPU, by stable tile coordinate.  dst ends, bit for bit, tile by tile and level by
 * level, as the map that was fed dst's keyframes and then src's: per pixel and level `if (srcW >= dstW) { dstL = srcL; dstW = srcW; }`
 * (MultiBandMap2DCPU.cpp:521,542 with src as the newer keyframe), for a TypeCPU / TypeGPU map `if (dst.a < src.a) dst = src`
 * (Map2DCPU.cpp:326); a tile only src holds is copied, one only dst holds is left alone.  Keyframes that still wait in either map are
 * rendered first; dst's grid grows to hold src's; src is not modified.  Both maps: one device, prepared with the same plane, camera
 * and poses, the same type, pyramid type, band number and weight type, not sharded -- anything else, or dst == src, returns 0 with
 * the reason in pf_last_error() and touches nothing.  Keyframes fed to dst afterwards are culled against both maps' weight bounds. */
int     pf_merge(pf_map* dst, pf_map* src);
/* the same merge from n slot images the caller holds in m's device memory (what pf_tile_export writes: pf_tile_bytes each, 16-byte
 * aligned), tile i at stable coordinates (xy[2i], xy[2i+1]): the transport-free primitive for maps of other devices or processes.
 * wlb16: 16 floats per tile, the exporting map's cull bounds, or NULL when nothing is known of them (entries that are not finite
 * count as unknown); a coordinate given twice is refused.  The images' content is trusted as pf_tile_import trusts it. */
int     pf_merge_tiles(pf_map* m, int n, const int* xy, const void* const* dev_slots, const float* wlb16);
/* the 16 cull bounds of tile (ix, iy), to travel with its pf_tile_export image; 0: the map holds no such tile */
int     pf_tile_bounds(pf_map* m, int ix, int iy, float wlb16[16]);
/* The state file: everything a map is -- options that shape its tiles, plane, camera, grid, every tile's pyramid, weights and cull
 * bounds -- little-endian, a pure function of the state (two saves of one state are the same bytes).  pf_save_state drains and
 * writes it (on failure no file is left); pf_load_state is "prepare from the file" for a map created with the file's type,
 * ForceFloat, BandNumber and WeightType (else refused): the old content goes as in a second pf_prepare, and feeding goes on as if
 * the process had never ended; pf_merge_state merges the file into a prepared map as pf_merge would merge the map that wrote it.
 * A file that is not what it claims (magic, version, length, slot size, unsorted or duplicate tiles, geometry that is not finite)
 * is refused with the reason and the map is left as it was; its pixel content is trusted as pf_tile_import trusts a slot. */
int     pf_save_state(pf_map* m, const char* path);
int     pf_load_state(pf_map* m, const char* path);
int     pf_merge_state(pf_map* m, const char* path);
/* what a state file holds, read by host code alone (no device): info = map type (PF_TYPE_CPU or PF_TYPE_MULTIBAND), pyramid type
 * (PF_8UC4 / PF_16SC3 / PF_32FC3), band number, weight type, tiles, grid width, grid height in tiles, and the format version of the
 * file; plane[7], cam[6] as pf_prepare takes them; geo[6] as pf_grid gives it.  Any output may be NULL.  0 for a file pf_load_state
 * would refuse on sight, with the reason in pf_last_error(). */
int     pf_state_info(const char* path, int info[8], double plane[7], double cam[6], double geo[6]);
/* diagnostics of m's most recent merge (tools/merge_rate.py): out = pairs of slots, pairs whose destination had no pyramid, ms
 * between HIP events around the launches, pixel-levels src won (-1: not counted), bytes of a slot, 0.  count_stores 1 / 0: count
 * the wins in the merges to come (an atomic per thread: for measuring only) or not; -1: leave the setting. */
void    pf_debug_merge_stats(pf_map* m, int count_stores, double out[6]);

/* --- Undistortion: frames of a distorted camera ("Undistortion").
 * The input camera is a GSLAM parameter vector in[n] as Camera::Camera(std::vector<double>) reads it (GSLAM/core/Camera.h:407-416):
 * n = 6 PinHole (w, h, fx, fy, cx, cy), n = 7 ATAN (..., d), n = 11 OpenCV (..., k1, k2, p1, p2, k3); in[0], in[1] are the input frame's
 * width and height.  The output camera out6 is a pinhole as pf_prepare takes it; the two sizes may differ.  Every output pixel (x, y) has
 * one table entry q = in.Project(out.UnProject(x, y)), computed in double as UndistorterImpl::prepareReMap does
 * (GSLAM/core/Undistorter.h:85-168) and stored as two floats, or (-1, -1) where q lies outside [0, w_in) x [0, h_in): an UNCOVERED
 * pixel, black in the undistorted frame.  The pixel is Undistorter::undistort's bilinear colour branch, byte for byte, with the taps
 * clamped into the source.
 *
 * pf_undistort_table: the table on the host, no GPU needed: x, y take out_w * out_h floats each (either may be NULL), *uncovered (may be
 * NULL) the number of uncovered pixels.  pf_undistort_fit_camera: out6 (in: the wanted output camera; out: the fitted one) keeps w, h,
 * cx, cy and has (fx, fy) multiplied by the smallest s = k / 4096 >= 1 at which every pixel of the output image's four border lines is
 * covered; 0 when there is none up to s = 64, out6 untouched.  Both return 0 with pf_last_error() for a camera that is not valid. */
int     pf_undistort_table(const double* in, int n, const double out6[6], float* x, float* y, long long* uncovered);
int     pf_undistort_fit_camera(const double* in, int n, double out6[6]);
/* One frame undistorted on the GPU (current device).  src: in[1] rows of in[0] pixels, PF_8UC3 or PF_8UC4 (the alpha byte is ignored),
 * any row step; dst: out_h rows of out_w packed BGR8 pixels, dst_step bytes apart (0: packed).  pf_undistort_bgr: host to host, complete
 * when it returns.  pf_undistort_device: src->data and dst are device pointers and the kernel is queued on hip_stream (NULL: the default
 * stream); the call returns without waiting for it.  The table of the most recent camera pair is kept in device memory, so a run of calls
 * with one pair builds it once. */
int     pf_undistort_bgr(const double* in, int n, const double out6[6], const pf_image* src, uint8_t* dst, size_t dst_step);
int     pf_undistort_device(const double* in, int n, const double out6[6], const pf_image* src, void* dst, size_t dst_step, void* hip_stream);
/* The map's input camera.  While one is set, every frame that comes in -- pf_feed, pf_feed_device, pf_feed_jpeg(_batch), the frames of
 * pf_prepare, with or without a render thread -- is a frame of THAT camera and of its size (any other size is rejected as pf_feed rejects
 * a mismatched frame) and is undistorted on the GPU into the camera of pf_prepare before the map sees it; a pf_feed_device frame is read
 * by that kernel in stream order, not later.  n = 0 clears it.  It may be set before or after pf_prepare and survives pf_prepare: the
 * table is built and uploaded as soon as both cameras are known.  pf_load_state clears it (a state file holds the output camera only):
 * set it again after loading.  n not in {0, 6, 7, 11}, a camera that is not valid or a failed allocation returns 0 with pf_last_error()
 * and leaves the map as it was.  pf_dist_feed / pf_dist_feed_jpeg refuse a map that has one. */
int     pf_set_input_camera(pf_map* m, const double* in, int n);
/* 0: no input camera.  Otherwise the size of the frames the map now expects and the number of uncovered pixels of its table (-1 while
 * the map is not prepared); any output may be NULL. */
int     pf_input_camera_info(pf_map* m, int* rows_in, int* cols_in, long long* uncovered);

/* --- the seam exchange inside the library ---------------------------------
 * What a reference-side caller (the Map2DHIP subclass of INTEGRATION.md) needs to run draw() and save() when the mosaic is
 * sharded over the GPUs of a node: one process per GPU, each with its own pf_map created with shard_rank / shard_count,
 * every keyframe fed to every rank (feed has no collective).  Reference semantics reproduced across ranks: the neighbour
 * gather of draw(), MultiBandMap2DCPU.cpp:724-741 with Ele::blend :77-146, and the per-level paste + single collapse of
 * save(), :806-836.  Transport: RCCL (grouped ncclSend/ncclRecv between tile owners over xGMI; librccl is loaded at run
 * time) or a caller-supplied host-buffer exchange (tests, gloo / MPI launchers).  Collective calls: every rank of the
 * group must make the same pf_dist_* call.                                                                          */
typedef struct pf_dist pf_dist;
/* all-to-all-v over host buffers, indexed by peer rank (own entry: 0 bytes); 1 = ok */
typedef int (*pf_exchange_fn)(void* user, const void* const* send, const size_t* send_bytes,
                              void* const* recv, const size_t* recv_bytes, int nranks);
/* ncclGetUniqueId: 128 bytes, made on one rank and handed to all (by the launcher's own means) */
int      pf_dist_unique_id(void* out128);
pf_dist* pf_dist_init_rccl(pf_map* m, const void* unique_id128, int rank, int nranks);
pf_dist* pf_dist_init_host(pf_map* m, int rank, int nranks, pf_exchange_fn fn, void* user);
void     pf_dist_destroy(pf_dist* d);
/* Map2D::feed across ranks ("one H2D + P2P over xGMI"): the tracker hands a keyframe to ONE rank -- `root`, the
 * only rank whose img->data (host pixels) is read; every rank makes the call with the same pose and the same frame
 * description (rows, cols, type, step).  From the pose alone all ranks derive which ranks own a tile of the frame's canvas;
 * the root copies the pixels to its GPU once and sends them, in one grouped point-to-point exchange, to exactly those
 * ranks; each rank then renders its tiles (a rank that holds none of the canvas only advances its grid).  thread=0 maps.
 * Returns 1 (accepted), 0 (rejected as Map2D::feed would: oblique view ...), -1 (failure, on every rank alike).          */
int      pf_dist_feed(pf_dist* d, const pf_image* img, const double pose[7], int root);
/* The same with the keyframe as the bytes of its .jpg file (pf_feed_jpeg across ranks): only the root reads `data`; every rank
 * makes the call with the same pose and the frame's size (rows, cols: the camera's).  The root decodes on its GPU straight into
 * the slot the exchange sends from.                                                                                       */
int      pf_dist_feed_jpeg(pf_dist* d, const uint8_t* data, size_t len, int rows, int cols, const double pose[7], int root);
/* draw() across ranks: every rank blends ITS changed tiles (at most cap) with the edge strips of neighbours that live on
 * other ranks and clears their Ischanged flags.  One pack launch, one grouped exchange, one batched blend per call.
 * Returns the number of tiles written to xy / bgr (cap tiles of 256x256x3 each), -1 on failure.                     */
int      pf_dist_blend_changed(pf_dist* d, int* xy, uint8_t* bgr, int cap);
/* save() across ranks: every tile travels once to rank 0, which runs the whole-mosaic collapse and (pf_dist_save) writes
 * the file.  On the other ranks the calls return 1 with rows = cols = 0.                                            */
int      pf_dist_save(pf_dist* d, const char* filename);
/* ... as the lossless pyramid TIFF: rank 0 writes pf_save_tiff_lossless's file of the gathered mosaic */
int      pf_dist_save_tiff_lossless(pf_dist* d, const char* filename, int masked, int force_bigtiff);
int      pf_dist_save_to_memory(pf_dist* d, uint8_t* bgr, int* rows, int* cols, int* tile_x0, int* tile_y0);
/* what the last pf_dist_* call moved */
typedef struct pf_dist_stats {
    unsigned long long bytes_sent, bytes_received;   /* payload, this rank */
    unsigned long long strips_sent, strips_received, tiles, peers;
    double plan_ms, pack_ms, exchange_ms, compute_ms;
    unsigned long long verified;                      /* data exchanges checked end to end in this call (PF_DIST_VERIFY=1: every
                                                       * rank hashes what it sent to and received from each peer; the hashes must agree) */
} pf_dist_stats;
int      pf_dist_last_stats(pf_dist* d, pf_dist_stats* out);
/* The plan of one pf_dist_blend_changed call as rank `me` derives it from the all-gathered tile lists -- a pure function
 * (no device, no transport), exported so that launchers and the CPU tests can inspect or replay the exchange the library
 * will make.  lists: for every rank, counts[r] records of 3 ints (ix, iy, Ischanged), ranks back to back; caps[r]: the most
 * tiles rank r blends in the call; halo_bytes9[j]: bytes of the strip set of neighbour j = 3*(dy+1)+(dx+1) (pf_halo_bytes).
 * send[i]: tile (ix,iy) of THIS rank hands the edge facing (-dx,-dy) to rank `peer`, at byte `offset` of the bytes for that
 * peer; recv[i]: this rank's tile number `tile` (index into mine_xy) gets neighbour j = 3*(dy+1)+(dx+1) from rank `peer` at
 * byte `offset` of the bytes from that peer.  Returns 1, or 0 when a capacity is too small (the n_* still say what is needed). */
typedef struct pf_strip_plan { int peer, ix, iy, dx, dy, tile; unsigned long long offset; } pf_strip_plan;
int      pf_dist_plan_blend(int nranks, int me, const int* counts, const int* lists3, const long long* caps, int high_quality,
                            const size_t halo_bytes9[9], pf_strip_plan* send, int send_cap, int* n_send,
                            pf_strip_plan* recv, int recv_cap, int* n_recv, int* mine_xy, int mine_cap, int* n_mine);
/* what the group looks like from this rank: its rank, the number of ranks the transport was brought up with, and the
 * transport's name ("rccl" / "host").  A launcher's first multi-GPU run checks these before it trusts a collective.  */
int      pf_dist_info(pf_dist* d, int* rank, int* nranks, const char** transport);
/* end-to-end check of every data exchange of the following pf_dist_* calls (default: on iff PF_DIST_VERIFY is set): each
 * rank hashes (FNV-1a) what it sent to and what it received from each peer, the hashes travel as a control message and
 * must agree; a mismatch fails the call ON EVERY RANK ALIKE (the verdict is agreed on after the hash exchange, so the sender of
 * wrong bytes returns -1 as well and no rank is left waiting in the next collective) and pf_last_error names the pair on the
 * receiving rank.  One rank asking is enough: the wish travels with the status word the ranks agree on before every data
 * exchange, so ranks started with different PF_DIST_VERIFY settings still run the same sequence of collectives.
 * Costs a device-to-host copy of the payload. */
int      pf_dist_set_verify(pf_dist* d, int on);

/* --- measurement -------------------------------------------------------- */
/* Per-kernel HIP-event timing on the map's own stream.  mode 0 = off,
 * 1 = every kernel, 2+k = only kernel k (index in pf_profile_read order); adding n << 8 times every
 * n-th launch only (an event pair costs a few microseconds of stream time per launch).  Read returns
 * the kernel count; names[i] are static strings; ms / launches / bytes cover the timed launches.    */
int     pf_profile_enable(pf_map* m, int mode);
int     pf_profile_read(pf_map* m, int cap, const char** names, double* total_ms, long long* launches,
                        double* alg_bytes);
/* The same, plus alg_bytes_run: the algorithmic bytes of the part of the canvases the timed launches' blocks actually processed
 * (SURVEY 8d's per-tile bytes x the share of each level's pixels covered by blocks that ran, + the frame read once).  The cull of
 * render_frame and a shard leave blocks of a canvas out; alg_bytes counts every tile of every canvas regardless.  Equal to
 * alg_bytes for kernels that always cover their whole window. */
int     pf_profile_read_run(pf_map* m, int cap, const char** names, double* total_ms, long long* launches,
                            double* alg_bytes, double* alg_bytes_run);
int     pf_profile_reset(pf_map* m);
/* sharding overhead since creation: {frames that put pixels on this rank, level-0 pixels computed (owned tiles + pyramid
 * halo, fused path), tile pixels owned in those frames, tiles held}: [1]/[2] is the halo recompute factor of a shard  */
int     pf_render_stats(pf_map* m, double out4[4]);
/* Host section timers with the reference's section names (pi::timer.enter / leave, PIL/src/base/time/Timer.h:43-85;
 * MultiBandMap2DCPU.cpp:476,555,563,602,628-630,722,742): "Map2D::feed", "MultiBandMap2DCPU::renderFrame",
 * "MultiBandMap2DCPU::Apply", "MultiBandMap2DCPU::spreadMap", "MultiBandMap2DCPU::updateTexture",
 * "MultiBandMap2DCPU::save" -- calls, mean / min / max seconds of HOST time per section (kernels run asynchronously: device
 * time is pf_profile_read's).  With PF_ROCTX=1 in the environment every section is also a roctx range.  Returns the count. */
int     pf_timer_read(pf_map* m, int cap, const char** names, long long* calls, double* mean_s, double* min_s, double* max_s);
int     pf_timer_reset(pf_map* m);
/* Tiles left out of launches so far because the keyframe fed could not win the max-weight select anywhere in them (the cull of
 * render_frame: bounds from the geometry alone; results are those of the full render, PF_CULL=0 switches it off). Diagnostics. */
long long pf_debug_culled_tiles(pf_map* m);
/* ... and the 64 x 64 cells (16 per tile) switched off inside tiles that were rendered.  Diagnostics. */
long long pf_debug_culled_cells(pf_map* m);
/* With PF_CULL_EXACT_STAT=1 in the environment: level-0 pixels of the blocks within the pyramid's reach of a rendered cell, summed
 * over the keyframes fed (what the in-kernel need test lets run; tools/cull_stats.py).  0 otherwise.  Diagnostics. */
double  pf_debug_level0_exact_px(pf_map* m);
/* The cull on (default, unless PF_CULL=0 is in the environment) or off: off renders every tile of every keyframe's canvas, as the
 * reference does; the mosaic is the same either way.  For measurements (bench.py reports both rates). */
/* Test hook: the pf_feed / pf_feed_device calls (0-based, counted since creation, geometry-only feeds included) whose keyframes renderFrame
 * accepted, in render order; writes the newest min(cap, count) of them and returns the count (at most the newest 65536 are kept).  With
 * thread = 1 and a queue that drops (MultiBandMap2DCPU.cpp:300-303) this is the only way to tell a checker which keyframes the map holds. */
int     pf_debug_render_log(pf_map* m, long long* out, int cap);
void    pf_set_cull(pf_map* m, int on);
/* Launches of the pipelined level kernel by form since the library was loaded: [0] block form with the computed weight (default),
 * [1] block form gathering the weight plane, [2] LDS-staged source patch, [3] rolling strips, [4] 64x64 blocks, [5] 64x28 blocks,
 * [6] stamped instantiation, [7] launches whose tile table travelled in the kernel arguments.  Diagnostics (variant tests). */
void    pf_debug_form_counts(long long out[8]);
/* By which rule the blocks of those launches decided whether they run, since the library was loaded (k_levels; which one a launch takes
 * follows from the size of the keyframe's canvas alone).  Per launch with a level-0 job: [0] tile table in the kernel arguments and the
 * block tests itself against it (need_r0), [1] need rectangles, [2] no filter, every block runs, [3] tile table staged and copied in the
 * stream instead of travelling in the arguments.  Per upper-level job: [4] need bitmap, [5] need rectangles, [6] no filter.  On the host:
 * [7] keyframes whose plan merged rectangles (more cells than a level-0 job carries rectangles, or than an upper-level job does).
 * Counted for launches of k_levels only: the experiments library's rolling-strip form (PF_STRIPS) moves none of them, and its compact
 * grid (PF_COMPACT), whose level-0 blocks lie inside the rectangles by construction, counts as [1].
 * Diagnostics (tests/test_gpu_large_canvas.py). */
void    pf_debug_admission_counts(long long out[8]);
/* ... and how many of them ran their level-0 job on the compact grid (one workgroup per block inside the need rectangles of a shard / of
 * the cull, instead of one per block of the canvas' bounding box) */
long long pf_debug_compact_launches(void);
/* frames rendered / rejected since creation */
int     pf_stats(pf_map* m, long long* rendered, long long* rejected, long long* dropped);
/* ... and `failed`: keyframes that were accepted (not rejected, not dropped from the queue) and are not in the map because an allocation
 * or a launch failed (see pf_feed, pf_sync).  Any of the four may be NULL. */
int     pf_stats_failed(pf_map* m, long long* rendered, long long* rejected, long long* dropped, long long* failed);
/* Allocator hint, no reference counterpart (MultiBandMap2DCPUEle's cv::Mat tiles, MultiBandMap2DCPU.h:32-51,
 * come from the heap one by one): HBM for n_tiles more tiles is allocated and touched now instead of slab by
 * slab while keyframes are being fused.  Call it after pf_prepare (which empties the store).                  */
int     pf_reserve_tiles(pf_map* m, long long n_tiles);

#ifdef __cplusplus
}
#endif
#endif /* PIFUSION_H */
