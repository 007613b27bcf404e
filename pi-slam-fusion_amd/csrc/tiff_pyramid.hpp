// tiff_pyramid.hpp -- the tiled pyramid TIFF behind save("x.tif"): image 0 is the mosaic, image k >= 1 the 2 x 2 mean of image
// k - 1, every image cut into 256 x 256 tiles, every tile a complete baseline JPEG stream (jpeg_encode.hpp), all-background tiles
// stored once.  The file is a pure function of (pixels, quality, background colour, the 16 doubles, the BigTIFF flag); its
// layout is written down in include/pifusion.h (pf_tiff_write_bgr) and decided in ONE function here, tiff::layout, which the host
// writer below and the GPU path (overview.hip) both call.
//
// Header-only host code, no device: image_io.cpp (pf_tiff_write_bgr, pf_write_image), overview.hip (the same file from an image
// in HBM), tests/cpp/san_tiff.cpp.
//
// The masked file (pf_tiff_write_bgr_masked) is the same file with a transparency mask behind every image: 1 bit per pixel,
// uncompressed tiles of 256 rows x 32 bytes, image k + 1's mask the OR of the 2 x 2 blocks of image k's, all-zero and all-one
// tiles stored once.  The same layout function places it; with no mask it places today's bytes.
//
// The lossless file (pf_tiff_write_bgr_lossless) is either of the two with Codec kDeflate: every colour tile a zlib stream of
// deflate_rle.hpp, the colour IFDs saying Compression 8, RGB, Predictor 2.  With kJpeg, the default, nothing changes.
#pragma once
#include "jpeg_encode.hpp"
#include "deflate_rle.hpp"
#include <cstdio>
#include <functional>
#include <string>

namespace pf {

void set_error(const std::string& msg);          // jpeg_decode.cpp

namespace tiff {

constexpr int kTile = 256;
// what a colour tile's stream is: a baseline JPEG (Compression 7, YCbCr 4:2:0), or a zlib stream of the tile's horizontally
// differenced RGB bytes (deflate_rle.hpp: Compression 8, Predictor 2).  Everything else about the file is the same.
enum Codec : int { kJpeg = 0, kDeflate = 1 };

struct Level {
    int rows, cols;          // the image
    int ty, tx;              // tiles down and across
    size_t first;            // index of its first tile among the tiles of all images (row-major inside the image)
    size_t tiles() const { return (size_t)ty * tx; }
};

// image 0 and its overviews: ceil(r / 2) x ceil(c / 2) each, down to the first image that fits one tile
inline std::vector<Level> levels(int rows, int cols)
{
    std::vector<Level> v;
    size_t first = 0;
    for (int r = rows, c = cols;; r = (r + 1) / 2, c = (c + 1) / 2) {
        Level l{ r, c, (r + kTile - 1) / kTile, (c + kTile - 1) / kTile, first };
        v.push_back(l);
        first += l.tiles();
        if (r <= kTile && c <= kTile) break;
    }
    return v;
}
inline size_t tile_count(const std::vector<Level>& lv) { return lv.back().first + lv.back().tiles(); }

// Result.BackGroundColor as save() paints it: cv::Scalar(bg, bg, bg) saturated to 8 bits
inline uint8_t background_byte(int bg) { return (uint8_t)(bg < 0 ? 0 : bg > 255 ? 255 : bg); }

// ---- the layout --------------------------------------------------------------------------------------------------------------
// header | per image, in order: its IFD, then the values that do not fit an entry (BitsPerSample, TileOffsets, TileByteCounts,
// the 16 doubles, the GeoKey directory) in tag order | the empty tile's stream, if any tile is empty | the streams of the other
// tiles, image by image, row-major.  Everything starts on an even offset.  Classic TIFF when the file ends below 4 GiB.
struct Layout {
    bool big = false;
    std::vector<uint8_t> head;          // the bytes in front of the first stream
    std::vector<uint64_t> offset;       // per tile: where its stream lies (empty tiles: the shared one)
    uint64_t empty_offset = 0;          // of the shared stream (0: no tile is empty)
    uint64_t total = 0;                 // bytes of the file
    // the masked file only
    std::vector<uint64_t> mask_offset;  // per tile: where its mask tile lies (all-zero and all-one tiles: the shared ones)
    uint64_t zero_offset = 0, one_offset = 0;          // of the shared mask tiles (0: no tile of that kind)
};

// a mask tile: 256 rows of 32 bytes, bit 7 of byte 0 = column 0, bits past the image 0.  Its kind decides where it is stored
constexpr size_t kMaskTileBytes = (size_t)kTile * kTile / 8;
enum MaskKind : uint8_t { kMaskZero = 0, kMaskOne = 1, kMaskOwn = 2 };          // all 65 536 bits 0 / all 1 (both stored once) / stored on its own

namespace detail {
struct Entry { uint16_t tag, type; uint64_t count; std::vector<uint8_t> value; };          // value: little-endian bytes
inline void put(std::vector<uint8_t>& b, uint64_t v, int n) { for (int i = 0; i < n; i++) b.push_back((uint8_t)(v >> (8 * i))); }
inline void poke(std::vector<uint8_t>& b, size_t at, uint64_t v, int n) { for (int i = 0; i < n; i++) b[at + i] = (uint8_t)(v >> (8 * i)); }
inline Entry shorts(uint16_t tag, std::initializer_list<unsigned> v) { Entry e{ tag, 3, v.size(), {} }; for (unsigned x : v) put(e.value, x, 2); return e; }
inline Entry longs(uint16_t tag, std::initializer_list<unsigned> v) { Entry e{ tag, 4, v.size(), {} }; for (unsigned x : v) put(e.value, x, 4); return e; }
}  // namespace detail

// len[i]: bytes of tile i's stream, 0 for an empty tile; empty_len: bytes of the shared stream.  model_transform may be null.
// mkind (null: the unmasked file): the MaskKind of tile i's mask tile.  Then every image's IFD is followed by its mask's, the two
// shared mask tiles lie behind the shared stream and the other mask tiles behind the last stream, image by image, row-major.
inline bool layout_as(const std::vector<Level>& lv, const std::vector<uint32_t>& len, uint32_t empty_len, const std::vector<uint8_t>* mkind, const double* model_transform, bool big, Layout& out, Codec codec = kJpeg)
{
    using namespace detail;
    out = Layout();
    out.big = big;
    const int osz = big ? 8 : 4, esz = big ? 20 : 12;          // bytes of an offset, of an IFD entry
    std::vector<uint8_t>& h = out.head;
    put(h, 0x4949, 2);
    if (big) { put(h, 43, 2); put(h, 8, 2); put(h, 0, 2); put(h, 16, 8); }
    else { put(h, 42, 2); put(h, 8, 4); }
    struct Fix { size_t at; size_t first; size_t n; bool mask; };          // where an image's TileOffsets values lie in `head`
    std::vector<Fix> fix;
    const int halves = mkind ? 2 : 1;                                       // the image, then its mask
    for (size_t k = 0; k < lv.size(); k++)
      for (int half = 0; half < halves; half++) {
        const Level& l = lv[k];
        const size_t n = l.tiles();
        const bool mask = half == 1;
        std::vector<Entry> e;
        e.push_back(longs(254, { (k ? 1u : 0u) | (mask ? 4u : 0u) }));
        e.push_back(longs(256, { (unsigned)l.cols }));
        e.push_back(longs(257, { (unsigned)l.rows }));
        if (mask) e.push_back(shorts(258, { 1 })); else e.push_back(shorts(258, { 8, 8, 8 }));
        e.push_back(shorts(259, { mask ? 1u : codec == kDeflate ? 8u : 7u }));
        e.push_back(shorts(262, { mask ? 4u : codec == kDeflate ? 2u : 6u }));
        e.push_back(shorts(277, { mask ? 1u : 3u }));
        e.push_back(shorts(284, { 1 }));
        if (!mask && codec == kDeflate) e.push_back(shorts(317, { 2 }));
        e.push_back(shorts(322, { (unsigned)kTile }));
        e.push_back(shorts(323, { (unsigned)kTile }));
        Entry to{ 324, (uint16_t)(big ? 16 : 4), n, std::vector<uint8_t>(n * osz, 0) };          // filled in below
        e.push_back(to);
        Entry tb{ 325, 4, n, {} };
        for (size_t i = 0; i < n; i++) put(tb.value, mask ? (uint32_t)kMaskTileBytes : len[l.first + i] ? len[l.first + i] : empty_len, 4);
        e.push_back(tb);
        if (!mask && codec == kJpeg) e.push_back(shorts(530, { 2, 2 }));
        if (k == 0 && !mask && model_transform) {
            Entry mt{ 34264, 12, 16, {} };
            for (int i = 0; i < 16; i++) { uint64_t bits; std::memcpy(&bits, &model_transform[i], 8); put(mt.value, bits, 8); }
            e.push_back(mt);
            // GeoKeyDirectory: version 1.1.0, two keys: GTModelType = user-defined, GTRasterType = RasterPixelIsArea
            e.push_back(shorts(34735, { 1, 1, 0, 2, 1024, 0, 1, 32767, 1025, 0, 1, 1 }));
        }
        const size_t ifd = h.size();
        size_t values = ifd + (big ? 8 : 2) + e.size() * esz + osz;          // behind the entries and the next-IFD offset
        values += values & 1;
        put(h, e.size(), big ? 8 : 2);
        std::vector<uint8_t> tail;
        for (const Entry& en : e) {
            put(h, en.tag, 2); put(h, en.type, 2); put(h, en.count, osz);
            if ((int)en.value.size() <= osz) {
                if (en.tag == 324) fix.push_back({ h.size(), l.first, n, mask });
                h.insert(h.end(), en.value.begin(), en.value.end());
                h.resize(h.size() + (osz - en.value.size()), 0);
            } else {
                if (en.tag == 324) fix.push_back({ values + tail.size(), l.first, n, mask });
                put(h, values + tail.size(), osz);
                tail.insert(tail.end(), en.value.begin(), en.value.end());
                if (tail.size() & 1) tail.push_back(0);
            }
        }
        const size_t next = values + tail.size();
        put(h, k + 1 < lv.size() || half + 1 < halves ? next : 0, osz);
        h.resize(values, 0);
        h.insert(h.end(), tail.begin(), tail.end());
      }
    // the streams
    const size_t nt = tile_count(lv);
    out.offset.assign(nt, 0);
    uint64_t at = h.size();
    bool any_empty = false;
    for (size_t i = 0; i < nt; i++) any_empty = any_empty || !len[i];
    if (any_empty) { out.empty_offset = at; at += empty_len; at += at & 1; }
    if (mkind) {          // the shared mask tiles (8192 bytes each: the offsets stay even)
        bool any_zero = false, any_one = false;
        for (size_t i = 0; i < nt; i++) { any_zero = any_zero || (*mkind)[i] == kMaskZero; any_one = any_one || (*mkind)[i] == kMaskOne; }
        if (any_zero) { out.zero_offset = at; at += kMaskTileBytes; }
        if (any_one) { out.one_offset = at; at += kMaskTileBytes; }
    }
    for (size_t i = 0; i < nt; i++) {
        if (!len[i]) { out.offset[i] = out.empty_offset; continue; }
        out.offset[i] = at; at += len[i]; at += at & 1;
    }
    if (mkind) {
        out.mask_offset.assign(nt, 0);
        for (size_t i = 0; i < nt; i++) {
            if ((*mkind)[i] == kMaskZero) out.mask_offset[i] = out.zero_offset;
            else if ((*mkind)[i] == kMaskOne) out.mask_offset[i] = out.one_offset;
            else { out.mask_offset[i] = at; at += kMaskTileBytes; }
        }
    }
    out.total = at;
    if (!big && at > 0xFFFFFFFFull) return false;
    for (const Fix& f : fix)
        for (size_t i = 0; i < f.n; i++) poke(h, f.at + i * osz, f.mask ? out.mask_offset[f.first + i] : out.offset[f.first + i], osz);
    return true;
}

inline void layout_masked(const std::vector<Level>& lv, const std::vector<uint32_t>& len, uint32_t empty_len, const std::vector<uint8_t>* mkind, const double* model_transform, bool force_bigtiff, Layout& out, Codec codec = kJpeg)
{
    if (force_bigtiff || !layout_as(lv, len, empty_len, mkind, model_transform, false, out, codec)) (void)layout_as(lv, len, empty_len, mkind, model_transform, true, out, codec);
}
inline void layout(const std::vector<Level>& lv, const std::vector<uint32_t>& len, uint32_t empty_len, const double* model_transform, bool force_bigtiff, Layout& out)
{ layout_masked(lv, len, empty_len, nullptr, model_transform, force_bigtiff, out); }

// the stream every empty tile points at: 256 x 256 pixels of the background colour
inline void encode_tile(Codec codec, const uint8_t* tile, int quality, std::vector<uint8_t>& out)
{
    if (codec == kDeflate) dfl::encode_tile(tile, (size_t)kTile * 3, out);
    else jenc::encode_bgr(tile, kTile, kTile, (size_t)kTile * 3, quality, out);
}
inline void empty_stream(int quality, int bg, std::vector<uint8_t>& out, Codec codec = kJpeg)
{
    std::vector<uint8_t> px((size_t)kTile * kTile * 3, background_byte(bg));
    out.clear();
    encode_tile(codec, px.data(), quality, out);
}

// The file: the head, then the streams where the layout put them.  stream(i): the bytes of tile i (len[i] of them, len[i] > 0),
// asked for in increasing i.  The masked file (mkind and mtile given): the two shared mask tiles behind the shared stream, and
// behind the last stream mtile(i), the 8192 bytes of every mask tile of kind kMaskOwn, in increasing i.  A file that cannot be
// written completely is removed.
inline bool write_file(const char* filename, const Layout& lo, const std::vector<uint32_t>& len, const std::vector<uint8_t>& empty,
                       const std::function<const uint8_t*(size_t)>& stream, const std::vector<uint8_t>* mkind = nullptr,
                       const std::function<const uint8_t*(size_t)>* mtile = nullptr)
{
    FILE* f = std::fopen(filename, "wb");
    if (!f) { set_error(std::string("save: cannot open ") + filename); return false; }
    uint64_t at = 0;
    auto put = [&](const uint8_t* p, size_t n) { at += n; return std::fwrite(p, 1, n, f) == n; };
    auto even = [&]() { const uint8_t z = 0; return !(at & 1) || put(&z, 1); };
    bool ok = put(lo.head.data(), lo.head.size());
    if (ok && lo.empty_offset) ok = put(empty.data(), empty.size()) && even();
    if (ok && mkind) {
        const std::vector<uint8_t> zero(kMaskTileBytes, 0), one(kMaskTileBytes, 0xFF);
        if (lo.zero_offset) ok = at == lo.zero_offset && put(zero.data(), zero.size());
        if (ok && lo.one_offset) ok = at == lo.one_offset && put(one.data(), one.size());
    }
    for (size_t i = 0; ok && i < len.size(); i++)
        if (len[i]) ok = at == lo.offset[i] && put(stream(i), len[i]) && even();
    if (mkind)
        for (size_t i = 0; ok && i < mkind->size(); i++)
            if ((*mkind)[i] == kMaskOwn) ok = at == lo.mask_offset[i] && put((*mtile)(i), kMaskTileBytes);
    ok = ok && at == lo.total;
    if (std::fclose(f) != 0) ok = false;
    if (!ok) { std::remove(filename); set_error("save: write failed"); }
    return ok;
}

// ---- the scalar model: overview chain, tile cutter, empty test ----------------------------------------------------------------
// image k from image k - 1 (packed rows): every channel (p00 + p01 + p10 + p11 + 2) >> 2, a missing last row or column repeats
// the one before it
inline void halve(const uint8_t* src, int rows, int cols, size_t step, std::vector<uint8_t>& dst)
{
    const int r2 = (rows + 1) / 2, c2 = (cols + 1) / 2;
    dst.resize((size_t)r2 * c2 * 3);
    for (int y = 0; y < r2; y++) {
        const uint8_t* a = src + (size_t)(2 * y) * step;
        const uint8_t* b = src + (size_t)std::min(2 * y + 1, rows - 1) * step;
        uint8_t* d = dst.data() + (size_t)y * c2 * 3;
        for (int x = 0; x < c2; x++) {
            const int x0 = 6 * x, x1 = 3 * std::min(2 * x + 1, cols - 1);
            for (int ch = 0; ch < 3; ch++) d[3 * x + ch] = (uint8_t)((a[x0 + ch] + a[x1 + ch] + b[x0 + ch] + b[x1 + ch] + 2) >> 2);
        }
    }
}
// tile (ty, tx) of an image: 256 x 256 packed pixels, past the image its last column, then its last row; returns "all background"
inline bool cut_tile(const uint8_t* img, int rows, int cols, size_t step, int ty, int tx, uint8_t bgv, uint8_t* tile)
{
    bool empty = true;
    for (int r = 0; r < kTile; r++) {
        const uint8_t* s = img + (size_t)std::min(ty * kTile + r, rows - 1) * step;
        uint8_t* d = tile + (size_t)r * kTile * 3;
        const int x0 = tx * kTile, n = std::min(kTile, cols - x0);
        std::memcpy(d, s + (size_t)x0 * 3, (size_t)n * 3);
        for (int x = n; x < kTile; x++) std::memcpy(d + 3 * x, d + 3 * (n - 1), 3);
        for (int i = 0; i < kTile * 3 && empty; i++) empty = d[i] == bgv;
    }
    return empty;
}

// the coverage of image k + 1 from that of image k (a byte per pixel, 0 or 1, packed rows): the OR of the 2 x 2 block, a missing
// last row or column repeats the one before it
inline void mask_halve(const uint8_t* src, int rows, int cols, std::vector<uint8_t>& dst)
{
    const int r2 = (rows + 1) / 2, c2 = (cols + 1) / 2;
    dst.resize((size_t)r2 * c2);
    for (int y = 0; y < r2; y++) {
        const uint8_t* a = src + (size_t)(2 * y) * cols;
        const uint8_t* b = src + (size_t)std::min(2 * y + 1, rows - 1) * cols;
        for (int x = 0; x < c2; x++) {
            const int x1 = std::min(2 * x + 1, cols - 1);
            dst[(size_t)y * c2 + x] = (uint8_t)(a[2 * x] | a[x1] | b[2 * x] | b[x1]);
        }
    }
}
// mask tile (ty, tx) of such a coverage: 256 rows of 32 bytes, bit 7 of byte 0 = column 0, bits past the image 0; returns its kind
inline MaskKind cut_mask_tile(const uint8_t* cov, int rows, int cols, int ty, int tx, uint8_t* tile)
{
    std::memset(tile, 0, kMaskTileBytes);
    size_t ones = 0;
    const int x0 = tx * kTile, n = std::min(kTile, cols - x0);
    for (int r = 0; r < kTile && ty * kTile + r < rows; r++) {
        const uint8_t* s = cov + (size_t)(ty * kTile + r) * cols + x0;
        uint8_t* d = tile + (size_t)r * (kTile / 8);
        for (int x = 0; x < n; x++)
            if (s[x]) { d[x >> 3] |= (uint8_t)(0x80 >> (x & 7)); ones++; }
    }
    return ones == 0 ? kMaskZero : ones == (size_t)kTile * kTile ? kMaskOne : kMaskOwn;
}

// pf_tiff_write_bgr (mask == null) and pf_tiff_write_bgr_masked (mask: a byte per pixel, non-zero = covered, rows of mask_step bytes)
inline bool write_pyramid(const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, const uint8_t* mask, size_t mask_step,
                          int quality, int bg, const double* model_transform, bool force_bigtiff, Codec codec = kJpeg)
{
    const std::vector<Level> lv = levels(rows, cols);
    const uint8_t bgv = background_byte(bg);
    std::vector<uint32_t> len(tile_count(lv), 0);
    std::vector<size_t> at(len.size(), 0);
    std::vector<uint8_t> streams, tile((size_t)kTile * kTile * 3), cur, next, empty;
    const uint8_t* img = bgr;
    for (size_t k = 0; k < lv.size(); k++) {
        const Level& l = lv[k];
        if (k) { halve(img, lv[k - 1].rows, lv[k - 1].cols, step, next); cur.swap(next); img = cur.data(); step = (size_t)l.cols * 3; }
        for (int ty = 0; ty < l.ty; ty++)
            for (int tx = 0; tx < l.tx; tx++) {
                if (cut_tile(img, l.rows, l.cols, step, ty, tx, bgv, tile.data())) continue;
                const size_t i = l.first + (size_t)ty * l.tx + tx;
                at[i] = streams.size();
                encode_tile(codec, tile.data(), quality, streams);
                len[i] = (uint32_t)(streams.size() - at[i]);
            }
    }
    empty_stream(quality, bg, empty, codec);
    Layout lo;
    if (!mask) {
        layout_masked(lv, len, (uint32_t)empty.size(), nullptr, model_transform, force_bigtiff, lo, codec);
        return write_file(filename, lo, len, empty, [&](size_t i) { return streams.data() + at[i]; });
    }
    // the masks: the OR chain, every tile packed and classed; the tiles that are stored on their own are kept back to back
    std::vector<uint8_t> mkind(len.size(), kMaskZero), mtiles, cov((size_t)rows * cols), cnext;
    std::vector<size_t> mat(len.size(), 0);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) cov[(size_t)y * cols + x] = mask[(size_t)y * mask_step + x] ? 1 : 0;
    for (size_t k = 0; k < lv.size(); k++) {
        const Level& l = lv[k];
        if (k) { mask_halve(cov.data(), lv[k - 1].rows, lv[k - 1].cols, cnext); cov.swap(cnext); }
        for (int ty = 0; ty < l.ty; ty++)
            for (int tx = 0; tx < l.tx; tx++) {
                const size_t i = l.first + (size_t)ty * l.tx + tx;
                mat[i] = mtiles.size();
                mtiles.resize(mtiles.size() + kMaskTileBytes);
                mkind[i] = cut_mask_tile(cov.data(), l.rows, l.cols, ty, tx, mtiles.data() + mat[i]);
                if (mkind[i] != kMaskOwn) mtiles.resize(mat[i]);
            }
    }
    layout_masked(lv, len, (uint32_t)empty.size(), &mkind, model_transform, force_bigtiff, lo, codec);
    const std::function<const uint8_t*(size_t)> mtile = [&](size_t i) { return (const uint8_t*)mtiles.data() + mat[i]; };
    return write_file(filename, lo, len, empty, [&](size_t i) { return streams.data() + at[i]; }, &mkind, &mtile);
}
inline bool write_bgr(const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, int quality, int bg, const double* model_transform, bool force_bigtiff)
{ return write_pyramid(filename, bgr, rows, cols, step, nullptr, 0, quality, bg, model_transform, force_bigtiff); }
inline bool write_bgr_masked(const char* filename, const uint8_t* bgr, int rows, int cols, size_t step, const uint8_t* mask, size_t mask_step,
                             int quality, int bg, const double* model_transform, bool force_bigtiff)
{ return write_pyramid(filename, bgr, rows, cols, step, mask, mask_step, quality, bg, model_transform, force_bigtiff); }

}  // namespace tiff

// The same file from an image in device memory (overview.hip): the overview chain and the empty test are kernels, the tiles are
// encoded by `enc` in bounded batches, only flags, offsets and streams come to the host.  One per consumer (a map, or the
// process-wide one behind pf_tiff_write_device); not thread-safe.  `stream` is a hipStream_t.
class TiffDevice {
public:
    TiffDevice() {}
    ~TiffDevice();
    void release();          // frees the device and page-locked buffers (the device they live on is current)
    TiffDevice(const TiffDevice&) = delete;
    TiffDevice& operator=(const TiffDevice&) = delete;
    // The masked file's coverage, if any: a byte per pixel in device memory (non-zero = covered, rows of `step` bytes), or the tile
    // table of a map's mosaic (wx x wy slots of 256 x 256, 0 = no tile; covered = the fp32 weight at w_off inside the slot is not 0).
    struct Mask {
        const void* dev_bytes = nullptr; size_t step = 0;
        const uint64_t* dev_table = nullptr; int wx = 0, wy = 0; uint32_t w_off = 0;
    };
    // `lossless` given: the colour tiles are its Deflate streams (Codec kDeflate; quality and `enc` are not used), else enc's JPEG ones
    bool write(const char* filename, const void* dev_bgr, int rows, int cols, size_t step, int quality, int bg, const double* model_transform, bool force_bigtiff,
               JpegEncoder& enc, void* stream, const Mask* mask = nullptr, DeflateEncoder* lossless = nullptr);
    // diagnostics of the last write: tiles of all images, the empty ones among them, bytes of device memory held for levels and flags
    void last_counts(size_t* tiles, size_t* empty, size_t* device_bytes) const;
    // ... of the last masked write: mask tiles that are all zero, all one, and the bytes of the others (what crossed to the host)
    void last_mask_counts(size_t* zero, size_t* one, size_t* own_bytes) const;
private:
    struct Impl;
    Impl* p_ = nullptr;
};

}  // namespace pf
