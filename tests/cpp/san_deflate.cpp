// san_deflate.cpp -- the scalar encoder of the lossless tile codec (csrc/deflate_rle.hpp behind pf_deflate_tile_bgr) and the lossless
// host writer (pf_tiff_write_bgr_lossless) under AddressSanitizer + UndefinedBehaviorSanitizer.  Tiles, images and masks are heap
// blocks of exactly the bytes a call may read ((rows - 1) * step + a row), the output block has exactly the bound: one byte past
// any of them is a finding.
//   san_deflate <dir> <tiles> <images>
//     tNNN.bgr / tNNN.z   a hostile tile (196 608 bytes) and its stream by tests/deflate_model.py: the encoder gives that stream, packed
//                         and with a padded step
//     iNNN.txt / .bgr / .msk / .z   a tiny image (rows cols bg masked), its pixels, its mask and the model's stream of its one tile: the
//                         writer's file holds that stream where TileOffsets says, packed and padded rows give the same file
#include "pifusion.h"
#include "deflate_rle.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace pf {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
const char* last_error() { return g_err.c_str(); }
}
extern "C" const char* pf_last_error(void) { return pf::last_error(); }

static bool slurp(const std::string& path, std::vector<uint8_t>& out)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[65536]; size_t n;
    out.clear();
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}
static uint64_t le(const std::vector<uint8_t>& b, size_t at, int n) { uint64_t v = 0; for (int i = 0; i < n && at + i < b.size(); i++) v |= (uint64_t)b[at + i] << (8 * i); return v; }

// the first IFD's value of a tag that fits its entry (classic TIFF)
static long tag_value(const std::vector<uint8_t>& b, int tag)
{
    const uint64_t ifd = le(b, 4, 4), n = le(b, (size_t)ifd, 2);
    for (uint64_t i = 0; i < n; i++) {
        const size_t e = (size_t)(ifd + 2 + i * 12);
        if ((int)le(b, e, 2) == tag) return (long)le(b, e + 8, le(b, e + 2, 2) == 3 ? 2 : 4);
    }
    return -1;
}

int main(int argc, char** argv)
{
    if (argc < 4) { std::printf("usage: san_deflate <dir> <tiles> <images>\n"); return 2; }
    const std::string dir = argv[1];
    const int n_tiles = std::atoi(argv[2]), n_images = std::atoi(argv[3]);
    int fails = 0, streams = 0, files = 0;
    char name[64];
    const size_t bound = pf::dfl::kStreamBound;
    for (int i = 0; i < n_tiles; i++) {
        std::vector<uint8_t> px, want;
        std::snprintf(name, sizeof name, "/t%03d", i);
        if (!slurp(dir + name + ".bgr", px) || !slurp(dir + name + ".z", want) || px.size() != (size_t)pf::dfl::kTileBytes) { std::printf("MISMATCH tile %d: no input\n", i); fails++; continue; }
        for (size_t step : { (size_t)768, (size_t)768 + 11 }) {
            const size_t bytes = 255 * step + 768;
            std::unique_ptr<uint8_t[]> tile(new uint8_t[bytes]);
            std::memset(tile.get(), 0x5A, bytes);
            for (int y = 0; y < 256; y++) std::memcpy(tile.get() + (size_t)y * step, px.data() + (size_t)y * 768, 768);
            std::unique_ptr<uint8_t[]> out(new uint8_t[bound]);
            size_t len = 0;
            if (!pf_deflate_tile_bgr(tile.get(), step == 768 ? 0 : step, out.get(), bound, &len) || len != want.size() || std::memcmp(out.get(), want.data(), len) != 0) {
                std::printf("MISMATCH tile %d step %zu: %zu bytes, the model has %zu\n", i, step, len, want.size()); fails++;
            }
            streams++;
        }
    }
    const double xf[16] = { 0.5, 0, 0, 10, 0, 0.5, 0, 20, 0, 0, 1, 0, 0, 0, 0, 1 };
    const std::string f1 = dir + "/a.tif", f2 = dir + "/b.tif";
    for (int i = 0; i < n_images; i++) {
        std::snprintf(name, sizeof name, "/i%03d", i);
        std::vector<uint8_t> txt, px, msk, want;
        int rows = 0, cols = 0, bg = 0, masked = 0;
        if (!slurp(dir + name + ".txt", txt) || !slurp(dir + name + ".bgr", px) || !slurp(dir + name + ".msk", msk) || !slurp(dir + name + ".z", want)) { std::printf("MISMATCH image %d: no input\n", i); fails++; continue; }
        txt.push_back(0);
        if (std::sscanf((const char*)txt.data(), "%d %d %d %d", &rows, &cols, &bg, &masked) != 4 || px.size() != (size_t)rows * cols * 3 || msk.size() != (size_t)rows * cols) {
            std::printf("MISMATCH image %d: bad input\n", i); fails++; continue;
        }
        std::vector<uint8_t> file[2];
        for (int padded = 0; padded < 2; padded++) {
            const size_t step = (size_t)cols * 3 + (padded ? 7 : 0), mstep = (size_t)cols + (padded ? 3 : 0);
            const size_t bytes = (size_t)(rows - 1) * step + (size_t)cols * 3, mbytes = (size_t)(rows - 1) * mstep + cols;
            std::unique_ptr<uint8_t[]> img(new uint8_t[bytes]), m(new uint8_t[mbytes]);
            std::memset(img.get(), 0x5A, bytes); std::memset(m.get(), 0xC3, mbytes);
            for (int y = 0; y < rows; y++) { std::memcpy(img.get() + (size_t)y * step, px.data() + (size_t)y * cols * 3, (size_t)cols * 3); std::memcpy(m.get() + (size_t)y * mstep, msk.data() + (size_t)y * cols, cols); }
            const std::string& f = padded ? f2 : f1;
            if (!pf_tiff_write_bgr_lossless(f.c_str(), img.get(), rows, cols, padded ? step : 0, masked ? m.get() : nullptr, padded ? mstep : 0, bg, i % 2 ? xf : nullptr, 0) || !slurp(f, file[padded])) {
                std::printf("MISMATCH image %d: the writer failed: %s\n", i, pf_last_error()); fails++; break;
            }
            files++;
        }
        if (file[0].empty() || file[0] != file[1]) { std::printf("MISMATCH image %d: packed and padded rows give two files\n", i); fails++; continue; }
        if (rows <= 256 && cols <= 256) {          // one image, one tile: its stream is the model's
            const long off = tag_value(file[0], 324), len = tag_value(file[0], 325);
            if (tag_value(file[0], 259) != 8 || tag_value(file[0], 317) != 2 || off < 8 || len != (long)want.size() || (size_t)(off + len) > file[0].size() ||
                std::memcmp(file[0].data() + off, want.data(), (size_t)len) != 0) { std::printf("MISMATCH image %d: the tile's stream is not the model's\n", i); fails++; }
        }
    }
    // bad calls leave no file; the length builder refuses what it cannot do and writes exactly n lengths
    const std::string bad = dir + "/missing/x.tif";
    uint8_t one[3] = { 1, 2, 3 };
    if (pf_tiff_write_bgr_lossless(bad.c_str(), one, 1, 1, 0, nullptr, 0, 0, nullptr, 0) || pf_tiff_write_bgr_lossless(f1.c_str(), one, 1, 1, 2, nullptr, 0, 0, nullptr, 0)) { std::printf("MISMATCH: a bad call succeeded\n"); fails++; }
    for (int n : { 2, 19, 286, 288 }) {
        std::unique_ptr<uint32_t[]> freq(new uint32_t[n]);
        std::unique_ptr<uint8_t[]> out(new uint8_t[n]);
        for (int k = 0; k < n; k++) freq[k] = (uint32_t)(k * 2654435761u) >> (k % 29);
        if (!pf_deflate_code_lengths(freq.get(), n, n <= 19 ? 7 : 15, out.get())) { std::printf("MISMATCH: the length builder refused n = %d\n", n); fails++; }
    }
    uint32_t f1c[1] = { 5 }; uint8_t o1[1];
    if (pf_deflate_code_lengths(f1c, 1, 15, o1)) { std::printf("MISMATCH: the length builder took n = 1\n"); fails++; }
    std::printf("tiles %d streams %d images %d files %d fails %d\n", n_tiles, streams, n_images, files, fails);
    return fails ? 1 : 0;
}
