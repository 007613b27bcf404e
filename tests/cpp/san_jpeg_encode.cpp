// san_jpeg_encode.cpp -- the host JPEG encoder (csrc/jpeg_encode.hpp behind pf_jpeg_encode_bgr / pf_write_image) under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Every output buffer is a heap block of exactly the stream's length and every
// image a heap block of exactly rows * step bytes, so one byte read or written past either is a finding.
//   san_jpeg_encode <dir> <n>     dir holds vNN.bgr (packed pixels), vNN.txt ("rows cols quality"), vNN.jpg (the expected stream)
// Then every size 1...40 x 1...40, noise, at a quality that walks 1...100: the bound holds, a buffer one byte short is refused,
// a padded step gives the packed stream, and the project's decoder reads the stream back at the image's size.
#include "pifusion.h"
#include "jpeg_decode.hpp"
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

// encodes into a block of exactly the stream's length; empty on failure
static std::vector<uint8_t> encode_exact(const uint8_t* bgr, int rows, int cols, size_t step, int quality, int* fails)
{
    size_t bound = 0, len = 0;
    if (!pf_jpeg_encode_bgr(bgr, rows, cols, step, quality, nullptr, 0, &bound)) { std::printf("MISMATCH no bound %dx%d\n", rows, cols); ++*fails; return {}; }
    std::unique_ptr<uint8_t[]> big(new uint8_t[bound]);
    if (!pf_jpeg_encode_bgr(bgr, rows, cols, step, quality, big.get(), bound, &len) || len > bound) { std::printf("MISMATCH bound %dx%d q%d\n", rows, cols, quality); ++*fails; return {}; }
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len]);
    size_t len2 = 0;
    if (!pf_jpeg_encode_bgr(bgr, rows, cols, step, quality, exact.get(), len, &len2) || len2 != len || std::memcmp(exact.get(), big.get(), len)) {
        std::printf("MISMATCH exact buffer %dx%d q%d\n", rows, cols, quality); ++*fails; return {};
    }
    if (len > 1) {
        std::unique_ptr<uint8_t[]> small(new uint8_t[len - 1]);
        if (pf_jpeg_encode_bgr(bgr, rows, cols, step, quality, small.get(), len - 1, &len2) || len2 != len) { std::printf("MISMATCH short buffer accepted %dx%d\n", rows, cols); ++*fails; }
    }
    return std::vector<uint8_t>(exact.get(), exact.get() + len);
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::printf("usage: san_jpeg_encode <dir> <n>\n"); return 2; }
    const std::string dir = argv[1];
    const int n = std::atoi(argv[2]);
    int fails = 0, vec_ok = 0, sizes = 0; long bytes = 0;
    for (int i = 0; i < n; i++) {
        char name[64];
        std::vector<uint8_t> px, want, txt;
        std::snprintf(name, sizeof name, "/v%02d", i);
        if (!slurp(dir + name + ".bgr", px) || !slurp(dir + name + ".jpg", want) || !slurp(dir + name + ".txt", txt)) { std::printf("MISMATCH cannot read vector %d\n", i); return 1; }
        txt.push_back(0);
        int rows = 0, cols = 0, q = 0;
        if (std::sscanf((const char*)txt.data(), "%d %d %d", &rows, &cols, &q) != 3 || px.size() != (size_t)rows * cols * 3) { std::printf("MISMATCH vector %d's description\n", i); return 1; }
        std::unique_ptr<uint8_t[]> img(new uint8_t[px.size()]);
        std::memcpy(img.get(), px.data(), px.size());
        const std::vector<uint8_t> got = encode_exact(img.get(), rows, cols, 0, q, &fails);
        if (got != want) { std::printf("MISMATCH vector %d (%d x %d, quality %d)\n", i, rows, cols, q); fails++; } else vec_ok++;
        const std::string f = dir + name + "_out.JPG";
        if (q == 95 && (!pf_write_image(f.c_str(), img.get(), rows, cols) || !slurp(f, txt) || txt != want)) { std::printf("MISMATCH pf_write_image vector %d\n", i); fails++; }
    }
    uint32_t s = 12345;
    for (int rows = 1; rows <= 40; rows++)
        for (int cols = 1; cols <= 40; cols++) {
            const int q = 1 + (rows * 41 + cols) % 100;
            const size_t step = (size_t)cols * 3 + (size_t)((rows + cols) % 5);
            std::unique_ptr<uint8_t[]> packed(new uint8_t[(size_t)rows * cols * 3]), padded(new uint8_t[(size_t)rows * step]);
            for (int y = 0; y < rows; y++)
                for (int x = 0; x < (int)step; x++) {
                    s = s * 1664525u + 1013904223u;
                    const uint8_t v = (rows % 7 == 0) ? (uint8_t)(x * 3 + y) : (uint8_t)(s >> 24);
                    padded[(size_t)y * step + x] = v;
                    if (x < cols * 3) packed[(size_t)y * cols * 3 + x] = v;
                }
            const std::vector<uint8_t> a = encode_exact(packed.get(), rows, cols, 0, q, &fails), b = encode_exact(padded.get(), rows, cols, step, q, &fails);
            if (a.empty() || a != b) { std::printf("MISMATCH padded step %d x %d\n", rows, cols); fails++; }
            int r = 0, c = 0, k = 0;
            std::unique_ptr<uint8_t[]> back(new uint8_t[(size_t)rows * cols * 3]);
            if (!pf::jpeg_info(a.data(), a.size(), &r, &c, &k) || r != rows || c != cols || k != 3 || !pf::jpeg_decode_bgr(a.data(), a.size(), back.get(), rows, cols, (size_t)cols * 3)) {
                std::printf("MISMATCH decode back %d x %d: %s\n", rows, cols, pf_last_error()); fails++;
            }
            sizes++; bytes += (long)a.size();
        }
    std::printf("vectors %d sizes %d bytes %ld fails %d\n", vec_ok, sizes, bytes, fails);
    return fails ? 1 : 0;
}
