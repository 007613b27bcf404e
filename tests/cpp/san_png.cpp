// san_png.cpp -- the scalar encoder of the PNG of save_png (csrc/png_encode.hpp behind pf_png_encode_bgr), its checksum functions and the
// host writer of single-band maps (pf::write_png_file) under AddressSanitizer + UndefinedBehaviorSanitizer.  Images and masks are heap
// blocks of exactly the bytes a call may read ((rows - 1) * step + a row), the output block has exactly the bound: one byte past any of
// them is a finding.
//   san_png <dir> <cases>
//     cNNN.txt / .bgr / .msk / .png   an image (rows cols masked), its pixels, its mask and the file by tests/png_model.py: the encoder
//                                     gives that file, packed and with padded steps, and the writer writes it
#include "pifusion.h"
#include "image_io.hpp"
#include "png_encode.hpp"
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

int main(int argc, char** argv)
{
    if (argc < 3) { std::printf("usage: san_png <dir> <cases>\n"); return 2; }
    const std::string dir = argv[1];
    const int n_cases = std::atoi(argv[2]);
    int fails = 0, files = 0, written = 0, sums = 0;
    char name[64];
    const std::string f1 = dir + "/a.png";
    for (int i = 0; i < n_cases; i++) {
        std::snprintf(name, sizeof name, "/c%03d", i);
        std::vector<uint8_t> txt, px, msk, want, back;
        int rows = 0, cols = 0, masked = 0;
        if (!slurp(dir + name + ".txt", txt) || !slurp(dir + name + ".bgr", px) || !slurp(dir + name + ".msk", msk) || !slurp(dir + name + ".png", want)) { std::printf("MISMATCH case %d: no input\n", i); fails++; continue; }
        txt.push_back(0);
        if (std::sscanf((const char*)txt.data(), "%d %d %d", &rows, &cols, &masked) != 3 || px.size() != (size_t)rows * cols * 3 || msk.size() != (size_t)rows * cols) {
            std::printf("MISMATCH case %d: bad input\n", i); fails++; continue;
        }
        for (int padded = 0; padded < 2; padded++) {
            const size_t step = (size_t)cols * 3 + (padded ? 7 : 0), mstep = (size_t)cols + (padded ? 3 : 0);
            const size_t bytes = (size_t)(rows - 1) * step + (size_t)cols * 3, mbytes = (size_t)(rows - 1) * mstep + cols;
            std::unique_ptr<uint8_t[]> img(new uint8_t[bytes]), m(new uint8_t[mbytes]);
            std::memset(img.get(), 0x5A, bytes); std::memset(m.get(), 0xC3, mbytes);
            for (int y = 0; y < rows; y++) { std::memcpy(img.get() + (size_t)y * step, px.data() + (size_t)y * cols * 3, (size_t)cols * 3); std::memcpy(m.get() + (size_t)y * mstep, msk.data() + (size_t)y * cols, cols); }
            const uint8_t* mk = masked ? m.get() : nullptr;
            size_t bound = 0, len = 0;
            if (!pf_png_encode_bgr(img.get(), rows, cols, padded ? step : 0, mk, padded ? mstep : 0, nullptr, 0, &bound) || bound < want.size()) { std::printf("MISMATCH case %d: bound %zu\n", i, bound); fails++; continue; }
            std::unique_ptr<uint8_t[]> out(new uint8_t[bound]);
            if (!pf_png_encode_bgr(img.get(), rows, cols, padded ? step : 0, mk, padded ? mstep : 0, out.get(), bound, &len) || len != want.size() || std::memcmp(out.get(), want.data(), len) != 0) {
                std::printf("MISMATCH case %d step %zu: %zu bytes, the model has %zu\n", i, step, len, want.size()); fails++;
            }
            files++;
            // an output block of exactly the file: it fits; one byte less: refused, the length reported
            std::unique_ptr<uint8_t[]> tight(new uint8_t[want.size()]);
            if (!pf_png_encode_bgr(img.get(), rows, cols, padded ? step : 0, mk, padded ? mstep : 0, tight.get(), want.size(), &len) || len != want.size()) { std::printf("MISMATCH case %d: the exact cap was refused\n", i); fails++; }
            if (pf_png_encode_bgr(img.get(), rows, cols, padded ? step : 0, mk, padded ? mstep : 0, tight.get(), want.size() - 1, &len) || len != want.size()) { std::printf("MISMATCH case %d: a short cap was taken\n", i); fails++; }
            // the host writer of single-band maps
            if (!pf::write_png_file("san_png", f1.c_str(), img.get(), rows, cols, padded ? step : 0, mk, padded ? mstep : 0) || !slurp(f1, back) || back != want) {
                std::printf("MISMATCH case %d: the writer's file is not the model's: %s\n", i, pf_last_error()); fails++;
            }
            written++;
        }
        // the checksums over the file itself: any split gives the whole
        const size_t n = want.size();
        const uint32_t crc = pf_png_crc32(0, want.data(), n), ad = pf_png_adler32(want.data(), n);
        for (size_t cut : { (size_t)0, (size_t)1, n / 3, n / 2, n - 1, n }) {
            if (cut > n) continue;
            std::unique_ptr<uint8_t[]> a(new uint8_t[cut ? cut : 1]), b(new uint8_t[n - cut ? n - cut : 1]);
            std::memcpy(a.get(), want.data(), cut); std::memcpy(b.get(), want.data() + cut, n - cut);
            const uint32_t ca = pf_png_crc32(0, a.get(), cut), cb = pf_png_crc32(0, b.get(), n - cut);
            if (pf_png_crc32_combine(ca, cb, n - cut) != crc || pf_png_crc32(ca, b.get(), n - cut) != crc) { std::printf("MISMATCH case %d: CRC combine at %zu\n", i, cut); fails++; }
            if (pf_png_adler32_combine(pf_png_adler32(a.get(), cut), pf_png_adler32(b.get(), n - cut), n - cut) != ad) { std::printf("MISMATCH case %d: Adler combine at %zu\n", i, cut); fails++; }
            sums++;
        }
    }
    // bad calls: no file is left, nothing is written
    const std::string bad = dir + "/missing/x.png";
    uint8_t one[3] = { 1, 2, 3 }, o[64]; size_t len = 0;
    if (pf::write_png_file("san_png", bad.c_str(), one, 1, 1, 0, nullptr, 0) || pf::write_png_file("san_png", f1.c_str(), one, 1, 1, 2, nullptr, 0) ||
        pf_png_encode_bgr(nullptr, 1, 1, 0, nullptr, 0, o, sizeof o, &len) || pf_png_encode_bgr(one, 0, 1, 0, nullptr, 0, o, sizeof o, &len) || pf_png_encode_bgr(one, 1, 1, 2, nullptr, 0, o, sizeof o, &len) ||
        pf_png_encode_bgr(one, 1, 1, 0, nullptr, 0, o, sizeof o, nullptr)) { std::printf("MISMATCH: a bad call succeeded\n"); fails++; }
    std::printf("cases %d files %d written %d sums %d fails %d\n", n_cases, files, written, sums, fails);
    return fails ? 1 : 0;
}
