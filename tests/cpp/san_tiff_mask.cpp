// san_tiff_mask.cpp -- the host writer of the masked pyramid TIFF (csrc/tiff_pyramid.hpp behind pf_tiff_write_bgr_masked) under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Image and mask are heap blocks of exactly the bytes the call may read
// ((rows - 1) * step + a row), so one byte read past either is a finding.
//   san_tiff_mask <dir>   the sweep of tests/test_tiff_mask.py (five sizes x six kinds of mask) and every size 1...40 x 1...40 with
//                         random masks: packed and padded rows give the same file, the header is what the flag says, the chain
//                         has two IFDs per image, an all-covered mask leaves the unmasked writer's colour tags alone, and the
//                         unmasked writer writes the same file before and after.  Bad calls leave no file.
#include "pifusion.h"
#include "tiff_pyramid.hpp"
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
static bool exists(const std::string& p) { FILE* f = std::fopen(p.c_str(), "rb"); if (f) std::fclose(f); return f != nullptr; }

// the IFDs of the chain: (NewSubfileType, BitsPerSample count) of each
static std::vector<std::pair<int, int>> chain(const std::vector<uint8_t>& b, bool big)
{
    const int osz = big ? 8 : 4, esz = big ? 20 : 12;
    std::vector<std::pair<int, int>> out;
    uint64_t ifd = le(b, big ? 8 : 4, osz);
    while (ifd && ifd + 2 < b.size() && out.size() < 64) {
        const uint64_t n = le(b, (size_t)ifd, big ? 8 : 2);
        int sub = -1, bits = -1;
        for (uint64_t i = 0; i < n; i++) {
            const size_t e = (size_t)(ifd + (big ? 8 : 2) + i * esz);
            const uint64_t tag = le(b, e, 2);
            if (tag == 254) sub = (int)le(b, e + 4 + osz, 4);
            if (tag == 258) bits = (int)le(b, e + 4, osz);
        }
        out.push_back({ sub, bits });
        ifd = le(b, (size_t)(ifd + (big ? 8 : 2) + n * esz), osz);
    }
    return out;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: san_tiff_mask <dir>\n"); return 2; }
    const std::string dir = argv[1];
    int fails = 0, files = 0;
    uint32_t s = 97531;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 24; };
    struct Case { int rows, cols, kind; };          // kind: 0 all, 1 none, 2 disc, 3 random, 4 the last pixel alone, 5 a single hole
    std::vector<Case> cases;
    for (auto p : { std::pair<int, int>{ 1, 1 }, { 255, 257 }, { 256, 256 }, { 257, 513 }, { 300, 1000 } })
        for (int k = 0; k < 6; k++) cases.push_back({ p.first, p.second, k });
    for (int r = 1; r <= 40; r++) for (int c = 1; c <= 40; c++) cases.push_back({ r, c, 3 });
    const double xf[16] = { 0.5, 0, 0, 10, 0, 0.5, 0, 20, 0, 0, 1, 0, 0, 0, 0, 1 };
    for (const Case& cs : cases) {
        const int rows = cs.rows, cols = cs.cols, q = 1 + (rows * 41 + cols) % 100, bg = (rows + cols) % 3 == 0 ? 255 : 0;
        const size_t step = (size_t)cols * 3 + (size_t)((rows + cols) % 5), mstep = (size_t)cols + (size_t)((rows * 3 + cols) % 7);
        std::unique_ptr<uint8_t[]> packed(new uint8_t[(size_t)rows * cols * 3]), padded(new uint8_t[(size_t)(rows - 1) * step + (size_t)cols * 3]);
        std::unique_ptr<uint8_t[]> mp(new uint8_t[(size_t)rows * cols]), mw(new uint8_t[(size_t)(rows - 1) * mstep + (size_t)cols]);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols * 3; x++) {
                const uint8_t v = (rows % 7 == 0) ? (uint8_t)bg : (uint8_t)rnd();
                padded[(size_t)y * step + x] = v; packed[(size_t)y * cols * 3 + x] = v;
            }
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols; x++) {
                uint8_t v;
                const double dy = (y - rows / 2.0) / (rows / 2.2 + 1), dx = (x - cols / 2.0) / (cols / 2.2 + 1);
                switch (cs.kind) {
                case 0: v = 255; break;
                case 1: v = 0; break;
                case 2: v = dy * dy + dx * dx <= 1 ? 9 : 0; break;
                case 3: v = (rnd() & 1) ? (uint8_t)(1 + rnd() % 255) : 0; break;
                case 4: v = y == rows - 1 && x == cols - 1 ? 128 : 0; break;
                default: v = y == rows / 2 && x == cols / 3 ? 0 : 1; break;
                }
                mw[(size_t)y * mstep + x] = v; mp[(size_t)y * cols + x] = v;
            }
        const bool big = (rows ^ cols) & 1;
        const double* t = cols % 2 ? xf : nullptr;
        const std::string fa = dir + "/ma.tif", fb = dir + "/mb.tif", fu = dir + "/u.tif", fv = dir + "/v.tif";
        std::vector<uint8_t> a, b, u, v;
        if (!pf_tiff_write_bgr(fu.c_str(), packed.get(), rows, cols, 0, q, bg, t, big) ||
            !pf_tiff_write_bgr_masked(fa.c_str(), packed.get(), rows, cols, 0, mp.get(), 0, q, bg, t, big) ||
            !pf_tiff_write_bgr_masked(fb.c_str(), padded.get(), rows, cols, step, mw.get(), mstep, q, bg, t, big) ||
            !pf_tiff_write_bgr(fv.c_str(), padded.get(), rows, cols, step, q, bg, t, big) ||
            !slurp(fa, a) || !slurp(fb, b) || !slurp(fu, u) || !slurp(fv, v) || a != b || a.size() < 16 || (a.size() & 1)) {
            std::printf("MISMATCH packed / padded %d x %d kind %d: %s\n", rows, cols, cs.kind, pf_last_error()); fails++; continue;
        }
        if (u != v) { std::printf("MISMATCH the unmasked file changed %d x %d\n", rows, cols); fails++; }
        if (a[0] != 'I' || a[1] != 'I' || a[2] != (big ? 43 : 42)) { std::printf("MISMATCH header %d x %d\n", rows, cols); fails++; }
        const std::vector<pf::tiff::Level> lv = pf::tiff::levels(rows, cols);
        const auto ch = chain(a, big), cu = chain(u, big);
        bool ok = ch.size() == 2 * lv.size() && cu.size() == lv.size();
        for (size_t k = 0; ok && k < lv.size(); k++)
            ok = ch[2 * k] == cu[k] && ch[2 * k].first == (k ? 1 : 0) && ch[2 * k].second == 3 && ch[2 * k + 1].first == (k ? 5 : 4) && ch[2 * k + 1].second == 1;
        if (!ok) { std::printf("MISMATCH chain %d x %d\n", rows, cols); fails++; }
        if (a.size() < u.size() + pf::tiff::kMaskTileBytes) { std::printf("MISMATCH size %d x %d\n", rows, cols); fails++; }
        files++;
    }
    const std::string gone = dir + "/no/such/dir/x.tif", z = dir + "/z.tif";
    uint8_t px[3] = { 1, 2, 3 }, m1[1] = { 1 };
    if (pf_tiff_write_bgr_masked(gone.c_str(), px, 1, 1, 0, m1, 0, 95, 0, nullptr, 0) || pf_tiff_write_bgr_masked(z.c_str(), px, 1, 1, 2, m1, 0, 95, 0, nullptr, 0) ||
        pf_tiff_write_bgr_masked(z.c_str(), px, 1, 1, 0, nullptr, 0, 95, 0, nullptr, 0) || pf_tiff_write_bgr_masked(z.c_str(), px, 1, 1, 0, m1, 0, 95, 0, nullptr, 0) != 1 ||
        !exists(z) || std::remove(z.c_str()) != 0 || exists(gone)) { std::printf("MISMATCH bad calls\n"); fails++; }
    std::printf("files %d fails %d\n", files, fails);
    return fails ? 1 : 0;
}
