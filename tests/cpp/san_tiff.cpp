// san_tiff.cpp -- the host writer of the tiled pyramid TIFF (csrc/tiff_pyramid.hpp behind pf_tiff_write_bgr / pf_write_image)
// under AddressSanitizer + UndefinedBehaviorSanitizer.  Every image is a heap block of exactly (rows - 1) * step + cols * 3
// bytes, so one byte read past it is a finding.
//   san_tiff <dir>     every size 1...40 x 1...40 and a few around the tile edge: packed and padded rows give the same file,
//                      classic and BigTIFF headers are what they say, the first tile's stream decodes at 256 x 256, a file
//                      that cannot be opened leaves none.  And the route of a save (save_route, image_io.cpp) for every kind of name,
//                      single-band and multi-band.
#include "pifusion.h"
#include "image_io.hpp"
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
static uint64_t le(const std::vector<uint8_t>& b, size_t at, int n) { uint64_t v = 0; for (int i = 0; i < n && at + i < b.size(); i++) v |= (uint64_t)b[at + i] << (8 * i); return v; }

// the first tile's (offset, bytes) of the first image: tags 324 / 325 of the IFD the header points at
static bool first_tile(const std::vector<uint8_t>& b, bool big, uint64_t* off, uint64_t* len)
{
    const int osz = big ? 8 : 4, esz = big ? 20 : 12;
    const uint64_t ifd = le(b, big ? 8 : 4, osz), n = le(b, ifd, big ? 8 : 2);
    bool a = false, c = false;
    for (uint64_t i = 0; i < n; i++) {
        const size_t e = (size_t)(ifd + (big ? 8 : 2) + i * esz);
        const uint64_t tag = le(b, e, 2), type = le(b, e + 2, 2), cnt = le(b, e + 4, osz);
        const int ts = type == 16 ? 8 : type == 4 ? 4 : 2;
        const size_t at = ts * cnt <= (uint64_t)osz ? e + 4 + osz : (size_t)le(b, e + 4 + osz, osz);
        if (tag == 324) { *off = le(b, at, ts); a = true; }
        if (tag == 325) { *len = le(b, at, ts); c = true; }
    }
    return a && c && *off + *len <= b.size();
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: san_tiff <dir>\n"); return 2; }
    const std::string dir = argv[1];
    int fails = 0, files = 0;
    uint32_t s = 4321;
    std::vector<std::pair<int, int>> sizes;
    for (int r = 1; r <= 40; r++) for (int c = 1; c <= 40; c++) sizes.push_back({ r, c });
    for (auto p : { std::pair<int, int>{ 255, 257 }, { 256, 256 }, { 257, 255 }, { 300, 520 }, { 1, 600 }, { 513, 2 } }) sizes.push_back(p);
    const double xf[16] = { 0.5, 0, 0, 10, 0, 0.5, 0, 20, 0, 0, 1, 0, 0, 0, 0, 1 };
    for (auto sz : sizes) {
        const int rows = sz.first, cols = sz.second, q = 1 + (rows * 41 + cols) % 100, bg = (rows + cols) % 3 == 0 ? 255 : 0;
        const size_t step = (size_t)cols * 3 + (size_t)((rows + cols) % 5);
        std::unique_ptr<uint8_t[]> packed(new uint8_t[(size_t)rows * cols * 3]), padded(new uint8_t[(size_t)(rows - 1) * step + (size_t)cols * 3]);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < cols * 3; x++) {
                s = s * 1664525u + 1013904223u;
                const uint8_t v = (rows % 7 == 0) ? (uint8_t)bg : (uint8_t)(s >> 24);
                padded[(size_t)y * step + x] = v; packed[(size_t)y * cols * 3 + x] = v;
            }
        const bool big = (rows ^ cols) & 1;
        const std::string fa = dir + "/a.tif", fb = dir + "/b.TIFF";
        std::vector<uint8_t> a, b;
        if (!pf_tiff_write_bgr(fa.c_str(), packed.get(), rows, cols, 0, q, bg, cols % 2 ? xf : nullptr, big) || !pf_tiff_write_bgr(fb.c_str(), padded.get(), rows, cols, step, q, bg, cols % 2 ? xf : nullptr, big) ||
            !slurp(fa, a) || !slurp(fb, b) || a != b || a.size() < 16 || (a.size() & 1)) { std::printf("MISMATCH packed / padded %d x %d: %s\n", rows, cols, pf_last_error()); fails++; continue; }
        if (a[0] != 'I' || a[1] != 'I' || a[2] != (big ? 43 : 42)) { std::printf("MISMATCH header %d x %d\n", rows, cols); fails++; }
        uint64_t off = 0, len = 0; int r = 0, c = 0, k = 0;
        if (!first_tile(a, big, &off, &len) || (off & 1) || !pf::jpeg_info(a.data() + off, (size_t)len, &r, &c, &k) || r != 256 || c != 256 || k != 3) { std::printf("MISMATCH first tile %d x %d\n", rows, cols); fails++; }
        if (bg == 0 && q == 95 && !big && cols % 2 == 0) {          // pf_write_image: quality 95, background 0, no geo tags
            const std::string fc = dir + "/c.tif";
            std::vector<uint8_t> c2;
            if (!pf_write_image(fc.c_str(), packed.get(), rows, cols) || !slurp(fc, c2) || c2 != a) { std::printf("MISMATCH pf_write_image %d x %d\n", rows, cols); fails++; }
        }
        files++;
    }
    const std::string gone = dir + "/no/such/dir/x.tif";
    uint8_t px[3] = { 1, 2, 3 };
    if (pf_tiff_write_bgr(gone.c_str(), px, 1, 1, 0, 95, 0, nullptr, 0) || pf_tiff_write_bgr((dir + "/z.tif").c_str(), px, 1, 1, 2, 95, 0, nullptr, 0)) { std::printf("MISMATCH a bad call succeeded\n"); fails++; }
    // who writes save(name): the extension decides, in either case; the GPU encoders serve multi-band maps only
    using R = pf::SaveRoute;
    const struct { const char* name; R multi, single; } routes[] = {
        { "m.png", R::HostImage, R::HostImage }, { "m.PPM", R::HostImage, R::HostImage }, { "m.jpg", R::DeviceJpeg, R::HostImage }, { "m.JPEG", R::DeviceJpeg, R::HostImage },
        { "m.tif", R::DeviceTiff, R::HostTiffGeo }, { "m.TIFF", R::DeviceTiff, R::HostTiffGeo }, { "mosaic", R::HostImage, R::HostImage },
        { "dir.tif/m", R::HostImage, R::HostImage }, { ".jpg", R::DeviceJpeg, R::HostImage }, { "tif", R::HostImage, R::HostImage }, { "", R::HostImage, R::HostImage },
    };
    for (auto& r : routes)
        if (pf::save_route(r.name, false) != r.multi || pf::save_route(r.name, true) != r.single) { std::printf("MISMATCH route of \"%s\"\n", r.name); fails++; }
    if (pf::tiff_route(false) != R::DeviceTiff || pf::tiff_route(true) != R::HostTiffGeo || !pf::route_on_device(R::DeviceJpeg) || !pf::route_on_device(R::DeviceTiff) ||
        pf::route_on_device(R::HostTiffGeo) || pf::route_on_device(R::HostImage)) { std::printf("MISMATCH tiff_route / route_on_device\n"); fails++; }
    std::printf("files %d fails %d\n", files, fails);
    return fails ? 1 : 0;
}
