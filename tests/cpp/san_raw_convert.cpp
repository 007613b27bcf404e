// san_raw_convert.cpp -- the host raw-frame converter (csrc/raw_convert.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer.
// usage: san_raw_convert <dir> <n>.  Case i: <dir>/c%03d.txt holds "format rows cols", c%03d.p0 .. .p2 the packed planes, c%03d.bgr the packed
// picture the numpy model gives.  Every plane and the destination are heap buffers of exactly the bytes the descriptor promises -- packed, and
// again with a row step 3 bytes longer than the row, where the last row still ends with its last pixel -- so that one byte read or written
// past a row's end is the sanitizer's.  Refused descriptors must leave the destination alone.
#include "raw_convert.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::vector<uint8_t> slurp(const std::string& path)
{
    std::vector<uint8_t> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return v;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

// the converter as pf_raw_to_bgr runs it
static bool convert(const pf_raw_frame& f, uint8_t* bgr, size_t step)
{
    std::string why;
    if (!pf::raw::check(f, why) || !pf::raw::check_bgr(f, step, why)) return false;
    pf::raw::to_bgr_host(f, bgr, step);
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: san_raw_convert <dir> <n>\n"); return 2; }
    const std::string dir = argv[1];
    const int n = std::atoi(argv[2]);
    int done = 0, bad = 0;
    for (int i = 0; i < n; i++) {
        char stem[32];
        std::snprintf(stem, sizeof stem, "/c%03d", i);
        const std::vector<uint8_t> txt = slurp(dir + stem + ".txt");
        pf_raw_frame f{};
        if (std::sscanf(std::string(txt.begin(), txt.end()).c_str(), "%d %d %d", &f.format, &f.rows, &f.cols) != 3) { std::printf("MISMATCH case %d: no header\n", i); bad++; continue; }
        const std::vector<uint8_t> want = slurp(dir + stem + ".bgr");
        const int np = pf::raw::planes_of(f.format);
        std::vector<uint8_t> packed[3];
        for (int k = 0; k < np; k++) packed[k] = slurp(dir + stem + ".p" + std::to_string(k));
        for (int pad = 0; pad <= 3; pad += 3) {
            uint8_t* heap[3] = { nullptr, nullptr, nullptr };
            bool ok = true;
            for (int k = 0; k < np; k++) {
                const size_t row = pf::raw::plane_row(f, k);
                const int rows = pf::raw::plane_rows(f, k);
                if (packed[k].size() != row * (size_t)rows) { ok = false; break; }
                f.step[k] = pad ? row + pad : 0;
                const size_t step = row + pad, bytes = (size_t)(rows - 1) * step + row;
                heap[k] = (uint8_t*)std::malloc(bytes);
                std::memset(heap[k], 0xA5, bytes);
                for (int y = 0; y < rows; y++) std::memcpy(heap[k] + (size_t)y * step, packed[k].data() + (size_t)y * row, row);
                f.plane[k] = heap[k];
            }
            const size_t orow = (size_t)f.cols * 3, ostep = orow + pad, obytes = (size_t)(f.rows - 1) * ostep + orow;
            uint8_t* out = (uint8_t*)std::malloc(obytes);
            std::memset(out, 0xA5, obytes);
            if (!ok || want.size() != orow * (size_t)f.rows || !convert(f, out, pad ? ostep : 0)) { std::printf("MISMATCH case %d: refused or files of the wrong size\n", i); bad++; }
            else {
                for (int y = 0; y < f.rows; y++) {
                    if (std::memcmp(out + (size_t)y * ostep, want.data() + (size_t)y * orow, orow)) { std::printf("MISMATCH case %d pad %d row %d\n", i, pad, y); bad++; break; }
                    for (int b = 0; b < pad && y + 1 < f.rows; b++)
                        if (out[(size_t)y * ostep + orow + b] != 0xA5) { std::printf("MISMATCH case %d pad %d row %d: padding written\n", i, pad, y); bad++; y = f.rows; break; }
                }
                done++;
            }
            // refusals: nothing may be touched (the destination is one byte: any write is the sanitizer's)
            uint8_t* one = (uint8_t*)std::malloc(1);
            *one = 0xA5;
            pf_raw_frame g = f;
            g.format = 7;
            if (convert(g, one, 0)) { std::printf("MISMATCH case %d: format 7 accepted\n", i); bad++; }
            g = f; g.plane[np - 1] = nullptr;
            if (convert(g, one, 0)) { std::printf("MISMATCH case %d: missing plane accepted\n", i); bad++; }
            g = f; g.step[0] = (size_t)f.cols - 1;
            if (f.cols > 1 && convert(g, one, 0)) { std::printf("MISMATCH case %d: short step accepted\n", i); bad++; }
            if (convert(f, one, orow - 1)) { std::printf("MISMATCH case %d: short destination step accepted\n", i); bad++; }
            if (*one != 0xA5) { std::printf("MISMATCH case %d: a refusal wrote\n", i); bad++; }
            std::free(one);
            std::free(out);
            for (int k = 0; k < np; k++) std::free(heap[k]);
        }
    }
    std::printf("cases %d conversions %d bad %d\n", n, done, bad);
    return bad ? 1 : 0;
}
