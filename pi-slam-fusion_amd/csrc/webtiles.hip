// webtiles.hip -- north-up Web-Mercator map tiles from a mosaic in HBM (webtiles.hpp): the two kernels and the pyramid driver.
//
//   k_webtile_sample   tiles of the sampling zoom.  A workgroup of four waves takes 16 rows of a 64-column strip of one tile, a wave one
//                      row at a time, a lane one pixel: the source position is ONE fp64 add per axis of two table entries
//                      (webtiles_plan.hpp: the column's entries are loaded once per lane, the row's are wave-uniform), everything after
//                      it is integer arithmetic -- floor, an 8-bit fraction per axis, four taps weighted (256 - fx, fx) x (256 - fy, fy),
//                      renormalised over the taps that lie inside the image AND are covered, so that the background colour never bleeds
//                      into a ragged edge; less than half of the weight covered: background, uncovered.  The taps are byte gathers (the
//                      four of a pixel and those of the neighbouring lanes share cache lines: rows of the source run along the wave
//                      but for the yaw), all sixteen of a pixel issued before the first is used (profiles/webtiles.md).  A __ballot of "covered" is the 8 mask bytes of the row's strip, stored by one lane; the BGR
//                      bytes of 64 pixels leave as 48 dword stores, put together from the lanes' packed pixels by two shuffles.
//   k_webtile_reduce   tile (z - 1, X, Y) from its up to four children: a parent pixel is the rounded mean of the COVERED ones of the
//                      2 x 2 child pixels under it, covered where any is (the OR chain of the masked TIFF's overviews); same block shape
//                      and the same way out.
// Both clear the flags "no pixel covered" / "all covered" of the tile they write as coverage.hip does: bytes preset to 1 by the caller,
// cleared with a plain store by one lane of each workgroup that has a reason to.
//
// The driver (webtiles_export) keeps device memory independent of the mosaic's size but for the tiles of the zooms <= zmax - 3: the
// sampling-zoom tiles are made in groups of 8 x 8 under one ancestor, reduced three times, encoded (JpegEncoder::encode on the slots
// where they lie) and handed over, and only the ancestor's pixels are carried on; the zooms from there up are reduced level by level.
#include "webtiles.hpp"
#include "webtiles_plan.hpp"
#include <atomic>
#include <string>
#include <vector>

namespace pf {

void set_error(const std::string& msg);

namespace {

// the way out of both kernels for one row of a 64-column strip: v = the lane's pixel as b | g << 8 | r << 16
__device__ inline void store_strip_row(uint32_t v, bool covered, uint8_t* px_row, uint8_t* mask_row, int lane, bool& any, bool& all)
{
    const unsigned long long b = __ballot(covered ? 1 : 0);
    any = any || b != 0; all = all && b == ~0ull;
    // lane i is column i of the strip: bit-reversed, column 0 sits in bit 63, and byte-swapped its byte is the first in memory
    if (lane == 0) *(unsigned long long*)mask_row = __builtin_bswap64(__brevll(b));
    // dword l holds bytes 4 l .. 4 l + 3 of the row's 192: from pixel p0 = 4 l / 3 on, (4 l) % 3 bytes into it
    const int l = lane < 48 ? lane : 47, p0 = (4 * l) / 3;
    const uint32_t lo = (uint32_t)__shfl((int)v, p0), hi = (uint32_t)__shfl((int)v, p0 + 1 < 64 ? p0 + 1 : 63);
    const unsigned long long w = (unsigned long long)lo | ((unsigned long long)hi << 24);
    if (lane < 48) *(uint32_t*)(px_row + 4 * lane) = (uint32_t)(w >> (8 * ((4 * l) % 3)));
}

__device__ inline void clear_tile_flags(bool any, bool all, uint8_t* fzero, uint8_t* fone, size_t tile)
{
    const int a = __syncthreads_or(any ? 1 : 0), b = __syncthreads_and(all ? 1 : 0);
    if (threadIdx.x == 0) {
        if (a) fzero[tile] = 0;
        if (!b) fone[tile] = 0;
    }
}

__global__ __launch_bounds__(256) void k_webtile_sample(WebSampleSource s, int gx0, int gy0, int gw, int slot0, int pitch, uint8_t* __restrict__ px, uint8_t* __restrict__ mask,
                                                        uint8_t* __restrict__ fzero, uint8_t* __restrict__ fone)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti = (int)blockIdx.z % gw, tj = (int)blockIdx.z / gw;
    const size_t slot = (size_t)slot0 + (size_t)tj * pitch + ti;
    const long long c = 256ll * (gx0 + ti) + 64 * (int)blockIdx.x + lane - s.c0, r0 = 256ll * (gy0 + tj) - s.r0;
    const double ux = s.ux[c], uy = s.uy[c];
    const double xlim = (double)s.cols + 1.0, ylim = (double)s.rows + 1.0;
    const uint32_t bgv = (uint32_t)s.bg * 0x010101u;
    uint8_t* tpx = px + slot * kWebTilePixels + 192 * blockIdx.x;
    uint8_t* tmask = mask + slot * kWebTileMask + 8 * blockIdx.x;
    bool any = false, all = true;
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int row = 16 * (int)blockIdx.y + 4 * it + wave;
        const double sx = ux + s.vx[r0 + row], sy = uy + s.vy[r0 + row];
        // Every load of the row is issued before anything depends on one: a tap that does not count is read all the same, from the nearest
        // pixel inside the image (a position that is not near the image, or not a number -- it fails every comparison -- reads pixel (0, 0)),
        // and dropped by its weight.  A chain of "mask, then pixel" per tap is eight memory latencies a row, this is one
        const bool near = sx > -2.0 && sx < xlim && sy > -2.0 && sy < ylim;
        const double qx = near ? sx : 0.0, qy = near ? sy : 0.0;
        const double flx = floor(qx), fly = floor(qy);
        const int x0 = (int)flx, y0 = (int)fly;
        const int fx = min((int)((qx - flx) * 256.0), 255), fy = min((int)((qy - fly) * 256.0), 255);
        const int xa = min(max(x0, 0), s.cols - 1), xb = min(max(x0 + 1, 0), s.cols - 1), ya = min(max(y0, 0), s.rows - 1), yb = min(max(y0 + 1, 0), s.rows - 1);
        const bool ina = x0 >= 0 && x0 < s.cols, inb = x0 + 1 >= 0 && x0 + 1 < s.cols, inc = y0 >= 0 && y0 < s.rows, ind = y0 + 1 >= 0 && y0 + 1 < s.rows;
        const uint8_t* ma = s.mask + (size_t)ya * s.mask_step; const uint8_t* mb = s.mask + (size_t)yb * s.mask_step;
        const uint8_t* pa = s.bgr + (size_t)ya * s.step; const uint8_t* pb = s.bgr + (size_t)yb * s.step;
        const uint32_t m00 = ma[xa], m01 = ma[xb], m10 = mb[xa], m11 = mb[xb];
        const uint8_t *t00 = pa + 3 * (size_t)xa, *t01 = pa + 3 * (size_t)xb, *t10 = pb + 3 * (size_t)xa, *t11 = pb + 3 * (size_t)xb;
        const uint32_t b00 = t00[0], g00 = t00[1], r00 = t00[2], b01 = t01[0], g01 = t01[1], r01 = t01[2];
        const uint32_t b10 = t10[0], g10 = t10[1], r10 = t10[2], b11 = t11[0], g11 = t11[1], r11 = t11[2];
        const uint32_t w00 = near && ina && inc && m00 ? (uint32_t)((256 - fx) * (256 - fy)) : 0u, w01 = near && inb && inc && m01 ? (uint32_t)(fx * (256 - fy)) : 0u;
        const uint32_t w10 = near && ina && ind && m10 ? (uint32_t)((256 - fx) * fy) : 0u, w11 = near && inb && ind && m11 ? (uint32_t)(fx * fy) : 0u;
        const uint32_t den = w00 + w01 + w10 + w11;
        uint32_t v = bgv;
        const bool covered = 2 * den >= 65536u;
        if (covered) {
            const uint32_t h = den >> 1;
            v = ((w00 * b00 + w01 * b01 + w10 * b10 + w11 * b11 + h) / den) | (((w00 * g00 + w01 * g01 + w10 * g10 + w11 * g11 + h) / den) << 8) |
                (((w00 * r00 + w01 * r01 + w10 * r10 + w11 * r11 + h) / den) << 16);
        }
        store_strip_row(v, covered, tpx + (size_t)row * 768, tmask + (size_t)row * 32, lane, any, all);
    }
    clear_tile_flags(any, all, fzero, fone, slot);
}

__global__ __launch_bounds__(256) void k_webtile_reduce(const int* __restrict__ desc, const uint8_t* __restrict__ spx, const uint8_t* __restrict__ smask, const uint8_t* __restrict__ sfzero,
                                                        uint8_t* __restrict__ dpx, uint8_t* __restrict__ dmask, uint8_t* __restrict__ dfzero, uint8_t* __restrict__ dfone, uint32_t bgv)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* d = desc + 5 * (size_t)blockIdx.z;
    const size_t out = (size_t)d[4];
    // a strip of 64 columns and 16 rows of the parent lies under ONE child: columns 0 .. 127 under the left ones, rows 0 .. 127 under the upper
    const int child = d[2 * ((int)blockIdx.y >> 3) + ((int)blockIdx.x >> 1)];
    const bool present = child >= 0 && !sfzero[child];
    const uint8_t* cpx = spx + (size_t)(present ? child : 0) * kWebTilePixels;
    const uint8_t* cmask = smask + (size_t)(present ? child : 0) * kWebTileMask;
    const int cx = 2 * ((64 * (int)blockIdx.x + lane) & 127);
    uint8_t* tpx = dpx + out * kWebTilePixels + 192 * blockIdx.x;
    uint8_t* tmask = dmask + out * kWebTileMask + 8 * blockIdx.x;
    bool any = false, all = true;
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int row = 16 * (int)blockIdx.y + 4 * it + wave, cy = 2 * (row & 127);
        uint32_t n = 0, a0 = 0, a1 = 0, a2 = 0;
        if (present) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const uint32_t m = cmask[(size_t)(cy + j) * 32 + (cx >> 3)];          // columns cx and cx + 1 share a byte: bits 7 - (cx & 7) and the one below
                const uint16_t* p = (const uint16_t*)(cpx + (size_t)(cy + j) * 768 + 3 * (size_t)cx);          // six bytes at an even address
                const uint32_t q0 = p[0], q1 = p[1], q2 = p[2];
                if (m & (0x80u >> (cx & 7))) { n++; a0 += q0 & 255; a1 += q0 >> 8; a2 += q1 & 255; }
                if (m & (0x40u >> (cx & 7))) { n++; a0 += q1 >> 8; a1 += q2 & 255; a2 += q2 >> 8; }
            }
        }
        uint32_t v = bgv;
        if (n) { const uint32_t h = n >> 1; v = ((a0 + h) / n) | (((a1 + h) / n) << 8) | (((a2 + h) / n) << 16); }
        store_strip_row(v, n != 0, tpx + (size_t)row * 768, tmask + (size_t)row * 32, lane, any, all);
    }
    clear_tile_flags(any, all, dfzero, dfone, out);
}

std::atomic<int> g_batch_edge{ 8 };
std::atomic<bool> g_timing{ false };
double g_last_timing[4] = { 0, 0, 0, 0 };

}  // namespace

void launch_webtile_sample(hipStream_t s, const WebSampleSource& src, int gx0, int gy0, int gw, int gh, int slot0, int pitch, uint8_t* px, uint8_t* mask, uint8_t* fzero, uint8_t* fone)
{
    if (gw <= 0 || gh <= 0) return;
    hipLaunchKernelGGL(k_webtile_sample, dim3(4, 16, (unsigned)(gw * gh)), dim3(256), 0, s, src, gx0, gy0, gw, slot0, pitch, px, mask, fzero, fone);
}

void launch_webtile_reduce(hipStream_t s, const int* desc_dev, int n, const uint8_t* src_px, const uint8_t* src_mask, const uint8_t* src_fzero,
                           uint8_t* dst_px, uint8_t* dst_mask, uint8_t* dst_fzero, uint8_t* dst_fone, int bg)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_webtile_reduce, dim3(4, 16, (unsigned)n), dim3(256), 0, s, desc_dev, src_px, src_mask, src_fzero, dst_px, dst_mask, dst_fzero, dst_fone, (uint32_t)bg * 0x010101u);
}

void webtiles_set_batch(int edge) { g_batch_edge = edge >= 8 ? 8 : edge >= 4 ? 4 : 2; }
int  webtiles_batch() { return g_batch_edge; }
void webtiles_set_timing(bool on) { g_timing = on; }
void webtiles_last_timing(double out[4]) { for (int i = 0; i < 4; i++) out[i] = g_last_timing[i]; }

// ------------------------------------------------------------------------------------------------------------------ the driver
namespace {

#define WT_OK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { (void)hipGetLastError(); set_error(std::string("webtiles: ") + #x + ": " + hipGetErrorString(e_)); return false; } } while (0)

struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    bool alloc(size_t bytes) { if (p) (void)hipFree(p); p = nullptr; if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("webtiles: out of device memory (" + std::to_string(bytes) + " bytes)"); return false; } return true; }
    uint8_t* u8() const { return (uint8_t*)p; }
};
struct PinMem {
    void* p = nullptr;
    ~PinMem() { if (p) (void)hipHostFree(p); }
    bool alloc(size_t bytes) { if (p) (void)hipHostFree(p); p = nullptr; if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("webtiles: out of page-locked memory (" + std::to_string(bytes) + " bytes)"); return false; } return true; }
    uint8_t* u8() const { return (uint8_t*)p; }
};
// the buffers of a set of tile slots
struct TileSet {
    DevMem px, mask, fzero, fone;
    size_t n = 0;
    bool alloc(size_t slots) { n = slots; return px.alloc(slots * kWebTilePixels) && mask.alloc(slots * kWebTileMask) && fzero.alloc(slots) && fone.alloc(slots); }
};
struct Range { int x0, y0, x1, y1; Range up(int k) const { return Range{ x0 >> k, y0 >> k, x1 >> k, y1 >> k }; } bool has(int x, int y) const { return x >= x0 && x <= x1 && y >= y0 && y <= y1; } };

// event pairs around the launches of one part, summed once the stream has drained
struct Stopwatch {
    bool on; hipStream_t s; std::vector<hipEvent_t> ev[3];
    Stopwatch(bool on_, hipStream_t s_) : on(on_), s(s_) {}
    ~Stopwatch() { for (auto& v : ev) for (hipEvent_t e : v) (void)hipEventDestroy(e); }
    void mark(int part) { if (!on) return; hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; (void)hipEventRecord(e, s); ev[part].push_back(e); }
    double total(int part) { double ms = 0; for (size_t i = 0; i + 1 < ev[part].size(); i += 2) { float t = 0; if (hipEventElapsedTime(&t, ev[part][i], ev[part][i + 1]) == hipSuccess) ms += t; } return ms; }
};

struct Emitter {
    JpegEncoder& enc; hipStream_t s; int quality; bool want_pixels; pf_webtile_sink sink; void* user; Stopwatch& sw;
    std::vector<size_t> off;
    // the tiles `slots` of the set (z, x, y of each in zxy), whose flags, masks and -- if asked for -- pixels already lie in the host copies
    bool emit(const TileSet& set, const std::vector<int>& slots, const std::vector<int>& zxy, const uint8_t* fone_h, const uint8_t* mask_h, const uint8_t* px_h)
    {
        for (size_t at = 0; at < slots.size(); at += 64) {
            const int n = (int)std::min<size_t>(64, slots.size() - at);
            off.assign((size_t)n + 1, 0);
            sw.mark(2);
            const bool ok = enc.encode(set.px.p, n, slots.data() + at, kWebTilePixels, 256, 256, 768, quality, off.data(), s);
            sw.mark(2);
            if (!ok) return false;
            const uint8_t* streams = enc.fetch_pinned(s);
            if (!streams) return false;
            for (int i = 0; i < n; i++) {
                const int slot = slots[at + i];
                pf_webtile t;
                t.z = zxy[3 * (at + i)]; t.x = zxy[3 * (at + i) + 1]; t.y = zxy[3 * (at + i) + 2];
                t.cover = fone_h[slot] ? 2 : 1;
                t.jpeg = streams + off[i]; t.jpeg_len = off[i + 1] - off[i];
                t.mask8192 = t.cover == 2 ? nullptr : mask_h + (size_t)slot * kWebTileMask;
                t.bgr = want_pixels ? px_h + (size_t)slot * kWebTilePixels : nullptr;
                if (!sink(user, &t)) { set_error("webtiles: the sink stopped the export at tile " + std::to_string(t.z) + "/" + std::to_string(t.x) + "/" + std::to_string(t.y)); return false; }
            }
        }
        return true;
    }
};

}  // namespace

bool webtiles_export(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, const double px2ll[6], int zmin, int zmax,
                     int quality, int bg, bool want_pixels, pf_webtile_sink sink, void* user, JpegEncoder& enc, hipStream_t stream)
{
    namespace wt = webtiles;
    if (!dev_bgr || !dev_mask || !px2ll || !sink || rows < 1 || cols < 1) { set_error("webtiles: no image, no mask, no georeference, no sink or a size that is not positive"); return false; }
    if (step == 0) step = (size_t)cols * 3;
    if (mask_step == 0) mask_step = (size_t)cols;
    if (step < (size_t)cols * 3 || mask_step < (size_t)cols) { set_error("webtiles: step is smaller than a row"); return false; }
    if (zmax < 0) {
        zmax = wt::native_zoom(px2ll, rows, cols);
        if (zmax < 0) { set_error("webtiles: no native zoom: the georeference is singular or the image lies beyond 85.05 degrees of latitude"); return false; }
    }
    int rg[4];
    const wt::PlanResult pr = wt::tile_range(px2ll, rows, cols, zmax, rg);
    if (pr != wt::kPlanOk) { set_error(std::string("webtiles: ") + wt::plan_message(pr)); return false; }
    const Range R{ rg[0], rg[1], rg[2], rg[3] };
    if (zmin < 0) { zmin = zmax; while (zmin > 0) { const Range q = R.up(zmax - zmin); if (q.x0 == q.x1 && q.y0 == q.y1) break; zmin--; } }
    if (zmin > zmax) { set_error("webtiles: zmin " + std::to_string(zmin) + " is above zmax " + std::to_string(zmax)); return false; }

    // the tables of the sampling zoom
    const long long nc = 256ll * (R.x1 - R.x0 + 1), nr = 256ll * (R.y1 - R.y0 + 1);
    std::vector<double> tab((size_t)(2 * nc + 2 * nr));
    if (wt::plan(px2ll, rows, cols, zmax, rg, tab.data(), tab.data() + nc, tab.data() + 2 * nc, tab.data() + 2 * nc + nr, nc, nr) != wt::kPlanOk) { set_error("webtiles: the plan failed"); return false; }
    DevMem dtab;
    if (!dtab.alloc(tab.size() * 8)) return false;
    WT_OK(hipMemcpyAsync(dtab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    WT_OK(hipStreamSynchronize(stream));
    WebSampleSource src;
    src.bgr = (const uint8_t*)dev_bgr; src.step = step; src.mask = (const uint8_t*)dev_mask; src.mask_step = mask_step; src.rows = rows; src.cols = cols;
    src.ux = (const double*)dtab.p; src.uy = src.ux + nc; src.vx = src.ux + 2 * nc; src.vy = src.vx + nr;
    src.c0 = 256ll * R.x0; src.r0 = 256ll * R.y0; src.bg = bg < 0 ? 0 : bg > 255 ? 255 : bg;

    // groups of E x E sampling-zoom tiles under one tile of zoom zmax - KB, reduced K times inside the group
    int KB = 0;
    while ((2 << KB) <= webtiles_batch()) KB++;
    const int K = std::min(KB, zmax - zmin), E = 1 << KB, za = zmax - K;
    const bool carry = za > zmin;                   // (then K == KB) the ancestors' pixels go on into the zooms above; otherwise the groups emit zoom za too
    const Range RA = R.up(KB);
    const int aw = RA.x1 - RA.x0 + 1, ah = RA.y1 - RA.y0 + 1;

    // one group: the slots of level d (zoom zmax - d) begin at base[d], (E >> d)^2 of them, row-major under the ancestor
    int base[5] = { 0, 0, 0, 0, 0 };
    for (int d = 0; d <= K; d++) base[d + 1] = base[d] + (E >> d) * (E >> d);
    const int S = base[K + 1];
    TileSet grp, top;
    if (!grp.alloc((size_t)S) || (carry && !top.alloc((size_t)aw * ah))) return false;
    DevMem ddesc;
    PinMem hdesc, hflags, hmask, hpx;
    if (!ddesc.alloc((size_t)S * 20) || !hdesc.alloc((size_t)S * 20) || !hflags.alloc((size_t)2 * S) || !hmask.alloc((size_t)S * kWebTileMask) || (want_pixels && !hpx.alloc((size_t)S * kWebTilePixels))) return false;
    if (carry) { WT_OK(hipMemsetAsync(top.fzero.p, 1, top.n, stream)); WT_OK(hipMemsetAsync(top.fone.p, 1, top.n, stream)); }
    Stopwatch sw(g_timing, stream);
    Emitter em{ enc, stream, quality, want_pixels, sink, user, sw, {} };
    long long sampled = 0;
    std::vector<int> slots, zxy;

    for (int ay = RA.y0; ay <= RA.y1; ay++)
        for (int ax = RA.x0; ax <= RA.x1; ax++) {
            WT_OK(hipMemsetAsync(grp.fzero.p, 1, (size_t)S, stream));
            WT_OK(hipMemsetAsync(grp.fone.p, 1, (size_t)S, stream));
            const int gx0 = std::max(ax * E, R.x0), gx1 = std::min(ax * E + E - 1, R.x1), gy0 = std::max(ay * E, R.y0), gy1 = std::min(ay * E + E - 1, R.y1);
            sw.mark(0);
            launch_webtile_sample(stream, src, gx0, gy0, gx1 - gx0 + 1, gy1 - gy0 + 1, (gy0 - ay * E) * E + (gx0 - ax * E), E, grp.px.u8(), grp.mask.u8(), grp.fzero.u8(), grp.fone.u8());
            sw.mark(0);
            sampled += (long long)(gx1 - gx0 + 1) * (gy1 - gy0 + 1);
            int* hd = (int*)hdesc.p;
            int used = 0;
            for (int d = 1; d <= K; d++) {
                const Range Rc = R.up(d - 1), Rp = R.up(d);
                const int ec = E >> (d - 1), ep = E >> d, cx0 = ax * ec, cy0 = ay * ec, px0 = ax * ep, py0 = ay * ep;
                const int first = used;
                for (int Y = std::max(py0, Rp.y0); Y <= std::min(py0 + ep - 1, Rp.y1); Y++)
                    for (int X = std::max(px0, Rp.x0); X <= std::min(px0 + ep - 1, Rp.x1); X++) {
                        int* q = hd + 5 * used++;
                        for (int j = 0; j < 2; j++)
                            for (int i = 0; i < 2; i++) q[2 * j + i] = Rc.has(2 * X + i, 2 * Y + j) ? base[d - 1] + (2 * Y + j - cy0) * ec + (2 * X + i - cx0) : -1;
                        q[4] = d == K && carry ? (Y - RA.y0) * aw + (X - RA.x0) : base[d] + (Y - py0) * ep + (X - px0);
                    }
                const int n = used - first;
                WT_OK(hipMemcpyAsync((int*)ddesc.p + 5 * first, hd + 5 * first, (size_t)n * 20, hipMemcpyHostToDevice, stream));
                const TileSet& dst = d == K && carry ? top : grp;
                sw.mark(1);
                launch_webtile_reduce(stream, (const int*)ddesc.p + 5 * first, n, grp.px.u8(), grp.mask.u8(), grp.fzero.u8(), dst.px.u8(), dst.mask.u8(), dst.fzero.u8(), dst.fone.u8(), src.bg);
                sw.mark(1);
            }
            WT_OK(hipGetLastError());
            uint8_t* fz = hflags.u8(); uint8_t* fo = fz + S;
            WT_OK(hipMemcpyAsync(fz, grp.fzero.p, (size_t)S, hipMemcpyDeviceToHost, stream));
            WT_OK(hipMemcpyAsync(fo, grp.fone.p, (size_t)S, hipMemcpyDeviceToHost, stream));
            WT_OK(hipStreamSynchronize(stream));
            slots.clear(); zxy.clear();
            bool partial = false;
            for (int d = 0; d <= (carry ? K - 1 : K); d++) {
                const Range Rd = R.up(d);
                const int ed = E >> d, x0 = ax * ed, y0 = ay * ed;
                for (int y = std::max(y0, Rd.y0); y <= std::min(y0 + ed - 1, Rd.y1); y++)
                    for (int x = std::max(x0, Rd.x0); x <= std::min(x0 + ed - 1, Rd.x1); x++) {
                        const int slot = base[d] + (y - y0) * ed + (x - x0);
                        if (fz[slot]) continue;
                        slots.push_back(slot); zxy.push_back(zmax - d); zxy.push_back(x); zxy.push_back(y);
                        partial = partial || !fo[slot];
                    }
            }
            if (slots.empty()) continue;
            if (partial) WT_OK(hipMemcpyAsync(hmask.p, grp.mask.p, (size_t)S * kWebTileMask, hipMemcpyDeviceToHost, stream));
            if (want_pixels) WT_OK(hipMemcpyAsync(hpx.p, grp.px.p, (size_t)S * kWebTilePixels, hipMemcpyDeviceToHost, stream));
            if (!em.emit(grp, slots, zxy, fo, hmask.u8(), hpx.u8())) return false;          // (the encoder waits for the stream: the copies are there)
        }

    // the zooms from za up: a whole level at a time, each a quarter of the one before
    TileSet sets[2];
    const TileSet* cur = &top;
    for (int z = za; carry; z--) {
        const Range Rz = R.up(zmax - z);
        const int w = Rz.x1 - Rz.x0 + 1, h = Rz.y1 - Rz.y0 + 1;
        const size_t n = (size_t)w * h;
        PinMem lflags, lmask, lpx;
        if (!lflags.alloc(2 * n) || !lmask.alloc(n * kWebTileMask) || (want_pixels && !lpx.alloc(n * kWebTilePixels))) return false;
        uint8_t* fz = lflags.u8(); uint8_t* fo = fz + n;
        WT_OK(hipMemcpyAsync(fz, cur->fzero.p, n, hipMemcpyDeviceToHost, stream));
        WT_OK(hipMemcpyAsync(fo, cur->fone.p, n, hipMemcpyDeviceToHost, stream));
        WT_OK(hipStreamSynchronize(stream));
        slots.clear(); zxy.clear();
        bool partial = false;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int slot = y * w + x;
                if (fz[slot]) continue;
                slots.push_back(slot); zxy.push_back(z); zxy.push_back(Rz.x0 + x); zxy.push_back(Rz.y0 + y);
                partial = partial || !fo[slot];
            }
        if (!slots.empty()) {
            if (partial) WT_OK(hipMemcpyAsync(lmask.p, cur->mask.p, n * kWebTileMask, hipMemcpyDeviceToHost, stream));
            if (want_pixels) WT_OK(hipMemcpyAsync(lpx.p, cur->px.p, n * kWebTilePixels, hipMemcpyDeviceToHost, stream));
            if (!em.emit(*cur, slots, zxy, fo, lmask.u8(), lpx.u8())) return false;
        }
        if (z == zmin) break;
        const Range Rp = Rz.up(1);
        const int pw = Rp.x1 - Rp.x0 + 1, ph = Rp.y1 - Rp.y0 + 1;
        TileSet& nxt = sets[(z - za) & 1];
        PinMem ld; DevMem dd;
        if (!nxt.alloc((size_t)pw * ph) || !ld.alloc((size_t)pw * ph * 20) || !dd.alloc((size_t)pw * ph * 20)) return false;
        WT_OK(hipMemsetAsync(nxt.fzero.p, 1, nxt.n, stream));
        WT_OK(hipMemsetAsync(nxt.fone.p, 1, nxt.n, stream));
        int* q = (int*)ld.p;
        for (int Y = Rp.y0; Y <= Rp.y1; Y++)
            for (int X = Rp.x0; X <= Rp.x1; X++, q += 5) {
                for (int j = 0; j < 2; j++)
                    for (int i = 0; i < 2; i++) q[2 * j + i] = Rz.has(2 * X + i, 2 * Y + j) ? (2 * Y + j - Rz.y0) * w + (2 * X + i - Rz.x0) : -1;
                q[4] = (Y - Rp.y0) * pw + (X - Rp.x0);
            }
        WT_OK(hipMemcpyAsync(dd.p, ld.p, (size_t)pw * ph * 20, hipMemcpyHostToDevice, stream));
        sw.mark(1);
        launch_webtile_reduce(stream, (const int*)dd.p, pw * ph, cur->px.u8(), cur->mask.u8(), cur->fzero.u8(), nxt.px.u8(), nxt.mask.u8(), nxt.fzero.u8(), nxt.fone.u8(), src.bg);
        sw.mark(1);
        WT_OK(hipGetLastError());
        WT_OK(hipStreamSynchronize(stream));          // the descriptors and the level below go away here
        cur = &nxt;
    }
    WT_OK(hipStreamSynchronize(stream));
    if (sw.on) { g_last_timing[0] = sw.total(0); g_last_timing[1] = sw.total(1); g_last_timing[2] = sw.total(2); g_last_timing[3] = (double)sampled; }
    return true;
}

}  // namespace pf
