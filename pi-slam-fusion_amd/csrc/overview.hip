// overview.hip -- the GPU side of save("x.tif") (tiff_pyramid.hpp): the overview chain of an image in HBM, the empty test per
// tile, and the driver that hands the tiles of every level to the JPEG encoder (jpeg_encode.hip) in bounded batches.
//
//   k_overview       one workgroup of 256 lanes per 64 x 64 block of level k: the block is read ONCE (16-byte loads where the
//                    rows allow it, rows and columns past the image repeated), reduced through LDS to 32 x 32, 16 x 16 and 8 x 8,
//                    and up to three levels are written from the one read (16-byte stores).  Along the way it clears the tile
//                    flag "all pixels equal the background" of every level it sees a different pixel of.
//   k_overview_pad   a level buffer is rounded up to whole tiles: the part past the image gets its last column, then its last
//                    row, so that every tile of every level is a plain 256 x 256 window for the encoder.
//   k_overview_copy  image 0 into such a buffer (only an image that is not whole tiles already: a mosaic of map tiles is used
//                    where it lies).
// Algorithmic bytes of the chain: 3 R C read + 3 sum_k r_k c_k written, about 1.33 x the mosaic.
// The masked file's masks are bit planes made by coverage.hip beside the chain; their flags travel with the chain's, and only the
// mask tiles that are neither all zero nor all one are gathered and fetched.
#include "tiff_pyramid.hpp"
#include "coverage.hpp"
#include "jpeg_decode.hpp"          // set_error
#include <hip/hip_runtime.h>

namespace pf {

using namespace tiff;

namespace {

struct OvArgs {
    const uint8_t* src; size_t sstep; int r0, c0;          // level k: the image's own size; rows of sstep bytes
    int nlev;                                              // levels to write: 0 (flags of level k only) ... 3
    uint8_t* dst[3]; size_t dstep[3]; int r[3], c[3];
    uint8_t* fsrc; int ftx_src;                            // flags of level k (null: they were cleared when it was written), tiles across
    uint8_t* fdst[3]; int ftx[3];
    int bg;
};

// 2 x 2 mean of four pixels' worth of one channel
__device__ inline int mean4(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }

__global__ __launch_bounds__(256) void k_overview(OvArgs a)
{
    __shared__ uint4 s0v[64 * 12];          // 64 rows of 192 bytes
    __shared__ uint4 s1v[32 * 6];           // 32 rows of 96
    __shared__ uint4 s2v[16 * 3];           // 16 rows of 48
    __shared__ uint2 s3v[8 * 3];            // 8 rows of 24
    __shared__ int snb;
    uint8_t* s0 = (uint8_t*)s0v; uint8_t* s1 = (uint8_t*)s1v; uint8_t* s2 = (uint8_t*)s2v; uint8_t* s3 = (uint8_t*)s3v;
    const int t = threadIdx.x, bx = blockIdx.x, by = blockIdx.y;
    const int y0 = 64 * by, x0 = 64 * bx;
    const uint32_t bg4 = 0x01010101u * (uint32_t)a.bg;
    int nb = 0;                              // bit j: a pixel of level k + j differs from the background
    if (t == 0) snb = 0;
    const bool wide = ((((size_t)a.src | a.sstep) & 15) == 0) && y0 + 64 <= a.r0 && x0 + 64 <= a.c0;
    if (wide) {
        for (int i = t; i < 64 * 12; i += 256) {
            const int row = i / 12, q = i - 12 * row;
            const uint4 v = *(const uint4*)(a.src + (size_t)(y0 + row) * a.sstep + (size_t)x0 * 3 + 16 * q);
            s0v[i] = v;
            nb |= (v.x != bg4 || v.y != bg4 || v.z != bg4 || v.w != bg4) ? 1 : 0;
        }
    } else {
        for (int i = t; i < 64 * 192; i += 256) {
            const int row = i / 192, b = i - 192 * row, px = b / 3;
            const uint8_t v = a.src[(size_t)min(y0 + row, a.r0 - 1) * a.sstep + (size_t)min(x0 + px, a.c0 - 1) * 3 + (b - 3 * px)];
            s0[i] = v;
            nb |= v != a.bg ? 1 : 0;
        }
    }
    __syncthreads();
    if (a.nlev >= 1) {          // 32 x 32: four pixels (12 bytes) per lane from two runs of 24 bytes; the block's copy is clamped already
        const int y = t >> 3, u = t & 7;
        const uint8_t* p = s0 + (2 * y) * 192 + 24 * u;
        uint8_t* d = s1 + y * 96 + 12 * u;
        const bool rowreal = 32 * by + y < a.r[0];
        for (int x = 0; x < 4; x++)
            for (int ch = 0; ch < 3; ch++) {
                const int v = mean4(p[6 * x + ch], p[6 * x + 3 + ch], p[192 + 6 * x + ch], p[192 + 6 * x + 3 + ch]);
                d[3 * x + ch] = (uint8_t)v;
                if (rowreal && 32 * bx + 4 * u + x < a.c[0] && v != a.bg) nb |= 2;
            }
    }
    __syncthreads();
    if (a.nlev >= 2) {          // 16 x 16: a pixel per lane; the level above ends inside the block where the image does
        const int y = t >> 4, x = t & 15;
        const int ya = min(2 * y, a.r[0] - 1 - 32 * by), yb = min(2 * y + 1, a.r[0] - 1 - 32 * by);
        const int xa = min(2 * x, a.c[0] - 1 - 32 * bx), xb = min(2 * x + 1, a.c[0] - 1 - 32 * bx);
        const bool real = 16 * by + y < a.r[1] && 16 * bx + x < a.c[1];
        for (int ch = 0; ch < 3; ch++) {
            const int v = mean4(s1[ya * 96 + 3 * xa + ch], s1[ya * 96 + 3 * xb + ch], s1[yb * 96 + 3 * xa + ch], s1[yb * 96 + 3 * xb + ch]);
            s2[y * 48 + 3 * x + ch] = (uint8_t)v;
            if (real && v != a.bg) nb |= 4;
        }
    }
    __syncthreads();
    if (a.nlev >= 3 && t < 64) {          // 8 x 8
        const int y = t >> 3, x = t & 7;
        const int ya = min(2 * y, a.r[1] - 1 - 16 * by), yb = min(2 * y + 1, a.r[1] - 1 - 16 * by);
        const int xa = min(2 * x, a.c[1] - 1 - 16 * bx), xb = min(2 * x + 1, a.c[1] - 1 - 16 * bx);
        const bool real = 8 * by + y < a.r[2] && 8 * bx + x < a.c[2];
        for (int ch = 0; ch < 3; ch++) {
            // (a block that holds pixels of level k holds pixels of every level below: the clamped indices are never negative)
            const int v = mean4(s2[ya * 48 + 3 * xa + ch], s2[ya * 48 + 3 * xb + ch], s2[yb * 48 + 3 * xa + ch], s2[yb * 48 + 3 * xb + ch]);
            s3[y * 24 + 3 * x + ch] = (uint8_t)v;
            if (real && v != a.bg) nb |= 8;
        }
    }
    for (int j = 0; j < 4; j++)
        if (__any(nb & (1 << j)) && (t & 63) == 0) atomicOr(&snb, 1 << j);
    __syncthreads();
    // the block's footprint in every level lies inside that level's buffer (whole tiles); what it writes past the image there
    // k_overview_pad overwrites
    if (a.nlev >= 1 && t < 32 * 6) { const int row = t / 6, q = t - 6 * row; *(uint4*)(a.dst[0] + (size_t)(32 * by + row) * a.dstep[0] + (size_t)96 * bx + 16 * q) = s1v[t]; }
    if (a.nlev >= 2 && t < 16 * 3) { const int row = t / 3, q = t - 3 * row; *(uint4*)(a.dst[1] + (size_t)(16 * by + row) * a.dstep[1] + (size_t)48 * bx + 16 * q) = s2v[t]; }
    if (a.nlev >= 3 && t < 8 * 3) { const int row = t / 3, q = t - 3 * row; *(uint2*)(a.dst[2] + (size_t)(8 * by + row) * a.dstep[2] + (size_t)24 * bx + 8 * q) = s3v[t]; }
    if (t == 0) {
        const int m = snb;
        if ((m & 1) && a.fsrc) a.fsrc[(size_t)(by >> 2) * a.ftx_src + (bx >> 2)] = 0;
        for (int j = 0; j < a.nlev; j++)
            if (m & (2 << j)) a.fdst[j][(size_t)(by >> (3 + j)) * a.ftx[j] + (bx >> (3 + j))] = 0;
    }
}

// buffer of prows x pcols pixels (whole tiles) that holds an image of r x c: pixel (y, x) past the image = (min(y, r - 1), min(x, c - 1))
__global__ void k_overview_pad(uint8_t* __restrict__ img, size_t step, int r, int c, int prows, int pcols)
{
    const long right = (long)r * (pcols - c), below = (long)(prows - r) * pcols;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= right + below) return;
    int y, x;
    if (i < right) { y = (int)(i / (pcols - c)); x = c + (int)(i - (long)y * (pcols - c)); }
    else { const long j = i - right; y = r + (int)(j / pcols); x = (int)(j - (long)(y - r) * pcols); }
    const uint8_t* s = img + (size_t)min(y, r - 1) * step + (size_t)min(x, c - 1) * 3;
    uint8_t* d = img + (size_t)y * step + (size_t)x * 3;
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
}

// one 32-bit word of the padded copy per lane
__global__ void k_overview_copy(const uint8_t* __restrict__ src, size_t sstep, int r, int c, uint8_t* __restrict__ dst, int prows, int pcols)
{
    const long words = (long)pcols * 3 / 4;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words * prows) return;
    const int y = (int)(i / words), w = (int)(i - (long)y * words);
    const uint8_t* s = src + (size_t)min(y, r - 1) * sstep;
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) {
        const int b = 4 * w + k, px = b / 3;
        v |= (uint32_t)s[(size_t)min(px, c - 1) * 3 + (b - 3 * px)] << (8 * k);
    }
    *(uint32_t*)(dst + (size_t)y * pcols * 3 + 4 * (size_t)w) = v;
}

struct Buf {
    void* p = nullptr; size_t cap = 0;
    bool reserve(size_t bytes)
    {
        if (bytes <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("tiff: hipMalloc of " + std::to_string(bytes) + " bytes failed"); return false; }
        cap = bytes;
        return true;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

inline size_t round_tile(int v) { return (size_t)((v + kTile - 1) / kTile) * kTile; }

}  // namespace

#define TIFF_OK(expr)                                                                                                  \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) { set_error(std::string("tiff: " #expr ": ") + hipGetErrorString(e_)); return false; }  \
    } while (0)

// tiles per encoder pass: bounds the encoder's scratch (JPEG: about 230 KB of coefficients and offsets per tile; Deflate: the
// worst-case stream, 197 KB, and 13 KB of block plans) whatever the mosaic's size
constexpr size_t kBatchTiles = 512;

struct TiffDevice::Impl {
    Buf levels, flags;                                   // levels 1... (and a padded copy of image 0 where needed) back to back; a byte per tile
    uint8_t* land = nullptr; size_t land_cap = 0;        // page-locked: the streams of all tiles, back to back
    uint8_t* hflags = nullptr; size_t hflags_cap = 0;    // page-locked: the flags
    size_t n_tiles = 0, n_empty = 0;
    // the masked file: the masks' bit planes of all levels back to back, (offset, row step) of the tiles to gather, those tiles
    Buf planes, where, gathered;
    uint8_t* mland = nullptr; size_t mland_cap = 0;      // page-locked: the gathered mask tiles
    size_t n_zero = 0, n_one = 0, own_bytes = 0;
    ~Impl()
    {
        levels.release(); flags.release(); planes.release(); where.release(); gathered.release();
        if (land) (void)hipHostFree(land);
        if (hflags) (void)hipHostFree(hflags);
        if (mland) (void)hipHostFree(mland);
    }
    bool grow_land(size_t need, size_t used, size_t hint)
    {
        if (need <= land_cap) return true;
        const size_t want = std::max(need, hint) + 4096;
        uint8_t* q = nullptr;
        if (hipHostMalloc((void**)&q, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); set_error("tiff: no page-locked memory for the streams"); return false; }
        if (used) std::memcpy(q, land, used);
        if (land) (void)hipHostFree(land);
        land = q; land_cap = want;
        return true;
    }
};

TiffDevice::~TiffDevice() { delete p_; }
void TiffDevice::release() { delete p_; p_ = nullptr; }
void TiffDevice::last_counts(size_t* tiles, size_t* empty, size_t* device_bytes) const
{
    if (tiles) *tiles = p_ ? p_->n_tiles : 0;
    if (empty) *empty = p_ ? p_->n_empty : 0;
    if (device_bytes) *device_bytes = p_ ? p_->levels.cap + p_->flags.cap : 0;
}

void TiffDevice::last_mask_counts(size_t* zero, size_t* one, size_t* own_bytes) const
{
    if (zero) *zero = p_ ? p_->n_zero : 0;
    if (one) *one = p_ ? p_->n_one : 0;
    if (own_bytes) *own_bytes = p_ ? p_->own_bytes : 0;
}

bool TiffDevice::write(const char* filename, const void* dev_bgr, int rows, int cols, size_t step, int quality, int bg, const double* model_transform, bool force_bigtiff,
                       JpegEncoder& enc, void* stream, const Mask* mask, DeflateEncoder* lossless)
{
    const Codec codec = lossless ? kDeflate : kJpeg;
    hipStream_t s = (hipStream_t)stream;
    if (!filename || !dev_bgr || rows < 1 || cols < 1) { set_error("tiff: no name, no image or a size that is not positive"); return false; }
    if (step == 0) step = (size_t)cols * 3;
    if (step < (size_t)cols * 3) { set_error("tiff: step is smaller than a row"); return false; }
    size_t mstep = 0;
    if (mask) {
        if (!mask->dev_bytes && !mask->dev_table) { set_error("tiff: no mask"); return false; }
        mstep = mask->step ? mask->step : (size_t)cols;
        if (mask->dev_bytes && mstep < (size_t)cols) { set_error("tiff: step is smaller than a row"); return false; }
        if (!mask->dev_bytes && (mask->wx < 1 || mask->wy < 1 || rows != mask->wy * kTile || cols != mask->wx * kTile)) { set_error("tiff: the tile table is not the mosaic's"); return false; }
    }
    if (!p_) p_ = new Impl();
    Impl& d = *p_;
    const std::vector<Level> lv = levels(rows, cols);
    const size_t nt = tile_count(lv), nl = lv.size();
    const uint8_t bgv = background_byte(bg);
    // where every level lies: image 0 in place when it is whole tiles, else a padded copy; the others in buffers of whole tiles
    const bool in_place = rows % kTile == 0 && cols % kTile == 0;
    std::vector<size_t> at(nl, 0), lstep(nl, 0);
    size_t bytes = 0;
    for (size_t k = in_place ? 1 : 0; k < nl; k++) { at[k] = bytes; lstep[k] = round_tile(lv[k].cols) * 3; bytes += round_tile(lv[k].rows) * lstep[k]; }
    const size_t nf = mask ? 3 * nt : nt;          // flags: "all background", then for the masks "all zero" and "all one"
    if (!d.levels.reserve(bytes + 16) || !d.flags.reserve(nf)) return false;
    if (nf > d.hflags_cap) {
        if (d.hflags) (void)hipHostFree(d.hflags);
        d.hflags = nullptr; d.hflags_cap = 0;
        TIFF_OK(hipHostMalloc((void**)&d.hflags, nf + 64, hipHostMallocDefault));
        d.hflags_cap = nf + 64;
    }
    std::vector<size_t> pat(nl, 0);                 // where every level's mask plane lies
    if (mask) {
        size_t pbytes = 0;
        for (size_t k = 0; k < nl; k++) { pat[k] = pbytes; pbytes += coverage_plane_rows(lv[k].rows) * coverage_plane_step(lv[k].cols); }
        if (!d.planes.reserve(pbytes)) return false;
    }
    std::vector<const uint8_t*> base(nl);
    for (size_t k = 0; k < nl; k++) base[k] = (uint8_t*)d.levels.p + at[k];
    if (in_place) { base[0] = (const uint8_t*)dev_bgr; lstep[0] = step; }
    else {
        const long words = (long)(lstep[0] / 4) * (long)round_tile(rows);
        hipLaunchKernelGGL(k_overview_copy, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, (const uint8_t*)dev_bgr, step, rows, cols, (uint8_t*)base[0], (int)round_tile(rows), (int)round_tile(cols));
    }
    uint8_t* flags = (uint8_t*)d.flags.p;
    TIFF_OK(hipMemsetAsync(flags, 1, nf, s));
    if (mask) {          // the masks' chain: level 0 from the bytes or from the map's weights, every other level from the one above
        uint8_t* const pl = (uint8_t*)d.planes.p;
        if (mask->dev_bytes) launch_coverage_bytes(s, (const uint8_t*)mask->dev_bytes, rows, cols, mstep, pl, flags + nt, flags + 2 * nt);
        else launch_coverage_tiles(s, mask->dev_table, mask->wx, mask->wy, mask->w_off, pl, flags + nt, flags + 2 * nt);
        for (size_t k = 1; k < nl; k++)
            launch_mask_overview(s, pl + pat[k - 1], lv[k - 1].rows, lv[k - 1].cols, pl + pat[k], flags + nt + lv[k].first, flags + 2 * nt + lv[k].first);
    }
    for (size_t k = 0; k == 0 || k + 1 < nl; k += 3) {
        OvArgs a{};
        a.src = base[k]; a.sstep = lstep[k]; a.r0 = lv[k].rows; a.c0 = lv[k].cols;
        a.nlev = (int)std::min<size_t>(3, nl - 1 - k);
        a.fsrc = k == 0 ? flags : nullptr; a.ftx_src = lv[k].tx; a.bg = bgv;
        for (int j = 0; j < a.nlev; j++) {
            const Level& l = lv[k + 1 + j];
            a.dst[j] = (uint8_t*)base[k + 1 + j]; a.dstep[j] = lstep[k + 1 + j]; a.r[j] = l.rows; a.c[j] = l.cols;
            a.fdst[j] = flags + l.first; a.ftx[j] = l.tx;
        }
        hipLaunchKernelGGL(k_overview, dim3((unsigned)((a.c0 + 63) / 64), (unsigned)((a.r0 + 63) / 64)), dim3(256), 0, s, a);
        for (int j = 0; j < a.nlev; j++) {
            const Level& l = lv[k + 1 + j];
            const int pr = (int)round_tile(l.rows), pc = (int)round_tile(l.cols);
            const long n = (long)l.rows * (pc - l.cols) + (long)(pr - l.rows) * pc;
            if (n) hipLaunchKernelGGL(k_overview_pad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.dst[j], a.dstep[j], l.rows, l.cols, pr, pc);
        }
        if (a.nlev < 3) break;
    }
    TIFF_OK(hipGetLastError());
    TIFF_OK(hipMemcpyAsync(d.hflags, flags, nf, hipMemcpyDeviceToHost, s));
    TIFF_OK(hipStreamSynchronize(s));
    // the mask tiles that are stored on their own are gathered and fetched behind the flags; the tile encode below runs meanwhile
    std::vector<uint8_t> mkind;
    std::vector<size_t> mwhere(mask ? nt : 0, 0);
    std::vector<uint64_t> gather;
    if (mask) {
        mkind.assign(nt, kMaskOwn);
        d.n_zero = d.n_one = 0;
        for (size_t k = 0; k < nl; k++) {
            const Level& l = lv[k];
            const size_t pstep = coverage_plane_step(l.cols);
            for (size_t i = 0; i < l.tiles(); i++) {
                const size_t g = l.first + i;
                if (d.hflags[nt + g]) { mkind[g] = kMaskZero; d.n_zero++; }
                else if (d.hflags[2 * nt + g]) { mkind[g] = kMaskOne; d.n_one++; }
                else {
                    mwhere[g] = gather.size() / 2 * kMaskTileBytes;
                    gather.push_back(pat[k] + (i / l.tx) * kTile * pstep + (i % l.tx) * (size_t)(kTile / 8));
                    gather.push_back(pstep);
                }
            }
        }
        const size_t n_own = gather.size() / 2;
        d.own_bytes = n_own * kMaskTileBytes;
        if (n_own) {
            if (!d.where.reserve(gather.size() * 8) || !d.gathered.reserve(d.own_bytes)) return false;
            if (d.own_bytes > d.mland_cap) {
                if (d.mland) (void)hipHostFree(d.mland);
                d.mland = nullptr; d.mland_cap = 0;
                TIFF_OK(hipHostMalloc((void**)&d.mland, d.own_bytes + 4096, hipHostMallocDefault));
                d.mland_cap = d.own_bytes + 4096;
            }
            TIFF_OK(hipMemcpyAsync(d.where.p, gather.data(), gather.size() * 8, hipMemcpyHostToDevice, s));
            launch_mask_gather(s, (const uint8_t*)d.planes.p, (const uint64_t*)d.where.p, (int)n_own, (uint8_t*)d.gathered.p);
            TIFF_OK(hipGetLastError());
            TIFF_OK(hipMemcpyAsync(d.mland, d.gathered.p, d.own_bytes, hipMemcpyDeviceToHost, s));
        }
    }
    // the tiles that are not empty, level by level, in batches: a tile is the window at (ty * 256) rows, (tx * 768) bytes of its level
    std::vector<uint32_t> len(nt, 0);
    std::vector<size_t> where(nt, 0), off(kBatchTiles + 1);
    std::vector<long long> win; win.reserve(kBatchTiles);
    std::vector<size_t> who; who.reserve(kBatchTiles);
    size_t used = 0, done = 0, n_full = 0;
    for (size_t i = 0; i < nt; i++) n_full += d.hflags[i] == 0;
    d.n_tiles = nt; d.n_empty = nt - n_full;
    for (size_t k = 0; k < nl; k++) {
        const Level& l = lv[k];
        for (size_t i0 = 0; i0 < l.tiles(); i0 += kBatchTiles) {
            win.clear(); who.clear();
            for (size_t i = i0; i < std::min(l.tiles(), i0 + kBatchTiles); i++) {
                if (d.hflags[l.first + i]) continue;
                win.push_back((long long)((i / l.tx) * kTile * lstep[k] + (i % l.tx) * (size_t)kTile * 3));
                who.push_back(l.first + i);
            }
            if (win.empty()) continue;
            const int n = (int)win.size();
            if (lossless ? !lossless->encode_windows(base[k], n, win.data(), lstep[k], off.data(), stream)
                         : !enc.encode_windows(base[k], n, win.data(), kTile, kTile, lstep[k], quality, off.data(), stream)) return false;
            done += (size_t)n;
            // room for the batch; the first time round the whole file's streams are guessed from the first batch
            if (!d.grow_land(used + off[n], used, (size_t)((double)(used + off[n]) / (double)done * (double)n_full * 1.15))) return false;
            if (lossless ? !lossless->fetch(d.land + used, stream) : !enc.fetch(d.land + used, stream)) return false;
            for (int j = 0; j < n; j++) { where[who[j]] = used + off[j]; len[who[j]] = (uint32_t)(off[j + 1] - off[j]); }
            used += off[n];
        }
    }
    std::vector<uint8_t> empty;
    empty_stream(quality, bg, empty, codec);
    Layout lo;
    if (!mask) {
        layout_masked(lv, len, (uint32_t)empty.size(), nullptr, model_transform, force_bigtiff, lo, codec);
        return write_file(filename, lo, len, empty, [&](size_t i) { return (const uint8_t*)d.land + where[i]; });
    }
    TIFF_OK(hipStreamSynchronize(s));          // the gathered mask tiles have landed
    layout_masked(lv, len, (uint32_t)empty.size(), &mkind, model_transform, force_bigtiff, lo, codec);
    const std::function<const uint8_t*(size_t)> mtile = [&](size_t i) { return (const uint8_t*)d.mland + mwhere[i]; };
    return write_file(filename, lo, len, empty, [&](size_t i) { return (const uint8_t*)d.land + where[i]; }, &mkind, &mtile);
}

}  // namespace pf
