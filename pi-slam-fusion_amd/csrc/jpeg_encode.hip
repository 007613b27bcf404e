// jpeg_encode.hip -- the baseline JPEG encoder of jpeg_encode.hpp on the GPU (gfx950), byte-equal to its scalar encoder.
// The pixels (a collapsed mosaic, or the tiles of one blend launch) are read from HBM once and only the finished streams
// leave it.  Nothing serial in the image size runs on the host; the host waits twice, for two sizes it has to allocate by.
//
//   k_jenc_transform  4 MCUs (16 x 16 pixels each) per group of 192 lanes: pixels -> LDS, colour conversion and h2v2
//                     down-sampling, the ISLOW DCT with 8 lanes per block (a row each, then a column each), quantisation;
//                     out: the coefficients as int16 in zig-zag order, each block's DC and the bits its AC part will take
//   k_jenc_bits       DC differences (the block of the same component coded before: no chain) -> bits per block
//   [scan]            exclusive sum -> each block's bit offset in its image
//   k_jenc_image_chunks + [scan]   each image's entropy-coded data starts on a 16-byte chunk of the unstuffed buffer
//   k_jenc_pack       one lane per block writes its code words at the block's bit offset: whole 32-bit words, OR-combined
//                     with the neighbours' at the joins (the buffer starts zeroed), the last byte of an image padded with 1s
//   k_jenc_count_ff + [scan]       0xFF bytes per chunk -> where each chunk lands once stuffed
//   k_jenc_image_len + [scan]      each stream's length and offset in the output (those come back to the host)
//   k_jenc_stuff      scatter with the 0x00 after every 0xFF;  k_jenc_frame: the marker segments in front, EOI behind
#include "jpeg_encode.hpp"
#include "jpeg_decode.hpp"          // set_error
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string>

namespace pf {

using namespace jenc;

namespace {

struct EncBlob { Tables t; uint8_t header[kHeaderBytes + 1]; };
typedef unsigned long long u64;

constexpr int kGroupMcus = 4, kTransformLanes = 48 * kGroupMcus;          // 6 blocks x 8 lanes per MCU

struct McuPos { bool valid; long img; int my, mx; };
__device__ inline McuPos mcu_pos(long mcu, long n_mcus, const Geometry& g)
{
    McuPos p; p.valid = mcu < n_mcus;
    const long per = (long)g.mcux * g.mcuy, m = p.valid ? mcu : 0;
    p.img = m / per;
    const int lm = (int)(m - p.img * per);
    p.my = lm / g.mcux; p.mx = lm - p.my * g.mcux;
    return p;
}

__global__ __launch_bounds__(kTransformLanes) void k_jenc_transform(const uint8_t* __restrict__ src, const long long* __restrict__ where, size_t image_stride,
                                                                    size_t step, Geometry g, long n_mcus, const EncBlob* __restrict__ blob,
                                                                    int16_t* __restrict__ coef, int16_t* __restrict__ dcv, uint32_t* __restrict__ acbits)
{
    __shared__ uint8_t raw[kGroupMcus][16][48];
    __shared__ int     ws[kGroupMcus * 6][64];
    __shared__ int16_t zz[kGroupMcus * 6][64];
    __shared__ u64     nzm[kGroupMcus * 6];
    const int t = threadIdx.x;
    const long mcu0 = (long)blockIdx.x * kGroupMcus;
    {   // the MCU's pixels; rows and columns past the image repeat the last (adjacent MCUs: one run of bytes per row)
        const int ml = t / 48, j = t - 48 * ml;
        const McuPos p = mcu_pos(mcu0 + ml, n_mcus, g);
        if (p.valid) {
            const uint8_t* base = src + (where ? (size_t)where[p.img] : (size_t)p.img * image_stride);          // where: byte offsets, 64 bits
            const int x = min(16 * p.mx + j / 3, g.cols - 1);
            for (int r = 0; r < 16; r++) {
                const int y = min(16 * p.my + r, g.rows - 1);
                raw[ml][r][j] = base[(size_t)y * step + (size_t)x * 3 + (j % 3)];
            }
        }
    }
    __syncthreads();
    for (int q = t; q < 64 * kGroupMcus; q += kTransformLanes) {          // one 2 x 2 quad: four luminance samples, one of each chroma plane
        const int ml = q >> 6, qy = (q >> 3) & 7, qx = q & 7;
        const McuPos p = mcu_pos(mcu0 + ml, n_mcus, g);
        if (!p.valid) continue;
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const uint8_t* px = &raw[ml][2 * qy + dy][(2 * qx + dx) * 3];
                ws[ml * 6 + (qy >> 2) * 2 + (qx >> 2)][((2 * qy + dy) & 7) * 8 + ((2 * qx + dx) & 7)] = ycc_y(px[2], px[1], px[0]) - 128;
            }
        // down-sampled rows past the image's repeat the last down-sampled row (not the last input row)
        const int cy = min(qy, g.ch - 8 * p.my - 1);
        int cb = 0, cr = 0;
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const uint8_t* px = &raw[ml][2 * cy + dy][(2 * qx + dx) * 3];
                cb += ycc_cb(px[2], px[1], px[0]); cr += ycc_cr(px[2], px[1], px[0]);
            }
        const int bias = 1 + (qx & 1);
        ws[ml * 6 + 4][qy * 8 + qx] = ((cb + bias) >> 2) - 128;
        ws[ml * 6 + 5][qy * 8 + qx] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    const int b = t >> 3, l = t & 7, ml = b / 6, k = b - 6 * ml, c = k < 4 ? 0 : 1;
    const McuPos p = mcu_pos(mcu0 + ml, n_mcus, g);
    if (p.valid) fdct_pass(&ws[b][8 * l], 1, true);
    __syncthreads();
    if (p.valid) {
        fdct_pass(&ws[b][l], 8, false);
        for (int i = 0; i < 8; i++) {
            const int zp = blob->t.nat2zz[8 * i + l];
            zz[b][zp] = (int16_t)quantise(ws[b][8 * i + l], blob->t.div[c][zp]);
        }
    }
    __syncthreads();
    // this lane's eight coefficients in zig-zag order; a dummy block has the DC of the block coded before it and nothing else
    int v[8];
    for (int j = 0; j < 8; j++) v[j] = p.valid ? zz[b][8 * l + j] : 0;
    if (p.valid && k < 4 && !luma_block_real(g, p.my, p.mx, k)) {
        int kk = k;
        while (kk > 0 && !luma_block_real(g, p.my, p.mx, kk)) kk--;
        for (int j = 0; j < 8; j++) v[j] = 0;
        if (l == 0) v[0] = zz[ml * 6 + kk][0];
    }
    unsigned m8 = 0;
    for (int j = 0; j < 8; j++) m8 |= (v[j] != 0 ? 1u : 0u) << j;
    ((uint8_t*)&nzm[b])[l] = (uint8_t)m8;
    __syncthreads();
    // every non-zero AC coefficient's code depends on the run of zeros before it alone: the distance to the non-zero before
    const u64 m = nzm[b] | 1ull;
    const uint32_t* ac = blob->t.ac[c];
    const int zrl = (int)(ac[0xF0] & 31);
    int bits = 0;
    for (int j = 0; j < 8; j++) {
        const int zp = 8 * l + j;
        if (zp == 0 || v[j] == 0) continue;
        const int prev = 63 - __clzll((long long)(m & ((1ull << zp) - 1)));
        const int run = zp - prev - 1, s = 32 - __clz(abs(v[j]));
        bits += (run >> 4) * zrl + (int)(ac[((run & 15) << 4) | s] & 31) + s;
    }
    if (l == 0 && !(m >> 63)) bits += (int)(ac[0] & 31);          // end of block
    bits += __shfl_xor(bits, 1); bits += __shfl_xor(bits, 2); bits += __shfl_xor(bits, 4);
    if (p.valid) {
        const long gb = (mcu0 + ml) * 6 + k;
        uint4 o;
        o.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16); o.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
        o.z = (uint32_t)(uint16_t)v[4] | ((uint32_t)(uint16_t)v[5] << 16); o.w = (uint32_t)(uint16_t)v[6] | ((uint32_t)(uint16_t)v[7] << 16);
        *(uint4*)(coef + gb * 64 + 8 * l) = o;
        if (l == 0) { dcv[gb] = (int16_t)v[0]; acbits[gb] = (uint32_t)bits; }
    }
}

// the DC the block's difference is taken against: the block of the same component coded before it in the image's one scan
__device__ inline int dc_before(const int16_t* __restrict__ dcv, long gb, long lb)
{
    const int k = (int)(lb % 6);
    if (k > 0 && k < 4) return dcv[gb - 1];
    if (lb < 6) return 0;
    return k == 0 ? dcv[gb - 3] : dcv[gb - 6];
}

__global__ void k_jenc_bits(const int16_t* __restrict__ dcv, const uint32_t* __restrict__ acbits, long nb_total, long nbi, const EncBlob* __restrict__ blob, u64* __restrict__ bits)
{
    const long gb = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb == 0) bits[nb_total] = 0;
    if (gb >= nb_total) return;
    const long lb = gb % nbi;
    const int d = dcv[gb] - dc_before(dcv, gb, lb), s = 32 - __clz(abs(d));
    bits[gb] = (u64)acbits[gb] + (blob->t.dc[lb % 6 < 4 ? 0 : 1][s] & 31) + (u64)s;
}

__global__ void k_jenc_image_chunks(const u64* __restrict__ off, int n, long nbi, u64* __restrict__ chunks)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    chunks[i] = i < n ? (off[(long)(i + 1) * nbi] - off[(long)i * nbi] + 127) >> 7 : 0;
}

__global__ __launch_bounds__(256) void k_jenc_pack(const int16_t* __restrict__ coef, const int16_t* __restrict__ dcv, const u64* __restrict__ off,
                                                   const u64* __restrict__ ubase, long nb_total, long nbi, const EncBlob* __restrict__ blob, uint32_t* __restrict__ ubuf)
{
    __shared__ uint32_t sdc[2][12], sac[2][256];
    for (int i = threadIdx.x; i < 24; i += blockDim.x) sdc[i / 12][i % 12] = blob->t.dc[i / 12][i % 12];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) sac[i >> 8][i & 255] = blob->t.ac[i >> 8][i & 255];
    __syncthreads();
    const long gb = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb >= nb_total) return;
    const long img = gb / nbi, lb = gb - img * nbi;
    const int c = lb % 6 < 4 ? 0 : 1;
    const u64 P = ubase[img] * 128 + (off[gb] - off[img * nbi]);
    size_t w = (size_t)(P >> 5);
    int fill = (int)(P & 31);
    u64 acc = 0;
    bool first = true;
    auto emit = [&](uint32_t code, int len) {          // len <= 27, fill < 32
        acc |= (u64)code << (64 - fill - len);
        fill += len;
        if (fill >= 32) {
            const uint32_t be = __builtin_bswap32((uint32_t)(acc >> 32));
            if (first) atomicOr(&ubuf[w], be); else ubuf[w] = be;          // past the first word the block owns every word it fills
            first = false; w++; acc <<= 32; fill -= 32;
        }
    };
    {
        const int d = dcv[gb] - dc_before(dcv, gb, lb), s = 32 - __clz(abs(d));
        const uint32_t e = sdc[c][s];
        emit(((e >> 5) << s) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1)), (int)(e & 31) + s);
    }
    const uint4* cp = (const uint4*)(coef + gb * 64);
    const uint32_t zrl = sac[c][0xF0];
    int run = 0;
    for (int i = 0; i < 8; i++) {
        const uint4 q = cp[i];
        const uint32_t wd[4] = { q.x, q.y, q.z, q.w };
        for (int j = (i == 0 ? 1 : 0); j < 8; j++) {
            const int v = (int)(int16_t)(wd[j >> 1] >> (16 * (j & 1)));
            if (!v) { run++; continue; }
            for (; run > 15; run -= 16) emit(zrl >> 5, (int)(zrl & 31));
            const int s = 32 - __clz(abs(v));
            const uint32_t e = sac[c][(run << 4) | s];
            emit(((e >> 5) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1)), (int)(e & 31) + s);
            run = 0;
        }
    }
    if (run) emit(sac[c][0] >> 5, (int)(sac[c][0] & 31));
    if (lb == nbi - 1 && (fill & 7)) { const int pad = 8 - (fill & 7); emit((1u << pad) - 1, pad); }
    if (fill > 0) atomicOr(&ubuf[w], __builtin_bswap32((uint32_t)(acc >> 32)));
}

// the image whose unstuffed data holds chunk c: the last i with ubase[i] <= c (every image has at least one chunk)
__device__ inline int image_of_chunk(const u64* __restrict__ ubase, int n, u64 c)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (ubase[mid] <= c) lo = mid; else hi = mid - 1; }
    return lo;
}
// bytes of chunk c that belong to the stream (the last chunk of an image is filled up with zeros)
__device__ inline int chunk_valid(const u64* __restrict__ off, const u64* __restrict__ ubase, long nbi, int img, u64 c)
{
    const u64 bytes = (off[(long)(img + 1) * nbi] - off[(long)img * nbi] + 7) >> 3, at = (c - ubase[img]) * 16;
    return (int)(bytes - at < 16 ? bytes - at : 16);
}

__global__ void k_jenc_count_ff(const uint4* __restrict__ ubuf, const u64* __restrict__ off, const u64* __restrict__ ubase, int n, long nbi, u64 n_chunks, uint32_t* __restrict__ ff)
{
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) ff[n_chunks] = 0;
    if (c >= n_chunks) return;
    const int img = image_of_chunk(ubase, n, c), valid = chunk_valid(off, ubase, nbi, img, c);
    const uint4 q = ubuf[c];
    const uint32_t wd[4] = { q.x, q.y, q.z, q.w };
    uint32_t cnt = 0;
    for (int i = 0; i < valid; i++) cnt += ((wd[i >> 2] >> (8 * (i & 3))) & 255) == 255;
    ff[c] = cnt;
}

__global__ void k_jenc_image_len(const u64* __restrict__ off, const u64* __restrict__ ubase, const uint32_t* __restrict__ ffoff, int n, long nbi, u64* __restrict__ flen)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    flen[i] = i < n ? (u64)(kHeaderBytes + kTrailerBytes) + ((off[(long)(i + 1) * nbi] - off[(long)i * nbi] + 7) >> 3) + (ffoff[ubase[i + 1]] - ffoff[ubase[i]]) : 0;
}

__global__ void k_jenc_stuff(const uint4* __restrict__ ubuf, const u64* __restrict__ off, const u64* __restrict__ ubase, const uint32_t* __restrict__ ffoff,
                             const u64* __restrict__ fbase, int n, long nbi, u64 n_chunks, uint8_t* __restrict__ out)
{
    const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const int img = image_of_chunk(ubase, n, c), valid = chunk_valid(off, ubase, nbi, img, c);
    uint8_t* d = out + fbase[img] + kHeaderBytes + (c - ubase[img]) * 16 + (ffoff[c] - ffoff[ubase[img]]);
    const uint4 q = ubuf[c];
    const uint32_t wd[4] = { q.x, q.y, q.z, q.w };
    for (int i = 0; i < valid; i++) {
        const uint8_t b = (uint8_t)(wd[i >> 2] >> (8 * (i & 3)));
        *d++ = b;
        if (b == 255) *d++ = 0;
    }
}

__global__ void k_jenc_frame(const EncBlob* __restrict__ blob, const u64* __restrict__ fbase, int n, uint8_t* __restrict__ out)
{
    constexpr int per = kHeaderBytes + kTrailerBytes;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)n * per) return;
    const int i = (int)(t / per), j = (int)(t - (long)i * per);
    if (j < kHeaderBytes) out[fbase[i] + j] = blob->header[j];
    else out[fbase[i + 1] - kTrailerBytes + (j - kHeaderBytes)] = j == kHeaderBytes ? 0xFF : 0xD9;
}

struct Buf {
    void* p = nullptr; size_t cap = 0;
    bool reserve(size_t bytes)
    {
        if (bytes <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("jpeg encoder: hipMalloc of " + std::to_string(want) + " bytes failed"); return false; }
        cap = want;
        return true;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

#define JENC_OK(expr)                                                                                                  \
    do {                                                                                                               \
        const hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) { set_error(std::string("jpeg encoder: " #expr ": ") + hipGetErrorString(e_)); return false; } \
    } while (0)

struct JpegEncoder::Impl {
    Buf blob, coef, dcv, acbits, bits, off, chunks, ubase, ubuf, ff, ffoff, flen, fbase, out, temp;
    void* pinned = nullptr; size_t pinned_cap = 0;
    void* land = nullptr; size_t land_cap = 0;     // fetch_pinned's landing buffer
    int quality = -1, rows = 0, cols = 0;          // what the blob in HBM was built for
    size_t total = 0;                              // bytes of the streams in `out`
    ~Impl()
    {
        for (Buf* b : { &blob, &coef, &dcv, &acbits, &bits, &off, &chunks, &ubase, &ubuf, &ff, &ffoff, &flen, &fbase, &out, &temp }) b->release();
        if (pinned) (void)hipHostFree(pinned);
        if (land) (void)hipHostFree(land);
    }
    bool pin(size_t bytes)
    {
        if (bytes <= pinned_cap) return true;
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr; pinned_cap = 0;
        JENC_OK(hipHostMalloc(&pinned, bytes + 4096, hipHostMallocDefault));
        pinned_cap = bytes + 4096;
        return true;
    }
    template <class In, class Out> bool scan(const In* in, Out* outp, size_t count, hipStream_t s)
    {
        size_t need = 0;
        JENC_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, outp, (int)count, s));
        if (!temp.reserve(need)) return false;
        JENC_OK(hipcub::DeviceScan::ExclusiveSum(temp.p, need, in, outp, (int)count, s));
        return true;
    }
};

JpegEncoder::~JpegEncoder() { delete p_; }
void JpegEncoder::release() { delete p_; p_ = nullptr; }

bool JpegEncoder::encode(const void* dev_bgr, int n, const int* slots, size_t image_stride, int rows, int cols, size_t step, int quality, size_t* offsets, void* stream)
{ return encode_at(dev_bgr, n, slots, nullptr, image_stride, rows, cols, step, quality, offsets, stream); }

bool JpegEncoder::encode_windows(const void* dev_base, int n, const long long* byte_offsets, int rows, int cols, size_t step, int quality, size_t* offsets, void* stream)
{
    if (!byte_offsets) { set_error("jpeg encoder: bad arguments"); return false; }
    return encode_at(dev_base, n, nullptr, byte_offsets, 0, rows, cols, step, quality, offsets, stream);
}

bool JpegEncoder::encode_at(const void* dev_bgr, int n, const int* slots, const long long* where, size_t image_stride, int rows, int cols, size_t step, int quality, size_t* offsets, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!dev_bgr || n < 1 || rows < 1 || cols < 1 || rows > kMaxDim || cols > kMaxDim || step < (size_t)cols * 3 || !offsets) { set_error("jpeg encoder: bad arguments"); return false; }
    if (!p_) p_ = new Impl();
    Impl& d = *p_;
    d.total = 0;
    quality = clamp_quality(quality);
    const Geometry g = geometry(rows, cols);
    const long nbi = g.blocks(), n_mcus = (long)g.mcux * g.mcuy * n, nb = nbi * n;
    if (nb >= (1l << 31) - 1) { set_error("jpeg encoder: too many blocks for one pass"); return false; }
    if (quality != d.quality || rows != d.rows || cols != d.cols) {
        EncBlob h;
        build_tables(quality, h.t);
        write_header(h.t, rows, cols, h.header);
        h.header[kHeaderBytes] = 0;
        if (!d.blob.reserve(sizeof h)) return false;
        JENC_OK(hipStreamSynchronize(s));          // an earlier call's kernels on this stream may still read the blob
        JENC_OK(hipMemcpy(d.blob.p, &h, sizeof h, hipMemcpyHostToDevice));
        d.quality = quality; d.rows = rows; d.cols = cols;
    }
    const EncBlob* blob = (const EncBlob*)d.blob.p;
    long long* dwhere = nullptr;
    const bool listed = slots || where;
    if (!d.coef.reserve((size_t)nb * 128) || !d.dcv.reserve((size_t)nb * 2) || !d.acbits.reserve((size_t)nb * 4) || !d.bits.reserve((size_t)(nb + 1) * 8) ||
        !d.off.reserve((size_t)(nb + 1) * 8) || !d.chunks.reserve((size_t)(n + 1) * 8 + (listed ? (size_t)n * 8 : 0)) || !d.ubase.reserve((size_t)(n + 1) * 8) ||
        !d.flen.reserve((size_t)(n + 1) * 8) || !d.fbase.reserve((size_t)(n + 1) * 8) || !d.pin((size_t)(n + 2) * 8 + (listed ? (size_t)n * 8 : 0))) return false;
    if (listed) {          // as byte offsets, through the pinned buffer: the caller's list may go away before the copy runs
        long long* hs = (long long*)((char*)d.pinned + (size_t)(n + 2) * 8);
        for (int i = 0; i < n; i++) hs[i] = where ? where[i] : (long long)slots[i] * (long long)image_stride;
        dwhere = (long long*)((char*)d.chunks.p + (size_t)(n + 1) * 8);
        JENC_OK(hipMemcpyAsync(dwhere, hs, (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    const unsigned per_img = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(k_jenc_transform, dim3((unsigned)((n_mcus + kGroupMcus - 1) / kGroupMcus)), dim3(kTransformLanes), 0, s, (const uint8_t*)dev_bgr, dwhere, image_stride, step, g,
                       n_mcus, blob, (int16_t*)d.coef.p, (int16_t*)d.dcv.p, (uint32_t*)d.acbits.p);
    hipLaunchKernelGGL(k_jenc_bits, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, (const int16_t*)d.dcv.p, (const uint32_t*)d.acbits.p, nb, nbi, blob, (u64*)d.bits.p);
    if (!d.scan((const u64*)d.bits.p, (u64*)d.off.p, (size_t)nb + 1, s)) return false;
    hipLaunchKernelGGL(k_jenc_image_chunks, dim3(per_img), dim3(256), 0, s, (const u64*)d.off.p, n, nbi, (u64*)d.chunks.p);
    if (!d.scan((const u64*)d.chunks.p, (u64*)d.ubase.p, (size_t)n + 1, s)) return false;
    u64* host = (u64*)d.pinned;
    JENC_OK(hipMemcpyAsync(host, (const u64*)d.ubase.p + n, 8, hipMemcpyDeviceToHost, s));
    JENC_OK(hipStreamSynchronize(s));
    const u64 n_chunks = host[0];
    if (n_chunks == 0 || n_chunks >= (1ull << 27)) { set_error("jpeg encoder: the entropy-coded data does not fit one pass (" + std::to_string(n_chunks * 16) + " bytes)"); return false; }
    if (!d.ubuf.reserve((size_t)n_chunks * 16) || !d.ff.reserve((size_t)(n_chunks + 1) * 4) || !d.ffoff.reserve((size_t)(n_chunks + 1) * 4)) return false;
    JENC_OK(hipMemsetAsync(d.ubuf.p, 0, (size_t)n_chunks * 16, s));
    hipLaunchKernelGGL(k_jenc_pack, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, (const int16_t*)d.coef.p, (const int16_t*)d.dcv.p, (const u64*)d.off.p, (const u64*)d.ubase.p, nb, nbi,
                       blob, (uint32_t*)d.ubuf.p);
    const unsigned per_chunk = (unsigned)((n_chunks + 255) / 256);
    hipLaunchKernelGGL(k_jenc_count_ff, dim3(per_chunk), dim3(256), 0, s, (const uint4*)d.ubuf.p, (const u64*)d.off.p, (const u64*)d.ubase.p, n, nbi, n_chunks, (uint32_t*)d.ff.p);
    if (!d.scan((const uint32_t*)d.ff.p, (uint32_t*)d.ffoff.p, (size_t)n_chunks + 1, s)) return false;
    hipLaunchKernelGGL(k_jenc_image_len, dim3(per_img), dim3(256), 0, s, (const u64*)d.off.p, (const u64*)d.ubase.p, (const uint32_t*)d.ffoff.p, n, nbi, (u64*)d.flen.p);
    if (!d.scan((const u64*)d.flen.p, (u64*)d.fbase.p, (size_t)n + 1, s)) return false;
    JENC_OK(hipMemcpyAsync(host, d.fbase.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
    JENC_OK(hipStreamSynchronize(s));
    for (int i = 0; i <= n; i++) offsets[i] = (size_t)host[i];
    const size_t total = (size_t)host[n];
    if (!d.out.reserve(total)) return false;
    hipLaunchKernelGGL(k_jenc_stuff, dim3(per_chunk), dim3(256), 0, s, (const uint4*)d.ubuf.p, (const u64*)d.off.p, (const u64*)d.ubase.p, (const uint32_t*)d.ffoff.p, (const u64*)d.fbase.p, n, nbi,
                       n_chunks, (uint8_t*)d.out.p);
    constexpr int per = kHeaderBytes + kTrailerBytes;
    hipLaunchKernelGGL(k_jenc_frame, dim3((unsigned)(((long)n * per + 255) / 256)), dim3(256), 0, s, blob, (const u64*)d.fbase.p, n, (uint8_t*)d.out.p);
    JENC_OK(hipGetLastError());
    d.total = total;
    return true;
}

bool JpegEncoder::fetch(uint8_t* out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!p_ || !p_->total || !out) { set_error("jpeg encoder: nothing to fetch"); return false; }
    JENC_OK(hipMemcpyAsync(out, p_->out.p, p_->total, hipMemcpyDeviceToHost, s));
    JENC_OK(hipStreamSynchronize(s));
    return true;
}

const uint8_t* JpegEncoder::fetch_pinned(void* stream)
{
    if (!p_ || !p_->total) { set_error("jpeg encoder: nothing to fetch"); return nullptr; }
    Impl& d = *p_;
    if (d.total > d.land_cap) {
        if (d.land) (void)hipHostFree(d.land);
        d.land = nullptr; d.land_cap = 0;
        const size_t want = d.total + d.total / 4 + 4096;
        if (hipHostMalloc(&d.land, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); d.land = nullptr; set_error("jpeg encoder: no page-locked memory for the stream"); return nullptr; }
        d.land_cap = want;
    }
    return fetch((uint8_t*)d.land, stream) ? (const uint8_t*)d.land : nullptr;
}

}  // namespace pf
