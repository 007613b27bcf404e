// png_encode.hip -- the GPU side of the PNG of save_png() (png_encode.hpp): an image of BGR8 pixels (and a mask) of any size in device
// memory in, the complete PNG file in one device buffer out.  Byte-equal to png::encode on every input: the stream's bytes, the token
// rule, the length builder, the block plan, the cost of a stored block and both checksums are the headers' functions, called from the
// kernels.
//
//   k_png_plan   one workgroup of 256 lanes per deflate block: the block's bytes of the filtered stream F are made in LDS straight from
//                the image and the mask (png::stream_byte: filter byte, channel swap, minus the left neighbour read from the image;
//                lane t takes bytes t, t + 256, ..: its (row, byte of the row) is resolved once and stepped), then run starts and ends,
//                tokens, the histogram, dfl::plan_block on lane 0 and the block's Adler sums, as k_dfl_plan does.
//   k_png_join   one lane per segment of 16 blocks: dynamic or stored at the bit each block begins at, the bit offsets, the segment's
//                length with its closing empty block (or the Adler-32) and its 12 bytes of chunk framing, the Adler-32 of its bytes.
//   (hipCUB)     exclusive sum of the segment lengths: where every IDAT chunk begins.
//   k_png_pack   per block again: tokens once more, canonical codes, the bits packed in LDS at the alignment the block has in the file,
//                whole words stored, the words a block shares with its neighbours by atomicOr into the zeroed output.
//   k_png_frame  one workgroup per segment: chunk length, "IDAT", and the chunk's CRC-32 -- a table in LDS, a piece per lane read as
//                aligned words, the pieces combined in a tree with png::crc_combine.  Segment 0 also writes the signature, IHDR and the
//                zlib header, the last one the Adler-32 of F (the segments' sums combined in order) and IEND.
// Algorithmic bytes: the image read twice, 824 bytes of plan a block written and read, the file written once and read once.
#include "png_encode.hpp"
#include "jpeg_decode.hpp"          // set_error
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string>

namespace pf {

using namespace dfl;

namespace {

typedef unsigned long long u64;

constexpr int kLanes = 256;
constexpr int kPiece = kBlockBytes / kLanes;          // 48 bytes a lane
// a block's bits in LDS: at most 31 bits of lead, then no more than a stored block takes (98 346 bits)
constexpr int kOutWords = 3080;

struct Src {
    const uint8_t* bgr; size_t step;
    const uint8_t* mask; size_t mask_step;
    int bpp; uint32_t row_len;
    u64 N, blocks, segs;
};

__device__ inline int block_bytes(const Src& src, u64 blk)
{
    const u64 left = src.N - blk * (u64)kBlockBytes;
    return left < (u64)kBlockBytes ? (int)left : kBlockBytes;
}

// The n bytes of block blk of F in P and every position's token in tok (dfl::token_at); sa, sb: 256 ints each.
// Returns with the block's lanes synchronised.
__device__ void stage_block(const Src& src, u64 blk, int n, uint8_t* P, uint16_t* tok, int* sa, int* sb, int* sprev)
{
    const int t = threadIdx.x;
    const u64 p0 = blk * (u64)kBlockBytes;
    {
        const u64 p = p0 + (u64)t;
        u64 row = p / src.row_len;
        uint32_t q = (uint32_t)(p - row * src.row_len);
        for (int i = t; i < n; i += kLanes) {
            P[i] = png::stream_byte(src.bgr, src.step, src.mask, src.mask_step, src.bpp, row, q);
            q += kLanes;
            if (q >= src.row_len) { const uint32_t k = q / src.row_len; q -= k * src.row_len; row += k; }
        }
    }
    if (t == 0) {          // the last byte of the block before
        int v = -1;
        if (blk) {
            const u64 p = p0 - 1, row = p / src.row_len;
            v = png::stream_byte(src.bgr, src.step, src.mask, src.mask_step, src.bpp, row, (uint32_t)(p - row * src.row_len));
        }
        *sprev = v;
    }
    __syncthreads();
    const int c0 = t * kPiece, c1 = min(c0 + kPiece, n);
    int first = n, last = -1;
    for (int i = c0; i < c1; i++)
        if (i == 0 || P[i] != P[i - 1]) { if (first == n) first = i; last = i; }
    sa[t] = last; sb[t] = first;
    __syncthreads();
    for (int d = 1; d < kLanes; d <<= 1) {          // running maximum of the last run start, running minimum from the right of the first
        const int va = t >= d ? sa[t - d] : -1, vb = t + d < kLanes ? sb[t + d] : n;
        __syncthreads();
        sa[t] = max(sa[t], va); sb[t] = min(sb[t], vb);
        __syncthreads();
    }
    const int next = t + 1 < kLanes ? sb[t + 1] : n;
    const bool lean0 = *sprev == (int)P[0];
    int s = t ? sa[t - 1] : 0, e = 0;
    for (int i = c0; i < c1; i++) {
        const bool st = i == 0 || P[i] != P[i - 1];
        if (st) s = i;
        if (st || i == c0) { int k = i + 1; while (k < c1 && P[k] == P[i]) k++; e = k < c1 ? k : next; }
        tok[i] = (uint16_t)token_at(i, s, e, s == 0 && lean0);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kLanes) void k_png_plan(Src src, Plan* __restrict__ plans, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t Pw[kBlockBytes / 4];
    __shared__ uint16_t tok[kBlockBytes];
    __shared__ uint32_t hist[kMaxSyms];
    __shared__ int sa[kLanes], sb[kLanes], sprev;
    __shared__ uint32_t sS, sT;
    __shared__ Work work;
    __shared__ Plan plan;
    uint8_t* P = (uint8_t*)Pw;
    const int t = threadIdx.x;
    const u64 blk = blockIdx.x;
    const int n = block_bytes(src, blk);
    for (int i = t; i < kMaxSyms; i += kLanes) hist[i] = 0;
    if (t == 0) { sS = 0; sT = 0; }
    stage_block(src, blk, n, P, tok, sa, sb, &sprev);
    const int c0 = t * kPiece, c1 = min(c0 + kPiece, n);
    uint32_t S = 0, T = 0;
    for (int i = c0; i < c1; i++) {
        const int x = P[i], tk = tok[i];
        S += (uint32_t)x; T += (uint32_t)(c1 - i) * (uint32_t)x;
        if (tk == 1) atomicAdd(&hist[x], 1u);
        else if (tk) { int sym, eb, ev; length_symbol(tk, sym, eb, ev); atomicAdd(&hist[sym], 1u); }
    }
    if (c0 < c1) {          // the piece's share of T = sum (n - k) x_k: its own weights count from the piece's end, n - c1 bytes follow it
        atomicAdd(&sS, S);
        atomicAdd(&sT, (T + S * (uint32_t)(n - c1)) % kAdlerMod);
    }
    __syncthreads();
    if (t == 0) { hist[256] = 1; plan_block(hist, blk == src.blocks - 1, plan, work); }
    __syncthreads();
    const uint32_t* from = (const uint32_t*)&plan;
    uint32_t* dst = (uint32_t*)(plans + blk);
    for (int i = t; i < (int)(sizeof(Plan) / 4); i += kLanes) dst[i] = from[i];
    if (t == 0) { sums[2 * blk] = sS % kAdlerMod; sums[2 * blk + 1] = sT % kAdlerMod; }
}

__global__ void k_png_join(Src src, const Plan* __restrict__ plans, const uint32_t* __restrict__ sums, uint8_t* __restrict__ dynamic, uint32_t* __restrict__ bitoff,
                           u64* __restrict__ len, uint32_t* __restrict__ seg_adler)
{
    const u64 seg = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (seg > src.segs) return;
    if (seg == src.segs) { len[seg] = 0; return; }
    uint32_t at = seg == 0 ? 16 : 0, a = 1, b = 0;          // (the zlib header lies in front of segment 0's blocks)
    const u64 b0 = seg * png::kSegBlocks, b1 = min(b0 + (u64)png::kSegBlocks, src.blocks);
    for (u64 g = b0; g < b1; g++) {
        const uint32_t n = (uint32_t)block_bytes(src, g);
        const uint32_t dyn = plans[g].dyn_bits, st = png::stored_bits(at, n);
        const bool d = dyn <= st;
        dynamic[g] = d ? 1 : 0; bitoff[g] = at;
        at += d ? dyn : st;
        adler_join(a, b, sums[2 * g], sums[2 * g + 1], n);
    }
    if (seg + 1 < src.segs) at = (at + 3 + 7) / 8 * 8 + 32;          // the empty stored block
    else at = (at + 7) / 8 * 8 + 32;                                  // the Adler-32
    len[seg] = (u64)(at / 8) + png::kChunkFrame;
    seg_adler[seg] = (b << 16) | a;
}

__device__ inline void or_byte(uint32_t* out, u64 byte_at, uint32_t v) { atomicOr(out + (byte_at >> 2), v << (8 * (uint32_t)(byte_at & 3))); }
__device__ inline void or_be32(uint32_t* out, u64 byte_at, uint32_t v) { for (int i = 0; i < 4; i++) or_byte(out, byte_at + i, (v >> (8 * (3 - i))) & 255); }

__global__ __launch_bounds__(kLanes) void k_png_pack(Src src, const Plan* __restrict__ plans, const uint8_t* __restrict__ dynamic, const uint32_t* __restrict__ bitoff,
                                                     const u64* __restrict__ off, uint32_t* __restrict__ out)
{
    __shared__ uint32_t Pw[kBlockBytes / 4];
    __shared__ uint16_t tok[kBlockBytes];
    __shared__ uint32_t outw[kOutWords];
    __shared__ uint16_t code[kMaxSyms];
    __shared__ uint8_t clen[kMaxSyms];
    __shared__ int sa[kLanes], sb[kLanes], sprev;
    uint8_t* P = (uint8_t*)Pw;
    const int t = threadIdx.x;
    const u64 blk = blockIdx.x, seg = blk / png::kSegBlocks;
    const int n = block_bytes(src, blk);
    const Plan& plan = plans[blk];
    const u64 data0 = png::kHeadBytes + off[seg] + 8;          // the chunk's data begin behind its length and type
    const u64 A = 8 * data0 + bitoff[blk];                     // where the block begins in the file, in bits
    const uint32_t lead = (uint32_t)(A & 31);
    const u64 word0 = A >> 5;
    const bool dyn = dynamic[blk] != 0;
    for (int i = t; i < kOutWords; i += kLanes) outw[i] = 0;
    for (int i = t; i < kMaxSyms; i += kLanes) clen[i] = plan.len[i];
    stage_block(src, blk, n, P, tok, sa, sb, &sprev);
    uint32_t nbits;
    if (dyn) {
        if (t == 0) canonical_codes(clen, kLitLen, code);
        const uint32_t hdr_bits = plan.hdr_bits;
        nbits = plan.dyn_bits;
        for (uint32_t w = t; w * 32 < hdr_bits; w += kLanes) {
            const uint32_t v = plan.hdr[w], pos = lead + 32 * w;
            atomicOr(&outw[pos >> 5], v << (pos & 31));
            if (pos & 31) atomicOr(&outw[(pos >> 5) + 1], v >> (32 - (pos & 31)));
        }
        const int c0 = t * kPiece, c1 = min(c0 + kPiece, n);
        int mine = 0;
        for (int i = c0; i < c1; i++) {
            const int tk = tok[i];
            if (tk == 1) mine += clen[P[i]];
            else if (tk) { int sym, eb, ev; length_symbol(tk, sym, eb, ev); mine += clen[sym] + eb + 1; }
        }
        sa[t] = mine;
        __syncthreads();          // (the codes are there too)
        for (int d = 1; d < kLanes; d <<= 1) {
            const int v = t >= d ? sa[t - d] : 0;
            __syncthreads();
            sa[t] += v;
            __syncthreads();
        }
        const uint32_t q = lead + hdr_bits + (uint32_t)(sa[t] - mine);
        uint32_t wi = q >> 5; int fill = (int)(q & 31); u64 acc = 0;
        auto emit = [&](uint32_t v, int nb) {
            acc |= (u64)v << fill; fill += nb;
            if (fill >= 32) { if (wi < (uint32_t)kOutWords) atomicOr(&outw[wi], (uint32_t)acc); wi++; acc >>= 32; fill -= 32; }
        };
        for (int i = c0; i < c1; i++) {
            const int tk = tok[i];
            if (tk == 1) { const int x = P[i]; emit(code[x], clen[x]); }
            else if (tk) { int sym, eb, ev; length_symbol(tk, sym, eb, ev); emit((uint32_t)code[sym] | ((uint32_t)ev << clen[sym]), clen[sym] + eb + 1); }
        }
        if (t == kLanes - 1) emit(code[256], clen[256]);
        if (fill > 0 && wi < (uint32_t)kOutWords) atomicOr(&outw[wi], (uint32_t)acc);
    } else {
        nbits = png::stored_bits(A, (uint32_t)n);          // (a segment begins on a byte: A and the block's bit offset agree mod 8)
        uint8_t* ob = (uint8_t*)outw;
        const uint32_t hb = (lead + 3 + 7) / 8;          // the byte LEN begins at
        if (t == 0) {
            if (blk == src.blocks - 1) atomicOr(&outw[0], 1u << lead);
            ob[hb] = (uint8_t)(n & 255); ob[hb + 1] = (uint8_t)(n >> 8);
            ob[hb + 2] = (uint8_t)(~n & 255); ob[hb + 3] = (uint8_t)((~n >> 8) & 255);
        }
        __syncthreads();          // the lanes' byte stores below share words with lane 0's
        for (int i = t; i < n; i += kLanes) ob[hb + 4 + i] = P[i];
    }
    __syncthreads();
    const int nwords = (int)((lead + nbits + 31) / 32);
    for (int w = t; w < nwords && w < kOutWords; w += kLanes) {
        const uint32_t v = outw[w];
        if (w == 0 || w == nwords - 1) atomicOr(out + word0 + w, v); else out[word0 + w] = v;
    }
    // the segment's closing empty stored block: zero bits up to a byte, LEN 0, NLEN FFFF, the last four bytes in front of the chunk's CRC
    if (t == 0 && seg + 1 < src.segs && blk == (seg + 1) * png::kSegBlocks - 1) {
        const u64 end = png::kHeadBytes + off[seg + 1] - 4;
        or_byte(out, end - 2, 0xFF); or_byte(out, end - 1, 0xFF);
    }
}

__device__ inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

__global__ __launch_bounds__(kLanes) void k_png_frame(Src src, int rows, int cols, const u64* __restrict__ off, const uint32_t* __restrict__ seg_adler, uint32_t* __restrict__ out)
{
    __shared__ uint32_t table[256];
    __shared__ uint32_t scrc[kLanes];
    __shared__ uint32_t slen[kLanes];
    const int t = threadIdx.x;
    const u64 seg = blockIdx.x;
    const bool first = seg == 0, last = seg + 1 == src.segs;
    table[t] = png::crc_table_entry((uint32_t)t);
    __syncthreads();
    const u64 chunk = png::kHeadBytes + off[seg], end = png::kHeadBytes + off[seg + 1] - 4;          // the chunk; its CRC
    // what the lanes read: the data without the zlib header and the Adler-32, which lane 0 folds in from their values
    const u64 s = chunk + 8 + (first ? 2 : 0), e = end - (last ? 4 : 0);
    const u64 w0 = s & ~3ull, pw = ((e - w0 + 3) / 4 + kLanes - 1) / kLanes;
    const u64 lo = max(s, w0 + (u64)t * pw * 4), hi = min(e, w0 + (u64)(t + 1) * pw * 4);
    uint32_t c = 0xFFFFFFFFu;
    if (t == 0) {
        c = png::crc_word(table, c, 'I' | 'D' << 8 | 'A' << 16 | (uint32_t)'T' << 24);
        if (first) { c = table[(c ^ 0x78) & 255] ^ (c >> 8); c = table[(c ^ 0x01) & 255] ^ (c >> 8); }
    }
    uint32_t mylen = 0;
    if (lo < hi) {
        const uint8_t* ob = (const uint8_t*)out;
        u64 p = lo;
        for (; p < hi && (p & 3); p++) c = table[(c ^ ob[p]) & 255] ^ (c >> 8);
        for (; p + 4 <= hi; p += 4) c = png::crc_word(table, c, out[p >> 2]);
        for (; p < hi; p++) c = table[(c ^ ob[p]) & 255] ^ (c >> 8);
        mylen = (uint32_t)(hi - lo);
    }
    scrc[t] = ~c; slen[t] = mylen;
    __syncthreads();
    for (int d = 1; d < kLanes; d <<= 1) {
        if ((t & (2 * d - 1)) == 0) {
            if (slen[t + d]) scrc[t] = png::crc_combine(scrc[t], scrc[t + d], slen[t + d]);
            slen[t] += slen[t + d];
        }
        __syncthreads();
    }
    if (t != 0) return;
    uint32_t crc = scrc[0];
    if (last) {          // the Adler-32 of F: the segments' in order; it ends the chunk's data
        uint32_t ad = seg_adler[0];
        for (u64 k = 1; k < src.segs; k++) {
            const u64 f0 = k * (u64)png::kSegBlocks * kBlockBytes, f1 = min(f0 + (u64)png::kSegBlocks * kBlockBytes, src.N);
            ad = png::adler_combine(ad, seg_adler[k], f1 - f0);
        }
        or_be32(out, end - 4, ad);
        crc = ~png::crc_word(table, ~crc, bswap32(ad));
    }
    or_be32(out, chunk, (uint32_t)(end - chunk - 8));
    or_be32(out, chunk + 4, 'I' << 24 | 'D' << 16 | 'A' << 8 | 'T');
    or_be32(out, end, crc);
    if (first) {
        or_be32(out, 0, 0x89504E47u); or_be32(out, 4, 0x0D0A1A0Au);
        or_be32(out, 8, 13); or_be32(out, 12, 'I' << 24 | 'H' << 16 | 'D' << 8 | 'R');
        or_be32(out, 16, (uint32_t)cols); or_be32(out, 20, (uint32_t)rows);
        const uint32_t ctype = src.bpp == 4 ? 6 : 2;
        or_byte(out, 24, 8); or_byte(out, 25, ctype);
        uint32_t h = 0xFFFFFFFFu;
        h = png::crc_word(table, h, 'I' | 'H' << 8 | 'D' << 16 | (uint32_t)'R' << 24);
        h = png::crc_word(table, h, bswap32((uint32_t)cols)); h = png::crc_word(table, h, bswap32((uint32_t)rows));
        h = png::crc_word(table, h, 8 | ctype << 8);
        h = table[h & 255] ^ (h >> 8);          // the interlace byte, 0
        or_be32(out, 29, ~h);
        or_byte(out, chunk + 8, 0x78); or_byte(out, chunk + 9, 0x01);
    }
    if (last) {
        const uint32_t h = png::crc_word(table, 0xFFFFFFFFu, 'I' | 'E' << 8 | 'N' << 16 | (uint32_t)'D' << 24);
        or_be32(out, end + 8, 'I' << 24 | 'E' << 16 | 'N' << 8 | 'D');          // (its length, 0, is there)
        or_be32(out, end + 12, ~h);
    }
}

struct Buf {
    void* p = nullptr; size_t cap = 0;
    bool reserve(size_t bytes)
    {
        if (bytes <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("png encoder: hipMalloc of " + std::to_string(want) + " bytes failed"); return false; }
        cap = want;
        return true;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

#define PNG_OK(expr)                                                                                                  \
    do {                                                                                                              \
        const hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) { set_error(std::string("png encoder: " #expr ": ") + hipGetErrorString(e_)); return false; } \
    } while (0)

struct PngEncoder::Impl {
    Buf plans, sums, dynamic, bitoff, len, off, seg_adler, out, temp;
    void* pinned = nullptr;
    void* land = nullptr; size_t land_cap = 0;
    size_t total = 0;
    ~Impl()
    {
        for (Buf* b : { &plans, &sums, &dynamic, &bitoff, &len, &off, &seg_adler, &out, &temp }) b->release();
        if (pinned) (void)hipHostFree(pinned);
        if (land) (void)hipHostFree(land);
    }
};

PngEncoder::~PngEncoder() { delete p_; }
void PngEncoder::release() { delete p_; p_ = nullptr; }

bool PngEncoder::encode(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, size_t* len, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    png::Geometry g;
    if (!dev_bgr || !len || !png::geometry(rows, cols, dev_mask != nullptr, g)) { set_error("png encoder: no image, no length or sizes the format's indices do not reach"); return false; }
    if (step < (size_t)cols * 3 || (dev_mask && mask_step < (size_t)cols)) { set_error("png encoder: step is smaller than a row"); return false; }
    if (!p_) p_ = new Impl();
    Impl& d = *p_;
    d.total = 0;
    const size_t nb = (size_t)g.blocks, ns = (size_t)g.segs;
    const size_t out_cap = ((size_t)g.bound + 3) / 4 * 4 + 8;
    if (!d.plans.reserve(nb * sizeof(Plan)) || !d.sums.reserve(nb * 8) || !d.dynamic.reserve(nb) || !d.bitoff.reserve(nb * 4) || !d.len.reserve((ns + 1) * 8) ||
        !d.off.reserve((ns + 1) * 8) || !d.seg_adler.reserve(ns * 4) || !d.out.reserve(out_cap)) return false;
    if (!d.pinned) PNG_OK(hipHostMalloc(&d.pinned, 64, hipHostMallocDefault));
    Src src;
    src.bgr = (const uint8_t*)dev_bgr; src.step = step; src.mask = (const uint8_t*)dev_mask; src.mask_step = mask_step;
    src.bpp = g.bpp; src.row_len = (uint32_t)g.row_len; src.N = g.N; src.blocks = g.blocks; src.segs = g.segs;
    PNG_OK(hipMemsetAsync(d.out.p, 0, out_cap, s));
    hipLaunchKernelGGL(k_png_plan, dim3((unsigned)nb), dim3(kLanes), 0, s, src, (Plan*)d.plans.p, (uint32_t*)d.sums.p);
    hipLaunchKernelGGL(k_png_join, dim3((unsigned)((ns + 1 + 255) / 256)), dim3(256), 0, s, src, (const Plan*)d.plans.p, (const uint32_t*)d.sums.p, (uint8_t*)d.dynamic.p, (uint32_t*)d.bitoff.p,
                       (u64*)d.len.p, (uint32_t*)d.seg_adler.p);
    size_t need = 0;
    PNG_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (const u64*)d.len.p, (u64*)d.off.p, (int)(ns + 1), s));
    if (!d.temp.reserve(need)) return false;
    PNG_OK(hipcub::DeviceScan::ExclusiveSum(d.temp.p, need, (const u64*)d.len.p, (u64*)d.off.p, (int)(ns + 1), s));
    hipLaunchKernelGGL(k_png_pack, dim3((unsigned)nb), dim3(kLanes), 0, s, src, (const Plan*)d.plans.p, (const uint8_t*)d.dynamic.p, (const uint32_t*)d.bitoff.p, (const u64*)d.off.p,
                       (uint32_t*)d.out.p);
    hipLaunchKernelGGL(k_png_frame, dim3((unsigned)ns), dim3(kLanes), 0, s, src, rows, cols, (const u64*)d.off.p, (const uint32_t*)d.seg_adler.p, (uint32_t*)d.out.p);
    PNG_OK(hipGetLastError());
    u64* host = (u64*)d.pinned;
    PNG_OK(hipMemcpyAsync(host, (const u64*)d.off.p + ns, 8, hipMemcpyDeviceToHost, s));
    PNG_OK(hipStreamSynchronize(s));
    const u64 total = png::kHeadBytes + host[0] + png::kChunkFrame;          // IEND behind the chunks
    *len = (size_t)total;
    if (total > g.bound) { set_error("png encoder: the file is longer than its bound"); return false; }
    d.total = (size_t)total;
    return true;
}

bool PngEncoder::fetch(uint8_t* out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!p_ || !p_->total || !out) { set_error("png encoder: nothing to fetch"); return false; }
    PNG_OK(hipMemcpyAsync(out, p_->out.p, p_->total, hipMemcpyDeviceToHost, s));
    PNG_OK(hipStreamSynchronize(s));
    return true;
}

const uint8_t* PngEncoder::fetch_pinned(void* stream)
{
    if (!p_ || !p_->total) { set_error("png encoder: nothing to fetch"); return nullptr; }
    Impl& d = *p_;
    if (d.total > d.land_cap) {
        if (d.land) (void)hipHostFree(d.land);
        d.land = nullptr; d.land_cap = 0;
        const size_t want = d.total + d.total / 4 + 4096;
        if (hipHostMalloc(&d.land, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); d.land = nullptr; set_error("png encoder: no page-locked memory for the file"); return nullptr; }
        d.land_cap = want;
    }
    return fetch((uint8_t*)d.land, stream) ? (const uint8_t*)d.land : nullptr;
}

}  // namespace pf
