// deflate_encode.hip -- the GPU side of the lossless tile codec (deflate_rle.hpp): n tiles of 256 x 256 BGR pixels anywhere in
// one allocation in, their zlib streams back to back and the offsets out.  Byte-equal to dfl::encode_tile on every input: the token
// rule, the length builder, the block plan and the cost of a stored block are the header's functions, called from the kernels.
//
//   k_dfl_plan   one workgroup of 256 lanes per (tile, block of 16 rows): the block's 12 288 predicted bytes are made in LDS (load,
//                BGR -> RGB, minus the sample before), run starts and ends come from two scans over the lanes' 48-byte pieces, every
//                position gets its token, the histogram is counted with LDS atomics, lane 0 runs dfl::plan_block (code lengths,
//                header bits, cost) and the lanes store the plan; the block's Adler sums go with it.
//   k_dfl_join   one lane per tile walks its 16 blocks in order: dynamic or stored at the bit the block begins at, every block's
//                bit offset, the tile's length, its Adler-32.
//   (hipCUB)     exclusive sum of the tile lengths: where every stream begins.
//   k_dfl_pack   per (tile, block) again: the tokens are made once more (reading 12 KB again costs less than storing and shifting
//                a block's bits), the canonical codes from the plan's lengths, an exclusive sum of the tokens' bit counts, the bits
//                packed into LDS at the alignment the block has in the output, then whole words stored -- the first and last word
//                of a block, which it shares with its neighbours, by atomicOr into the zeroed output.
// Algorithmic bytes: the tiles read twice (2 x 196 608 a tile), 824 bytes of plan a block written and read, the streams written.
#include "deflate_rle.hpp"
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

// The block's predicted bytes in P and every position's token in tok (dfl::token_at); sa, sb: 256 ints each.
// Returns with the block's lanes synchronised.
__device__ void stage_block(const uint8_t* __restrict__ win, size_t step, int blk, uint8_t* P, uint16_t* tok, int* sa, int* sb, int* sprev)
{
    const int t = threadIdx.x;
    for (int rr = 0; rr < kBlockRows; rr++) {
        const uint8_t* s = win + (size_t)(blk * kBlockRows + rr) * step + 3 * t;
        const int b = s[0], g = s[1], r = s[2];
        int pb = 0, pg = 0, pr = 0;
        if (t) { pb = s[-3]; pg = s[-2]; pr = s[-1]; }
        uint8_t* d = P + rr * kRowBytes + 3 * t;
        d[0] = (uint8_t)(r - pr); d[1] = (uint8_t)(g - pg); d[2] = (uint8_t)(b - pb);
    }
    if (t == 0) {          // the last predicted byte of the block before: the blue sample of the last pixel of the row above
        int v = -1;
        if (blk) { const uint8_t* s = win + (size_t)(blk * kBlockRows - 1) * step + 3 * (kTile - 1); v = (uint8_t)(s[0] - s[-3]); }
        *sprev = v;
    }
    __syncthreads();
    const int c0 = t * kPiece, c1 = c0 + kPiece;
    int first = kBlockBytes, last = -1;
    for (int i = c0; i < c1; i++)
        if (i == 0 || P[i] != P[i - 1]) { if (first == kBlockBytes) first = i; last = i; }
    sa[t] = last; sb[t] = first;
    __syncthreads();
    for (int d = 1; d < kLanes; d <<= 1) {          // running maximum of the last run start, running minimum from the right of the first
        const int va = t >= d ? sa[t - d] : -1, vb = t + d < kLanes ? sb[t + d] : kBlockBytes;
        __syncthreads();
        sa[t] = max(sa[t], va); sb[t] = min(sb[t], vb);
        __syncthreads();
    }
    const int next = t + 1 < kLanes ? sb[t + 1] : kBlockBytes;
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

__global__ __launch_bounds__(kLanes) void k_dfl_plan(const uint8_t* __restrict__ base, const long long* __restrict__ where, size_t step, Plan* __restrict__ plans, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t Pw[kBlockBytes / 4];
    __shared__ uint16_t tok[kBlockBytes];
    __shared__ uint32_t hist[kMaxSyms];
    __shared__ int sa[kLanes], sb[kLanes], sprev;
    __shared__ uint32_t sS, sT;
    __shared__ Work work;
    __shared__ Plan plan;
    uint8_t* P = (uint8_t*)Pw;
    const int t = threadIdx.x, tile = blockIdx.x / kBlocks, blk = blockIdx.x % kBlocks;
    for (int i = t; i < kMaxSyms; i += kLanes) hist[i] = 0;
    if (t == 0) { sS = 0; sT = 0; }
    stage_block(base + where[tile], step, blk, P, tok, sa, sb, &sprev);
    const int c0 = t * kPiece;
    uint32_t S = 0, T = 0;
    for (int k = 0; k < kPiece; k++) {
        const int x = P[c0 + k], tk = tok[c0 + k];
        S += (uint32_t)x; T += (uint32_t)(kPiece - k) * (uint32_t)x;
        if (tk == 1) atomicAdd(&hist[x], 1u);
        else if (tk) { int sym, eb, ev; length_symbol(tk, sym, eb, ev); atomicAdd(&hist[sym], 1u); }
    }
    // the piece's share of T = sum (n - k) x_k: its own weights count from the piece's end, n - c1 bytes follow it
    atomicAdd(&sS, S);
    atomicAdd(&sT, (T + S * (uint32_t)(kBlockBytes - c0 - kPiece)) % kAdlerMod);
    __syncthreads();
    if (t == 0) { hist[256] = 1; plan_block(hist, blk == kBlocks - 1, plan, work); }
    __syncthreads();
    const uint32_t* src = (const uint32_t*)&plan;
    uint32_t* dst = (uint32_t*)(plans + blockIdx.x);
    for (int i = t; i < (int)(sizeof(Plan) / 4); i += kLanes) dst[i] = src[i];
    if (t == 0) { sums[2 * (size_t)blockIdx.x] = sS % kAdlerMod; sums[2 * (size_t)blockIdx.x + 1] = sT % kAdlerMod; }
}

__global__ void k_dfl_join(const Plan* __restrict__ plans, const uint32_t* __restrict__ sums, int n, uint8_t* __restrict__ dynamic, uint32_t* __restrict__ bitoff, u64* __restrict__ len,
                           uint32_t* __restrict__ adler)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { len[n] = 0; return; }
    uint32_t at = 16, a = 1, b = 0;
    for (int blk = 0; blk < kBlocks; blk++) {
        const size_t g = (size_t)i * kBlocks + blk;
        const uint32_t dyn = plans[g].dyn_bits, st = stored_bits(at);
        const bool d = dyn <= st;
        dynamic[g] = d ? 1 : 0; bitoff[g] = at;
        at += d ? dyn : st;
        adler_join(a, b, sums[2 * g], sums[2 * g + 1], kBlockBytes);
    }
    len[i] = (u64)((at + 7) / 8 + 4);
    adler[i] = (b << 16) | a;
}

__device__ inline void or_byte(uint32_t* out, u64 byte_at, uint32_t v) { atomicOr(out + (byte_at >> 2), v << (8 * (uint32_t)(byte_at & 3))); }

__global__ __launch_bounds__(kLanes) void k_dfl_pack(const uint8_t* __restrict__ base, const long long* __restrict__ where, size_t step, const Plan* __restrict__ plans,
                                                     const uint8_t* __restrict__ dynamic, const uint32_t* __restrict__ bitoff, const u64* __restrict__ off, const uint32_t* __restrict__ adler,
                                                     uint32_t* __restrict__ out)
{
    __shared__ uint32_t Pw[kBlockBytes / 4];
    __shared__ uint16_t tok[kBlockBytes];
    __shared__ uint32_t outw[kOutWords];
    __shared__ uint16_t code[kMaxSyms];
    __shared__ uint8_t clen[kMaxSyms];
    __shared__ int sa[kLanes], sb[kLanes], sprev;
    uint8_t* P = (uint8_t*)Pw;
    const int t = threadIdx.x, tile = blockIdx.x / kBlocks, blk = blockIdx.x % kBlocks;
    const Plan& plan = plans[blockIdx.x];
    const u64 A = 8 * off[tile] + bitoff[blockIdx.x];          // where the block begins in the output, in bits
    const uint32_t lead = (uint32_t)(A & 31);
    const u64 word0 = A >> 5;
    const bool dyn = dynamic[blockIdx.x] != 0;
    for (int i = t; i < kOutWords; i += kLanes) outw[i] = 0;
    for (int i = t; i < kMaxSyms; i += kLanes) clen[i] = plan.len[i];
    stage_block(base + where[tile], step, blk, P, tok, sa, sb, &sprev);
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
        const int c0 = t * kPiece;
        int mine = 0;
        for (int k = 0; k < kPiece; k++) {
            const int tk = tok[c0 + k];
            if (tk == 1) mine += clen[P[c0 + k]];
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
        for (int k = 0; k < kPiece; k++) {
            const int tk = tok[c0 + k];
            if (tk == 1) { const int x = P[c0 + k]; emit(code[x], clen[x]); }
            else if (tk) { int sym, eb, ev; length_symbol(tk, sym, eb, ev); emit((uint32_t)code[sym] | ((uint32_t)ev << clen[sym]), clen[sym] + eb + 1); }
        }
        if (t == kLanes - 1) emit(code[256], clen[256]);
        if (fill > 0 && wi < (uint32_t)kOutWords) atomicOr(&outw[wi], (uint32_t)acc);
    } else {
        nbits = stored_bits(A);          // (a stream begins on a byte: A and the block's bit offset agree mod 8)
        uint8_t* ob = (uint8_t*)outw;
        const uint32_t hb = (lead + 3 + 7) / 8;          // the byte LEN begins at
        if (t == 0) {
            if (blk == kBlocks - 1) atomicOr(&outw[0], 1u << lead);
            ob[hb] = (uint8_t)(kBlockBytes & 255); ob[hb + 1] = (uint8_t)(kBlockBytes >> 8);
            ob[hb + 2] = (uint8_t)(~kBlockBytes & 255); ob[hb + 3] = (uint8_t)((~kBlockBytes >> 8) & 255);
        }
        __syncthreads();          // the lanes' byte stores below share words with lane 0's
        for (int i = t; i < kBlockBytes; i += kLanes) ob[hb + 4 + i] = P[i];
    }
    __syncthreads();
    const int nwords = (int)((lead + nbits + 31) / 32);
    for (int w = t; w < nwords && w < kOutWords; w += kLanes) {
        const uint32_t v = outw[w];
        if (w == 0 || w == nwords - 1) atomicOr(out + word0 + w, v); else out[word0 + w] = v;
    }
    if (t == 0 && blk == 0) { or_byte(out, off[tile], 0x78); or_byte(out, off[tile] + 1, 0x01); }
    if (t == 0 && blk == kBlocks - 1) {
        const uint32_t ad = adler[tile];
        const u64 at = off[tile + 1] - 4;
        for (int i = 0; i < 4; i++) or_byte(out, at + i, (ad >> (8 * (3 - i))) & 255);
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
        if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("deflate encoder: hipMalloc of " + std::to_string(want) + " bytes failed"); return false; }
        cap = want;
        return true;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

#define DFL_OK(expr)                                                                                                      \
    do {                                                                                                                  \
        const hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess) { set_error(std::string("deflate encoder: " #expr ": ") + hipGetErrorString(e_)); return false; } \
    } while (0)

struct DeflateEncoder::Impl {
    Buf where, plans, sums, dynamic, bitoff, len, off, adler, out, temp;
    void* pinned = nullptr; size_t pinned_cap = 0;
    void* land = nullptr; size_t land_cap = 0;
    size_t total = 0;
    ~Impl()
    {
        for (Buf* b : { &where, &plans, &sums, &dynamic, &bitoff, &len, &off, &adler, &out, &temp }) b->release();
        if (pinned) (void)hipHostFree(pinned);
        if (land) (void)hipHostFree(land);
    }
    bool pin(size_t bytes)
    {
        if (bytes <= pinned_cap) return true;
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr; pinned_cap = 0;
        DFL_OK(hipHostMalloc(&pinned, bytes + 4096, hipHostMallocDefault));
        pinned_cap = bytes + 4096;
        return true;
    }
};

DeflateEncoder::~DeflateEncoder() { delete p_; }
void DeflateEncoder::release() { delete p_; p_ = nullptr; }

bool DeflateEncoder::encode_windows(const void* dev_base, int n, const long long* byte_offsets, size_t step, size_t* offsets, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!dev_base || n < 1 || n > (1 << 20) || !byte_offsets || step < (size_t)kRowBytes || !offsets) { set_error("deflate encoder: bad arguments"); return false; }
    if (!p_) p_ = new Impl();
    Impl& d = *p_;
    d.total = 0;
    const size_t nb = (size_t)n * kBlocks;
    const size_t out_cap = ((size_t)n * kStreamBound + 3) / 4 * 4 + 8;
    if (!d.where.reserve((size_t)n * 8) || !d.plans.reserve(nb * sizeof(Plan)) || !d.sums.reserve(nb * 8) || !d.dynamic.reserve(nb) || !d.bitoff.reserve(nb * 4) ||
        !d.len.reserve((size_t)(n + 1) * 8) || !d.off.reserve((size_t)(n + 1) * 8) || !d.adler.reserve((size_t)n * 4) || !d.out.reserve(out_cap) || !d.pin((size_t)(2 * n + 2) * 8)) return false;
    // through the pinned buffer: the caller's list may go away before the copy runs
    long long* hs = (long long*)((char*)d.pinned + (size_t)(n + 2) * 8);
    for (int i = 0; i < n; i++) hs[i] = byte_offsets[i];
    DFL_OK(hipMemcpyAsync(d.where.p, hs, (size_t)n * 8, hipMemcpyHostToDevice, s));
    DFL_OK(hipMemsetAsync(d.out.p, 0, out_cap, s));
    hipLaunchKernelGGL(k_dfl_plan, dim3((unsigned)nb), dim3(kLanes), 0, s, (const uint8_t*)dev_base, (const long long*)d.where.p, step, (Plan*)d.plans.p, (uint32_t*)d.sums.p);
    hipLaunchKernelGGL(k_dfl_join, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, s, (const Plan*)d.plans.p, (const uint32_t*)d.sums.p, n, (uint8_t*)d.dynamic.p, (uint32_t*)d.bitoff.p,
                       (u64*)d.len.p, (uint32_t*)d.adler.p);
    size_t need = 0;
    DFL_OK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (const u64*)d.len.p, (u64*)d.off.p, n + 1, s));
    if (!d.temp.reserve(need)) return false;
    DFL_OK(hipcub::DeviceScan::ExclusiveSum(d.temp.p, need, (const u64*)d.len.p, (u64*)d.off.p, n + 1, s));
    hipLaunchKernelGGL(k_dfl_pack, dim3((unsigned)nb), dim3(kLanes), 0, s, (const uint8_t*)dev_base, (const long long*)d.where.p, step, (const Plan*)d.plans.p, (const uint8_t*)d.dynamic.p,
                       (const uint32_t*)d.bitoff.p, (const u64*)d.off.p, (const uint32_t*)d.adler.p, (uint32_t*)d.out.p);
    DFL_OK(hipGetLastError());
    u64* host = (u64*)d.pinned;
    DFL_OK(hipMemcpyAsync(host, d.off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
    DFL_OK(hipStreamSynchronize(s));
    for (int i = 0; i <= n; i++) offsets[i] = (size_t)host[i];
    if (host[n] > (u64)n * kStreamBound) { set_error("deflate encoder: a stream is longer than its bound"); return false; }
    d.total = (size_t)host[n];
    return true;
}

bool DeflateEncoder::fetch(uint8_t* out, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!p_ || !p_->total || !out) { set_error("deflate encoder: nothing to fetch"); return false; }
    DFL_OK(hipMemcpyAsync(out, p_->out.p, p_->total, hipMemcpyDeviceToHost, s));
    DFL_OK(hipStreamSynchronize(s));
    return true;
}

const uint8_t* DeflateEncoder::fetch_pinned(void* stream)
{
    if (!p_ || !p_->total) { set_error("deflate encoder: nothing to fetch"); return nullptr; }
    Impl& d = *p_;
    if (d.total > d.land_cap) {
        if (d.land) (void)hipHostFree(d.land);
        d.land = nullptr; d.land_cap = 0;
        const size_t want = d.total + d.total / 4 + 4096;
        if (hipHostMalloc(&d.land, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); d.land = nullptr; set_error("deflate encoder: no page-locked memory for the streams"); return nullptr; }
        d.land_cap = want;
    }
    return fetch((uint8_t*)d.land, stream) ? (const uint8_t*)d.land : nullptr;
}

}  // namespace pf
