// deflate_rle.hpp -- the lossless tile codec behind save_tiff_lossless(): a 256 x 256 BGR tile as one complete zlib stream of its
// predicted bytes (TIFF Compression 8 with Predictor 2).  The format is written down in include/pifusion.h (pf_deflate_tile_bgr);
// this header is its one definition: the token rule, the length builder, the block plan (tables, header bits, cost) and the
// framing are functions compiled for host and device, the scalar encoder below and the kernels of deflate_encode.hip call the same
// ones.
//
// Header-only.  Users: image_io.cpp (pf_deflate_tile_bgr, pf_deflate_code_lengths, the host writer through tiff_pyramid.hpp),
// deflate_encode.hip (the GPU encoder), tests/cpp/san_deflate.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define PF_DFL_HD __host__ __device__ inline
#else
#define PF_DFL_HD inline
#endif

namespace pf {
namespace dfl {

constexpr int kTile = 256;
constexpr int kRowBytes = kTile * 3;                      // a row of predicted bytes
constexpr int kBlockRows = 16;
constexpr int kBlockBytes = kBlockRows * kRowBytes;       // 12 288: what one deflate block covers
constexpr int kBlocks = kTile / kBlockRows;               // 16 blocks a tile
constexpr int kTileBytes = kTile * kRowBytes;             // N = 196 608
constexpr int kLitLen = 286;                              // literal / length alphabet
constexpr int kClen = 19;                                 // code-length alphabet
constexpr int kMaxSyms = 288;                             // most symbols the length builder takes
constexpr uint32_t kAdlerMod = 65521;
// no stream is longer: all blocks stored, each 5 bytes of header, plus the zlib header and the Adler-32
constexpr size_t kStreamBound = (size_t)kTileBytes + 5 * kBlocks + 6;
// bits of a stored block that begins at bit `at` of the stream: 3 header bits, the padding to a byte, LEN and NLEN, the bytes
PF_DFL_HD uint32_t stored_bits(uint64_t at) { return 3u + (uint32_t)((8 - ((at + 3) & 7)) & 7) + 32u + 8u * (uint32_t)kBlockBytes; }

// the header of a dynamic block: 17 bits, 19 x 3 bits, at most 288 code lengths of at most 7 + 7 bits
constexpr int kHdrWords = 132;

// ---- tokens ----------------------------------------------------------------------------------------------------------------
// Position i of a block lies in the maximal run [s, e) of equal bytes inside the block; `lean`: the run begins the block, the block
// is not the tile's first and the byte before it has the run's value.  Returns what begins at i: 0 nothing (a match covers it),
// 1 a literal, 3..258 a match of that length at distance 1.
PF_DFL_HD int token_at(int i, int s, int e, bool lean)
{
    const int m0 = s + (lean ? 0 : 1);                    // the first byte that can lie in a match
    if (i < m0) return 1;
    const int R = e - m0, j = i - m0, full = (R / 258) * 258;
    if (j < full) return j % 258 == 0 ? 258 : 0;
    const int rest = R - full, k = j - full;
    if (rest >= 3) return k == 0 ? rest : 0;
    return 1;
}
// RFC 1951 3.2.5: the length code of a match, its extra bits and their value
PF_DFL_HD void length_symbol(int len, int& sym, int& ebits, int& eval)
{
    if (len == 258) { sym = 285; ebits = 0; eval = 0; return; }
    const int l = len - 3;
    if (l < 8) { sym = 257 + l; ebits = 0; eval = 0; return; }
    int n = 3; while ((l >> (n + 1)) != 0) n++;            // floor(log2(l))
    const int e = n - 2, base = 1 << n;
    sym = 261 + 4 * e + ((l - base) >> e); ebits = e; eval = (l - base) & ((1 << e) - 1);
}
PF_DFL_HD int length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }

// ---- the length builder -------------------------------------------------------------------------------------------------------
// Work space of code_lengths and plan_block: plain data, in LDS on the device
struct Work {
    uint16_t sym[kMaxSyms], tmp[kMaxSyms];               // the used symbols, sorted
    uint64_t wt[kMaxSyms];                                // weights of the inner nodes, in the order they are made
    uint16_t par_leaf[kMaxSyms], par_node[kMaxSyms], depth[kMaxSyms];
    uint32_t radix[256];
    uint32_t count[16];                                   // codes per length
    uint32_t clfreq[kClen];
    uint8_t  cllen[kClen];
    uint16_t clcode[kClen];
    uint8_t  rsym[kMaxSyms + 2], rext[kMaxSyms + 2];      // the run-length coded code lengths: symbol, value of its extra bits
};

// Code lengths of a prefix code for freq[0..n), none longer than max_len (2 <= n <= 288, max_len <= 15, 2^max_len >= n; false otherwise):
//   a symbol with count 0 gets length 0; one used symbol gets length 1 and so does symbol 0 (symbol 1 if it is symbol 0 itself);
//   else the used symbols are sorted by (count, index) ascending, a Huffman tree is built with two queues (the leaves in that
//   order, the inner nodes in the order they are made; of two equal weights the leaf is taken first), the leaves' depths are
//   counted, depths past max_len count as max_len, and while the Kraft sum exceeds 1 one code of length max_len is dropped and the
//   deepest length below it that has a code trades one code for two of the next length (miniz's repair); the lengths are then dealt
//   out in increasing order from the end of the sorted list, the most frequent symbol first.
PF_DFL_HD bool code_lengths(const uint32_t* freq, int n, int max_len, uint8_t* out, Work& w)
{
    if (n < 2 || n > kMaxSyms || max_len < 1 || max_len > 15 || (1 << max_len) < n) return false;
    int m = 0; uint32_t top = 0;
    for (int i = 0; i < n; i++) { out[i] = 0; if (freq[i]) { w.sym[m++] = (uint16_t)i; if (freq[i] > top) top = freq[i]; } }
    if (m == 0) return true;
    if (m == 1) { out[w.sym[0]] = 1; out[w.sym[0] == 0 ? 1 : 0] = 1; return true; }          // (n == 1 cannot hold two codes)
    // stable LSD radix sort by count, a byte a pass: ties keep the index order
    for (int shift = 0; shift < 32 && (top >> shift) != 0; shift += 8) {
        for (int i = 0; i < 256; i++) w.radix[i] = 0;
        for (int i = 0; i < m; i++) w.radix[(freq[w.sym[i]] >> shift) & 255]++;
        uint32_t at = 0;
        for (int i = 0; i < 256; i++) { const uint32_t c = w.radix[i]; w.radix[i] = at; at += c; }
        for (int i = 0; i < m; i++) w.tmp[w.radix[(freq[w.sym[i]] >> shift) & 255]++] = w.sym[i];
        for (int i = 0; i < m; i++) w.sym[i] = w.tmp[i];
    }
    // two queues
    int leaf = 0, head = 0;
    for (int k = 0; k < m - 1; k++) {
        uint64_t sum = 0;
        for (int pick = 0; pick < 2; pick++) {
            if (leaf < m && (head >= k || (uint64_t)freq[w.sym[leaf]] <= w.wt[head])) { sum += freq[w.sym[leaf]]; w.par_leaf[leaf++] = (uint16_t)k; }
            else { sum += w.wt[head]; w.par_node[head++] = (uint16_t)k; }
        }
        w.wt[k] = sum;
    }
    w.depth[m - 2] = 0;
    for (int k = m - 3; k >= 0; k--) w.depth[k] = (uint16_t)(w.depth[w.par_node[k]] + 1);
    for (int l = 0; l < 16; l++) w.count[l] = 0;
    for (int i = 0; i < m; i++) { const int d = w.depth[w.par_leaf[i]] + 1; w.count[d > max_len ? max_len : d]++; }
    uint64_t total = 0;
    for (int l = 1; l <= max_len; l++) total += (uint64_t)w.count[l] << (max_len - l);
    while (total > (1ull << max_len)) {
        w.count[max_len]--;
        for (int l = max_len - 1; l >= 1; l--) if (w.count[l]) { w.count[l]--; w.count[l + 1] += 2; break; }
        total--;
    }
    int j = m;
    for (int l = 1; l <= max_len; l++) for (uint32_t c = w.count[l]; c > 0; c--) out[w.sym[--j]] = (uint8_t)l;
    return true;
}

// RFC 1951 3.2.2: canonical codes of the lengths, each stored with its bits reversed (deflate writes a code's first bit first,
// into the low end of the byte)
PF_DFL_HD void canonical_codes(const uint8_t* len, int n, uint16_t* code)
{
    uint32_t next[17]; uint32_t cnt[17];
    for (int l = 0; l <= 16; l++) cnt[l] = 0;
    for (int i = 0; i < n; i++) cnt[len[i]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    for (int l = 1; l <= 16; l++) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
    for (int i = 0; i < n; i++) {
        const int l = len[i];
        uint32_t v = l ? next[l]++ : 0, r = 0;
        for (int b = 0; b < l; b++) { r = (r << 1) | (v & 1); v >>= 1; }
        code[i] = (uint16_t)r;
    }
}

// ---- the plan of one dynamic block ----------------------------------------------------------------------------------------------
// What a block's histogram decides: the literal / length code lengths, the header (BFINAL, BTYPE = 2, HLIT, HDIST = 1, HCLEN, the
// code-length code, the run-length coded lengths) as bits, and the bits of the whole block.  Plain data.
struct Plan {
    uint8_t  len[kMaxSyms];
    uint32_t hdr[kHdrWords];
    uint32_t hdr_bits;
    uint32_t dyn_bits;             // header + tokens + end-of-block
};
struct BitPut {                    // appends to p[] low bit first; the words were zero
    uint32_t* p; uint32_t at;
    PF_DFL_HD void put(uint32_t v, int n)
    {
        if (!n) return;
        const uint32_t w = at >> 5, sh = at & 31;
        p[w] |= v << sh;
        if (sh + (uint32_t)n > 32) p[w + 1] |= v >> (32 - sh);
        at += (uint32_t)n;
    }
};
// the order the code-length code's own lengths are sent in
PF_DFL_HD int clen_order(int i)
{
    const uint8_t o[kClen] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    return o[i];
}

// hist[0..286): how often each literal / length symbol occurs in the block, end-of-block (256) counted once.
// The code lengths sent are len[0..nlit) followed by the distance code's {1, 1}, nlit = max(257, last used symbol + 1), as one
// sequence, run-length coded greedily: a run of r zeros: 18 (up to 138) while r >= 11, then 17 (3..10) if r >= 3, then single
// zeros; a run of r equal lengths v > 0: v itself, then 16 (up to 6) while the rest is >= 3, then v for each that remains.
PF_DFL_HD void plan_block(const uint32_t* hist, bool final_block, Plan& p, Work& w)
{
    (void)code_lengths(hist, kLitLen, 15, p.len, w);
    p.len[286] = p.len[287] = 0;
    int nlit = kLitLen;
    while (nlit > 257 && p.len[nlit - 1] == 0) nlit--;
    const int nseq = nlit + 2;
    auto at = [&](int i) -> int { return i < nlit ? p.len[i] : 1; };
    for (int i = 0; i < kClen; i++) w.clfreq[i] = 0;
    int nr = 0;
    for (int i = 0; i < nseq;) {
        const int v = at(i);
        int r = 1; while (i + r < nseq && at(i + r) == v) r++;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int c = r > 138 ? 138 : r; w.rsym[nr] = 18; w.rext[nr++] = (uint8_t)(c - 11); r -= c; }
            if (r >= 3) { w.rsym[nr] = 17; w.rext[nr++] = (uint8_t)(r - 3); r = 0; }
            for (; r > 0; r--) { w.rsym[nr] = 0; w.rext[nr++] = 0; }
        } else {
            w.rsym[nr] = (uint8_t)v; w.rext[nr++] = 0; r--;
            while (r >= 3) { const int c = r > 6 ? 6 : r; w.rsym[nr] = 16; w.rext[nr++] = (uint8_t)(c - 3); r -= c; }
            for (; r > 0; r--) { w.rsym[nr] = (uint8_t)v; w.rext[nr++] = 0; }
        }
    }
    for (int i = 0; i < nr; i++) w.clfreq[w.rsym[i]]++;
    (void)code_lengths(w.clfreq, kClen, 7, w.cllen, w);
    canonical_codes(w.cllen, kClen, w.clcode);
    int ncl = kClen;
    while (ncl > 4 && w.cllen[clen_order(ncl - 1)] == 0) ncl--;
    for (int i = 0; i < kHdrWords; i++) p.hdr[i] = 0;
    BitPut b{ p.hdr, 0 };
    b.put(final_block ? 1u : 0u, 1); b.put(2, 2);
    b.put((uint32_t)(nlit - 257), 5); b.put(1, 5); b.put((uint32_t)(ncl - 4), 4);
    for (int i = 0; i < ncl; i++) b.put(w.cllen[clen_order(i)], 3);
    for (int i = 0; i < nr; i++) {
        const int s = w.rsym[i];
        b.put(w.clcode[s], w.cllen[s]);
        if (s == 16) b.put(w.rext[i], 2); else if (s == 17) b.put(w.rext[i], 3); else if (s == 18) b.put(w.rext[i], 7);
    }
    p.hdr_bits = b.at;
    uint32_t bits = b.at;
    for (int s = 0; s < kLitLen; s++) if (hist[s]) bits += hist[s] * (uint32_t)(p.len[s] + (s > 256 ? length_extra_bits(s) + 1 : 0));
    p.dyn_bits = bits;
}

// Adler-32 of a block from its plain sums: S = sum x_k, T = sum (n - k) x_k over its n bytes, both mod 65521
PF_DFL_HD void adler_join(uint32_t& a, uint32_t& b, uint32_t S, uint32_t T, uint32_t n)
{
    b = (uint32_t)(((uint64_t)b + (uint64_t)n * a + T) % kAdlerMod);
    a = (a + S) % kAdlerMod;
}

// ---- the scalar encoder -------------------------------------------------------------------------------------------------------
// the predicted bytes of a tile of BGR pixels, rows of `step` bytes: RGB order, every sample minus the one before it in its row
inline void predict_tile(const uint8_t* bgr, size_t step, uint8_t* P)
{
    for (int y = 0; y < kTile; y++) {
        const uint8_t* s = bgr + (size_t)y * step;
        uint8_t* d = P + (size_t)y * kRowBytes;
        for (int x = 0; x < kTile; x++)
            for (int c = 0; c < 3; c++) d[3 * x + c] = (uint8_t)(s[3 * x + 2 - c] - (x ? s[3 * x - 1 - c] : 0));
    }
}

// The whole stream of a tile, appended to `out`
inline void encode_tile(const uint8_t* bgr, size_t step, std::vector<uint8_t>& out)
{
    std::vector<uint8_t> P((size_t)kTileBytes);
    predict_tile(bgr, step, P.data());
    std::vector<uint16_t> tok((size_t)kBlockBytes);
    std::vector<uint32_t> words((kStreamBound + 8) / 4 + 2, 0);
    BitPut bp{ words.data(), 0 };
    bp.put(0x78, 8); bp.put(0x01, 8);
    Work w; Plan plan; uint16_t code[kMaxSyms];
    uint32_t a = 1, b = 0;
    for (int blk = 0; blk < kBlocks; blk++) {
        const uint8_t* B = P.data() + (size_t)blk * kBlockBytes;
        uint32_t hist[kLitLen] = { 0 };
        uint64_t S = 0, T = 0;
        for (int s = 0; s < kBlockBytes;) {
            int e = s + 1; while (e < kBlockBytes && B[e] == B[s]) e++;
            const bool lean = s == 0 && blk > 0 && B[-1] == B[0];
            for (int i = s; i < e; i++) {
                const int t = token_at(i, s, e, lean);
                tok[i] = (uint16_t)t;
                if (t == 1) hist[B[i]]++;
                else if (t) { int sym, eb, ev; length_symbol(t, sym, eb, ev); hist[sym]++; }
            }
            s = e;
        }
        for (int k = 0; k < kBlockBytes; k++) { S += B[k]; T += (uint64_t)(kBlockBytes - k) * B[k]; }
        adler_join(a, b, (uint32_t)(S % kAdlerMod), (uint32_t)(T % kAdlerMod), kBlockBytes);
        hist[256] = 1;
        const bool final_block = blk == kBlocks - 1;
        plan_block(hist, final_block, plan, w);
        if (plan.dyn_bits <= stored_bits(bp.at)) {
            canonical_codes(plan.len, kLitLen, code);
            for (uint32_t i = 0; i < plan.hdr_bits; i += 32) bp.put(plan.hdr[i >> 5], (int)(plan.hdr_bits - i < 32 ? plan.hdr_bits - i : 32));
            for (int i = 0; i < kBlockBytes; i++) {
                const int t = tok[i];
                if (t == 1) bp.put(code[B[i]], plan.len[B[i]]);
                else if (t) {
                    int sym, eb, ev; length_symbol(t, sym, eb, ev);
                    bp.put(code[sym], plan.len[sym]); bp.put((uint32_t)ev, eb); bp.put(0, 1);
                }
            }
            bp.put(code[256], plan.len[256]);
        } else {
            bp.put(final_block ? 1u : 0u, 1); bp.put(0, 2);
            bp.put(0, (int)((8 - (bp.at & 7)) & 7));
            bp.put((uint32_t)kBlockBytes, 16); bp.put((uint32_t)kBlockBytes ^ 0xFFFFu, 16);
            for (int i = 0; i < kBlockBytes; i++) bp.put(B[i], 8);
        }
    }
    bp.put(0, (int)((8 - (bp.at & 7)) & 7));
    const uint32_t adler = (b << 16) | a;
    for (int i = 3; i >= 0; i--) bp.put((adler >> (8 * i)) & 255, 8);
    const size_t n = bp.at / 8, at0 = out.size();
    out.resize(at0 + n);
    for (size_t i = 0; i < n; i++) out[at0 + i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
}

}  // namespace dfl

// The GPU encoder (deflate_encode.hip), with JpegEncoder's batch interface.  One per consumer; not thread-safe.  encode_windows()
// queues the passes on `stream` (a hipStream_t) for n tiles of 256 x 256 BGR8 pixels, rows of `step` bytes, tile i beginning
// byte_offsets[i] bytes behind dev_base, and returns with the n streams laid back to back in a device buffer of its own:
// offsets[0..n] say where each begins and the last ends.  fetch() copies them to host memory and returns when they are there.
class DeflateEncoder {
public:
    DeflateEncoder() {}
    ~DeflateEncoder();
    void release();
    DeflateEncoder(const DeflateEncoder&) = delete;
    DeflateEncoder& operator=(const DeflateEncoder&) = delete;
    bool encode_windows(const void* dev_base, int n, const long long* byte_offsets, size_t step, size_t* offsets, void* stream);
    bool fetch(uint8_t* out, void* stream);
    const uint8_t* fetch_pinned(void* stream);
private:
    struct Impl;
    Impl* p_ = nullptr;
};

}  // namespace pf
