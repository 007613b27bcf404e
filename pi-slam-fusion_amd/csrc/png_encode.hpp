// png_encode.hpp -- the PNG behind save_png(): the mosaic (and, masked, its coverage as alpha) as one PNG file whose zlib stream is made of
// the blocks of the lossless tile codec (deflate_rle.hpp): Sub-filtered rows, run-length tokens at distance 1, dynamic Huffman or stored
// blocks of 12 288 stream bytes, sixteen blocks a byte-aligned segment, one segment an IDAT chunk.  The format is written down in
// include/pifusion.h (pf_png_encode_bgr); this header is its one definition: the stream's bytes, the geometry and the bound, CRC-32 and
// Adler-32 with their combine functions are compiled for host and device, the scalar encoder below and the kernels of png_encode.hip
// call the same ones.
//
// Header-only.  Users: image_io.cpp (pf_png_encode_bgr, the checksum entry points, the host writer of single-band maps), png_encode.hip
// (the GPU encoder), tests/cpp/san_png.cpp.
#pragma once
#include "deflate_rle.hpp"
#include <algorithm>

namespace pf {
namespace png {

constexpr int kSegBlocks = 16;                            // deflate blocks a segment = an IDAT chunk
constexpr uint32_t kCrcPoly = 0xEDB88320u;                // CRC-32, reflected
constexpr size_t kHeadBytes = 8 + 25;                     // signature, IHDR chunk
constexpr size_t kChunkFrame = 12;                        // length, type, CRC
constexpr size_t kFixedBytes = kHeadBytes + kChunkFrame + 2 + 4;      // + IEND, the zlib header, the Adler-32

// bits of a stored block of n bytes that begins at bit `at`: dfl::stored_bits with the block's own length
PF_DFL_HD uint32_t stored_bits(uint64_t at, uint32_t n) { return 3u + (uint32_t)((8 - ((at + 3) & 7)) & 7) + 32u + 8u * n; }

// What the sizes decide.  bpp 3 (RGB) or 4 (RGBA, a mask is given)
struct Geometry {
    int bpp;
    uint64_t row_len;          // 1 + cols * bpp: the filter byte and the samples
    uint64_t N;                // bytes of the filtered stream F
    uint64_t blocks, segs;
    uint64_t bound;            // no file is longer
};
// false: sizes that are not positive, a row of F past 2^31 - 1 bytes, more than 2^31 - 1 blocks or a bound past 2^62: refused by
// both encoders before anything is written
PF_DFL_HD bool geometry(int rows, int cols, bool masked, Geometry& g)
{
    if (rows <= 0 || cols <= 0) return false;
    g.bpp = masked ? 4 : 3;
    g.row_len = 1 + (uint64_t)cols * (uint64_t)g.bpp;
    if (g.row_len > 0x7fffffffull) return false;
    g.N = (uint64_t)rows * g.row_len;
    g.blocks = (g.N + dfl::kBlockBytes - 1) / dfl::kBlockBytes;
    g.segs = (g.blocks + kSegBlocks - 1) / kSegBlocks;
    if (g.blocks > 0x7fffffffull) return false;
    // every block ends no later than storing it would: its bytes and 5 more; a segment's closing empty block (or the Adler-32) 5, its chunk 12
    g.bound = g.N + 5 * g.blocks + (5 + kChunkFrame) * g.segs + kFixedBytes;
    return g.bound < (1ull << 62);
}
PF_DFL_HD uint32_t block_len(const Geometry& g, uint64_t blk)
{
    const uint64_t left = g.N - blk * (uint64_t)dfl::kBlockBytes;
    return left < (uint64_t)dfl::kBlockBytes ? (uint32_t)left : (uint32_t)dfl::kBlockBytes;
}

// Byte q of row `row` of F: the filter type 1 (Sub), then R, G, B (, A) of every pixel minus the same channel of the pixel to its left
// (the first pixel as it is).  A = 255 where the mask byte is not 0, else 0
PF_DFL_HD uint8_t stream_byte(const uint8_t* bgr, size_t step, const uint8_t* mask, size_t mask_step, int bpp, uint64_t row, uint32_t q)
{
    if (q == 0) return 1;
    const uint32_t u = q - 1, x = bpp == 4 ? u >> 2 : u / 3u, c = u - x * (uint32_t)bpp;
    if (c == 3) {
        const uint8_t* m = mask + row * mask_step + x;
        const int a = m[0] ? 255 : 0, pa = x && m[-1] ? 255 : 0;
        return (uint8_t)(a - pa);
    }
    const uint8_t* s = bgr + row * step + 3 * (size_t)x + (2 - c);
    return (uint8_t)(s[0] - (x ? s[-3] : 0));
}

// ---- CRC-32 ---------------------------------------------------------------------------------------------------------------------
PF_DFL_HD uint32_t crc_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1) ? kCrcPoly ^ (c >> 1) : c >> 1;
    return c;
}
// the CRC of A || B from crc = the CRC of A (0 for nothing) and the n bytes of B; table: the 256 entries above
PF_DFL_HD uint32_t crc_piece(const uint32_t* table, uint32_t crc, const uint8_t* p, size_t n)
{
    uint32_t c = ~crc;
    for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
    return ~c;
}
PF_DFL_HD uint32_t crc_word(const uint32_t* table, uint32_t c, uint32_t w)          // four bytes, low byte first, on the raw register
{
    for (int k = 0; k < 4; k++) { c = table[(c ^ w) & 255] ^ (c >> 8); w >>= 8; }
    return c;
}
// a(x) * b(x) mod P, polynomials with the coefficient of x^0 in bit 31
PF_DFL_HD uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(8 n) mod P
PF_DFL_HD uint32_t crc_shift(uint64_t n)
{
    uint32_t base = 0x40000000u;                          // x^1
    for (int k = 0; k < 3; k++) base = crc_mul(base, base);          // x^8
    uint32_t p = 0x80000000u;                             // x^0
    for (; n; n >>= 1) { if (n & 1) p = crc_mul(base, p); base = crc_mul(base, base); }
    return p;
}
// the CRC of A || B from the CRCs of A and of B and the length of B
PF_DFL_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_mul(crc_shift(len_b), crc_a) ^ crc_b; }

// ---- Adler-32 -------------------------------------------------------------------------------------------------------------------
// the Adler-32 of A || B from those of A and of B and the length of B
PF_DFL_HD uint32_t adler_combine(uint32_t ad_a, uint32_t ad_b, uint64_t len_b)
{
    const uint64_t M = dfl::kAdlerMod;
    const uint64_t a1 = ad_a & 0xffff, b1 = ad_a >> 16, a2 = ad_b & 0xffff, b2 = ad_b >> 16;
    const uint64_t a = (a1 + a2 + M - 1) % M;
    const uint64_t b = (b1 + b2 + (len_b % M) * ((a1 + M - 1) % M)) % M;
    return (uint32_t)((b << 16) | a);
}

inline void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
inline const uint32_t* crc_table()
{
    static const struct T { uint32_t v[256]; T() { for (uint32_t i = 0; i < 256; i++) v[i] = crc_table_entry(i); } } t;
    return t.v;
}
inline uint32_t crc32(uint32_t crc, const uint8_t* p, size_t n) { return crc_piece(crc_table(), crc, p, n); }
// the Adler-32 of n bytes, block by block from the sums S and T as the kernels make them
inline uint32_t adler32(const uint8_t* p, size_t n)
{
    uint32_t a = 1, b = 0;
    for (size_t at = 0; at < n; at += dfl::kBlockBytes) {
        const size_t m = n - at < (size_t)dfl::kBlockBytes ? n - at : (size_t)dfl::kBlockBytes;
        uint64_t S = 0, T = 0;
        for (size_t k = 0; k < m; k++) { S += p[at + k]; T += (uint64_t)(m - k) * p[at + k]; }
        dfl::adler_join(a, b, (uint32_t)(S % dfl::kAdlerMod), (uint32_t)(T % dfl::kAdlerMod), (uint32_t)m);
    }
    return (b << 16) | a;
}

// ---- the scalar encoder -----------------------------------------------------------------------------------------------------------
// The whole file of rows x cols BGR pixels, rows of `step` bytes, appended to `out`; mask (may be null: an RGB file): a byte per pixel,
// rows of `mask_step` bytes.  false: geometry() refuses the sizes (nothing is appended)
inline bool encode(const uint8_t* bgr, int rows, int cols, size_t step, const uint8_t* mask, size_t mask_step, std::vector<uint8_t>& out)
{
    using namespace dfl;
    Geometry g;
    if (!geometry(rows, cols, mask != nullptr, g)) return false;
    std::vector<uint8_t> F((size_t)g.N);
    for (int y = 0; y < rows; y++)
        for (uint32_t q = 0; q < (uint32_t)g.row_len; q++) F[(size_t)y * (size_t)g.row_len + q] = stream_byte(bgr, step, mask, mask_step, g.bpp, (uint64_t)y, q);
    const size_t at0 = out.size();
    out.reserve(at0 + (size_t)g.bound);
    static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n' };
    out.insert(out.end(), sig, sig + 8);
    auto chunk = [&](const char* type, const uint8_t* data, size_t n) {
        uint8_t h[8]; put_be32(h, (uint32_t)n); std::memcpy(h + 4, type, 4);
        out.insert(out.end(), h, h + 8);
        if (n) out.insert(out.end(), data, data + n);
        uint8_t t[4]; put_be32(t, crc32(crc32(0, h + 4, 4), data, n));
        out.insert(out.end(), t, t + 4);
    };
    uint8_t ihdr[13];
    put_be32(ihdr, (uint32_t)cols); put_be32(ihdr + 4, (uint32_t)rows);
    ihdr[8] = 8; ihdr[9] = (uint8_t)(g.bpp == 4 ? 6 : 2); ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    chunk("IHDR", ihdr, 13);
    std::vector<uint16_t> tok((size_t)kBlockBytes);
    const size_t seg_words = ((size_t)kSegBlocks * (kBlockBytes + 5) + 16) / 4 + 2;
    std::vector<uint32_t> words(seg_words);
    std::vector<uint8_t> data;
    Work w; Plan plan; uint16_t code[kMaxSyms];
    uint32_t a = 1, b = 0;
    for (uint64_t seg = 0; seg < g.segs; seg++) {
        std::fill(words.begin(), words.end(), 0u);
        BitPut bp{ words.data(), 0 };
        if (seg == 0) { bp.put(0x78, 8); bp.put(0x01, 8); }
        const uint64_t b0 = seg * kSegBlocks, b1 = b0 + kSegBlocks < g.blocks ? b0 + kSegBlocks : g.blocks;
        for (uint64_t blk = b0; blk < b1; blk++) {
            const uint8_t* B = F.data() + (size_t)blk * kBlockBytes;
            const int n = (int)block_len(g, blk);
            uint32_t hist[kLitLen] = { 0 };
            uint64_t S = 0, T = 0;
            for (int s = 0; s < n;) {
                int e = s + 1; while (e < n && B[e] == B[s]) e++;
                const bool lean = s == 0 && blk > 0 && B[-1] == B[0];
                for (int i = s; i < e; i++) {
                    const int t = token_at(i, s, e, lean);
                    tok[i] = (uint16_t)t;
                    if (t == 1) hist[B[i]]++;
                    else if (t) { int sym, eb, ev; length_symbol(t, sym, eb, ev); hist[sym]++; }
                }
                s = e;
            }
            for (int k = 0; k < n; k++) { S += B[k]; T += (uint64_t)(n - k) * B[k]; }
            adler_join(a, b, (uint32_t)(S % kAdlerMod), (uint32_t)(T % kAdlerMod), (uint32_t)n);
            hist[256] = 1;
            const bool final_block = blk == g.blocks - 1;
            plan_block(hist, final_block, plan, w);
            if (plan.dyn_bits <= stored_bits(bp.at, (uint32_t)n)) {
                canonical_codes(plan.len, kLitLen, code);
                for (uint32_t i = 0; i < plan.hdr_bits; i += 32) bp.put(plan.hdr[i >> 5], (int)(plan.hdr_bits - i < 32 ? plan.hdr_bits - i : 32));
                for (int i = 0; i < n; i++) {
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
                bp.put((uint32_t)n, 16); bp.put((uint32_t)n ^ 0xFFFFu, 16);
                for (int i = 0; i < n; i++) bp.put(B[i], 8);
            }
        }
        if (seg + 1 < g.segs) {          // an empty stored block brings the segment to a byte boundary
            bp.put(0, 3); bp.put(0, (int)((8 - (bp.at & 7)) & 7));
            bp.put(0, 16); bp.put(0xFFFFu, 16);
        } else {
            bp.put(0, (int)((8 - (bp.at & 7)) & 7));
            const uint32_t adler = (b << 16) | a;
            for (int i = 3; i >= 0; i--) bp.put((adler >> (8 * i)) & 255, 8);
        }
        const size_t nbytes = bp.at / 8;
        data.resize(nbytes);
        for (size_t i = 0; i < nbytes; i++) data[i] = (uint8_t)(words[i >> 2] >> (8 * (i & 3)));
        chunk("IDAT", data.data(), nbytes);
    }
    chunk("IEND", nullptr, 0);
    return true;
}

}  // namespace png

// The GPU encoder (png_encode.hip), with JpegEncoder's interface.  One per consumer; not thread-safe.  encode() queues the passes on
// `stream` (a hipStream_t) for rows x cols BGR8 pixels in device memory, rows of `step` bytes, and dev_mask (may be null) beside them,
// and returns with the complete file in a device buffer of its own, *len its length; fetch() copies it to host memory and returns when
// it is there, fetch_pinned() into the encoder's page-locked landing buffer.
class PngEncoder {
public:
    PngEncoder() {}
    ~PngEncoder();
    void release();
    PngEncoder(const PngEncoder&) = delete;
    PngEncoder& operator=(const PngEncoder&) = delete;
    bool encode(const void* dev_bgr, int rows, int cols, size_t step, const void* dev_mask, size_t mask_step, size_t* len, void* stream);
    bool fetch(uint8_t* out, void* stream);
    const uint8_t* fetch_pinned(void* stream);
private:
    struct Impl;
    Impl* p_ = nullptr;
};

}  // namespace pf
