// jpeg_encode.hpp -- the baseline JPEG encoder behind save("x.jpg"): the file cv::imwrite of OpenCV 2.4.9 writes for an 8-bit
// BGR image (MultiBandMap2DCPU.cpp:841), i.e. libjpeg after jpeg_set_defaults, JCS_RGB input, jpeg_set_quality(q, TRUE):
// JFIF 1.01, the Annex K quantisation tables scaled for the quality, 4:2:0, the Annex K Huffman tables, one interleaved scan,
// libjpeg's integer colour conversion, h2v2 down-sampling and ISLOW forward DCT.  Byte for byte.
//
// Header-only.  Three users: image_io.cpp (pf_jpeg_encode_bgr, pf_write_image: the scalar encoder below, no device), the GPU
// encoder (jpeg_encode.hip: the tables and the marker segments built here are the ones its kernels are handed, and its kernels
// call the same colour / DCT / quantisation functions), and the host tests (tests/cpp/san_jpeg_encode.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define PF_JENC_HD __host__ __device__ inline
#else
#define PF_JENC_HD inline
#endif

namespace pf {
namespace jenc {

constexpr int kHeaderBytes = 623;        // SOI, APP0, 2 x DQT, SOF0, 4 x DHT, SOS: the same for every image
constexpr int kTrailerBytes = 2;         // EOI
constexpr int kMaxDim = 65535;           // SOF0 carries 16-bit sizes
// Most bits one block can take: DC code (<= 11 bits) + 11 value bits, 63 x (AC code <= 16 bits + 10 value bits)
constexpr size_t kMaxBlockBits = 22 + 63 * 26;

// zig-zag position -> natural (row-major) position, and back
static const uint8_t kZigzag[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
// ITU-T T.81 Annex K.1: luminance, chrominance (natural order)
static const uint8_t kStdQuant[2][64] = {
    { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
    { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 } };
// Annex K.3: code counts per length 1..16 and the symbols in code order; [0] luminance, [1] chrominance
static const uint8_t kDcBits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
static const uint8_t kDcVals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
static const uint8_t kAcBits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125 }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119 } };
static const uint8_t kAcVals[2][162] = {
    { 0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
      0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
      0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
      0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa },
    { 0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
      0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
      0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa } };

// What the encoder -- scalar or kernels -- needs for one quality.  Huffman entries are (code << 5) | length, 0 for a symbol
// without a code.  Plain data: the GPU encoder uploads the struct as it is.
struct Tables {
    uint16_t div[2][64];       // the divisor 8 * q of the coefficient at zig-zag position k ([0] luminance, [1] chrominance)
    uint8_t  nat2zz[64];       // natural position -> zig-zag position
    uint8_t  q[2][64];         // the DQT payload: q in zig-zag order
    uint32_t dc[2][12];
    uint32_t ac[2][256];
};

// jpeg_set_quality's clamp (0 -> 1) and jpeg_quality_scaling
inline int clamp_quality(int quality) { return quality < 1 ? 1 : quality > 100 ? 100 : quality; }

inline void build_tables(int quality, Tables& t)
{
    const int q = clamp_quality(quality), scale = q < 50 ? 5000 / q : 200 - 2 * q;
    std::memset(&t, 0, sizeof t);
    for (int k = 0; k < 64; k++) t.nat2zz[kZigzag[k]] = (uint8_t)k;
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < 64; k++) {
            long v = ((long)kStdQuant[c][kZigzag[k]] * scale + 50) / 100;          // jpeg_add_quant_table, force_baseline
            v = v < 1 ? 1 : v > 255 ? 255 : v;
            t.q[c][k] = (uint8_t)v; t.div[c][k] = (uint16_t)(8 * v);
        }
    for (int c = 0; c < 2; c++) {
        uint32_t code = 0; int k = 0;
        for (int len = 1; len <= 16; len++) { for (int i = 0; i < kDcBits[c][len - 1]; i++) t.dc[c][kDcVals[k++]] = (code++ << 5) | (uint32_t)len; code <<= 1; }
        code = 0; k = 0;
        for (int len = 1; len <= 16; len++) { for (int i = 0; i < kAcBits[c][len - 1]; i++) t.ac[c][kAcVals[c][k++]] = (code++ << 5) | (uint32_t)len; code <<= 1; }
    }
}

// The kHeaderBytes bytes in front of the entropy-coded data
inline void write_header(const Tables& t, int rows, int cols, uint8_t* out)
{
    uint8_t* p = out;
    auto seg = [&](int marker, int payload) { *p++ = 0xFF; *p++ = (uint8_t)marker; *p++ = (uint8_t)((payload + 2) >> 8); *p++ = (uint8_t)(payload + 2); };
    *p++ = 0xFF; *p++ = 0xD8;
    seg(0xE0, 14);
    static const uint8_t jfif[14] = { 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 };
    std::memcpy(p, jfif, 14); p += 14;
    for (int c = 0; c < 2; c++) { seg(0xDB, 65); *p++ = (uint8_t)c; std::memcpy(p, t.q[c], 64); p += 64; }
    seg(0xC0, 15);
    *p++ = 8; *p++ = (uint8_t)(rows >> 8); *p++ = (uint8_t)rows; *p++ = (uint8_t)(cols >> 8); *p++ = (uint8_t)cols; *p++ = 3;
    static const uint8_t comps[9] = { 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1 };
    std::memcpy(p, comps, 9); p += 9;
    for (int c = 0; c < 2; c++) {
        seg(0xC4, 1 + 16 + 12); *p++ = (uint8_t)c; std::memcpy(p, kDcBits[c], 16); p += 16; std::memcpy(p, kDcVals, 12); p += 12;
        seg(0xC4, 1 + 16 + 162); *p++ = (uint8_t)(0x10 | c); std::memcpy(p, kAcBits[c], 16); p += 16; std::memcpy(p, kAcVals[c], 162); p += 162;
    }
    seg(0xDA, 10);
    static const uint8_t sos[10] = { 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0 };
    std::memcpy(p, sos, 10); p += 10;
}

struct Geometry {
    int rows, cols;
    int mcux, mcuy;            // MCUs (16 x 16 pixels) across and down
    int ywb, yhb;              // luminance blocks that hold real samples; the others of an edge MCU are dummy blocks
    int ch;                    // rows of the down-sampled chroma planes that come from the image: the ones below repeat the last
    PF_JENC_HD long blocks() const { return (long)mcux * mcuy * 6; }
};
PF_JENC_HD Geometry geometry(int rows, int cols)
{
    Geometry g;
    g.rows = rows; g.cols = cols;
    g.mcux = (cols + 15) / 16; g.mcuy = (rows + 15) / 16;
    g.ywb = (cols + 7) / 8; g.yhb = (rows + 7) / 8;
    g.ch = (rows + 1) / 2;
    return g;
}
// a bound of the whole stream for any content: every byte of the entropy-coded data stuffed
inline size_t stream_bound(int rows, int cols)
{ return (size_t)kHeaderBytes + kTrailerBytes + 2 * (((size_t)geometry(rows, cols).blocks() * kMaxBlockBits + 7) / 8 + 1); }

// ---- the arithmetic, shared with the kernels ---------------------------------------------------------------------------------
// jccolor.c: FIX(x) = (int)(x * 65536 + 0.5)
PF_JENC_HD int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
PF_JENC_HD int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
PF_JENC_HD int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// jfdctint.c, one 8-point pass in place over d[0], d[stride], ...: the row pass (first) scales up by PASS1_BITS = 2, the column
// pass takes that back out and leaves the factor 8 of the whole transform
PF_JENC_HD int jdescale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
PF_JENC_HD void fdct_pass(int* d, int stride, bool first)
{
    const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride], d7 = d[7 * stride];
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int n = first ? 11 : 15;
    if (first) { d[0] = (t10 + t11) * 4; d[4 * stride] = (t10 - t11) * 4; }
    else { d[0] = jdescale(t10 + t11, 2); d[4 * stride] = jdescale(t10 - t11, 2); }
    int z1 = (t12 + t13) * 4433;
    d[2 * stride] = jdescale(z1 + t13 * 6270, n);
    d[6 * stride] = jdescale(z1 - t12 * 15137, n);
    z1 = t4 + t7; int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7 * stride] = jdescale(t4 + z1 + z3, n);
    d[5 * stride] = jdescale(t5 + z2 + z4, n);
    d[3 * stride] = jdescale(t6 + z2 + z3, n);
    d[stride] = jdescale(t7 + z1 + z4, n);
}
// jcdctmgr.c: round half away from zero, in integers
PF_JENC_HD int quantise(int v, int divisor) { return v < 0 ? -((-v + (divisor >> 1)) / divisor) : (v + (divisor >> 1)) / divisor; }
// bits of the magnitude category (jchuff.c's nbits)
PF_JENC_HD int magnitude_bits(int v) { unsigned a = (unsigned)(v < 0 ? -v : v); int n = 0; while (a) { n++; a >>= 1; } return n; }
// Which block of the MCU before it a dummy luminance block copies its DC from is decided by which blocks are real:
// block k = 2 * v + h of MCU (my, mx) is real when its row and column of blocks hold image samples (jccoefct.c)
PF_JENC_HD bool luma_block_real(const Geometry& g, int my, int mx, int k) { return 2 * my + (k >> 1) < g.yhb && 2 * mx + (k & 1) < g.ywb; }

// ---- the scalar encoder -------------------------------------------------------------------------------------------------------
class BitSink {
public:
    explicit BitSink(std::vector<uint8_t>& out) : out_(out) {}
    void put(uint32_t code, int len)
    {
        acc_ = (acc_ << len) | (code & ((1u << len) - 1)); n_ += len;
        while (n_ >= 8) { const uint8_t b = (uint8_t)(acc_ >> (n_ - 8)); out_.push_back(b); if (b == 0xFF) out_.push_back(0); n_ -= 8; }
    }
    void flush() { if (n_) put((1u << (8 - n_)) - 1, 8 - n_); }
private:
    std::vector<uint8_t>& out_;
    uint64_t acc_ = 0; int n_ = 0;
};

// one block of quantised coefficients in zig-zag order (jchuff.c encode_one_block)
inline void encode_block(BitSink& bs, const int16_t* zz, int pred, const uint32_t* dc, const uint32_t* ac)
{
    int d = zz[0] - pred, s = magnitude_bits(d);
    bs.put(dc[s] >> 5, (int)(dc[s] & 31));
    if (s) bs.put((uint32_t)(d < 0 ? d - 1 : d), s);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int v = zz[k];
        if (!v) { run++; continue; }
        for (; run > 15; run -= 16) bs.put(ac[0xF0] >> 5, (int)(ac[0xF0] & 31));
        s = magnitude_bits(v);
        const uint32_t e = ac[(run << 4) | s];
        bs.put(e >> 5, (int)(e & 31));
        bs.put((uint32_t)(v < 0 ? v - 1 : v), s);
        run = 0;
    }
    if (run) bs.put(ac[0] >> 5, (int)(ac[0] & 31));
}

// 8 x 8 samples (0..255, row-major) -> quantised coefficients in zig-zag order
inline void transform_block(const uint8_t* s, int stride, const Tables& t, int c, int16_t* zz)
{
    int w[64];
    for (int y = 0; y < 8; y++) for (int x = 0; x < 8; x++) w[8 * y + x] = (int)s[(size_t)y * stride + x] - 128;
    for (int y = 0; y < 8; y++) fdct_pass(w + 8 * y, 1, true);
    for (int x = 0; x < 8; x++) fdct_pass(w + x, 8, false);
    for (int k = 0; k < 64; k++) zz[k] = (int16_t)quantise(w[kZigzag[k]], t.div[c][k]);
}

// The whole stream for a BGR8 image of `step` bytes per row, appended to `out`.  One MCU row at a time: its 16 luminance rows
// and 8 rows of each down-sampled chroma plane, edges filled as libjpeg fills them (see Geometry).
inline void encode_bgr(const uint8_t* bgr, int rows, int cols, size_t step, int quality, std::vector<uint8_t>& out)
{
    Tables t; build_tables(quality, t);
    const Geometry g = geometry(rows, cols);
    const size_t at = out.size();
    out.resize(at + kHeaderBytes);
    write_header(t, rows, cols, out.data() + at);
    const int W = g.mcux * 16, CW = g.mcux * 8;
    std::vector<uint8_t> Y((size_t)16 * W), C[2] = { std::vector<uint8_t>((size_t)8 * CW), std::vector<uint8_t>((size_t)8 * CW) };
    std::vector<uint8_t> cbf((size_t)2 * W), crf((size_t)2 * W);
    BitSink bs(out);
    int pred[3] = { 0, 0, 0 };
    int16_t zz[64];
    for (int my = 0; my < g.mcuy; my++) {
        for (int r = 0; r < 16; r++) {                                       // luminance: rows and columns past the image repeat the last
            const int y = std::min(16 * my + r, rows - 1);
            const uint8_t* s = bgr + (size_t)y * step;
            uint8_t* d = Y.data() + (size_t)r * W;
            for (int x = 0; x < cols; x++) d[x] = (uint8_t)ycc_y(s[3 * x + 2], s[3 * x + 1], s[3 * x]);
            for (int x = cols; x < W; x++) d[x] = d[cols - 1];
        }
        for (int r = 0; r < 8; r++) {                                        // chroma: down-sampled rows past the image repeat the last down-sampled row
            const int cr = std::min(8 * my + r, g.ch - 1);
            for (int k = 0; k < 2; k++) {
                const int y = std::min(2 * cr + k, rows - 1);
                const uint8_t* s = bgr + (size_t)y * step;
                uint8_t* db = cbf.data() + (size_t)k * W; uint8_t* dr = crf.data() + (size_t)k * W;
                for (int x = 0; x < cols; x++) { db[x] = (uint8_t)ycc_cb(s[3 * x + 2], s[3 * x + 1], s[3 * x]); dr[x] = (uint8_t)ycc_cr(s[3 * x + 2], s[3 * x + 1], s[3 * x]); }
                for (int x = cols; x < W; x++) { db[x] = db[cols - 1]; dr[x] = dr[cols - 1]; }
            }
            for (int x = 0; x < CW; x++) {                                   // h2v2_downsample: bias 1, 2, 1, 2 ...
                const int bias = 1 + (x & 1);
                C[0][(size_t)r * CW + x] = (uint8_t)((cbf[2 * x] + cbf[2 * x + 1] + cbf[W + 2 * x] + cbf[W + 2 * x + 1] + bias) >> 2);
                C[1][(size_t)r * CW + x] = (uint8_t)((crf[2 * x] + crf[2 * x + 1] + crf[W + 2 * x] + crf[W + 2 * x + 1] + bias) >> 2);
            }
        }
        for (int mx = 0; mx < g.mcux; mx++) {
            for (int k = 0; k < 4; k++) {
                if (luma_block_real(g, my, mx, k)) transform_block(Y.data() + (size_t)(8 * (k >> 1)) * W + 16 * mx + 8 * (k & 1), W, t, 0, zz);
                else { const int16_t dc = (int16_t)pred[0]; std::memset(zz, 0, sizeof zz); zz[0] = dc; }      // dummy: the DC of the block coded before it
                encode_block(bs, zz, pred[0], t.dc[0], t.ac[0]);
                pred[0] = zz[0];
            }
            for (int c = 0; c < 2; c++) {
                transform_block(C[c].data() + 8 * mx, CW, t, 1, zz);
                encode_block(bs, zz, pred[1 + c], t.dc[1], t.ac[1]);
                pred[1 + c] = zz[0];
            }
        }
    }
    bs.flush();
    out.push_back(0xFF); out.push_back(0xD9);
}

}  // namespace jenc

// The GPU encoder (jpeg_encode.hip).  One per consumer (a map, or the process-wide one behind pf_jpeg_encode_device); not
// thread-safe.  encode() queues the passes on `stream` (a hipStream_t) for n images of rows x cols BGR8 pixels, `step` bytes per
// row, image i at dev_bgr + slots[i] * image_stride (slots == nullptr: i), and returns with the n complete streams laid back to
// back in a device buffer of its own: offsets[0..n] say where each begins and the last ends.  fetch() copies them to host memory
// (pinned or not) and returns when they are there.
class JpegEncoder {
public:
    JpegEncoder() {}
    ~JpegEncoder();
    void release();          // frees the device buffers (the device they live on is current)
    JpegEncoder(const JpegEncoder&) = delete;
    JpegEncoder& operator=(const JpegEncoder&) = delete;
    bool encode(const void* dev_bgr, int n, const int* slots, size_t image_stride, int rows, int cols, size_t step, int quality, size_t* offsets, void* stream);
    // the same for n windows of rows x cols pixels anywhere in one allocation: window i begins byte_offsets[i] bytes behind dev_base
    // (64 bits: a tile of a mosaic of any size; the tiles of a pyramid TIFF, overview.hip)
    bool encode_windows(const void* dev_base, int n, const long long* byte_offsets, int rows, int cols, size_t step, int quality, size_t* offsets, void* stream);
    bool fetch(uint8_t* out, void* stream);
    // the same into a page-locked buffer of the encoder's own (grow-only, valid until the next call; nullptr on failure): for a
    // caller that only passes the bytes on -- save() writes them to the file -- and would otherwise land them in pageable memory
    const uint8_t* fetch_pinned(void* stream);
private:
    bool encode_at(const void* dev_bgr, int n, const int* slots, const long long* where, size_t image_stride, int rows, int cols, size_t step, int quality, size_t* offsets, void* stream);
    struct Impl;
    Impl* p_ = nullptr;
};

}  // namespace pf
