"""Test infrastructure for the JPEG encoder (csrc/jpeg_encode.hpp, jpeg_encode.hip): the pictures the committed vectors were made from
(rebuilt from a seed with integer arithmetic alone, so only Pillow's streams are stored), and a plain numpy restatement of libjpeg's
baseline encoder at its defaults -- integer colour conversion (jccolor.c), h2v2 down-sampling with the 1, 2 bias, the ISLOW forward DCT
(jfdctint.c), integer quantisation, edge and dummy-block rules of jccoefct.c -- as a second witness that needs no Pillow.  The Huffman
tables are read out of a reference stream's DHT segments.  Not part of the product."""
import numpy as np

from jpeg_enc import BitWriter, ZIGZAG, encode_block, segment

LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# the committed cases: (rows, cols, kind, quality); kind: "noise" | "smooth" | "zero" | "white" | "steps"
CASES = [(16, 16, "noise", 95), (16, 16, "smooth", 75), (16, 16, "zero", 95), (16, 16, "white", 1), (8, 8, "noise", 100), (8, 8, "smooth", 25),
         (1, 1, "noise", 95), (1, 1, "white", 50), (37, 53, "noise", 100), (37, 53, "smooth", 95), (37, 53, "steps", 1), (17, 16, "noise", 75),
         (17, 16, "smooth", 100), (16, 17, "noise", 50), (16, 17, "steps", 95), (100, 260, "noise", 100), (100, 260, "smooth", 25),
         (100, 260, "zero", 100), (256, 256, "noise", 75), (256, 256, "smooth", 95), (256, 256, "white", 95), (256, 256, "steps", 50)]


def noise(h, w, seed):
    """h x w x 3 bytes from an integer hash of the sample's index: the same on every numpy"""
    i = np.arange(h * w * 3, dtype=np.uint64) + np.uint64(seed) * np.uint64(1000003)
    x = (i * np.uint64(2654435761)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15); x = (x * np.uint64(2246822519)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13); x = (x * np.uint64(3266489917)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return (x >> np.uint64(24)).astype(np.uint8).reshape(h, w, 3)


def content(h, w, kind, seed=0):
    """BGR picture of one content class: noise (every code length, many 0xFF bytes at quality 100), smooth, constant 0 / 255 (nothing but
    end-of-block codes), steps (flat squares with noise islands: long zero runs, ZRL)"""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return noise(h, w, seed + 1)
    if kind == "smooth":
        return np.stack([(y * 5 + x * 3 + seed) % 256, (x * 7 + seed) % 256, (y * x + 3 * seed) % 256], -1).astype(np.uint8)
    if kind == "zero":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    a = ((((x // 8 + y // 8) * 37 + seed) % 5) * 60).astype(np.uint8)[..., None].repeat(3, 2)
    n = noise(h, w, seed + 7)
    a[(n[..., 0] > 250)] = n[(n[..., 0] > 250)]
    return a


def quant_table(base, q):
    q = max(1, min(100, q)); s = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([min(255, max(1, (b * s + 50) // 100)) for b in base], np.int64)


def dht_of(stream):
    """{Tc<<4|Th: (payload bytes, {symbol: (code, length)})} of a stream's DHT segments"""
    tabs = {}; i = 2
    while True:
        m = stream[i + 1]; n = (stream[i + 2] << 8) | stream[i + 3]
        if m == 0xC4:
            p = stream[i + 4:i + 2 + n]
            while p:
                bits = list(p[1:17]); cnt = sum(bits); vals = list(p[17:17 + cnt])
                codes = {}; code = 0; k = 0
                for ln in range(1, 17):
                    for _ in range(bits[ln - 1]):
                        codes[vals[k]] = (code, ln); code += 1; k += 1
                    code <<= 1
                tabs[p[0]] = (bytes(p[:17 + cnt]), codes)
                p = p[17 + cnt:]
        if m == 0xDA:
            return tabs
        i += 2 + n


def fdct(b):
    """jfdctint.c on an 8 x 8 list of level-shifted ints: rows (PASS1_BITS = 2), then columns"""
    def D(x, n):
        return (x + (1 << (n - 1))) >> n

    def p1(d, first):
        t0 = d[0] + d[7]; t7 = d[0] - d[7]; t1 = d[1] + d[6]; t6 = d[1] - d[6]; t2 = d[2] + d[5]; t5 = d[2] - d[5]; t3 = d[3] + d[4]; t4 = d[3] - d[4]
        t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
        o = [0] * 8
        if first:
            o[0] = (t10 + t11) << 2; o[4] = (t10 - t11) << 2; n = 11
        else:
            o[0] = D(t10 + t11, 2); o[4] = D(t10 - t11, 2); n = 15
        z1 = (t12 + t13) * 4433; o[2] = D(z1 + t13 * 6270, n); o[6] = D(z1 - t12 * 15137, n)
        z1 = t4 + t7; z2 = t5 + t6; z3 = t4 + t6; z4 = t5 + t7; z5 = (z3 + z4) * 9633
        t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299
        z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196
        z3 += z5; z4 += z5
        o[7] = D(t4 + z1 + z3, n); o[5] = D(t5 + z2 + z4, n); o[3] = D(t6 + z2 + z3, n); o[1] = D(t7 + z1 + z4, n)
        return o
    rows = [p1([int(v) for v in r], True) for r in b]
    cols = [p1([rows[r][c] for r in range(8)], False) for c in range(8)]
    return np.array([[cols[c][r] for c in range(8)] for r in range(8)], np.int64)


def encode(bgr, q, tabs):
    """the whole stream for an H x W x 3 BGR array; tabs = dht_of(a reference stream)"""
    H, W, _ = bgr.shape
    b, g, r = [bgr[..., i].astype(np.int64) for i in range(3)]
    F = lambda v: int(v * 65536 + 0.5)
    half = 1 << 15; cbias = (128 << 16) + half - 1
    Y = (F(.299) * r + F(.587) * g + F(.114) * b + half) >> 16
    Cb = (-F(.16874) * r - F(.33126) * g + F(.5) * b + cbias) >> 16
    Cr = (F(.5) * r - F(.41869) * g - F(.08131) * b + cbias) >> 16
    mx = -(-W // 16); my = -(-H // 16)
    ywb = -(-W // 8); yhb = -(-H // 8); cw = -(-W // 2); ch = -(-H // 2); cwb = -(-cw // 8); chb = -(-ch // 8)
    Yp = np.pad(Y, ((0, yhb * 8 - H), (0, ywb * 8 - W)), mode="edge")

    def down(p):
        p = np.pad(p, ((0, H % 2), (0, cwb * 16 - W)), mode="edge")
        bias = np.tile(np.array([1, 2]), cwb * 4)[None, :]
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        return np.pad(d, ((0, chb * 8 - d.shape[0]), (0, 0)), mode="edge")          # AFTER down-sampling
    planes = [(Yp, ywb, yhb, 2, quant_table(LUM, q)), (down(Cb), cwb, chb, 1, quant_table(CHR, q)), (down(Cr), cwb, chb, 1, quant_table(CHR, q))]

    def coef(p, by, bx, qt):
        c = fdct(p[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] - 128).reshape(64)
        d = qt * 8
        return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)
    out = bytearray(b"\xff\xd8") + segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for n, base in enumerate((LUM, CHR)):
        out += segment(0xDB, bytes([n]) + bytes(int(quant_table(base, q)[ZIGZAG[i]]) for i in range(64)))
    out += segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc in (0x00, 0x10, 0x01, 0x11):
        out += segment(0xC4, tabs[tc][0])
    out += segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    bw = BitWriter(); pred = [0, 0, 0]
    for y in range(my):
        for x in range(mx):
            for ci, (p, wb, hb, s, qt) in enumerate(planes):
                dc, ac = (tabs[0x00][1], tabs[0x10][1]) if ci == 0 else (tabs[0x01][1], tabs[0x11][1])
                last = None
                for v in range(s):
                    for h in range(s):
                        by, bx = y * s + v, x * s + h
                        if by < hb and bx < wb:
                            z = np.take(coef(p, by, bx, qt), ZIGZAG)
                        else:                                                     # dummy block: the DC of the block coded before it, no AC
                            z = np.zeros(64, np.int64); z[0] = last
                        last = int(z[0]); pred[ci] = encode_block(bw, z, pred[ci], dc, ac)
    bw.flush()
    return bytes(out + bw.out + b"\xff\xd9")
