"""Test infrastructure for the PNG of save_png (include/pifusion.h, pf_png_encode_bgr): a plain Python encoder written from the format's
text -- the filtered stream, the block cut, tokens with history across blocks, dynamic or stored with the block's own length, segments
closed by an empty stored block, one IDAT chunk a segment, CRC-32 and Adler-32 with their combine rules -- and the images the tests
share.  What a block is (tokens, the length builder, the plan, bit order) comes from tests/deflate_model.py; zlib (the library) judges
validity and supplies the checksums of the file.  Not part of the product."""
import struct
import zlib

import numpy as np

import deflate_model as dm

BLOCK = 12288
SEG_BLOCKS = 16
SIG = b"\x89PNG\r\n\x1a\n"
POLY = 0xEDB88320
ADLER_MOD = 65521


def filtered(bgr, mask=None):
    """HxWx3 BGR (and an HxW mask) -> the bytes of F: per row the filter byte 1, then R,G,B(,A), each minus its left neighbour"""
    a = np.asarray(bgr, np.uint8)
    px = a[:, :, ::-1]
    if mask is not None:
        alpha = np.where(np.asarray(mask) != 0, 255, 0).astype(np.uint8)
        px = np.concatenate([px, alpha[:, :, None]], axis=2)
    sub = px.copy()
    sub[:, 1:] = px[:, 1:] - px[:, :-1]
    rows = np.concatenate([np.ones((a.shape[0], 1), np.uint8), sub.reshape(a.shape[0], -1)], axis=1)
    return np.ascontiguousarray(rows).reshape(-1)


def bound(rows, cols, masked):
    n = rows * (1 + cols * (4 if masked else 3))
    blocks = -(-n // BLOCK)
    return n + 5 * blocks + 17 * (-(-blocks // SEG_BLOCKS)) + 51


def put_block(w, blk, prev, final, info=None):
    """one deflate block of len(blk) <= 12 288 bytes appended to the bit writer w"""
    toks = dm.tokens(blk, prev)
    ll, nlit, rle, cl, ncl, bits = dm.plan(toks)
    stored = 3 + (-(w.at + 3)) % 8 + 32 + 8 * len(blk)
    if bits <= stored:
        if info is not None:
            info.append("dynamic")
        w.put(final, 1); w.put(2, 2)
        w.put(nlit - 257, 5); w.put(1, 5); w.put(ncl - 4, 4)
        for i in range(ncl):
            w.put(cl[dm.CL_ORDER[i]], 3)
        clc = dm.canonical(cl)
        for s, e, v in rle:
            w.huff(clc[s])
            w.put(v, e)
        rev = [int(format(c, "0%db" % l)[::-1], 2) if l else 0 for c, l in dm.canonical(ll)]
        for kind, v in toks:
            if kind == 0:
                w.put(rev[v], ll[v])
            else:
                s, e, x = dm.length_symbol(v)
                w.put(rev[s], ll[s]); w.put(x, e); w.put(0, 1)
        w.put(rev[256], ll[256])
    else:
        if info is not None:
            info.append("stored")
        w.put(final, 1); w.put(0, 2)
        w.align()
        w.put(len(blk), 16); w.put(len(blk) ^ 0xFFFF, 16)
        assert w.n == 0
        w.out += bytes(blk)


def segments(F, info=None):
    """the zlib stream of F as the list of its byte-aligned segments (the data of the IDAT chunks)"""
    F = np.asarray(F, np.uint8)
    n = F.size
    blocks = -(-n // BLOCK)
    segs = -(-blocks // SEG_BLOCKS)
    out = []
    for s in range(segs):
        w = dm.Bits()
        if s == 0:
            w.put(0x78, 8); w.put(0x01, 8)
        for b in range(s * SEG_BLOCKS, min((s + 1) * SEG_BLOCKS, blocks)):
            blk = F[b * BLOCK:min((b + 1) * BLOCK, n)]
            put_block(w, blk, int(F[b * BLOCK - 1]) if b else None, 1 if b == blocks - 1 else 0, info)
        if s < segs - 1:
            w.put(0, 3); w.align(); w.put(0, 16); w.put(0xFFFF, 16)
            out.append(bytes(w.out))
        else:
            w.align()
            out.append(bytes(w.out) + struct.pack(">I", zlib.adler32(F.tobytes())))
    return out


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode(bgr, mask=None, info=None):
    """the whole file"""
    a = np.asarray(bgr, np.uint8)
    ihdr = struct.pack(">IIBBBBB", a.shape[1], a.shape[0], 8, 6 if mask is not None else 2, 0, 0, 0)
    return SIG + chunk(b"IHDR", ihdr) + b"".join(chunk(b"IDAT", s) for s in segments(filtered(a, mask), info)) + chunk(b"IEND", b"")


def walk(png):
    """the file's chunks [(type, data)]; every CRC is checked against zlib.crc32 and nothing follows IEND"""
    assert png[:8] == SIG
    at, out = 8, []
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        kind, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert len(data) == n
        crc, = struct.unpack(">I", png[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + data), (kind, at)
        out.append((kind, data))
        at += 12 + n
    assert at == len(png) and out[-1] == (b"IEND", b"")
    return out


# ---- the checksums' combine rules, from their definitions -------------------------------------------------------------------------
def crc32_bitwise(data, crc=0):
    c = crc ^ 0xFFFFFFFF
    for x in bytes(data):
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ POLY if c & 1 else c >> 1
    return c ^ 0xFFFFFFFF


def _unreflect(v):
    return int(format(v, "032b")[::-1], 2)


def _polymod(v):
    """v(x) mod P(x), P = x^32 + the polynomial, coefficients as bits of a Python integer (bit i = x^i)"""
    p = (1 << 32) | _unreflect(POLY)
    while v.bit_length() > 32:
        v ^= p << (v.bit_length() - 33)
    return v


def crc_combine(crc_a, crc_b, len_b):
    """crc(A || B) = crc(A) * x^(8 |B|) mod P + crc(B)"""
    x, e, sh = 2, 8 * len_b, 1                            # x^e mod P by square and multiply
    while e:
        if e & 1:
            sh = _polymod(_clmul(sh, x))
        x = _polymod(_clmul(x, x))
        e >>= 1
    return _unreflect(_polymod(_clmul(_unreflect(crc_a), sh))) ^ crc_b


def _clmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return r


def adler_combine(ad_a, ad_b, len_b):
    a1, b1, a2, b2 = ad_a & 0xFFFF, ad_a >> 16, ad_b & 0xFFFF, ad_b >> 16
    return ((b1 + b2 + len_b * (a1 - 1)) % ADLER_MOD) << 16 | (a1 + a2 - 1) % ADLER_MOD


# ---- the images -------------------------------------------------------------------------------------------------------------------
def random_image(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def structured_image(rows, cols, seed):
    """smooth ramps with flat patches and a few sharp edges: runs of every length, dynamic blocks"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    a = np.stack([(x // 7 + y // 3) & 255, (x // 64 * 40 + y // 16) & 255, np.where((x // 50 + y // 40) % 2, 200, 30)], axis=2).astype(np.uint8)
    n = max(1, rows * cols // 500)
    a[rng.integers(0, rows, n), rng.integers(0, cols, n)] = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    return a


def stripes(rows, cols, period):
    x = np.arange(cols)
    line = np.where((x // period) % 2, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(line[None, :, None], (rows, cols, 3)))


def shape_with_tail(tail, bpp=3):
    """the smallest (rows, cols) above one block with N mod 12 288 == tail"""
    for n in range(BLOCK + tail, 40 * BLOCK, BLOCK):
        for rows in range(1, 64):
            if n % rows == 0 and (n // rows - 1) % bpp == 0 and n // rows > 1:
                return rows, (n // rows - 1) // bpp
    raise AssertionError("no shape")


def mask_of(kind, rows, cols):
    y, x = np.mgrid[0:rows, 0:cols]
    if kind == "zero":
        return np.zeros((rows, cols), np.uint8)
    if kind == "one":
        return np.ones((rows, cols), np.uint8)
    if kind == "seven":                                    # any non-zero byte counts as covered
        return np.where((x // 5 + y // 3) % 2, 7, 0).astype(np.uint8)
    return np.where((x + y) % 2, 255, 0).astype(np.uint8)  # "checker"


def cases():
    """[(name, bgr, mask or None)]: the smallest shapes at which each rule of the format can go wrong"""
    out = []
    rgb_shapes = [(1, 1), (1, 4095), (1, 4096), (1, 4097), (3, 4097), (17, 241), shape_with_tail(2), shape_with_tail(3)]
    for i, (r, c) in enumerate(rgb_shapes):
        out.append(("random_%dx%d" % (r, c), random_image(r, c, 100 + i), None))
        out.append(("structured_%dx%d" % (r, c), structured_image(r, c, 200 + i), None))
    r, c = shape_with_tail(3, 4)
    out.append(("rgba_tail3_%dx%d" % (r, c), structured_image(r, c, 7), mask_of("checker", r, c)))
    for kind in ("zero", "one", "checker", "seven"):
        out.append(("rgba_random_16x256_" + kind, random_image(16, 256, 300), mask_of(kind, 16, 256)))
        out.append(("rgba_structured_16x256_" + kind, structured_image(16, 256, 301), mask_of(kind, 16, 256)))
    out.append(("noise_700x600", random_image(700, 600, 5), None))
    out.append(("const0_700x600", np.zeros((700, 600, 3), np.uint8), None))
    out.append(("const255_700x600", np.full((700, 600, 3), 255, np.uint8), None))
    for p in (1, 2, 3):
        out.append(("stripes%d_40x333" % p, stripes(40, 333, p), None))
    out.append(("structured_300x1030", structured_image(300, 1030, 9), mask_of("seven", 300, 1030)))
    out.append(("random_300x1030", random_image(300, 1030, 10), None))
    return out


def padded(a, extra):
    """a copy of the 2-D or 3-D array in a buffer whose rows are `extra` bytes longer; the view has the same values"""
    a = np.asarray(a)
    flat = a.reshape(a.shape[0], -1)
    buf = np.full((a.shape[0], flat.shape[1] + extra), 0x5A, np.uint8)
    buf[:, :flat.shape[1]] = flat
    view = buf[:, :flat.shape[1]].reshape(a.shape)
    assert view.base is not None and np.array_equal(view, a)
    return view
