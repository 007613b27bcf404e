"""The PNG of save_png on the host (csrc/png_encode.hpp behind pf_png_encode_bgr) against the format's text in include/pifusion.h,
restated in tests/png_model.py: every case's file equals the model's byte for byte and is valid to three judges -- the chunk walker here
(every CRC against zlib.crc32, zlib.decompress of the joined IDAT data, the filter bytes, the zlib header, the Adler-32), Pillow, and the
library's own reader; refusals leave the guard band alone; the CRC and Adler combine functions against zlib on random splits; the size
against zlib's own Z_RLE.  No device."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest

import jpeg_encode_model as model
import png_model as pm

CASES = pm.cases()
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
_FILES = {}


def file_of(pf, name):
    """the library's file of a case, made once"""
    if name not in _FILES:
        _, bgr, mask = BY_NAME[name]
        _FILES[name] = pf.png_encode(bgr, mask)
    return _FILES[name]


@pytest.mark.parametrize("name", NAMES)
def test_file_is_the_models_and_valid_to_the_walker(pf, name):
    _, bgr, mask = BY_NAME[name]
    rows, cols = bgr.shape[:2]
    bpp = 4 if mask is not None else 3
    info = []
    want = pm.encode(bgr, mask, info)
    got = file_of(pf, name)
    assert got == want
    assert len(got) <= pm.bound(rows, cols, mask is not None)
    chunks = pm.walk(got)                                              # every CRC against zlib.crc32
    assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (len(chunks) - 2) + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", cols, rows, 8, 6 if bpp == 4 else 2, 0, 0, 0)
    idat = [d for k, d in chunks if k == b"IDAT"]
    n = rows * (1 + cols * bpp)
    blocks = -(-n // pm.BLOCK)
    assert len(idat) == -(-blocks // pm.SEG_BLOCKS) and len(info) == blocks
    assert idat[0][:2] == b"\x78\x01"
    F = zlib.decompress(b"".join(idat))
    assert len(F) == n and F == pm.filtered(bgr, mask).tobytes()
    assert set(F[::1 + cols * bpp]) == {1}                             # filter type 1 on every row
    assert idat[-1][-4:] == struct.pack(">I", zlib.adler32(F))
    for d in idat[:-1]:
        assert d[-4:] == b"\x00\x00\xff\xff"                          # every segment but the last ends with the empty stored block
    if name == "noise_700x600":
        assert info == ["stored"] * 103 and len(idat) == 7
    if name.startswith("const"):
        assert info == ["dynamic"] * blocks


@pytest.mark.parametrize("name", NAMES)
def test_pillow_and_the_librarys_reader_give_the_pixels_back(pf, name, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    Image.MAX_IMAGE_PIXELS = None
    _, bgr, mask = BY_NAME[name]
    got = file_of(pf, name)
    im = Image.open(io.BytesIO(got))
    im.load()
    a = np.asarray(im)
    if mask is None:
        assert im.mode == "RGB" and np.array_equal(a[:, :, ::-1], bgr)
    else:
        assert im.mode == "RGBA" and np.array_equal(a[:, :, 2::-1], bgr)          # the colour under alpha 0 stays
        assert np.array_equal(a[:, :, 3], np.where(mask != 0, 255, 0))
    # the library's reader drops alpha as IMREAD_COLOR does: the pixels come back, for RGBA files too
    f = str(tmp_path / "x.png")
    open(f, "wb").write(got)
    r, c = C.c_int(), C.c_int()
    assert pf.lib().pf_image_info(f.encode(), C.byref(r), C.byref(c)) and (r.value, c.value) == bgr.shape[:2]
    back = np.zeros(bgr.shape, np.uint8)
    assert pf.lib().pf_read_image(f.encode(), back.ctypes.data, bgr.shape[0], bgr.shape[1])
    assert np.array_equal(back, bgr)


def test_padded_steps_give_the_same_file(pf):
    for name in ("structured_300x1030", "random_17x241", "rgba_random_16x256_seven"):
        _, bgr, mask = BY_NAME[name]
        a = pm.padded(bgr, 13)
        m = pm.padded(mask, 5) if mask is not None else None
        assert a.strides[0] == bgr.shape[1] * 3 + 13 and (m is None or m.strides[0] == bgr.shape[1] + 5)
        assert pf.png_encode(a, m) == file_of(pf, name)


def test_refusals_leave_the_guard_band_alone(pf):
    L = pf.lib()
    a = pm.structured_image(20, 30, 1)
    good = pf.png_encode(a)
    n = C.c_size_t(77)

    def call(ptr, rows, cols, step, out, cap, mask=None, mask_step=0):
        n.value = 77
        return L.pf_png_encode_bgr(ptr, rows, cols, step, mask, mask_step, out.ctypes.data if out is not None else None, cap, C.byref(n))
    guard = np.full(len(good) + 64, 0xA5, np.uint8)
    assert call(None, 20, 30, 0, guard, guard.size) == 0 and n.value == 0 and (guard == 0xA5).all()
    for rows, cols in ((0, 30), (20, 0), (-1, 30), (20, -5)):
        assert call(a.ctypes.data, rows, cols, 0, guard, guard.size) == 0 and n.value == 0 and (guard == 0xA5).all()
    assert call(a.ctypes.data, 20, 30, 89, guard, guard.size) == 0 and n.value == 0 and (guard == 0xA5).all()          # a step smaller than a row
    m = np.ones((20, 30), np.uint8)
    assert call(a.ctypes.data, 20, 30, 0, guard, guard.size, m.ctypes.data, 29) == 0 and n.value == 0 and (guard == 0xA5).all()
    assert L.pf_png_encode_bgr(a.ctypes.data, 20, 30, 0, None, 0, guard.ctypes.data, guard.size, None) == 0 and (guard == 0xA5).all()
    # a cap too small: 0, *len = the file's length, nothing written
    for cap in (0, 1, len(good) - 1):
        assert call(a.ctypes.data, 20, 30, 0, guard, cap) == 0 and n.value == len(good) and (guard == 0xA5).all()
    # a cap that fits exactly: the file, and nothing behind it
    assert call(a.ctypes.data, 20, 30, 0, guard, len(good)) == 1 and n.value == len(good)
    assert guard[:len(good)].tobytes() == good and (guard[len(good):] == 0xA5).all()
    # out = NULL: the bound of the format's text
    assert call(a.ctypes.data, 20, 30, 0, None, 0) == 1 and n.value == pm.bound(20, 30, False)
    assert call(a.ctypes.data, 20, 30, 0, None, 0, m.ctypes.data, 0) == 1 and n.value == pm.bound(20, 30, True)
    # sizes past what the encoder indexes: a row of F of 2^31 bytes or more
    assert call(a.ctypes.data, 1, 715827883, 0, None, 0) == 0 and n.value == 0
    assert "indexes" in L.pf_last_error().decode()


def test_crc_and_adler_combine_against_zlib(pf):
    L = pf.lib()
    rng = np.random.default_rng(12)
    data = rng.integers(0, 256, 200000, dtype=np.uint8).tobytes()
    splits = [(0, 0), (0, 1), (1, 0), (1, 1), (5, 0), (0, 70000), (70000, 0), (65520, 65521), (65521, 65522), (3, 131075), (100000, 100000), (12288, 12287)]
    splits += [tuple(int(v) for v in rng.integers(0, 100000, 2)) for _ in range(20)]
    for la, lb in splits:
        A, B = data[:la], data[la:la + lb]
        ca, cb, ad_a, ad_b = zlib.crc32(A), zlib.crc32(B), zlib.adler32(A), zlib.adler32(B)
        assert L.pf_png_crc32(0, A, la) == ca and L.pf_png_crc32(ca, B, lb) == zlib.crc32(A + B)          # a piece, and a piece continued
        assert L.pf_png_crc32_combine(ca, cb, lb) == zlib.crc32(A + B)
        assert L.pf_png_adler32(B, lb) == ad_b
        assert L.pf_png_adler32_combine(ad_a, ad_b, lb) == zlib.adler32(A + B)
    # lengths past 2^32 (no data of that size is made: the rule is the model's, which the small cases pin against zlib)
    for lb in (1 << 32, (1 << 33) + 12345, 65521 << 20):
        assert L.pf_png_crc32_combine(0x12345678, 0x9ABCDEF0, lb) == pm.crc_combine(0x12345678, 0x9ABCDEF0, lb)
        assert L.pf_png_adler32_combine(0x12345678 % 65521 | (777 << 16), 0x00010001, lb) == pm.adler_combine(0x12345678 % 65521 | (777 << 16), 0x00010001, lb)


def test_the_models_combine_rules_are_zlibs():
    """A self-check of tests/png_model.py, not of the library: it passes without the feature"""
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    assert pm.crc32_bitwise(data) == zlib.crc32(data)
    for la, lb in ((0, 0), (0, 9), (9, 0), (1000, 2000), (2999, 1), (17, 100)):
        A, B = data[:la], data[la:la + lb]
        assert pm.crc_combine(zlib.crc32(A), zlib.crc32(B), lb) == zlib.crc32(A + B)
        assert pm.adler_combine(zlib.adler32(A), zlib.adler32(B), lb) == zlib.adler32(A + B)


# Size against zlib's own Z_RLE (level 6, window 15) of the same filtered stream F, summed over noise / smooth / steps images, by the method
# of test_tiff_lossless.py::test_size_against_zlib_rle.  zlib is the yardstick.  Measured here on the CPU (profiles/png_encode.md):
# MEASURED_PER_BLOCK bytes a block.  The margin is that test's, 28 bytes a block (the smallest table set there is, which a block of a
# constant image carries and zlib does not), plus 5 bytes a segment for the empty stored block that closes it.
SIZE_SHAPES = [(7, 5), (255, 257), (300, 1030), (513, 700)]
MEASURED_PER_BLOCK = -38.9          # 3 216 827 bytes against zlib's 3 238 082 over 546 blocks (noise +0.01 %, smooth -4.15 %, steps +3.17 %)
MARGIN_PER_BLOCK = 28
MARGIN_PER_SEGMENT = 5


def test_size_against_zlib_rle(pf):
    ours = theirs = blocks = segs = 0
    rows = []
    for n, (h, w) in enumerate(SIZE_SHAPES):
        for kind in ("noise", "smooth", "steps"):
            a = model.content(h, w, kind, n)
            idat = b"".join(d for k, d in pm.walk(pf.png_encode(a)) if k == b"IDAT")
            z = len(pm.dm.zrle(pm.filtered(a)))
            nb = -(-(h * (1 + 3 * w)) // pm.BLOCK)
            ours += len(idat); theirs += z; blocks += nb; segs += -(-nb // pm.SEG_BLOCKS)
            rows.append((kind, len(idat), z))
    print("png IDAT payload: %d bytes, zlib Z_RLE: %d bytes, %d blocks, %d segments, excess %.3f %%, %.1f bytes a block" % (
        ours, theirs, blocks, segs, 100.0 * (ours - theirs) / theirs, (ours - theirs) / blocks))
    for kind in ("noise", "smooth", "steps"):
        o = sum(r[1] for r in rows if r[0] == kind); z = sum(r[2] for r in rows if r[0] == kind)
        print("  %-7s ours %9d  zlib %9d  %+.3f %%" % (kind, o, z, 100.0 * (o - z) / z))
    assert ours - theirs <= blocks * (MEASURED_PER_BLOCK + MARGIN_PER_BLOCK) + segs * MARGIN_PER_SEGMENT
