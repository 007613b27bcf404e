"""Raw frames on the host: pf_raw_to_bgr (csrc/raw_convert.hpp) against the numpy model of tests/raw_model.py, byte for byte, and
against values worked out by hand from the specification (DESIGN.md "Raw frames").  No GPU."""
import ctypes as C

import numpy as np
import pytest

import raw_frames as rf
import raw_model as rm


def last_error(pf):
    return pf.lib().pf_last_error().decode()


def one_pixel_block(pf, fmt, Y, U, V):
    """the 2 x 2 frame whose four pixels are (Y, U, V), through the library"""
    y = np.full((2, 2), Y, np.uint8)
    if fmt == rm.I420:
        planes = (y, np.array([[U]], np.uint8), np.array([[V]], np.uint8))
    else:
        planes = (y, np.array([[U, V] if fmt == rm.NV12 else [V, U]], np.uint8))
    out = pf.raw_to_bgr(planes, fmt, 2, 2)
    assert (out == out[0, 0]).all()
    return tuple(int(v) for v in out[0, 0])


# (Y, U, V) -> (B, G, R), by hand.  H = 2^19 = 524288; a result is sat8(floor(sum / 2^20)), 2^20 = 1048576.
HAND = [
    # y = 0, u = v = 0: every sum is H, floor(0.5) = 0
    ((16, 128, 128), (0, 0, 0)),
    # y = 219 * 1220542 = 267298698; + H = 267822986 = 255.4 * 2^20
    ((235, 128, 128), (255, 255, 255)),
    # y = 0 (Y below 16 is clamped), u = v = -128:  B: H - 2116026 * 128 = -270327040 < 0 -> 0
    # G: H + 852492 * 128 + 409993 * 128 = 162122368 = 154.6 * 2^20 -> 154          R: H - 1673527 * 128 = -213687168 < 0 -> 0
    ((0, 0, 0), (0, 154, 0)),
    # y = 239 * 1220542 = 291709538, u = v = 127:  B: y + H + 268735302 = 560969128 = 534.9 * 2^20 -> 255
    # G: y + H - 108266484 - 52069111 = 131898231 = 125.8 * 2^20 -> 125            R: y + H + 212537929 = 504771755 = 481.4 * 2^20 -> 255
    ((255, 255, 255), (255, 125, 255)),
    # "red": y = 65 * 1220542 = 79335230, u = -38, v = 112:  B: y + H - 80408988 = -549470: floor(-0.52) = -1 -> 0
    # G: y + H - 95479104 + 15579734 = -39852: floor(-0.04) = -1 -> 0 (the arithmetic shift)        R: y + H + 187435024 = 267294542 = 254.9 * 2^20 -> 254
    ((81, 90, 240), (0, 0, 254)),
    # "green": y = 129 * 1220542 = 157449918, u = -74, v = -94:  B: y + H - 156585924 = 1388282 = 1.3 * 2^20 -> 1
    # G: y + H + 80134248 + 30339482 = 268447936 = 256.01 * 2^20 -> 255 (saturated)               R: y + H - 157311538 = 662668 = 0.6 * 2^20 -> 0
    ((145, 54, 34), (1, 255, 0)),
]


@pytest.mark.parametrize("fmt", rm.YUV, ids=lambda f: rm.NAMES[f])
def test_yuv_hand_values(pf, fmt):
    for (Y, U, V), bgr in HAND:
        assert one_pixel_block(pf, fmt, Y, U, V) == bgr, (Y, U, V)
        assert tuple(int(v) for v in rm.yuv_to_bgr(Y, U, V)) == bgr, (Y, U, V)


def test_every_yuv_triple(pf):
    """all 256^3 (Y, U, V) once each in one 4096 x 4096 NV12 frame: block b = 64 (256 U + V) + j of the 2048 x 2048 blocks carries (U, V) and
    the four lumas 4 j .. 4 j + 3"""
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    uv, j = b >> 6, b & 63
    U, V = (uv >> 8).astype(np.uint8), (uv & 255).astype(np.uint8)
    Y = np.empty((4096, 4096), np.uint8)
    Y[0::2, 0::2] = 4 * j; Y[0::2, 1::2] = 4 * j + 1; Y[1::2, 0::2] = 4 * j + 2; Y[1::2, 1::2] = 4 * j + 3
    UV = np.empty((2048, 4096), np.uint8)
    UV[:, 0::2] = U; UV[:, 1::2] = V
    # every triple occurs exactly once
    key = (Y.astype(np.int64) << 16) | (np.repeat(np.repeat(U, 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(V, 2, 0), 2, 1)
    assert np.array_equal(np.sort(key.reshape(-1)), np.arange(1 << 24))
    del key
    got = pf.raw_to_bgr((Y, UV), rm.NV12, 4096, 4096)
    for r0 in range(0, 4096, 512):            # the model in strips: int64 intermediates
        want = rm.to_bgr(rm.NV12, (Y[r0:r0 + 512], UV[r0 // 2:r0 // 2 + 256]), 512, 4096)
        assert np.array_equal(got[r0:r0 + 512], want), r0


def test_nv12_nv21_i420_agree(pf):
    rng = np.random.default_rng(3)
    rows, cols = 10, 18
    Y = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    U = rng.integers(0, 256, (rows // 2, cols // 2), dtype=np.uint8)
    V = rng.integers(0, 256, (rows // 2, cols // 2), dtype=np.uint8)
    uv = np.empty((rows // 2, cols), np.uint8); uv[:, 0::2] = U; uv[:, 1::2] = V
    vu = np.empty((rows // 2, cols), np.uint8); vu[:, 0::2] = V; vu[:, 1::2] = U
    a = pf.raw_to_bgr((Y, uv), rm.NV12, rows, cols)
    assert np.array_equal(a, pf.raw_to_bgr((Y, vu), rm.NV21, rows, cols))
    assert np.array_equal(a, pf.raw_to_bgr((Y, U, V), rm.I420, rows, cols))
    assert np.array_equal(a, rm.to_bgr(rm.I420, (Y, U, V), rows, cols))
    assert not np.array_equal(a, pf.raw_to_bgr((Y, V, U), rm.I420, rows, cols))            # YV12 is I420 with the pointers swapped
    # the packed layouts of the binding: one array, rows * 3 / 2 x cols
    assert np.array_equal(a, pf.raw_to_bgr(rm.pack(rm.NV12, (Y, uv)).reshape(rows * 3 // 2, cols), rm.NV12))
    assert np.array_equal(a, pf.raw_to_bgr(rm.pack(rm.I420, (Y, U, V)), rm.I420, rows, cols))


@pytest.mark.parametrize("case", rf.cases(), ids=rf.case_id)
def test_every_format_and_size(pf, case):
    """packed planes, and planes in separate buffers with rows 3, 5 and 7 bytes longer than the row (padding 0xA5); destination packed and
    with 5 bytes between its rows, guarded"""
    fmt, rows, cols = case
    rng = np.random.default_rng(100 * fmt + rows + cols)
    for pad in ((0, 0, 0), (3, 5, 7)):
        views, bufs = rm.random_planes(fmt, rows, cols, rng, pad=pad)
        want = rm.to_bgr(fmt, views, rows, cols)
        assert want.shape == (rows, cols, 3)
        for dst_pad in (0, 5):
            assert np.array_equal(rf.convert_host(pf, fmt, views, rows, cols, dst_pad), want), (pad, dst_pad)
        assert all((b[:, b.shape[1] - p:] == rf.PAD).all() for b, p in zip(bufs, pad) if p)


def constant_mosaic(fmt, rows, cols, r, g, b):
    cell = {rm.BAYER_RGGB: (r, g, g, b), rm.BAYER_BGGR: (b, g, g, r), rm.BAYER_GRBG: (g, r, b, g), rm.BAYER_GBRG: (g, b, r, g)}[fmt]
    m = np.empty((rows, cols), np.uint8)
    m[0::2, 0::2], m[0::2, 1::2], m[1::2, 0::2], m[1::2, 1::2] = cell
    return m


@pytest.mark.parametrize("fmt", rm.BAYER, ids=lambda f: rm.NAMES[f])
@pytest.mark.parametrize("size", [(3, 3), (4, 5), (29, 37), (6, 530)])
def test_bayer_constant_planes(pf, fmt, size):
    """a mosaic constant per colour demosaics to that colour everywhere, borders included: pins the site table and the clamp rule"""
    rows, cols = size
    m = constant_mosaic(fmt, rows, cols, 200, 90, 31)
    out = pf.raw_to_bgr((m,), fmt, rows, cols)
    assert (out == np.array([31, 90, 200], np.uint8)).all()
    assert np.array_equal(rm.to_bgr(fmt, (m,), rows, cols), out)


def test_bayer_formats_are_swaps_and_shifts_of_each_other(pf):
    rng = np.random.default_rng(8)
    p = rng.integers(0, 256, (14, 19), dtype=np.uint8)
    conv = lambda a, f: pf.raw_to_bgr((np.ascontiguousarray(a),), f, a.shape[0], a.shape[1])
    rggb, bggr, grbg, gbrg = (conv(p, f) for f in rm.BAYER)
    # the same sites with red and blue exchanged
    assert np.array_equal(bggr, rggb[:, :, ::-1]) and np.array_equal(gbrg, grbg[:, :, ::-1])
    assert not np.array_equal(rggb, grbg)
    # GRBG is RGGB seen from one column further right, GBRG from one row further down: equal wherever both pixels are interior
    assert np.array_equal(conv(p[:, 1:], rm.BAYER_GRBG)[1:-1, 1:-1], rggb[1:-1, 2:-1])
    assert np.array_equal(conv(p[1:, :], rm.BAYER_GBRG)[1:-1, 1:-1], rggb[2:-1, 1:-1])
    # the one-pixel frame repeats the nearest interior pixel
    for out in (rggb, grbg):
        assert np.array_equal(out[0], out[1]) and np.array_equal(out[-1], out[-2])
        assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, -1], out[:, -2])


def test_refusals_write_nothing(pf):
    L = pf.lib()
    rng = np.random.default_rng(5)
    dst = np.full(64 * 64 * 3, rf.PAD, np.uint8)

    def refused(f, words, step=0):
        assert L.pf_raw_to_bgr(C.byref(f), dst.ctypes.data, step) == 0
        assert words in last_error(pf), last_error(pf)
        assert (dst == rf.PAD).all()
    y = rng.integers(0, 256, (8, 8), dtype=np.uint8)
    uv = rng.integers(0, 256, (4, 8), dtype=np.uint8)
    refused(rf.descriptor(pf, 0, (y,), 8, 8), "unknown raw format")
    refused(rf.descriptor(pf, 7, (y,), 8, 8), "unknown raw format")
    refused(rf.descriptor(pf, 12, (y,), 8, 8), "unknown raw format")
    for fmt, planes in ((rm.GREY, ()), (rm.NV12, (y,)), (rm.NV21, (y,)), (rm.I420, (y, uv)), (rm.BAYER_GBRG, ())):
        refused(rf.descriptor(pf, fmt, planes, 8, 8), "is missing")
    f = rf.descriptor(pf, rm.NV12, (y, uv), 8, 8); f.step[1] = 7
    refused(f, "step of plane 1")
    f = rf.descriptor(pf, rm.I420, (y, uv, uv), 8, 8); f.step[2] = 3
    refused(f, "step of plane 2")
    f = rf.descriptor(pf, rm.GREY, (y,), 8, 8); f.step[0] = 7
    refused(f, "step of plane 0")
    refused(rf.descriptor(pf, rm.GREY, (y,), 8, 8), "bgr_step", step=23)
    for fmt in rm.YUV:
        refused(rf.descriptor(pf, fmt, (y, uv, uv)[:rm.n_planes(fmt)], 7, 8), "even")
        refused(rf.descriptor(pf, fmt, (y, uv, uv)[:rm.n_planes(fmt)], 8, 5), "even")
    for fmt in rm.BAYER:
        refused(rf.descriptor(pf, fmt, (y,), 2, 8), "3 x 3")
        refused(rf.descriptor(pf, fmt, (y,), 8, 2), "3 x 3")
    refused(rf.descriptor(pf, rm.GREY, (y,), 0, 8), "at least 1")
    refused(rf.descriptor(pf, rm.GREY, (y,), 8, -1), "at least 1")
    # a plane of 2 GiB: refused on its description alone, before any byte is touched
    f = rf.descriptor(pf, rm.GREY, (y,), 2, 8); f.step[0] = 1 << 30
    refused(f, "2 GiB")
    f = rf.descriptor(pf, rm.NV12, (y, uv), 8, 8); f.step[1] = 1 << 29
    refused(f, "2 GiB")
    f = rf.descriptor(pf, rm.GREY, (y,), 8, 8)
    assert L.pf_raw_to_bgr(None, dst.ctypes.data, 0) == 0 and L.pf_raw_to_bgr(C.byref(f), None, 0) == 0
    with pytest.raises(ValueError):
        pf.raw_to_bgr((y, uv), rm.NV12, 7, 8)


def test_map_entry_points_refuse_without_a_map(pf):
    f = rf.descriptor(pf, rm.GREY, (np.zeros((4, 4), np.uint8),), 4, 4)
    pose = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
    assert pf.lib().pf_feed_raw(None, C.byref(f), pose) == 0 and pf.lib().pf_feed_raw_device(None, C.byref(f), pose) == 0
