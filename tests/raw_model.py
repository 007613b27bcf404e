"""numpy model of the raw-frame formats (DESIGN.md "Raw frames"), written from the specification's text, not from csrc/raw_convert.hpp:
the yardstick of pf_raw_to_bgr, pf_raw_to_bgr_device and the raw feeds.

YUV 4:2:0 (NV12, NV21, I420), all integer:
    CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527
    u = U - 128, v = V - 128                 one U, V per 2 x 2 block, no interpolation
    ruv = 2^19 + CVR v,  guv = 2^19 + CVG v + CUG u,  buv = 2^19 + CUB u,  y = max(0, Y - 16) CY
    B, G, R = sat8((y + buv) >> 20), sat8((y + guv) >> 20), sat8((y + ruv) >> 20)          (arithmetic shift)
Grey: B = G = R = the byte.
Bayer, bilinear, formats named by the first two pixels of row 0.  Interior pixel: on a red / blue site its own colour is the byte,
green = (N + S + W + E + 2) >> 2, the opposite colour = (NW + NE + SW + SE + 2) >> 2; on a green site green is the byte, the colour of its
row neighbours = (W + E + 1) >> 1, of its column neighbours = (N + S + 1) >> 1.  The one-pixel frame: the interior pixel at
(clamp(y, 1, rows - 2), clamp(x, 1, cols - 2)).

Planes are 2-D uint8 arrays with any row stride (a view into a padded buffer is fine)."""
import numpy as np

GREY, NV12, NV21, I420 = 1, 2, 3, 4
BAYER_RGGB, BAYER_BGGR, BAYER_GRBG, BAYER_GBRG = 8, 9, 10, 11
YUV = (NV12, NV21, I420)
BAYER = (BAYER_RGGB, BAYER_BGGR, BAYER_GRBG, BAYER_GBRG)
FORMATS = (GREY,) + YUV + BAYER
NAMES = {GREY: "grey", NV12: "nv12", NV21: "nv21", I420: "i420", BAYER_RGGB: "rggb", BAYER_BGGR: "bggr", BAYER_GRBG: "grbg", BAYER_GBRG: "gbrg"}

CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527

# the colour of the four sites of a 2 x 2 cell, row-major, as letters
_CELL = {BAYER_RGGB: "RGGB", BAYER_BGGR: "BGGR", BAYER_GRBG: "GRBG", BAYER_GBRG: "GBRG"}
_CHANNEL = {"B": 0, "G": 1, "R": 2}


def yuv_to_bgr(Y, U, V):
    """element-wise: arrays of equal shape (any integer type) -> uint8 array of shape + (3,)"""
    y = np.maximum(np.asarray(Y, np.int64) - 16, 0) * CY
    u = np.asarray(U, np.int64) - 128
    v = np.asarray(V, np.int64) - 128
    half = 1 << 19
    b = (y + half + CUB * u) >> 20
    g = (y + half + CVG * v + CUG * u) >> 20
    r = (y + half + CVR * v) >> 20
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def _yuv420(format, planes, rows, cols):
    Y = np.asarray(planes[0])[:rows, :cols]
    if format == I420:
        U = np.asarray(planes[1])[:rows // 2, :cols // 2]
        V = np.asarray(planes[2])[:rows // 2, :cols // 2]
    else:
        UV = np.asarray(planes[1])[:rows // 2, :cols]
        first, second = UV[:, 0::2], UV[:, 1::2]
        U, V = (first, second) if format == NV12 else (second, first)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    return yuv_to_bgr(Y, up(U), up(V))


def _bayer(format, plane, rows, cols):
    p = np.asarray(plane)[:rows, :cols].astype(np.int32)
    # the interior, rows 1 .. rows - 2 and columns 1 .. cols - 2, from shifted views
    c = p[1:-1, 1:-1]
    n, s, w, e = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    nw, ne, sw, se = p[:-2, :-2], p[:-2, 2:], p[2:, :-2], p[2:, 2:]
    cross = (n + s + w + e + 2) >> 2
    diag = (nw + ne + sw + se + 2) >> 2
    horiz = (w + e + 1) >> 1
    vert = (n + s + 1) >> 1
    yy, xx = np.mgrid[1:rows - 1, 1:cols - 1]
    cell = _CELL[format]
    out = np.zeros((rows - 2, cols - 2, 3), np.int32)
    for py in (0, 1):
        for px in (0, 1):
            m = ((yy & 1) == py) & ((xx & 1) == px)
            letter = cell[2 * py + px]
            if letter == "G":
                row_letter = cell[2 * py + (1 - px)]            # its row neighbours
                col_letter = cell[2 * (1 - py) + px]            # its column neighbours
                out[..., 1][m] = c[m]
                out[..., _CHANNEL[row_letter]][m] = horiz[m]
                out[..., _CHANNEL[col_letter]][m] = vert[m]
            else:
                other = "B" if letter == "R" else "R"
                out[..., _CHANNEL[letter]][m] = c[m]
                out[..., 1][m] = cross[m]
                out[..., _CHANNEL[other]][m] = diag[m]
    iy = np.clip(np.arange(rows), 1, rows - 2) - 1
    ix = np.clip(np.arange(cols), 1, cols - 2) - 1
    return out[iy][:, ix].astype(np.uint8)


def to_bgr(format, planes, rows, cols):
    """rows x cols x 3 uint8 BGR of a raw frame; planes: a sequence of 2-D uint8 arrays (NV12 / NV21: Y, UV; I420: Y, U, V; else one)"""
    if format == GREY:
        g = np.asarray(planes[0])[:rows, :cols]
        return np.repeat(g[:, :, None], 3, axis=2).astype(np.uint8)
    if format in YUV:
        assert rows % 2 == 0 and cols % 2 == 0
        return _yuv420(format, planes, rows, cols)
    assert format in BAYER and rows >= 3 and cols >= 3
    return _bayer(format, planes[0], rows, cols)


def n_planes(format):
    return 3 if format == I420 else 2 if format in (NV12, NV21) else 1


def plane_shapes(format, rows, cols):
    """(rows, bytes per row) of every plane of a frame"""
    if format == I420:
        return [(rows, cols), (rows // 2, cols // 2), (rows // 2, cols // 2)]
    if format in (NV12, NV21):
        return [(rows, cols), (rows // 2, cols)]
    return [(rows, cols)]


def valid_size(format, rows, cols):
    if format in YUV:
        return rows >= 2 and cols >= 2 and rows % 2 == 0 and cols % 2 == 0
    if format in BAYER:
        return rows >= 3 and cols >= 3
    return rows >= 1 and cols >= 1


def random_planes(format, rows, cols, rng, pad=(0, 0, 0), fill=0xA5):
    """the planes of a random frame as views into separate buffers whose rows are pad[k] bytes longer than the row, padding = fill.
    Returns (views, buffers): buffers[k] is the 2-D array views[k] is cut from."""
    views, bufs = [], []
    for k, (r, c) in enumerate(plane_shapes(format, rows, cols)):
        buf = np.full((r, c + pad[k]), fill, np.uint8)
        buf[:, :c] = rng.integers(0, 256, (r, c), dtype=np.uint8)
        bufs.append(buf)
        views.append(buf[:, :c])
    return views, bufs


def pack(format, planes):
    """the usual packed file layout of a frame: the planes' rows back to back (NV12: rows * 3 / 2 x cols)"""
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])
