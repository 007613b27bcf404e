"""Test infrastructure for the tiled pyramid TIFF (include/pifusion.h, pf_tiff_write_bgr): a small reader (header, IFD chain, tags, tile
offsets; classic and BigTIFF) and a plain numpy restatement of what the file holds -- the 2 x 2-mean overview chain, the tile cutter with its
edge fill, the empty test.  Written from the format's description, not from the C++.  Not part of the product."""
import struct

import numpy as np

TILE = 256
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 7: 1, 11: 4, 12: 8, 16: 8}
TYPE_FMT = {1: "B", 2: "c", 3: "H", 4: "I", 7: "B", 11: "f", 12: "d", 16: "Q"}


def parse(data):
    """-> (big, [ifd, ...]); ifd: {"offset": where it lies, "tags": {tag: (type, [values])}, "order": [tags as they lie],
    "extents": [(offset, bytes) of every out-of-line value]}"""
    assert data[:2] == b"II", "little-endian expected"
    magic = struct.unpack_from("<H", data, 2)[0]
    assert magic in (42, 43)
    big = magic == 43
    if big:
        assert struct.unpack_from("<HH", data, 4) == (8, 0)
        off = struct.unpack_from("<Q", data, 8)[0]
    else:
        off = struct.unpack_from("<I", data, 4)[0]
    osz, esz, ofmt = (8, 20, "<Q") if big else (4, 12, "<I")
    ifds = []
    while off:
        assert off % 2 == 0 and off < len(data) and len(ifds) < 64
        n = struct.unpack_from("<Q" if big else "<H", data, off)[0]
        p = off + (8 if big else 2)
        tags, order, extents = {}, [], []
        for i in range(n):
            tag, typ = struct.unpack_from("<HH", data, p + i * esz)
            cnt = struct.unpack_from(ofmt, data, p + i * esz + 4)[0]
            size = TYPE_SIZE[typ] * cnt
            at = p + i * esz + 4 + osz
            if size > osz:
                at = struct.unpack_from(ofmt, data, at)[0]
                assert at % 2 == 0 and at + size <= len(data), (tag, at)
                extents.append((at, size))
            tags[tag] = (typ, list(struct.unpack_from("<%d%s" % (cnt, TYPE_FMT[typ]), data, at)))
            order.append(tag)
        ifds.append({"offset": off, "tags": tags, "order": order, "extents": extents, "bytes": (8 if big else 2) + n * esz + osz})
        off = struct.unpack_from(ofmt, data, p + n * esz)[0]
    return big, ifds


def tile_streams(data, ifd):
    """[(offset, bytes)] of an image's tiles, row-major"""
    return list(zip(ifd["tags"][324][1], ifd["tags"][325][1]))


def halve(a):
    """image k from image k - 1: every channel (p00 + p01 + p10 + p11 + 2) >> 2, a missing last row or column repeats the one before it"""
    h, w = a.shape[:2]
    p = np.pad(a, ((0, h % 2), (0, w % 2), (0, 0)), mode="edge").astype(np.uint16)
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def chain(a):
    """[image 0, image 1, ...]: down to the first image that fits one tile"""
    out = [np.ascontiguousarray(a)]
    while out[-1].shape[0] > TILE or out[-1].shape[1] > TILE:
        out.append(halve(out[-1]))
    return out


def tiles_of(a):
    """the image's 256 x 256 tiles, row-major; past the image its last column, then its last row"""
    h, w = a.shape[:2]
    ty, tx = -(-h // TILE), -(-w // TILE)
    p = np.pad(a, ((0, ty * TILE - h), (0, tx * TILE - w), (0, 0)), mode="edge")
    return [p[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE] for y in range(ty) for x in range(tx)]


def is_empty(tile, bg):
    return bool((tile == min(255, max(0, bg))).all())


def check_file(data, image, bg, encode, transform=None, big=None):
    """every structural property of the format for the file `data` of `image`; encode(tile) -> the expected stream.  Returns
    (number of images, number of tiles, number of empty tiles)."""
    isbig, ifds = parse(data)
    if big is not None:
        assert isbig == big
    levels = chain(image)
    assert len(ifds) == len(levels)
    claimed = [(0, 16 if isbig else 8)]
    empty_at = set()
    full = {}
    n_tiles = n_empty = 0
    for k, (ifd, lv) in enumerate(zip(ifds, levels)):
        t = ifd["tags"]
        assert ifd["order"] == sorted(ifd["order"]) and len(set(ifd["order"])) == len(ifd["order"])
        want = {254: [1 if k else 0], 256: [lv.shape[1]], 257: [lv.shape[0]], 258: [8, 8, 8], 259: [7], 262: [6], 277: [3], 284: [1], 322: [TILE], 323: [TILE], 530: [2, 2]}
        for tag, v in want.items():
            assert t[tag][1] == v, (k, tag, t[tag])
        assert 347 not in t                                               # no JPEGTables
        if k == 0 and transform is not None:
            assert t[34264][0] == 12 and t[34264][1] == [float(v) for v in np.asarray(transform, np.float64).reshape(16)]
            assert t[34735][1] == [1, 1, 0, 2, 1024, 0, 1, 32767, 1025, 0, 1, 1]
        else:
            assert 34264 not in t and 34735 not in t
        claimed.append((ifd["offset"], ifd["bytes"]))
        claimed += ifd["extents"]
        tl = tiles_of(lv)
        st = tile_streams(data, ifd)
        assert len(st) == len(tl)
        for tile, (off, n) in zip(tl, st):
            assert off % 2 == 0 and n > 0 and off + n <= len(data)
            n_tiles += 1
            if is_empty(tile, bg):
                n_empty += 1
                empty_at.add((off, n))
            else:
                assert (off, n) not in full
                full[(off, n)] = 1
            assert data[off:off + n] == encode(tile), (k, off)
    assert len(empty_at) <= 1 and not (empty_at & set(full))
    claimed += sorted(full) + sorted(empty_at)
    claimed.sort()
    for (a, n), (b, _) in zip(claimed, claimed[1:]):
        assert a + n <= b, ("overlap", a, n, b)
    assert claimed[-1][0] + claimed[-1][1] <= len(data)
    if empty_at:
        stream = data[slice(*[(o, o + n) for o, n in empty_at][0])]
        assert data.count(stream) == 1                                   # stored once
    return len(ifds), n_tiles, n_empty
