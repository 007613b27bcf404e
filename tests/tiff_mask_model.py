"""Test infrastructure for the masked pyramid TIFF (include/pifusion.h, pf_tiff_write_bgr_masked): a plain numpy restatement of what the
masks hold -- the OR chain, the MSB-first bit packer with its zero fill, the two sharing tests -- and a checker of the whole file that walks
the interleaved IFD chain with tiff_model.parse.  Written from the format's description, not from the C++.  Not part of the product."""
import numpy as np

import tiff_model as tm

TILE = tm.TILE
TILE_BYTES = TILE * TILE // 8
MASK_TAGS = [254, 256, 257, 258, 259, 262, 277, 284, 322, 323, 324, 325]


def mask_halve(m):
    """M_k+1 from M_k (bool): the OR of every 2 x 2 block, a missing last row or column repeats the one before it"""
    h, w = m.shape
    p = np.pad(m, ((0, h % 2), (0, w % 2)), mode="edge")
    return p[0::2, 0::2] | p[0::2, 1::2] | p[1::2, 0::2] | p[1::2, 1::2]


def mask_chain(mask):
    """[M_0, M_1, ...] as bool arrays: covered = non-zero; down to the first image that fits one tile, as the colour chain"""
    out = [np.ascontiguousarray(np.asarray(mask) != 0)]
    while out[-1].shape[0] > TILE or out[-1].shape[1] > TILE:
        out.append(mask_halve(out[-1]))
    return out


def mask_tiles_of(m):
    """the mask's tiles, row-major, each 256 rows of 32 bytes: bit 7 of byte 0 is column 0, bits past the image are 0"""
    h, w = m.shape
    ty, tx = -(-h // TILE), -(-w // TILE)
    p = np.zeros((ty * TILE, tx * TILE), np.uint8)
    p[:h, :w] = m
    return [np.packbits(p[y * TILE:(y + 1) * TILE, x * TILE:(x + 1) * TILE], axis=1, bitorder="big").tobytes() for y in range(ty) for x in range(tx)]


ALL_ZERO = bytes(TILE_BYTES)
ALL_ONE = b"\xff" * TILE_BYTES


def kind_of(tile_bytes):
    """"zero": all 65 536 bits are 0 (stored once); "one": all are 1 (stored once); "own": stored on its own"""
    return "zero" if tile_bytes == ALL_ZERO else "one" if tile_bytes == ALL_ONE else "own"


def check_masked_file(data, image, mask, bg, encode, transform=None, big=None):
    """every property of the masked format for the file `data` of (image, mask); encode(tile) -> the expected colour stream.
    Returns {"images", "tiles", "empty", "zero", "one", "own"}."""
    isbig, ifds = tm.parse(data)
    if big is not None:
        assert isbig == big
    levels = tm.chain(image)
    masks = mask_chain(mask)
    assert [m.shape for m in masks] == [lv.shape[:2] for lv in levels]
    assert len(ifds) == 2 * len(levels)                                   # image 0, mask 0, image 1, mask 1, ...
    claimed = [(0, 16 if isbig else 8)]
    for a, b in zip(ifds, ifds[1:]):
        assert a["offset"] < b["offset"]                                  # the head holds the IFDs in chain order
    head_end = 0
    for ifd in ifds:
        assert ifd["order"] == sorted(ifd["order"]) and len(set(ifd["order"])) == len(ifd["order"])
        claimed.append((ifd["offset"], ifd["bytes"]))
        claimed += ifd["extents"]
        head_end = max([head_end, ifd["offset"] + ifd["bytes"]] + [o + n for o, n in ifd["extents"]])
    # ---- the colour half: what tiff_model.check_file demands of the unmasked file
    empty_at, full, colour_order = set(), {}, []
    n_tiles = n_empty = 0
    for k, (ifd, lv) in enumerate(zip(ifds[0::2], levels)):
        t = ifd["tags"]
        want = {254: [1 if k else 0], 256: [lv.shape[1]], 257: [lv.shape[0]], 258: [8, 8, 8], 259: [7], 262: [6], 277: [3], 284: [1], 322: [TILE], 323: [TILE], 530: [2, 2]}
        for tag, v in want.items():
            assert t[tag][1] == v, (k, tag, t[tag])
        assert 347 not in t
        if k == 0 and transform is not None:
            assert t[34264][0] == 12 and t[34264][1] == [float(v) for v in np.asarray(transform, np.float64).reshape(16)]
            assert t[34735][1] == [1, 1, 0, 2, 1024, 0, 1, 32767, 1025, 0, 1, 1]
        else:
            assert 34264 not in t and 34735 not in t
        assert sorted(t) == sorted(list(want) + [324, 325] + ([34264, 34735] if k == 0 and transform is not None else []))
        tl = tm.tiles_of(lv)
        st = tm.tile_streams(data, ifd)
        assert len(st) == len(tl)
        for tile, (off, n) in zip(tl, st):
            assert off % 2 == 0 and n > 0 and off + n <= len(data)
            n_tiles += 1
            if tm.is_empty(tile, bg):
                n_empty += 1
                empty_at.add((off, n))
            else:
                assert (off, n) not in full
                full[(off, n)] = 1
                colour_order.append(off)
            assert data[off:off + n] == encode(tile), (k, off)
    assert len(empty_at) <= 1 and not (empty_at & set(full))
    assert colour_order == sorted(colour_order)                           # image by image, row-major
    # ---- the masks
    zero_at, one_at, own, own_order = set(), set(), {}, []
    for k, (ifd, m) in enumerate(zip(ifds[1::2], masks)):
        t = ifd["tags"]
        assert ifd["order"] == MASK_TAGS, (k, ifd["order"])               # no FillOrder (266), nothing else
        tl = mask_tiles_of(m)
        want = {254: [5 if k else 4], 256: [m.shape[1]], 257: [m.shape[0]], 258: [1], 259: [1], 262: [4], 277: [1], 284: [1], 322: [TILE], 323: [TILE],
                325: [TILE_BYTES] * len(tl)}
        for tag, v in want.items():
            assert t[tag][1] == v, (k, tag, t[tag])
        assert t[254][0] == 4 and t[258][0] == 3 and t[324][0] == (16 if isbig else 4) and t[325][0] == 4
        offs = t[324][1]
        assert len(offs) == len(tl)
        for i, (tile, off) in enumerate(zip(tl, offs)):
            assert off % 2 == 0 and off + TILE_BYTES <= len(data)
            assert data[off:off + TILE_BYTES] == tile, ("mask tile", k, i)
            kd = kind_of(tile)
            if kd == "zero":
                zero_at.add(off)
            elif kd == "one":
                one_at.add(off)
            else:
                assert off not in own, ("an unshared mask tile is stored twice", k, i)
                own[off] = 1
                own_order.append(off)
    assert len(zero_at) <= 1 and len(one_at) <= 1                          # shared tiles are stored once
    assert not (zero_at & one_at) and not ((zero_at | one_at) & set(own))
    assert own_order == sorted(own_order)                                  # image by image, row-major
    # ---- placement: head | shared empty stream | shared all-zero tile | shared all-one tile | colour streams | the other mask tiles
    order = [("head", 0, head_end)]
    order += [("empty", o, n) for o, n in empty_at]
    order += [("zero", o, TILE_BYTES) for o in zero_at] + [("one", o, TILE_BYTES) for o in one_at]
    order += [("stream", o, n) for o, n in sorted(full)] + [("mask", o, TILE_BYTES) for o in own_order]
    for (na, a, n), (nb, b, _) in zip(order, order[1:]):
        assert a + n <= b and b - (a + n) <= 1, ("placement", na, a, n, nb, b)          # back to back, but for the byte that makes an offset even
    assert 0 <= len(data) - (order[-1][1] + order[-1][2]) <= 1
    claimed += sorted(full) + sorted(empty_at) + [(o, TILE_BYTES) for o in sorted(zero_at | one_at | set(own))]
    claimed.sort()
    for (a, n), (b, _) in zip(claimed, claimed[1:]):
        assert a + n <= b, ("overlap", a, n, b)
    return {"images": len(levels), "tiles": n_tiles, "empty": n_empty,
            "zero": sum(kind_of(t) == "zero" for m in masks for t in mask_tiles_of(m)), "one": sum(kind_of(t) == "one" for m in masks for t in mask_tiles_of(m)), "own": len(own)}
