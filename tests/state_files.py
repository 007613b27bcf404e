"""Map state files written by hand (the format of pi-slam-fusion_amd/csrc/state_file.hpp, restated): a good one and hostile variants,
for test_state_file.py (host parser, pf_state_info) and test_gpu_merge.py (a map must refuse them untouched)."""
import struct

import numpy as np

MAGIC = b"PIFUMAP\n"
HEADER_BYTES, HEAD_BYTES = 256, 72
TYPE_SINGLE, TYPE_MULTI, T8UC4, T16SC3, T32FC3 = 1, 3, 24, 19, 21


def slot_bytes(map_type, pyramid_type, bands):
    if map_type == TYPE_SINGLE:
        return 256 * 256 * 4
    es = 4 if pyramid_type == T32FC3 else 2
    pad = lambda n: (n + 255) // 256 * 256
    px = [(256 >> i) ** 2 for i in range(bands + 1)]
    return sum(pad(n * 3 * es) for n in px) + sum(pad(n * 4) for n in px)


DEFAULT = dict(magic=MAGIC, version=1, header_bytes=HEADER_BYTES, map_type=TYPE_MULTI, pyramid_type=T16SC3, band_number=0, weight_type=0,
               slot_bytes=None, n_tiles=None, plane=[0, 0, 0, 0, 0, 0, 1], cam=[640, 480, 500, 500, 320, 240],
               min0=[-10.0, -20.0, -100.0], min=[-61.2, -20.0, -100.0], max=[92.4, 82.4, 100.0], ele_size=51.2, length_pixel=0.2,
               w=3, h=2, off_x=-1, off_y=0)


def header(**over):
    """the 256 header bytes; slot_bytes / n_tiles None: what the other fields imply (n_tiles: given by the caller of state_file)"""
    f = dict(DEFAULT); f.update(over)
    if f["slot_bytes"] is None:
        f["slot_bytes"] = slot_bytes(f["map_type"], f["pyramid_type"], f["band_number"])
    b = struct.pack("<8sII4iQQ", f["magic"], f["version"], f["header_bytes"], f["map_type"], f["pyramid_type"], f["band_number"], f["weight_type"],
                    f["slot_bytes"], f["n_tiles"])
    b += struct.pack("<24d", *(list(f["plane"]) + list(f["cam"]) + list(f["min0"]) + list(f["min"]) + list(f["max"]) + [f["ele_size"], f["length_pixel"]]))
    b += struct.pack("<4i", f["w"], f["h"], f["off_x"], f["off_y"])
    assert len(b) == HEADER_BYTES
    return b


def record(ix, iy, nbytes, seed=0, wlb=None, image=None):
    """one tile record; image: the slot image (nbytes of uint8, e.g. pyramid_inject.pack's), None: random bytes of `seed`"""
    w = np.full(16, -1.0, np.float32) if wlb is None else np.asarray(wlb, np.float32)
    if image is None:
        body = np.random.RandomState(seed).randint(0, 256, nbytes).astype(np.uint8).tobytes()
    else:
        body = np.ascontiguousarray(image, np.uint8).tobytes()
        assert len(body) == nbytes
    return struct.pack("<2i", ix, iy) + w.tobytes() + body


def with_tile_count(head, n):
    """a header (the first 256 bytes of a real map's file) with n_tiles = n: the header of a file of n records"""
    assert len(head) == HEADER_BYTES and head[:8] == MAGIC
    return head[:40] + struct.pack("<Q", n) + head[48:]


def grid_of(head):
    """(w, h, off_x, off_y) of a header: the tile coordinates its records may carry"""
    return struct.unpack("<4i", head[HEADER_BYTES - 16:HEADER_BYTES])


def state_file(tiles=((-1, 0), (1, 1)), wlbs=None, **over):
    """bytes of a file holding `tiles` (given in file order) with random slot images"""
    over.setdefault("n_tiles", len(tiles))
    h = header(**over)
    sb = slot_bytes(*(over.get(k, DEFAULT[k]) for k in ("map_type", "pyramid_type", "band_number")))
    return h + b"".join(record(ix, iy, sb, seed=k, wlb=None if wlbs is None else wlbs[k]) for k, (ix, iy) in enumerate(tiles))


def hostile_files(**over):
    """{name: bytes}: every one of them a file load_state / pf_state_info must refuse; over: the options of the good file they are made from"""
    good = state_file(**over)
    sb = slot_bytes(*(over.get(k, DEFAULT[k]) for k in ("map_type", "pyramid_type", "band_number")))
    rec = HEAD_BYTES + sb
    out = {"empty": b"", "half_header": good[:100], "header_only": good[:HEADER_BYTES], "first_head": good[:HEADER_BYTES + HEAD_BYTES],
           "first_record": good[:HEADER_BYTES + rec], "second_head": good[:HEADER_BYTES + rec + HEAD_BYTES], "one_byte_short": good[:-1],
           "one_byte_long": good + b"\0"}
    v = lambda **kw: state_file(**dict(over, **kw))
    out["bad_magic"] = b"PIFUMAQ\n" + good[8:]
    out["bad_version"] = v(version=2)
    out["bad_header_bytes"] = v(header_bytes=128)
    out["wrong_slot_bytes"] = v(slot_bytes=sb - 256)
    out["slot_bytes_zero"] = v(slot_bytes=0)
    out["tiles_2_60"] = v(n_tiles=1 << 60)
    out["tiles_wrap"] = v(n_tiles=(1 << 64) // rec + 2)          # n * record wraps around 2^64
    out["duplicate_tile"] = v(tiles=((1, 1), (1, 1)))
    out["unsorted_tiles"] = v(tiles=((1, 1), (-1, 0)))
    out["tile_outside_grid"] = v(tiles=((-1, 0), (2, 1)))
    out["nan_ele_size"] = v(ele_size=float("nan"))
    out["inf_length_pixel"] = v(length_pixel=float("inf"))
    out["nan_min"] = v(min=[float("nan"), -20.0, -100.0])
    out["negative_ele_size"] = v(ele_size=-51.2)
    out["no_such_pyramid_type"] = v(pyramid_type=7, slot_bytes=sb)
    out["no_such_bands"] = v(band_number=9, slot_bytes=sb)
    out["zero_grid"] = v(w=0)
    return out
