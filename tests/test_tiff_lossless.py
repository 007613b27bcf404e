"""The lossless tile codec (csrc/deflate_rle.hpp behind pf_deflate_tile_bgr, pf_deflate_code_lengths) and the lossless pyramid TIFF of the
host writer (pf_tiff_write_bgr_lossless) against the format's text in include/pifusion.h, restated in tests/deflate_model.py: every hostile
tile's stream equals the model's, zlib inflates it to the predicted bytes, no stream passes the stored bound; the length builder against
the model and Kraft; files parsed with tests/tiff_model.py, every tile inflated, the masks those of the JPEG file, Pillow (libtiff) as the
independent reader; the size against zlib's own Z_RLE.  No device."""
import zlib

import numpy as np
import pytest

import deflate_model as dm
import jpeg_encode_model as model
import tiff_mask_model as mm
import tiff_model as tm
from test_tiff import XF
from test_tiff_mask import make_mask

SHAPES = [(1, 1), (7, 5), (255, 257), (256, 256), (300, 1030), (513, 700)]
TILES = dm.hostile_tiles()


@pytest.mark.parametrize("name", sorted(TILES))
def test_tile_stream_is_the_models_and_inflates_to_the_predicted_bytes(pf, name):
    tile = TILES[name]
    info = []
    want = dm.encode_tile(tile, info)
    got = pf.deflate_tile(tile)
    assert got == want
    assert got[:2] == b"\x78\x01" and len(got) <= dm.BOUND
    pred = zlib.decompress(got)
    assert pred == dm.predict(tile).tobytes() and np.array_equal(dm.unpredict(np.frombuffer(pred, np.uint8)), tile)
    if name == "noise":
        assert info == ["stored"] * 16 and len(got) == dm.BOUND            # 2 + 16 * (5 + 12 288) + 4
    if name in ("zeros", "all255", "one_literal", "last_differs") or name.startswith("runs_"):
        assert info == ["dynamic"] * 16
    if name == "fibonacci":
        assert info[2] == "dynamic"
    if name == "two_symbols":
        assert info[3] == "dynamic"


def test_the_hostile_tiles_are_hostile():
    """A self-check of the fixtures, not of the codec: it runs tests/deflate_model.py alone and passes without the feature.  It states, on
    the model's own tokens and plans, that the hostile tiles hold what they are there for."""
    p = dm.hostile_preds()
    # runs of every length, and what becomes of them
    toks = dm.tokens(p["runs_first"][6 * dm.BLOCK:7 * dm.BLOCK], int(p["runs_first"][6 * dm.BLOCK - 1]))
    assert toks[:2] == [(0, 255), (1, 257)]                                # block 6 begins with the run of 258: a literal and one match of 257
    toks = dm.tokens(p["runs_first"][7 * dm.BLOCK:8 * dm.BLOCK], int(p["runs_first"][7 * dm.BLOCK - 1]))
    assert toks[:2] == [(0, 255), (1, 258)] and toks[2][0] == 0 and toks[2][1] != 255          # 259: literal + 258
    toks = dm.tokens(p["runs_first"][9 * dm.BLOCK:10 * dm.BLOCK], int(p["runs_first"][9 * dm.BLOCK - 1]))
    assert toks[:4] == [(0, 255), (1, 258), (0, 255), (0, 255)]            # 261: literal + 258 + two literals
    # a run across a block boundary leans in the block it goes on in: no literal there
    q = p["runs_across_lean"]
    b = 7                                                                  # the run of 258 ends in block 7
    toks = dm.tokens(q[b * dm.BLOCK:(b + 1) * dm.BLOCK], int(q[b * dm.BLOCK - 1]))
    assert int(q[b * dm.BLOCK - 1]) == int(q[b * dm.BLOCK]) == 254 and toks[0] == (1, 128)
    toks = dm.tokens(q[14 * dm.BLOCK:15 * dm.BLOCK], int(q[14 * dm.BLOCK - 1]))
    assert toks == [(1, 258)] * 47 + [(1, 162)]                            # a whole block that leans: 12 288 = 47 * 258 + 162
    toks = dm.tokens(p["runs_last"][14 * dm.BLOCK:15 * dm.BLOCK], int(p["runs_last"][14 * dm.BLOCK - 1]))
    assert toks == [(0, 10)] + [(1, 258)] * 47 + [(1, 161)]                # ... and one that does not
    # one literal value in a block: literal, length codes and end-of-block only
    toks = dm.tokens(p["one_literal"][5 * dm.BLOCK:6 * dm.BLOCK], 0)
    assert {t for t in toks if t[0] == 0} == {(0, 42)}
    # Fibonacci counts: the unlimited tree is deeper than 15
    hist = [0] * 286
    for k, v in dm.tokens(p["fibonacci"][2 * dm.BLOCK:3 * dm.BLOCK], int(p["fibonacci"][2 * dm.BLOCK - 1])):
        assert k == 0
        hist[v] += 1
    hist[256] = 1
    used = sorted(c for c in hist if c)
    assert hist[:18] == [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181]
    free = dm.code_lengths([c for c in hist] + [0, 0], 15)
    assert max(free) == 15
    import heapq
    h = [(c, 0) for c in used]
    heapq.heapify(h)
    while len(h) > 1:
        a, b_ = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b_[0], max(a[1], b_[1]) + 1))
    assert h[0][1] > 15


def test_a_step_larger_than_the_row(pf):
    t = TILES["smooth"]
    wide = np.full((256, 256 + 9, 3), 0xA5, np.uint8)
    wide[:, :256] = t
    assert pf.deflate_tile(wide[:, :256]) == pf.deflate_tile(t)
    import ctypes as C
    n = C.c_size_t(0)
    L = pf.lib()
    assert L.pf_deflate_tile_bgr(t.ctypes.data, 0, None, 0, C.byref(n)) == 1 and n.value == dm.BOUND
    out = np.empty(16, np.uint8)
    assert L.pf_deflate_tile_bgr(t.ctypes.data, 0, out.ctypes.data, 16, C.byref(n)) == 0 and n.value == len(pf.deflate_tile(t))
    assert L.pf_deflate_tile_bgr(t.ctypes.data, 767, out.ctypes.data, 16, C.byref(n)) == 0 and b"step" in L.pf_last_error()


def kraft(lengths, limit):
    return sum(1 << (limit - l) for l in lengths if l)


def test_length_builder(pf):
    rng = np.random.default_rng(5)
    cases = []
    for limit, n in ((15, 286), (7, 19), (15, 288), (7, 100), (9, 286)):
        for _ in range(12):
            f = rng.integers(0, 4, n) * rng.integers(0, 2 ** rng.integers(1, 14), n)
            cases.append((limit, f))
        fib = [1, 1]
        while len(fib) < min(n, 40):
            fib.append(fib[-1] + fib[-2])
        f = np.zeros(n, np.int64); f[rng.permutation(n)[:len(fib)]] = fib
        cases.append((limit, f))
        f = np.zeros(n, np.int64); f[:len(fib)] = fib[::-1]
        cases.append((limit, f))
        cases.append((limit, np.ones(n, np.int64)))                       # all tied
        cases.append((limit, np.full(n, 2 ** 31, np.int64)))              # large counts
        two = np.zeros(n, np.int64); two[[3, n - 1]] = [7, 7]
        cases.append((limit, two))
    for limit, f in cases:
        got = pf.deflate_code_lengths(f, limit).tolist()
        assert got == dm.code_lengths(f.tolist(), limit), (limit, f.tolist())
        assert all((l == 0) == (c == 0) for l, c in zip(got, f.tolist())) and max(got) <= limit
        if np.count_nonzero(f) >= 2:
            assert kraft(got, limit) == 1 << limit
    for n, limit in ((286, 15), (19, 7)):                                 # one used symbol: a two-code tree
        for s in (0, 1, n - 1):
            f = np.zeros(n, np.int64); f[s] = 9
            got = pf.deflate_code_lengths(f, limit).tolist()
            assert got == dm.code_lengths(f.tolist(), limit) and got[s] == 1 and got[1 if s == 0 else 0] == 1 and sum(got) == 2
        assert pf.deflate_code_lengths(np.zeros(n, np.int64), limit).tolist() == [0] * n
    for n, limit in ((1, 15), (289, 15), (286, 8), (19, 16), (19, 0)):
        with pytest.raises(ValueError):
            pf.deflate_code_lengths(np.ones(n, np.int64), limit)


def inflate_image(data, ifd, h, w):
    ty, tx = -(-h // 256), -(-w // 256)
    full = np.zeros((ty * 256, tx * 256, 3), np.uint8)
    for i, (off, n) in enumerate(tm.tile_streams(data, ifd)):
        pred = np.frombuffer(zlib.decompress(data[off:off + n]), np.uint8)
        assert pred.size == dm.N and n <= dm.BOUND
        full[(i // tx) * 256:(i // tx + 1) * 256, (i % tx) * 256:(i % tx + 1) * 256] = dm.unpredict(pred)
    return full


def check_lossless_file(pf, data, a, mask, bg, xf, big):
    isbig, ifds = tm.parse(data)
    assert isbig == big
    levels = tm.chain(a)
    colour = ifds[0::2] if mask is not None else ifds
    assert len(ifds) == len(levels) * (2 if mask is not None else 1)
    empty_at, full_at = set(), set()
    for k, (ifd, lv) in enumerate(zip(colour, levels)):
        t = ifd["tags"]
        assert ifd["order"] == sorted(ifd["order"]) and len(set(ifd["order"])) == len(ifd["order"])
        want = {254: [1 if k else 0], 256: [lv.shape[1]], 257: [lv.shape[0]], 258: [8, 8, 8], 259: [8], 262: [2], 277: [3], 284: [1], 317: [2], 322: [256], 323: [256]}
        for tag, v in want.items():
            assert t[tag][1] == v, (k, tag, t[tag])
        assert 530 not in t and 347 not in t and ifd["order"].index(317) == ifd["order"].index(284) + 1 == ifd["order"].index(322) - 1
        if k == 0 and xf is not None:
            assert t[34264][1] == [float(v) for v in xf] and t[34735][1] == [1, 1, 0, 2, 1024, 0, 1, 32767, 1025, 0, 1, 1]
        else:
            assert 34264 not in t and 34735 not in t
        tl = tm.tiles_of(lv)
        st = tm.tile_streams(data, ifd)
        assert len(st) == len(tl)
        for tile, (off, n) in zip(tl, st):
            assert off % 2 == 0 and n > 0 and off + n <= len(data)
            (empty_at if tm.is_empty(tile, bg) else full_at).add((off, n))
        got = inflate_image(data, ifd, *lv.shape[:2])
        assert np.array_equal(got, np.stack(tl).reshape(-(-lv.shape[0] // 256), -(-lv.shape[1] // 256), 256, 256, 3).swapaxes(1, 2).reshape(got.shape)), k
    assert len(empty_at) <= 1 and not (empty_at & full_at)
    if empty_at:
        off, n = list(empty_at)[0]
        assert data[off:off + n] == pf.deflate_tile(np.full((256, 256, 3), min(255, max(0, bg)), np.uint8))
    return ifds, len(empty_at)


def pillow_frames(path, pages):
    """the colour pages `pages` of the file through Pillow (libtiff)"""
    from PIL import Image
    im = Image.open(path)
    out = []
    for k in pages:
        im.seek(k)
        out.append((im.mode, np.asarray(im).copy()))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_files(pf, tmp_path, shape):
    from PIL import features
    assert features.check("libtiff")
    h, w = shape
    n = 0
    for kind in ("noise", "smooth"):
        for masked in (False, True):
            for bg in (0, 255):
                n += 1
                xf = XF if n % 2 else None
                big = n % 4 == 2
                a = model.content(h, w, kind, n + h)
                if w > 600:
                    a[:, w // 2:] = bg                                     # empty tiles on several levels
                m = make_mask(h, w, ("disc", "random", "hole", "all")[n % 4], n) if masked else None
                f = str(tmp_path / ("f%d.tif" % n))
                assert pf.tiff_write_lossless(f, a, m, bg, xf, big)
                data = open(f, "rb").read()
                ifds, n_empty = check_lossless_file(pf, data, a, m, bg, xf, big)
                assert n_empty == (1 if w > 600 else 0)
                if masked:                                                 # the masks are the JPEG file's: same tags, same tile bytes
                    j = str(tmp_path / "j.tif")
                    assert pf.tiff_write_masked(j, a, m, 95, bg, xf, big)
                    jdata = open(j, "rb").read()
                    _, jifds = tm.parse(jdata)
                    for ifd, jifd, mk in zip(ifds[1::2], jifds[1::2], mm.mask_chain(m)):
                        assert ifd["order"] == jifd["order"] == mm.MASK_TAGS
                        assert [ifd["tags"][t] for t in mm.MASK_TAGS if t != 324] == [jifd["tags"][t] for t in mm.MASK_TAGS if t != 324]
                        for off, tile in zip(ifd["tags"][324][1], mm.mask_tiles_of(mk)):
                            assert data[off:off + mm.TILE_BYTES] == tile
                nlev = len(tm.chain(a))
                frames = pillow_frames(f, range(0, 2 * nlev, 2) if masked else range(nlev))
                if masked:
                    # the mask pages (1, 3, ...), byte for byte those of the JPEG file (above): Pillow reads a 1-bit transparency mask
                    # (Photometric 4) only in some versions and says "unknown pixel mode" in others, as tests/test_tiff_mask.py
                    # records for the JPEG file; where it reads them, they are the masks
                    for k, mk in enumerate(mm.mask_chain(m)):
                        try:
                            _, px = pillow_frames(f, [2 * k + 1])[0]
                        except (OSError, ValueError, SyntaxError, NotImplementedError):
                            break
                        assert np.array_equal(px != 0, mk), (k, "pillow mask")
                for k, lv in enumerate(tm.chain(a)):
                    mode, px = frames[k]
                    assert mode == "RGB" and np.array_equal(px[:, :, ::-1], lv), (k, "pillow")
    # a padded row step gives the packed file
    wide = np.full((h, w + 5, 3), 0x5A, np.uint8); wide[:, :w] = a
    f2 = str(tmp_path / "padded.tif")
    assert pf.tiff_write_lossless(f2, wide[:, :w], m, bg, xf, big) and open(f2, "rb").read() == data


def test_writer_refuses_what_it_cannot_do(pf, tmp_path):
    import os
    L = pf.lib()
    a = model.content(40, 56, "noise", 1)
    f = str(tmp_path / "x.tif").encode()
    assert L.pf_tiff_write_bgr_lossless(f, None, 40, 56, 0, None, 0, 0, None, 0) == 0
    assert L.pf_tiff_write_bgr_lossless(f, a.ctypes.data, 0, 56, 0, None, 0, 0, None, 0) == 0
    assert L.pf_tiff_write_bgr_lossless(f, a.ctypes.data, 40, 56, 100, None, 0, 0, None, 0) == 0 and b"step" in L.pf_last_error()
    assert not os.path.exists(f.decode())
    g = str(tmp_path / "missing" / "x.tif").encode()
    assert L.pf_tiff_write_bgr_lossless(g, a.ctypes.data, 40, 56, 0, None, 0, 0, None, 0) == 0 and b"cannot open" in L.pf_last_error()
    assert L.pf_tiff_write_bgr_lossless(f, a.ctypes.data, 40, 56, 0, None, 0, 0, None, 0) == 1
    # the JPEG file is what it was: Compression 7, YCbCr, no Predictor
    assert pf.tiff_write(f.decode(), a)
    t = tm.parse(open(f.decode(), "rb").read())[1][0]["tags"]
    assert t[259][1] == [7] and t[262][1] == [6] and 317 not in t and t[530][1] == [2, 2]


# Size against zlib's own Z_RLE (level 6, window 15) of the same predicted tiles, summed over the tiles of the test images.  zlib is the
# yardstick.  Measured (profiles/tiff_lossless.md): 7 713 509 bytes against zlib's 7 733 402 over 1 728 blocks, i.e. -11.5 bytes a block
# (noise +0.20 %, smooth -2.60 %, steps +1.88 %).  The one structural difference is the tables: 16 sets a tile here, one per about 16 K
# symbols there.  The margin is the smallest table set there is, the one a block of a constant tile carries and zlib does not: the
# all-zero tile's stream has 441 bytes, 6 of them framing, so (441 - 6) / 16 = 27.2, rounded up to 28 bytes a block.
MEASURED_PER_BLOCK = -11.5
MARGIN_PER_BLOCK = 28


def test_size_against_zlib_rle(pf):
    ours = theirs = blocks = 0
    rows = []
    for n, (h, w) in enumerate(SHAPES):
        for kind in ("noise", "smooth", "steps"):
            a = model.content(h, w, kind, n)
            for lv in tm.chain(a):
                for tile in tm.tiles_of(lv):
                    s, z = len(pf.deflate_tile(np.ascontiguousarray(tile))), len(dm.zrle(dm.predict(tile)))
                    ours += s; theirs += z; blocks += 16
                    rows.append((kind, s, z))
    print("lossless tiles: %d bytes, zlib Z_RLE: %d bytes, %d blocks, excess %.3f %%, %.1f bytes a block" % (ours, theirs, blocks, 100.0 * (ours - theirs) / theirs, (ours - theirs) / blocks))
    for kind in ("noise", "smooth", "steps"):
        o = sum(r[1] for r in rows if r[0] == kind); z = sum(r[2] for r in rows if r[0] == kind)
        print("  %-7s ours %9d  zlib %9d  %+.3f %%" % (kind, o, z, 100.0 * (o - z) / z))
    assert ours - theirs <= blocks * (MEASURED_PER_BLOCK + MARGIN_PER_BLOCK)
