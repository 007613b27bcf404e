"""The tiled pyramid TIFF of the host writer (csrc/tiff_pyramid.hpp behind pf_tiff_write_bgr / pf_write_image("x.tif")) against the format's
description in include/pifusion.h, restated in tests/tiff_model.py: structure, every tile's bytes (pf_jpeg_encode_bgr of the numpy model's
tile: overview arithmetic, edge fill and encoder in one go), the shared empty stream, an independent reader (Pillow + libtiff), BigTIFF, an
image wider than a JPEG can be, failure without a file.  No device."""
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_encode_model as model
import tiff_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [(1, 1), (255, 257), (256, 256), (300, 1000), (1024, 768)]
XF = [0.05, 0, 0, -12.5, 0, 0.05, 0, 33.25, 0, 0, 1, 0, 0, 0, 0, 1]


def encoder(pf, q):
    memo = {}
    def enc(tile):
        k = tile.tobytes()
        if k not in memo:
            memo[k] = pf.jpeg_encode(np.ascontiguousarray(tile), q)
        return memo[k]
    return enc


def with_background(a, bg, seed=0):
    """`a` with background-coloured regions that cover whole tiles at several levels: the right half, and the top-left 512 x 512 except one pixel"""
    a = a.copy()
    h, w = a.shape[:2]
    a[:, w // 2:] = bg
    a[:min(h, 512), :min(w, 512)] = bg
    if h > 300 and w > 300:
        a[300, 290] = (bg + 128) % 256          # one pixel in tile (1, 1) of image 0
    return a


def pillow_frames(path):
    from PIL import Image
    im = Image.open(path)
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append(np.asarray(im.convert("RGB")).copy())
    return im, out


def per_tile_decode(data, shape_chain):
    """every image of the file from its tile streams alone: each stream through libjpeg (Pillow's JPEG reader), pasted together and cropped"""
    from PIL import Image
    _, ifds = tm.parse(data)
    out = []
    for ifd, (h, w) in zip(ifds, shape_chain):
        ty, tx = -(-h // 256), -(-w // 256)
        full = np.zeros((ty * 256, tx * 256, 3), np.uint8)
        memo = {}
        for i, (off, n) in enumerate(tm.tile_streams(data, ifd)):
            if (off, n) not in memo:
                memo[(off, n)] = np.asarray(Image.open(io.BytesIO(data[off:off + n])).convert("RGB"))
            full[(i // tx) * 256:(i // tx + 1) * 256, (i % tx) * 256:(i % tx + 1) * 256] = memo[(off, n)]
        out.append(full[:h, :w])
    return out


@pytest.mark.parametrize("kind", ["noise", "smooth", "zero"])
def test_structure_and_streams(pf, tmp_path, kind):
    for n, (h, w) in enumerate(SIZES):
        a = model.content(h, w, kind, n)
        for q in (95, 30):
            f = str(tmp_path / ("s%d_%d.tif" % (n, q)))
            assert pf.tiff_write(f, a, q, 0, XF if n % 2 else None)
            data = open(f, "rb").read()
            ni, nt, ne = tm.check_file(data, a, 0, encoder(pf, q), XF if n % 2 else None, big=False)
            assert ni == len(tm.chain(a)) and (ne == nt if kind == "zero" else ne == 0 if kind == "noise" else True)
    # a padded row step gives the packed file; pf_write_image("x.tif") is quality 95, background 0, no geo tags; .TIFF too
    a = model.content(300, 1000, "smooth", 3)
    wide = np.full((300, 1000 + 7, 3), 0x5A, np.uint8); wide[:, :1000] = a
    f1, f2, f3 = (str(tmp_path / n) for n in ("packed.tif", "padded.tif", "plain.TIFF"))
    assert pf.tiff_write(f1, a) and pf.tiff_write(f2, wide[:, :1000]) and pf.write_image(f3, a)
    assert open(f1, "rb").read() == open(f2, "rb").read() == open(f3, "rb").read()
    assert open(f1, "rb").read(4) == b"II*\0"


@pytest.mark.parametrize("bg", [0, 255])
def test_empty_tiles_share_one_stream(pf, tmp_path, bg):
    a = with_background(model.content(1100, 2100, "noise", 5), bg)
    f = str(tmp_path / "e.tif")
    assert pf.tiff_write(f, a, 95, bg)
    data = open(f, "rb").read()
    ni, nt, ne = tm.check_file(data, a, bg, encoder(pf, 95))
    _, ifds = tm.parse(data)
    empties = [[tm.is_empty(t, bg) for t in tm.tiles_of(lv)] for lv in tm.chain(a)]
    assert sum(any(e) for e in empties) >= 3                              # empty tiles at several levels
    st0 = tm.tile_streams(data, ifds[0])
    shared = {s for lv, ifd in zip(empties, ifds) for e, s in zip(lv, tm.tile_streams(data, ifd)) if e}
    assert len(shared) == 1
    tx = -(-2100 // 256)
    assert not empties[0][tx + 1] and empties[0][0] and empties[0][1] and st0[tx + 1] not in shared           # background but one pixel
    assert data[slice(list(shared)[0][0], sum(list(shared)[0]))] == pf.jpeg_encode(np.full((256, 256, 3), bg, np.uint8), 95)
    # the other colour is not background: no tile is empty then
    assert pf.tiff_write(f, a, 95, 255 - bg)
    assert tm.check_file(open(f, "rb").read(), a, 255 - bg, encoder(pf, 95))[2] == 0


def test_pillow_reads_every_image_as_its_tiles_decode(pf, tmp_path):
    from PIL import features
    assert features.check("libtiff")
    for n, (h, w, bg) in enumerate([(300, 1000, 0), (1024, 768, 255), (255, 257, 0), (1, 1, 0)]):
        a = with_background(model.content(h, w, "smooth" if n % 2 else "noise", n), bg)
        files = []
        for big in (False, True):
            f = str(tmp_path / ("p%d_%d.tif" % (n, big)))
            assert pf.tiff_write(f, a, 95, bg, XF, big)
            data = open(f, "rb").read()
            tm.check_file(data, a, bg, encoder(pf, 95), XF, big=big)
            assert data[2] == (43 if big else 42)
            im, frames = pillow_frames(f)
            shapes = [lv.shape[:2] for lv in tm.chain(a)]
            assert im.n_frames == len(shapes)
            want = per_tile_decode(data, shapes)
            for k, (got, w_) in enumerate(zip(frames, want)):
                assert got.shape == w_.shape and np.array_equal(got, w_), (h, w, big, k)
            im.seek(0)
            assert [float(v) for v in im.tag_v2[34264]] == XF and list(im.tag_v2[34735]) == [1, 1, 0, 2, 1024, 0, 1, 32767, 1025, 0, 1, 1]
            files.append((data, frames))
        # BigTIFF: 8-byte offsets, the same streams, the same pictures
        (c, cf), (b, bf) = files
        _, ci = tm.parse(c); _, bi = tm.parse(b)
        for x, y in zip(ci, bi):
            assert y["tags"][324][0] == 16 and x["tags"][324][0] == 4
            assert [c[o:o + n_] for o, n_ in tm.tile_streams(c, x)] == [b[o:o + n_] for o, n_ in tm.tile_streams(b, y)]
        assert all(np.array_equal(p, q) for p, q in zip(cf, bf))


def test_wider_than_a_jpeg_can_be(pf, tmp_path):
    h, w = 256, 65792
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x // 7 + y) % 256, (x // 300 * 37 + y * 2) % 256, (x + y * 3) % 251], -1).astype(np.uint8)
    a[:, 20000:30000] = 0
    f = str(tmp_path / "wide.tif")
    assert pf.tiff_write(f, a)
    data = open(f, "rb").read()
    ni, nt, ne = tm.check_file(data, a, 0, encoder(pf, 95))
    assert ni == 10 and ne > 30
    shapes = [lv.shape[:2] for lv in tm.chain(a)]
    assert shapes[8] == (1, 257) and shapes[9] == (1, 129)
    from PIL import Image
    limit, Image.MAX_IMAGE_PIXELS = Image.MAX_IMAGE_PIXELS, None
    try:
        im = Image.open(f)
        assert im.n_frames == 10 and im.size == (w, h)
        assert np.array_equal(np.asarray(im.convert("RGB")), per_tile_decode(data, shapes[:1])[0])
    finally:
        Image.MAX_IMAGE_PIXELS = limit
    j = str(tmp_path / "wide.jpg")
    assert not pf.write_image(j, a) and not os.path.exists(j) and b"65535" in pf.lib().pf_last_error()


def test_failure_leaves_no_file(pf, tmp_path):
    L = pf.lib()
    a = model.content(40, 56, "noise", 1)
    f = str(tmp_path / "missing" / "x.tif")
    assert not pf.tiff_write(f, a) and not os.path.exists(f) and b"cannot open" in L.pf_last_error()
    assert not pf.write_image(f, a) and b"cannot open" in L.pf_last_error()
    g = str(tmp_path / "bad.tif")
    assert L.pf_tiff_write_bgr(g.encode(), a.ctypes.data, 0, 56, 0, 95, 0, None, 0) == 0 and not os.path.exists(g) and b"size" in L.pf_last_error()
    assert L.pf_tiff_write_bgr(g.encode(), a.ctypes.data, 40, 56, 100, 95, 0, None, 0) == 0 and not os.path.exists(g) and b"step" in L.pf_last_error()
    assert L.pf_tiff_write_bgr(g.encode(), None, 40, 56, 0, 95, 0, None, 0) == 0 and not os.path.exists(g)
    assert L.pf_tiff_write_bgr(None, a.ctypes.data, 40, 56, 0, 95, 0, None, 0) == 0


def test_host_writer_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/san_tiff.cpp: every size 1...40 x 1...40 and a few around the tile edge, from heap blocks of exactly rows * step bytes"""
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "-f", "tiff.mk", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "san_tiff"), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "MISMATCH" not in text, text[-4000:]
    line = [l for l in text.splitlines() if l.startswith("files ")][-1].split()
    assert int(line[1]) > 1600 and int(line[3]) == 0
