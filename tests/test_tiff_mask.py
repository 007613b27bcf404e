"""The masked pyramid TIFF of the host writer (csrc/tiff_pyramid.hpp behind pf_tiff_write_bgr_masked) against the format's description in
include/pifusion.h, restated in tests/tiff_mask_model.py: the interleaved IFD chain, every tag of every mask IFD, every mask tile's bytes
(OR chain, MSB-first packing, zero fill), the two shared mask tiles, the placement; the colour half is the unmasked file's and the unmasked
writer writes what it wrote; an independent reader (Pillow + libtiff); failure without a file; the sanitizer build.  No device."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import jpeg_encode_model as model
import tiff_mask_model as mm
import tiff_model as tm
from test_tiff import XF, encoder

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [(1, 1), (255, 257), (256, 256), (257, 513), (300, 1000)]
KINDS = ["all", "none", "disc", "random", "last_pixel", "hole"]


def make_mask(h, w, kind, seed=0):
    """a byte per pixel, non-zero = covered (the covered values vary: any non-zero byte counts)"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "all":
        return np.full((h, w), 255, np.uint8)
    if kind == "none":
        return np.zeros((h, w), np.uint8)
    if kind == "disc":
        y, x = np.mgrid[0:h, 0:w]
        return (((y - h / 2.0) ** 2 / max(h / 2.2, 1) ** 2 + (x - w / 2.0) ** 2 / max(w / 2.2, 1) ** 2) <= 1).astype(np.uint8) * 7
    if kind == "random":
        return (rng.integers(0, 2, (h, w)) * rng.integers(1, 256, (h, w))).astype(np.uint8)
    m = np.zeros((h, w), np.uint8) if kind == "last_pixel" else np.full((h, w), 1, np.uint8)
    if kind == "last_pixel":
        m[h - 1, w - 1] = 128
    else:
        m[h // 2, w // 3] = 0
    return m


@pytest.mark.parametrize("kind", KINDS)
def test_structure_and_bytes(pf, tmp_path, kind):
    enc = {95: encoder(pf, 95), 30: encoder(pf, 30)}
    for n, (h, w) in enumerate(SIZES):
        a = model.content(h, w, ("noise", "smooth", "zero")[n % 3], n)
        m = make_mask(h, w, kind, n)
        for v in range(2):
            q = (95, 30)[(n + v) % 2]; big = bool((n + v) % 2); xf = XF if v else None; bg = (0, 255)[v]
            f = str(tmp_path / ("m%d_%d.tif" % (n, v)))
            if v:                                                         # a padded mask step (and a padded image step) give the packed file
                wide = np.full((h, w + 5), 0x5A, np.uint8); wide[:, :w] = m
                img = np.full((h, w + 3, 3), 0xA5, np.uint8); img[:, :w] = a
                assert pf.tiff_write_masked(f, img[:, :w], wide[:, :w], q, bg, xf, big)
            else:
                assert pf.tiff_write_masked(f, a, m, q, bg, xf, big)
            data = open(f, "rb").read()
            got = mm.check_masked_file(data, a, m, bg, enc[q], xf, big=big)
            assert data[2] == (43 if big else 42)
            tiles = sum(len(tm.tiles_of(lv)) for lv in tm.chain(a))
            assert got["zero"] + got["one"] + got["own"] == tiles
            if kind == "none":
                assert got["zero"] == tiles
            if kind == "all" and (h, w) == (300, 1000):
                assert got["one"] == 3 and got["zero"] == 0               # tiles (0, 0...2) of image 0; every other tile ends inside itself
            if kind == "all" and (h, w) == (256, 256):
                assert got == dict(got, one=1, own=0, zero=0)
            if kind == "last_pixel":
                assert got["own"] == len(tm.chain(a))                     # the one pixel survives the OR chain down to the last image
            if kind == "hole" and h > 2 and w > 3:
                assert not mm.mask_chain(m)[0].all() and (len(tm.chain(a)) == 1 or mm.mask_chain(m)[1].all())          # ... and the hole does not


def test_colour_half_is_the_unmasked_file_and_the_unmasked_writer_is_untouched(pf, tmp_path):
    digest = lambda f: hashlib.sha256(open(f, "rb").read()).hexdigest()
    for n, (h, w) in enumerate(SIZES):
        a = model.content(h, w, "smooth", n)
        a[: h // 2] = 0                                                   # some empty colour tiles
        plain, masked, again = (str(tmp_path / x) for x in ("plain.tif", "masked.tif", "again.tif"))
        assert pf.tiff_write(plain, a, 95, 0, XF)
        before = digest(plain)
        assert pf.tiff_write_masked(masked, a, np.full((h, w), 255, np.uint8), 95, 0, XF)
        assert pf.tiff_write(again, a, 95, 0, XF) and pf.tiff_write(plain, a, 95, 0, XF)
        assert digest(again) == before == digest(plain)
        p, d = open(plain, "rb").read(), open(masked, "rb").read()
        tm.check_file(p, a, 0, encoder(pf, 95), XF, big=False)             # the unmasked file is still the format's
        _, pi = tm.parse(p); _, di = tm.parse(d)
        assert len(di) == 2 * len(pi)
        for x, y in zip(pi, di[0::2]):
            assert x["order"] == y["order"]
            for tag in x["order"]:
                if tag != 324:
                    assert x["tags"][tag] == y["tags"][tag], tag
            assert [p[o:o + k] for o, k in tm.tile_streams(p, x)] == [d[o:o + k] for o, k in tm.tile_streams(d, y)]
            sx, sy = tm.tile_streams(p, x), tm.tile_streams(d, y)
            assert [sx.index(s) for s in sx] == [sy.index(s) for s in sy]          # the same tiles share the empty stream


def test_pillow_reads_page_1_as_the_mask(pf, tmp_path):
    from PIL import Image
    h, w = 300, 1000
    a = model.content(h, w, "smooth", 2)
    m = make_mask(h, w, "disc", 2)
    f = str(tmp_path / "p.tif")
    assert pf.tiff_write_masked(f, a, m, 95, 0, XF)
    try:
        im = Image.open(f)
        assert im.n_frames == 2 * len(tm.chain(a))
        im.seek(1)
        got = np.asarray(im.convert("L")).copy()
    except (OSError, ValueError, SyntaxError, NotImplementedError) as e:
        pytest.skip("Pillow refuses the 1-bit tiles of page 1: %r" % (e,))
    assert got.shape == (h, w) and np.array_equal(got != 0, m != 0)
    im.seek(3)
    assert np.array_equal(np.asarray(im.convert("L")) != 0, mm.mask_chain(m)[1])
    im.seek(0)
    assert im.size == (w, h) and [float(v) for v in im.tag_v2[34264]] == XF


def test_failure_leaves_no_file(pf, tmp_path):
    L = pf.lib()
    a = model.content(40, 56, "noise", 1)
    m = np.full((40, 56), 255, np.uint8)
    f = str(tmp_path / "missing" / "x.tif")
    assert not pf.tiff_write_masked(f, a, m) and not os.path.exists(f) and b"cannot open" in L.pf_last_error()
    g = str(tmp_path / "bad.tif")
    call = lambda name, img, rows, cols, step, mask, mstep: L.pf_tiff_write_bgr_masked(name, img, rows, cols, step, mask, mstep, 95, 0, None, 0)
    assert call(g.encode(), a.ctypes.data, 40, 56, 0, None, 0) == 0 and not os.path.exists(g) and b"mask" in L.pf_last_error()
    assert call(g.encode(), None, 40, 56, 0, m.ctypes.data, 0) == 0 and not os.path.exists(g)
    assert call(g.encode(), a.ctypes.data, 0, 56, 0, m.ctypes.data, 0) == 0 and not os.path.exists(g) and b"size" in L.pf_last_error()
    assert call(g.encode(), a.ctypes.data, 40, 56, 100, m.ctypes.data, 0) == 0 and not os.path.exists(g) and b"step" in L.pf_last_error()
    assert call(g.encode(), a.ctypes.data, 40, 56, 0, m.ctypes.data, 55) == 0 and not os.path.exists(g) and b"step" in L.pf_last_error()
    assert call(None, a.ctypes.data, 40, 56, 0, m.ctypes.data, 0) == 0
    assert call(g.encode(), a.ctypes.data, 40, 56, 0, m.ctypes.data, 0) == 1 and os.path.exists(g)


def test_masked_host_writer_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/san_tiff_mask.cpp: the sweep of this file and every size 1...40 x 1...40 with random masks, from heap blocks of exactly
    the bytes the call may read; a stand-alone program, nothing is loaded into this process"""
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "-f", "tiff_mask.mk", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "san_tiff_mask"), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "MISMATCH" not in text, text[-4000:]
    line = [l for l in text.splitlines() if l.startswith("files ")][-1].split()
    assert int(line[1]) >= 1600 + 30 and int(line[3]) == 0
