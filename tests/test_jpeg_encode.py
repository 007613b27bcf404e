"""The JPEG leg of save(): cv::imwrite(filename, result) (MultiBandMap2DCPU.cpp:841) writes a JPEG when the name ends in .jpg -- libjpeg
at OpenCV 2.4.9's defaults: quality 95, 4:2:0, baseline.  The host encoder (csrc/jpeg_encode.hpp: pf_jpeg_encode_bgr, pf_write_image)
must give libjpeg-turbo's file byte for byte.  Judges: the committed streams Pillow wrote (tests/golden/jpeg_encode_vectors.npz), Pillow
itself where it is installed, and a numpy restatement of libjpeg's rules (tests/jpeg_encode_model.py) that needs neither."""
import ctypes as C
import io
import json
import os
import subprocess

import numpy as np
import pytest

import jpeg_encode_model as model

HERE = os.path.dirname(os.path.abspath(__file__))


def vectors():
    z = np.load(os.path.join(HERE, "golden", "jpeg_encode_vectors.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return [(h, w, kind, q, bytes(z["stream%02d" % i])) for i, (h, w, kind, q) in enumerate(meta["cases"])]


def test_vectors_are_the_cases_of_the_model_file():
    vs = vectors()
    assert [tuple(v[:4]) for v in vs] == model.CASES
    assert {(v[0], v[1]) for v in vs} == {(16, 16), (256, 256), (8, 8), (1, 1), (37, 53), (17, 16), (16, 17), (100, 260)}
    assert {v[3] for v in vs} == {1, 25, 50, 75, 95, 100} and {v[2] for v in vs} == {"noise", "smooth", "zero", "white", "steps"}
    for h, w, kind, q, s in vs:
        assert s[:2] == b"\xff\xd8" and s[-2:] == b"\xff\xd9" and s[2:20] == bytes.fromhex("ffe000104a46494600010100000100010000")


def test_host_encoder_equals_the_committed_streams(pf):
    for i, (h, w, kind, q, stream) in enumerate(vectors()):
        assert pf.jpeg_encode(model.content(h, w, kind, i), q) == stream, (h, w, kind, q)


def test_numpy_model_is_a_second_witness(pf):
    """the rules as the model states them reproduce the committed streams, and the encoder follows the model on sizes the vectors lack"""
    vs = vectors()
    tabs = model.dht_of(vs[0][4])
    for i, (h, w, kind, q, stream) in enumerate(vs):
        if h * w <= 37 * 53:
            assert model.encode(model.content(h, w, kind, i), q, tabs) == stream, (h, w, kind, q)
    for n, (h, w, q) in enumerate([(24, 24, 95), (40, 40, 60), (50, 30, 95), (20, 36, 100), (23, 70, 25), (40, 24, 1), (2, 2, 75), (15, 33, 95), (31, 1, 50), (1, 31, 90)]):
        a = model.content(h, w, ("noise", "steps", "smooth")[n % 3], 40 + n)
        assert pf.jpeg_encode(a, q) == model.encode(a, q, tabs), (h, w, q)


def pillow_stream(Image, a, q):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a[:, :, ::-1])).save(b, "JPEG", quality=q, subsampling=2)
    return b.getvalue()


def test_live_against_pillow(pf):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20261016)
    kinds = ("noise", "smooth", "zero", "white", "steps")
    shapes = [tuple(int(v) for v in rng.integers(1, 71, 2)) for _ in range(150)] + [(1, 70), (70, 1), (256, 256), (481, 643), (768, 1024), (1024, 768)]
    for n, (h, w) in enumerate(shapes):
        q = int(rng.choice([1, 10, 25, 49, 50, 60, 75, 90, 95, 100]))
        a = model.content(h, w, kinds[n % len(kinds)], n)
        assert pf.jpeg_encode(a, q) == pillow_stream(Image, a, q), (h, w, kinds[n % len(kinds)], q)
    # a row-padded image gives the packed one's stream
    for (h, w, pad) in [(37, 53, 1), (16, 16, 48), (100, 260, 7)]:
        a = model.content(h, w, "noise", h)
        wide = np.full((h, w + pad, 3), 0x5A, np.uint8); wide[:, :w] = a
        assert not wide[:, :w].flags["C_CONTIGUOUS"]
        assert pf.jpeg_encode(wide[:, :w], 95) == pillow_stream(Image, a, 95)
    # quality outside 1...100 is clamped as jpeg_set_quality clamps it
    a = model.content(33, 47, "noise", 2)
    assert pf.jpeg_encode(a, 0) == pf.jpeg_encode(a, -5) == pillow_stream(Image, a, 1) and pf.jpeg_encode(a, 101) == pillow_stream(Image, a, 100)


def test_own_decoder_reads_the_stream_as_libjpeg_does(pf):
    """encoder and decoder tied together with no tolerance: pf_jpeg_decode_bgr(pf_jpeg_encode_bgr(a)) == libjpeg-turbo's decode of it"""
    Image = pytest.importorskip("PIL.Image")
    for n, (h, w, q) in enumerate([(1, 1, 95), (16, 16, 50), (37, 53, 95), (100, 260, 100), (256, 256, 75), (17, 16, 1), (300, 200, 95)]):
        s = pf.jpeg_encode(model.content(h, w, ("noise", "smooth", "steps")[n % 3], n), q)
        assert pf.jpeg_info(s) == (h, w, 3)
        assert np.array_equal(pf.decode_jpeg(s)[:, :, ::-1], np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))), (h, w, q)


def test_write_image_jpg_is_quality_95(pf, tmp_path):
    from test_output_side import decode_png, decode_ppm
    a = model.content(45, 70, "steps", 3)
    want = pf.jpeg_encode(a, 95)
    for name in ("a.jpg", "a.JPEG", "a.jpeg", "a.JPG", "dots.in.name.Jpg"):
        f = str(tmp_path / name)
        assert pf.write_image(f, a) and open(f, "rb").read() == want, name
        assert np.array_equal(pf.read_image(f), pf.decode_jpeg(want))
    # the other extensions write what they wrote: PNG and PPM with the image's pixels
    for name, dec in (("a.png", decode_png), ("a.ppm", decode_ppm), ("a.jpg.ppm", decode_ppm), ("jpg", decode_ppm)):
        f = str(tmp_path / name)
        assert pf.write_image(f, a) and np.array_equal(dec(f)[:, :, ::-1], a), name
    assert open(str(tmp_path / "a.png"), "rb").read(4) == b"\x89PNG" and open(str(tmp_path / "jpg"), "rb").read(2) == b"P6"
    assert not pf.write_image(str(tmp_path / "missing" / "a.jpg"), a)
    # more pixels on a side than a JPEG holds: refused with a message, and no file
    wide = np.zeros((1, 65536, 3), np.uint8)
    f = str(tmp_path / "wide.jpg")
    assert not pf.write_image(f, wide) and not os.path.exists(f) and b"65535" in pf.lib().pf_last_error()
    assert pf.write_image(str(tmp_path / "fits.jpg"), wide[:, :65535])
    assert pf.jpeg_info(open(str(tmp_path / "fits.jpg"), "rb").read()) == (1, 65535, 3)


def test_bad_arguments_and_bounds(pf):
    L = pf.lib()
    n = C.c_size_t(0)
    for i, (h, w, kind, q, stream) in enumerate(vectors()):
        a = model.content(h, w, kind, i)
        assert L.pf_jpeg_encode_bgr(a.ctypes.data, h, w, 0, q, None, 0, C.byref(n)) == 1 and n.value >= len(stream), (h, w, kind, q)
        out = np.full(len(stream) + 4, 0xA5, np.uint8)
        assert L.pf_jpeg_encode_bgr(a.ctypes.data, h, w, 0, q, out.ctypes.data, len(stream) - 1, C.byref(n)) == 0
        assert n.value == len(stream) and (out == 0xA5).all() and b"buffer" in L.pf_last_error()          # nothing written, not even below cap
        assert L.pf_jpeg_encode_bgr(a.ctypes.data, h, w, 0, q, out.ctypes.data, len(stream), C.byref(n)) == 1
        assert out[:len(stream)].tobytes() == stream and (out[len(stream):] == 0xA5).all()
    a = model.content(8, 8, "noise", 0); out = np.zeros(4096, np.uint8)
    assert L.pf_jpeg_encode_bgr(None, 8, 8, 0, 95, out.ctypes.data, out.size, C.byref(n)) == 0
    assert L.pf_jpeg_encode_bgr(a.ctypes.data, 8, 8, 0, 95, out.ctypes.data, out.size, None) == 0
    assert L.pf_jpeg_encode_bgr(a.ctypes.data, 0, 8, 0, 95, out.ctypes.data, out.size, C.byref(n)) == 0
    assert L.pf_jpeg_encode_bgr(a.ctypes.data, 8, -1, 0, 95, out.ctypes.data, out.size, C.byref(n)) == 0
    assert L.pf_jpeg_encode_bgr(a.ctypes.data, 8, 8, 23, 95, out.ctypes.data, out.size, C.byref(n)) == 0 and b"step" in L.pf_last_error()
    assert L.pf_jpeg_encode_bgr(a.ctypes.data, 8, 65536, 0, 95, out.ctypes.data, out.size, C.byref(n)) == 0 and b"65535" in L.pf_last_error()


def test_divisions_of_the_quantiser_are_exact_integers():
    """The kernels and the scalar encoder divide in integers, as libjpeg's C path does (no reciprocal): the one property to hold is
    round-half-away-from-zero, for every divisor 8 * 1 ... 8 * 255 over the DCT's whole output range."""
    v = np.arange(-16384, 16385, dtype=np.int64)
    for qv in range(1, 256):
        d = 8 * qv
        got = np.sign(v) * ((np.abs(v) + (d >> 1)) // d)
        assert np.array_equal(got, np.sign(v) * np.floor(np.abs(v) / d + 0.5).astype(np.int64)), qv


def test_host_encoder_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/san_jpeg_encode.cpp: every vector and every size 1...40 x 1...40 into a buffer of exactly the stream's length"""
    out = str(tmp_path / "build")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "cpp"), "-f", "jpeg_encode.mk", "OUT=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    d = tmp_path / "vec"; d.mkdir()
    for i, (h, w, kind, q, stream) in enumerate(vectors()):
        (d / ("v%02d.bgr" % i)).write_bytes(model.content(h, w, kind, i).tobytes())
        (d / ("v%02d.jpg" % i)).write_bytes(stream)
        (d / ("v%02d.txt" % i)).write_text("%d %d %d\n" % (h, w, q))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(out, "san_jpeg_encode"), str(d), str(len(vectors()))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "MISMATCH" not in text, text[-4000:]
    line = [l for l in text.splitlines() if l.startswith("vectors ")][-1].split()
    assert int(line[1]) == len(vectors()) and int(line[3]) == 1600 and int(line[5]) > 0
