"""The PNG of save_png made on the GPU (csrc/png_encode.hip) against the host encoder (csrc/png_encode.hpp; itself pinned to the format by
tests/test_png_encode.py): byte-equal files for every shape and mask of the host list, padded steps, an image pointer that is not 16-byte
aligned, a caller's stream, one encoder object reused large then small; then the map: save_png against png_encode of save_to_memory's
pixels, masked against save_to_memory_mask and the oracle's level-0 weights on a mosaic with holes, the map left as it was, a single-band
map, a failed save, an empty map."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import png_model as pm
from helpers import jitter_poses, workloads
from test_gpu_jpeg_encode import build_map
from test_gpu_tiff_mask import oracle_mask
from test_output_side import decode_png

pytestmark = pytest.mark.gpu

CASES = pm.cases()
GUARD = 64


def device_file(pf, bgr, mask=None, extra=0, mextra=0, shift=0, stream=None):
    """pf_png_encode_device of the image copied to the GPU: rows `extra` (`mextra`) bytes longer than the pixels, the first pixel `shift`
    bytes behind an aligned address; the output buffer has the bound and a guard band, which stays untouched"""
    import torch
    rows, cols = bgr.shape[:2]
    step = 3 * cols + extra
    flat = torch.full((rows * step + shift,), 0x5A, dtype=torch.uint8, device="cuda")
    flat[shift:].view(rows, step)[:, :3 * cols] = torch.from_numpy(np.ascontiguousarray(bgr).reshape(rows, 3 * cols)).cuda()
    mp, ms, mbuf = None, 0, None
    if mask is not None:
        ms = cols + mextra
        mbuf = torch.full((rows * ms + shift,), 0xC3, dtype=torch.uint8, device="cuda")
        mbuf[shift:].view(rows, ms)[:, :cols] = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
        mp = mbuf.data_ptr() + shift
    torch.cuda.synchronize()
    L = pf.lib()
    n = C.c_size_t(0)
    ptr = flat.data_ptr() + shift
    assert L.pf_png_encode_device(ptr, rows, cols, step if extra else 0, mp, ms if mextra else 0, None, 0, C.byref(n), stream) == 1
    assert n.value == pm.bound(rows, cols, mask is not None)
    out = np.full(n.value + GUARD, 0xA5, np.uint8)
    assert L.pf_png_encode_device(ptr, rows, cols, step if extra else 0, mp, ms if mextra else 0, out.ctypes.data, n.value, C.byref(n), stream) == 1, L.pf_last_error()
    assert n.value <= out.size - GUARD and (out[n.value:] == 0xA5).all()
    return out[:n.value].tobytes()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_device_file_equals_host_file(pf, name):
    _, bgr, mask = next(c for c in CASES if c[0] == name)
    want = pf.png_encode(bgr, mask)
    assert device_file(pf, bgr, mask) == want
    # padded steps, and an image (and a mask) that begin 3 bytes behind an aligned address
    assert device_file(pf, bgr, mask, extra=13, mextra=5, shift=3) == want


def test_callers_stream_and_exact_cap(pf):
    import torch
    _, bgr, mask = next(c for c in CASES if c[0] == "structured_300x1030")
    want = pf.png_encode(bgr, mask)
    side = torch.cuda.Stream()
    assert device_file(pf, bgr, mask, stream=side.cuda_stream) == want
    # a cap one byte short: 0 with the length, nothing written; the exact cap: the file
    dev, dm = torch.from_numpy(bgr).cuda(), torch.from_numpy(mask).cuda()
    L = pf.lib(); n = C.c_size_t(0)
    out = np.full(len(want) + GUARD, 0xA5, np.uint8)
    assert L.pf_png_encode_device(dev.data_ptr(), 300, 1030, 0, dm.data_ptr(), 0, out.ctypes.data, len(want) - 1, C.byref(n), None) == 0
    assert n.value == len(want) and (out == 0xA5).all()
    assert L.pf_png_encode_device(dev.data_ptr(), 300, 1030, 0, dm.data_ptr(), 0, out.ctypes.data, len(want), C.byref(n), None) == 1
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
    # refusals: a host pointer, a step smaller than a row, no image
    assert L.pf_png_encode_device(bgr.ctypes.data, 300, 1030, 0, None, 0, out.ctypes.data, out.size, C.byref(n), None) == 0 and b"device memory" in L.pf_last_error()
    assert L.pf_png_encode_device(dev.data_ptr(), 300, 1030, 3089, None, 0, out.ctypes.data, out.size, C.byref(n), None) == 0 and b"step" in L.pf_last_error()
    assert L.pf_png_encode_device(None, 300, 1030, 0, None, 0, out.ctypes.data, out.size, C.byref(n), None) == 0


def test_one_encoder_large_then_small(pf):
    """the process-wide encoder keeps its buffers: a small file after a large one holds nothing of the large one's plans, bytes or offsets"""
    big = next(c for c in CASES if c[0] == "noise_700x600")
    for name in ("random_1x1", "structured_17x241", "rgba_structured_16x256_checker", "const255_700x600"):
        _, bgr, mask = next(c for c in CASES if c[0] == name)
        assert device_file(pf, big[1]) == pf.png_encode(big[1])
        assert device_file(pf, bgr, mask) == pf.png_encode(bgr, mask), name


def rgba_of(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == "RGBA"
    return np.asarray(im)


@pytest.mark.parametrize("ff,bands,bg", [(0, 5, 0), (1, 5, 255), (0, 0, 255), (1, 0, 0)])
def test_save_png_is_the_host_encoding_of_the_mosaic_and_leaves_the_map_alone(pf, orc, tmp_path, ff, bands, bg):
    g, o = build_map(pf, orc, ff, bands, bg)
    ref, oorg = o.save()
    mem, mask, org = g.save_to_memory_mask()
    assert org == oorg and np.array_equal(mem, ref)
    g.blend_changed()                                                     # clears Ischanged: what follows must not be touched by the save
    tiles = g.tiles()
    before = g.blend_tiles(tiles)
    f = str(tmp_path / "m.png")
    assert g.save_png(f), pf.lib().pf_last_error()
    assert open(f, "rb").read() == pf.png_encode(mem)
    assert g.save_png(f, masked=True), pf.lib().pf_last_error()
    data = open(f, "rb").read()
    assert data == pf.png_encode(mem, mask)
    a = rgba_of(data)
    assert np.array_equal(a[:, :, 2::-1], ref) and np.array_equal(a[:, :, 3] == 0, mask == 0)
    if bands == 5:
        assert np.array_equal(a[:, :, 3] == 0, oracle_mask(o, mem.shape[:2], org) == 0)
    assert g.save_png(f) and open(f, "rb").read() == pf.png_encode(mem)          # unmasked after masked: no option of the save lives in the map
    # the map, its flags and the other saves are as before
    assert g.blend_changed()[0] == [] and np.array_equal(g.blend_tiles(tiles), before)
    again, org2 = g.save_to_memory()
    assert org2 == org and np.array_equal(again, ref)
    u = str(tmp_path / "u.png")
    assert g.save(u) and np.array_equal(decode_png(u)[:, :, ::-1], ref)          # save("x.png") keeps filter type 0 (decode_png asserts it)
    assert open(u, "rb").read() != open(f, "rb").read()
    g.close()


def test_masked_save_of_a_mosaic_with_holes(pf, orc, tmp_path):
    """two sorties far apart on a diagonal: the mosaic's bounding box has tile slots without a map tile; alpha is 0 there and wherever the
    oracle's level-0 weight is 0, and nowhere else"""
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    a = jitter_poses(3, seed=5)
    b = [[p[0] + 300.0, p[1] + 250.0] + list(p[2:]) for p in jitter_poses(3, seed=6)]
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, bg_color=255)
    o = orc.OracleMap(band_num=5, force_float=0, bg_color=255)
    assert g.prepare(wl.IDENTITY_PLANE, cam, a) and o.prepare(wl.IDENTITY_PLANE, cam, a)
    for k, p in enumerate(a + b):
        img = wl.smooth_frame(480, 640, k) ^ (wl.noise_frame(480, 640, 300 + k) >> 3)
        assert g.feed(img, p) and o.feed(img, p)
    mem, mask, org = g.save_to_memory_mask()
    assert (mem.shape[0] // 256) * (mem.shape[1] // 256) > len(g.tiles())          # holes
    f = str(tmp_path / "holes.png")
    assert g.save_png(f, True), pf.lib().pf_last_error()
    data = open(f, "rb").read()
    assert data == pf.png_encode(mem, mask)
    want = oracle_mask(o, mem.shape[:2], org)
    rgba = rgba_of(data)
    assert np.array_equal(rgba[:, :, 3] == 0, want == 0) and 0 < int((want == 0).sum()) < want.size
    assert np.array_equal(rgba[:, :, 2::-1], mem)
    g.close()


def test_single_band_map_takes_the_host_encoder_with_alpha_as_coverage(pf, tmp_path):
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    poses = jitter_poses(4, seed=3)
    g = pf.Map2D.create(pf.TypeCPU, False)
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses)
    for k, p in enumerate(poses):
        assert g.feed(wl.smooth_frame(480, 640, k), p)
    mem, org = g.save_to_memory()
    want = np.zeros(mem.shape[:2], np.uint8)
    for (ix, iy) in g.tiles():
        want[(iy - org[1]) * 256:(iy - org[1] + 1) * 256, (ix - org[0]) * 256:(ix - org[0] + 1) * 256] = (g.tile_bgra(ix, iy)[:, :, 3] != 0) * 255
    assert 0 < int((want != 0).sum()) < want.size
    f = str(tmp_path / "s.png")
    assert g.save_png(f) and open(f, "rb").read() == pf.png_encode(mem)
    assert g.save_png(f, True) and open(f, "rb").read() == pf.png_encode(mem, want)
    assert not g.save_png(str(tmp_path / "missing" / "s.png"))
    g.close()


def test_missing_directory_and_empty_map_return_false(pf, orc, tmp_path):
    g, _ = build_map(pf, orc, 0, 5)
    bad = str(tmp_path / "missing" / "x.png")
    assert not g.save_png(bad) and not g.save_png(bad, True) and not os.path.exists(bad)
    mem, org = g.save_to_memory()
    f = str(tmp_path / "x.png")
    assert g.save_png(f) and open(f, "rb").read() == pf.png_encode(mem)          # the next save is right
    g.close()
    wl = workloads()
    e = pf.Map2D.create(pf.TypeMultiBandCPU, False)
    assert e.prepare(wl.IDENTITY_PLANE, [640, 480, 500, 500, 320, 240], jitter_poses(2, seed=1))
    f = str(tmp_path / "e.png")
    assert not e.save_png(f, True) and not e.save_png(f) and not os.path.exists(f)
    e.close()
