"""The masked pyramid TIFF made on the GPU (csrc/coverage.hip: the masks' bit planes, their OR chain, flags and gather; overview.hip and
jpeg_encode.hip: the colour half) against the host writer (csrc/tiff_pyramid.hpp, itself pinned to the format by tests/test_tiff_mask.py):
byte-equal files.  First for images and masks of any size in device memory (pf_tiff_write_device_masked), then for the map:
save_to_memory_mask against the oracle's weights, save_tiff_masked against the host writer of those arrays, a map with holes, a map with
waiting keyframes, a single-band map, two threads."""
import os

import numpy as np
import pytest

import jpeg_encode_model as model
import tiff_mask_model as mm
import tiff_model as tm
from helpers import jitter_poses, workloads
from test_gpu_jpeg_encode import build_map
from test_gpu_tiff import host_file, transform_of
from test_tiff import XF, encoder
from test_tiff_mask import KINDS, SIZES, make_mask

pytestmark = pytest.mark.gpu


def device_masked(pf, path, a, m, q=95, bg=0, xf=None, big=False, step=0, mstep=0, stream=None):
    import torch
    h, w = a.shape[:2]
    if step:
        buf = torch.full((h, step), 0x5A, dtype=torch.uint8, device="cuda")
        buf[:, :3 * w] = torch.from_numpy(np.ascontiguousarray(a).reshape(h, 3 * w)).cuda()
    else:
        buf = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if mstep:
        mb = torch.full((h, mstep), 0xC3, dtype=torch.uint8, device="cuda")
        mb[:, :w] = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    else:
        mb = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    torch.cuda.synchronize()
    assert pf.tiff_write_device_masked(path, buf.data_ptr(), h, w, mb.data_ptr(), q, bg, xf, big, step, mstep, stream), pf.lib().pf_last_error()
    return open(path, "rb").read()


def host_masked(pf, path, a, m, q=95, bg=0, xf=None, big=False):
    assert pf.tiff_write_masked(path, a, m, q, bg, xf, big)
    return open(path, "rb").read()


def test_device_file_equals_host_file_sweep(pf, tmp_path):
    import torch
    rng = np.random.default_rng(20261018)
    shapes = SIZES + [(512, 1024)] + [tuple(int(v) for v in rng.integers(1, 700, 2)) for _ in range(12)]
    side = torch.cuda.Stream()
    d, h_ = str(tmp_path / "d.tif"), str(tmp_path / "h.tif")
    n = 0
    for (h, w) in shapes:
        for kind in (KINDS if (h, w) in SIZES or (h, w) == (512, 1024) else [KINDS[(h + w) % len(KINDS)], "random"]):
            n += 1
            q = (95, 30)[n % 2]; bg = (0, 255)[(n // 2) % 2]; big = n % 7 == 3; xf = XF if n % 2 else None
            a = model.content(h, w, ("noise", "smooth", "zero")[n % 3], n)
            m = make_mask(h, w, kind, n)
            want = host_masked(pf, h_, a, m, q, bg, xf, big)
            assert device_masked(pf, d, a, m, q, bg, xf, big) == want, ("packed", h, w, kind)
            if n % 3 == 0:
                assert device_masked(pf, d, a, m, q, bg, xf, big, step=3 * w + 1 + n % 29, mstep=w + 1 + n % 13) == want, ("padded steps", h, w, kind)
            if n % 3 == 1:
                assert device_masked(pf, d, a, m, q, bg, xf, big, step=3 * w + 16 - (3 * w) % 16, mstep=w + 16 - w % 16) == want, ("aligned padded steps", h, w, kind)
            if n % 5 == 0:
                assert device_masked(pf, d, a, m, q, bg, xf, big, stream=side.cuda_stream) == want, ("side stream", h, w, kind)
    # and the file is what the format says, not only what the host writer says; the unmasked device file is what it was
    a = model.content(600, 1100, "noise", 5); a[:, 700:] = 255
    m = make_mask(600, 1100, "disc", 5)
    got = mm.check_masked_file(device_masked(pf, d, a, m, 95, 255, XF), a, m, 255, encoder(pf, 95), XF)
    assert got["zero"] and got["one"] and got["own"]
    buf = torch.from_numpy(a).cuda()
    assert pf.tiff_write_device(d, buf.data_ptr(), 600, 1100, 95, 255, XF) and open(d, "rb").read() == host_file(pf, h_, a, 95, 255, XF)


def test_masked_device_writer_refuses_what_it_cannot_do(pf, tmp_path):
    import torch
    L = pf.lib()
    a = model.content(40, 56, "noise", 1)
    m = np.full((40, 56), 255, np.uint8)
    dev, dm = torch.from_numpy(a).cuda(), torch.from_numpy(m).cuda()
    f = str(tmp_path / "x.tif").encode()
    call = lambda name, img, rows, cols, step, mask, mstep: L.pf_tiff_write_device_masked(name, img, rows, cols, step, mask, mstep, 95, 0, None, 0, None)
    assert call(f, None, 40, 56, 0, dm.data_ptr(), 0) == 0
    assert call(f, dev.data_ptr(), 40, 56, 0, None, 0) == 0
    assert call(f, dev.data_ptr(), 0, 56, 0, dm.data_ptr(), 0) == 0
    assert call(f, dev.data_ptr(), 40, 56, 100, dm.data_ptr(), 0) == 0 and b"step" in L.pf_last_error()
    assert call(f, dev.data_ptr(), 40, 56, 0, dm.data_ptr(), 55) == 0 and b"step" in L.pf_last_error()
    assert call(f, a.ctypes.data, 40, 56, 0, dm.data_ptr(), 0) == 0 and b"device memory" in L.pf_last_error()
    assert call(f, dev.data_ptr(), 40, 56, 0, m.ctypes.data, 0) == 0 and b"device memory" in L.pf_last_error()
    assert not os.path.exists(f.decode())
    g = str(tmp_path / "missing" / "x.tif").encode()
    assert call(g, dev.data_ptr(), 40, 56, 0, dm.data_ptr(), 0) == 0 and b"cannot open" in L.pf_last_error()
    assert call(f, dev.data_ptr(), 40, 56, 0, dm.data_ptr(), 0) == 1


def oracle_mask(o, shape, org):
    """(w != 0) * 255 of the oracle's level-0 weights over the bounding box, zeros where it has no tile"""
    want = np.zeros(shape, np.uint8)
    for (ix, iy) in o.tiles():
        w = o.tile_level(ix, iy, 0)[1]
        want[(iy - org[1]) * 256:(iy - org[1] + 1) * 256, (ix - org[0]) * 256:(ix - org[0] + 1) * 256] = (w != 0) * 255
    return want


@pytest.mark.parametrize("ff,bg", [(0, 0), (1, 255), (0, 255), (1, 0)])
def test_map_mask_is_the_oracles_weights_and_the_file_the_host_writers(pf, orc, tmp_path, ff, bg):
    g, o = build_map(pf, orc, ff, 5, bg)
    ref, oorg = o.save()
    mem, mask, org = g.save_to_memory_mask()
    assert org == oorg and np.array_equal(mem, ref)
    want = oracle_mask(o, mem.shape[:2], org)
    assert np.array_equal(mask, want) and 0 < int((mask != 0).sum()) < mask.size
    assert np.array_equal(mem[mask == 0], np.full((int((mask == 0).sum()), 3), bg, np.uint8))          # what save() paints there
    # either half alone, once the extent is known
    import ctypes as C
    r, c, x0, y0 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    only = np.empty_like(mask)
    assert pf.lib().pf_save_to_memory_mask(g._h, None, only.ctypes.data, C.byref(r), C.byref(c), C.byref(x0), C.byref(y0)) and np.array_equal(only, want)
    only = np.empty_like(mem)
    assert pf.lib().pf_save_to_memory_mask(g._h, only.ctypes.data, None, C.byref(r), C.byref(c), C.byref(x0), C.byref(y0)) and np.array_equal(only, ref)
    assert (r.value, c.value, x0.value, y0.value) == mem.shape[:2] + org
    xf = transform_of(g, org)
    g.blend_changed()                                                     # clears Ischanged: what follows must not be touched by the save
    tiles = g.tiles()
    before = g.blend_tiles(tiles)
    f, h_ = str(tmp_path / "m.tif"), str(tmp_path / "h.tif")
    assert g.save_tiff_masked(f)
    data = open(f, "rb").read()
    assert data == host_masked(pf, h_, mem, mask, 95, bg, xf)
    mm.check_masked_file(data, mem, mask, bg, encoder(pf, 95), xf, big=False)
    assert g.save_tiff_masked(f, 30) and open(f, "rb").read() == host_masked(pf, h_, mem, mask, 30, bg, xf)
    assert g.save_tiff_masked(f, 95, True) and open(f, "rb").read() == host_masked(pf, h_, mem, mask, 95, bg, xf, True)
    # the map, its flags and the other saves are as before
    assert g.blend_changed()[0] == [] and np.array_equal(g.blend_tiles(tiles), before)
    again, org2 = g.save_to_memory()
    assert org2 == org and np.array_equal(again, ref)
    assert g.save(str(tmp_path / "u.tif")) and open(str(tmp_path / "u.tif"), "rb").read() == host_file(pf, h_, mem, 95, bg, xf)
    assert g.save(str(tmp_path / "u.jpg")) and open(str(tmp_path / "u.jpg"), "rb").read() == pf.jpeg_encode(mem, 95)
    assert not g.save_tiff_masked(str(tmp_path / "missing" / "x.tif"))
    g.close()


@pytest.mark.parametrize("bg", [0, 255])
def test_map_with_holes_points_at_the_shared_zero_tile_on_every_level(pf, tmp_path, bg):
    """two sorties far apart on a diagonal: the mosaic's bounding box has tile slots without a map tile"""
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    a = jitter_poses(3, seed=5)
    b = [[p[0] + 300.0, p[1] + 250.0] + list(p[2:]) for p in jitter_poses(3, seed=6)]
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, bg_color=bg)
    assert g.prepare(wl.IDENTITY_PLANE, cam, a)
    for k, p in enumerate(a + b):
        assert g.feed(wl.smooth_frame(480, 640, k) ^ (wl.noise_frame(480, 640, 300 + k) >> 3), p)
    mem, mask, org = g.save_to_memory_mask()
    have = {(ix - org[0], iy - org[1]) for ix, iy in g.tiles()}
    tx, ty = mem.shape[1] // 256, mem.shape[0] // 256
    assert tx * ty > len(have)                                            # holes
    xf = transform_of(g, org)
    f = str(tmp_path / "holes.tif")
    assert g.save_tiff_masked(f)
    data = open(f, "rb").read()
    assert data == host_masked(pf, str(tmp_path / "h.tif"), mem, mask, 95, bg, xf)
    got = mm.check_masked_file(data, mem, mask, bg, encoder(pf, 95), xf)
    _, ifds = tm.parse(data)
    masks = mm.mask_chain(mask)
    zero = {o for ifd, m in zip(ifds[1::2], masks) for o, t in zip(ifd["tags"][324][1], mm.mask_tiles_of(m)) if mm.kind_of(t) == "zero"}
    assert len(zero) == 1 and got["zero"] >= tx * ty - len(have)
    lv0 = ifds[1]["tags"][324][1]
    for y in range(ty):
        for x in range(tx):
            if (x, y) not in have:
                assert lv0[y * tx + x] in zero and not mask[y * 256:(y + 1) * 256, x * 256:(x + 1) * 256].any()
    assert sum(any(mm.kind_of(t) == "zero" for t in mm.mask_tiles_of(m)) for m in masks) >= 2          # ... on more than one level
    g.close()


def test_mask_covers_the_keyframes_that_still_wait(pf, orc, tmp_path):
    """default lookahead, no sync: keyframes are held back for the cull; the save drains them under its one hold of the map"""
    g, o = build_map(pf, orc, 0, 5)
    mem, mask, org = g.save_to_memory_mask()                              # no sync before
    ref, oorg = o.save()
    assert org == oorg and np.array_equal(mem, ref) and np.array_equal(mask, oracle_mask(o, mem.shape[:2], org))
    h, _ = build_map(pf, orc, 0, 5)
    f1, f2 = str(tmp_path / "waiting.tif"), str(tmp_path / "synced.tif")
    assert h.save_tiff_masked(f1)                                         # the file too, from a map that has not been drained yet
    assert h.sync() and h.save_tiff_masked(f2)
    assert open(f1, "rb").read() == open(f2, "rb").read() == host_masked(pf, str(tmp_path / "h.tif"), mem, mask, 95, 0, transform_of(g, org))
    g.close(); h.close()


def test_single_band_map_takes_the_host_route_with_alpha_as_coverage(pf, tmp_path):
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    poses = jitter_poses(4, seed=3)
    g = pf.Map2D.create(pf.TypeCPU, False)
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses)
    for k, p in enumerate(poses):
        assert g.feed(wl.smooth_frame(480, 640, k), p)
    mem, mask, org = g.save_to_memory_mask()
    plain, org2 = g.save_to_memory()
    assert org2 == org and np.array_equal(plain, mem)
    want = np.zeros(mem.shape[:2], np.uint8)
    for (ix, iy) in g.tiles():
        want[(iy - org[1]) * 256:(iy - org[1] + 1) * 256, (ix - org[0]) * 256:(ix - org[0] + 1) * 256] = (g.tile_bgra(ix, iy)[:, :, 3] != 0) * 255
    assert np.array_equal(mask, want) and 0 < int((mask != 0).sum()) < mask.size
    f = str(tmp_path / "s.tif")
    assert g.save_tiff_masked(f) and open(f, "rb").read() == host_masked(pf, str(tmp_path / "h.tif"), mem, want, 95, 0, transform_of(g, org))
    g.close()


def test_empty_map_returns_0(pf, tmp_path):
    wl = workloads()
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False)
    assert g.prepare(wl.IDENTITY_PLANE, [640, 480, 500, 500, 320, 240], jitter_poses(2, seed=1))
    f = str(tmp_path / "e.tif")
    assert not g.save_tiff_masked(f) and not os.path.exists(f) and g.save_to_memory_mask() is None
    g.close()


def test_save_tiff_masked_and_save_jpg_from_two_threads_keep_their_kinds(pf, orc, tmp_path):
    """one map, two callers: each file is what its own call asked for, every time (8 calls each, no more)"""
    import threading
    g, _ = build_map(pf, orc, 0, 5)
    a, b = str(tmp_path / "a.tif"), str(tmp_path / "b.jpg")
    assert g.save_tiff_masked(a)
    want = open(a, "rb").read()
    seen = {"a": [], "b": []}

    def tiffs():
        for _ in range(8):
            seen["a"].append((g.save_tiff_masked(a), open(a, "rb").read() == want))

    def jpegs():
        for _ in range(8):
            seen["b"].append((g.save(b), open(b, "rb").read(2)))

    th = [threading.Thread(target=tiffs), threading.Thread(target=jpegs)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not any(t.is_alive() for t in th)
    assert seen["a"] == [(True, True)] * 8
    assert seen["b"] == [(True, b"\xff\xd8")] * 8
    assert len(tm.parse(want)[1]) == 2 * len(tm.chain(np.zeros(g.save_to_memory()[0].shape, np.uint8)))
    g.close()
