"""The lossless tile codec and the lossless pyramid TIFF made on the GPU (csrc/deflate_encode.hip behind overview.hip) against the host
encoder and writer (csrc/deflate_rle.hpp, tiff_pyramid.hpp; themselves pinned to the format by tests/test_tiff_lossless.py): byte-equal
streams and files.  Tiles alone, in a batch, as windows of one image, across the driver's batch size; images of any size with padded rows,
masks and a caller's stream; then the map: save_tiff_lossless against the host writer of save_to_memory's pixels, holes, a single-band
map, thread-ranks, a failed save, two threads."""
import importlib
import os
import zlib

import numpy as np
import pytest

import deflate_model as dm
import jpeg_encode_model as model
import tiff_model as tm
from helpers import jitter_poses, workloads
from test_gpu_jpeg_encode import build_map
from test_gpu_tiff import host_file, transform_of
from test_tiff import XF
from test_tiff_mask import make_mask

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (255, 257), (256, 256), (300, 1030), (513, 700)]


@pytest.fixture(scope="module")
def hostile(pf):
    tiles = dm.hostile_tiles()
    return tiles, {k: pf.deflate_tile(v) for k, v in tiles.items()}


def test_device_streams_equal_host_streams(pf, hostile):
    import torch
    tiles, want = hostile
    names = sorted(tiles)
    # alone
    for k in names:
        buf = torch.from_numpy(tiles[k]).cuda()
        assert pf.deflate_tiles_device(buf.data_ptr(), [0], 768) == [want[k]], k
    # in one batch: the tiles back to back in one allocation, in an order that is not the allocation's
    buf = torch.from_numpy(np.stack([tiles[k] for k in names])).cuda()
    order = list(range(len(names)))[::-1]
    got = pf.deflate_tiles_device(buf.data_ptr(), [i * dm.N for i in order], 768)
    assert got == [want[names[i]] for i in order]
    # as windows of one padded image: tiles side by side, rows of 768 * n + 13 bytes
    step = 768 * len(names) + 13
    img = np.full((256, step), 0x5A, np.uint8)
    for i, k in enumerate(names):
        img[:, 768 * i:768 * (i + 1)] = tiles[k].reshape(256, 768)
    buf = torch.from_numpy(img).cuda()
    side = torch.cuda.Stream()
    got = pf.deflate_tiles_device(buf.data_ptr(), [768 * i for i in range(len(names))], step, side.cuda_stream)
    assert got == [want[k] for k in names]
    for s, k in zip(got, names):
        assert zlib.decompress(s) == dm.predict(tiles[k]).tobytes() and len(s) <= dm.BOUND


def test_strip_of_513_tiles_crosses_the_drivers_batch(pf, hostile, tmp_path):
    import torch
    tiles, _ = hostile
    names = sorted(tiles)
    a = np.concatenate([tiles[names[i % len(names)]] for i in range(513)], axis=1)          # 256 x 131 328
    a[:, 256 * 100:256 * 103] = 0                                                             # empty tiles inside the first batch
    buf = torch.from_numpy(a).cuda()
    d, h = str(tmp_path / "d.tif"), str(tmp_path / "h.tif")
    assert pf.tiff_write_lossless(h, a)
    assert pf.tiff_write_device_lossless(d, buf.data_ptr(), 256, a.shape[1]), pf.lib().pf_last_error()
    assert open(d, "rb").read() == open(h, "rb").read()


def device_lossless(pf, path, a, m=None, bg=0, xf=None, big=False, step=0, mstep=0, stream=None):
    import torch
    h, w = a.shape[:2]
    if step:
        buf = torch.full((h, step), 0x5A, dtype=torch.uint8, device="cuda")
        buf[:, :3 * w] = torch.from_numpy(np.ascontiguousarray(a).reshape(h, 3 * w)).cuda()
    else:
        buf = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    mb = None
    if m is not None:
        if mstep:
            mb = torch.full((h, mstep), 0xC3, dtype=torch.uint8, device="cuda")
            mb[:, :w] = torch.from_numpy(np.ascontiguousarray(m)).cuda()
        else:
            mb = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    torch.cuda.synchronize()
    assert pf.tiff_write_device_lossless(path, buf.data_ptr(), h, w, None if mb is None else mb.data_ptr(), bg, xf, big, step, mstep, stream), pf.lib().pf_last_error()
    return open(path, "rb").read()


def host_lossless(pf, path, a, m=None, bg=0, xf=None, big=False):
    assert pf.tiff_write_lossless(path, a, m, bg, xf, big)
    return open(path, "rb").read()


def test_device_file_equals_host_file(pf, tmp_path):
    import torch
    side = torch.cuda.Stream()
    d, h_ = str(tmp_path / "d.tif"), str(tmp_path / "h.tif")
    n = 0
    for (h, w) in SHAPES:
        for kind in ("noise", "smooth", "zero"):
            n += 1
            bg = (0, 255)[n % 2]; big = n % 5 == 3; xf = XF if n % 2 else None
            a = model.content(h, w, kind, n)
            if n % 3 == 0 and w > 300:
                a[:, w // 2:] = bg
            for m in (None, make_mask(h, w, ("disc", "random", "all", "none")[n % 4], n)):
                want = host_lossless(pf, h_, a, m, bg, xf, big)
                assert device_lossless(pf, d, a, m, bg, xf, big) == want, ("packed", h, w, kind, m is not None)
                assert device_lossless(pf, d, a, m, bg, xf, big, step=3 * w + 1 + n % 29, mstep=w + 1 + n % 13) == want, ("padded", h, w, kind)
            assert device_lossless(pf, d, a, m, bg, xf, big, stream=side.cuda_stream) == want, ("side stream", h, w, kind)
    # the process-wide writer's counts: all tiles, and as empty the model's background tiles of every level
    a = model.content(513, 700, "noise", 9); a[:, 256:] = 255
    device_lossless(pf, d, a, None, 255)
    empties = [tm.is_empty(t, 255) for lv in tm.chain(a) for t in tm.tiles_of(lv)]
    assert pf.tiff_counts()[:2] == (len(empties), sum(empties)) and 0 < sum(empties) < len(empties)
    # the JPEG file of the same call sequence is what it was
    a = model.content(300, 1030, "smooth", 2)
    buf = torch.from_numpy(a).cuda()
    assert pf.tiff_write_device(d, buf.data_ptr(), 300, 1030, 95, 0, XF) and open(d, "rb").read() == host_file(pf, h_, a, 95, 0, XF)


def pillow_page0(path):
    from PIL import Image
    im = Image.open(path)
    im.seek(0)
    return np.asarray(im.convert("RGB"))[:, :, ::-1]


@pytest.mark.parametrize("ff,bands,bg", [(0, 5, 0), (1, 5, 255), (0, 0, 255), (1, 0, 0)])
def test_save_tiff_lossless_is_the_host_file_of_the_mosaic(pf, orc, tmp_path, ff, bands, bg):
    g, o = build_map(pf, orc, ff, bands, bg)
    ref, oorg = o.save()
    mem, mask, org = g.save_to_memory_mask()
    assert org == oorg and np.array_equal(mem, ref)
    xf = transform_of(g, org)
    f, h_ = str(tmp_path / "m.tif"), str(tmp_path / "h.tif")
    assert g.save_tiff_lossless(f)
    assert open(f, "rb").read() == host_lossless(pf, h_, mem, None, bg, xf)
    assert np.array_equal(pillow_page0(f), ref)                            # exact pixels, through an independent reader
    assert g.save_tiff_lossless(f, True) and open(f, "rb").read() == host_lossless(pf, h_, mem, mask, bg, xf)
    assert g.save_tiff_lossless(f, False, True) and open(f, "rb").read() == host_lossless(pf, h_, mem, None, bg, xf, True)
    # the other saves are what they were
    assert g.save(str(tmp_path / "u.tif")) and open(str(tmp_path / "u.tif"), "rb").read() == host_file(pf, h_, mem, 95, bg, xf)
    assert g.save(str(tmp_path / "u.jpg")) and open(str(tmp_path / "u.jpg"), "rb").read() == pf.jpeg_encode(mem, 95)
    g.close()


@pytest.mark.parametrize("bg", [0, 255])
def test_map_with_holes_points_every_empty_tile_at_one_stream(pf, tmp_path, bg):
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    a = jitter_poses(3, seed=5)
    b = [[p[0] + 300.0, p[1] + 250.0] + list(p[2:]) for p in jitter_poses(3, seed=6)]
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, bg_color=bg)
    assert g.prepare(wl.IDENTITY_PLANE, cam, a)
    for k, p in enumerate(a + b):
        assert g.feed(wl.smooth_frame(480, 640, k) ^ (wl.noise_frame(480, 640, 300 + k) >> 3), p)
    mem, org = g.save_to_memory()
    slots = (mem.shape[0] // 256) * (mem.shape[1] // 256)
    assert slots > len(g.tiles())
    f = str(tmp_path / "holes.tif")
    assert g.save_tiff_lossless(f)
    data = open(f, "rb").read()
    assert data == host_lossless(pf, str(tmp_path / "h.tif"), mem, None, bg, transform_of(g, org))
    _, ifds = tm.parse(data)
    empties = [[tm.is_empty(t, bg) for t in tm.tiles_of(lv)] for lv in tm.chain(mem)]
    assert sum(any(e) for e in empties) >= 2 and sum(sum(e) for e in empties) >= slots - len(g.tiles())
    shared = {s for lv, ifd in zip(empties, ifds) for e, s in zip(lv, tm.tile_streams(data, ifd)) if e}
    assert len(shared) == 1
    # what the device path counted: every tile of every level, and as empty exactly the model's background tiles (none was encoded)
    n_tiles, n_empty, dev_bytes = pf.tiff_counts(g)
    assert n_tiles == sum(len(e) for e in empties) == sum(len(tm.tile_streams(data, ifd)) for ifd in ifds)
    assert n_empty == sum(sum(e) for e in empties) and dev_bytes > 0
    off, n = list(shared)[0]
    assert data[off:off + n] == pf.deflate_tile(np.full((256, 256, 3), bg, np.uint8))
    g.close()


def test_single_band_map_writes_the_host_file(pf, tmp_path):
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    poses = jitter_poses(4, seed=3)
    g = pf.Map2D.create(pf.TypeCPU, False)
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses)
    for k, p in enumerate(poses):
        assert g.feed(wl.smooth_frame(480, 640, k), p)
    mem, mask, org = g.save_to_memory_mask()
    f, h_ = str(tmp_path / "s.tif"), str(tmp_path / "h.tif")
    xf = transform_of(g, org)
    assert g.save_tiff_lossless(f) and open(f, "rb").read() == host_lossless(pf, h_, mem, None, 0, xf)
    assert g.save_tiff_lossless(f, True) and open(f, "rb").read() == host_lossless(pf, h_, mem, mask, 0, xf)
    g.close()


def test_three_thread_ranks_rank_0_writes_the_unsharded_file(pf, orc, tmp_path):
    from test_gpu_dist import Rendezvous, collective, workload
    sh = importlib.import_module("pi_slam_fusion_amd.sharding")
    wl = workloads()
    cam, poses, frames = workload(wl)
    world = 3
    whole = pf.Map2D.create(pf.TypeMultiBandCPU, False, scale=2.0)
    maps = [pf.Map2D.create(pf.TypeMultiBandCPU, False, scale=2.0, shard_rank=r, shard_count=world, shard_block=1) for r in range(world)]
    for m in maps + [whole]:
        assert m.prepare(wl.IDENTITY_PLANE, cam, poses[:2])
        for f, p in zip(frames, poses):
            assert m.feed(f, p)
    rv = Rendezvous(world)
    dms = [sh.DistMap(m, r, world, backend="host", exchange=rv.fn(r)) for r, m in enumerate(maps)]
    names = [str(tmp_path / ("rank%d.tif" % r)) for r in range(world)]
    assert collective(world, rv, lambda r: dms[r].save_tiff_lossless(names[r])) == [True] * world
    one = str(tmp_path / "whole.tif")
    assert whole.save_tiff_lossless(one)
    mem, org = whole.save_to_memory()
    assert open(names[0], "rb").read() == open(one, "rb").read() == host_lossless(pf, str(tmp_path / "h.tif"), mem, None, 0, transform_of(whole, org))
    assert not os.path.exists(names[1]) and not os.path.exists(names[2])
    for d in dms:
        d.close()
    for m in maps + [whole]:
        m.close()


def test_unwritable_path_returns_0_and_the_next_saves_are_right(pf, orc, tmp_path):
    g, _ = build_map(pf, orc, 0, 5)
    bad = str(tmp_path / "missing" / "x.tif")
    assert not g.save_tiff_lossless(bad) and not os.path.exists(bad)
    mem, org = g.save_to_memory()
    f = str(tmp_path / "x.tif")
    assert g.save_tiff_lossless(f) and open(f, "rb").read() == host_lossless(pf, str(tmp_path / "h.tif"), mem, None, 0, transform_of(g, org))
    j = str(tmp_path / "x.jpg")
    assert g.save(j) and open(j, "rb").read() == pf.jpeg_encode(mem, 95)
    assert g.save(f) and open(f, "rb").read() == host_file(pf, str(tmp_path / "h.tif"), mem, 95, 0, transform_of(g, org))
    g.close()


def test_lossless_save_and_jpg_save_from_two_threads_keep_their_formats(pf, orc, tmp_path):
    """one map, two callers: each file is what its own call asked for, every time (6 calls each, no more)"""
    import threading
    g, _ = build_map(pf, orc, 0, 5)
    a, b = str(tmp_path / "a.tif"), str(tmp_path / "b.jpg")
    assert g.save_tiff_lossless(a)
    want = open(a, "rb").read()
    seen = {"a": [], "b": []}

    def tiffs():
        for _ in range(6):
            seen["a"].append((g.save_tiff_lossless(a), open(a, "rb").read() == want))

    def jpegs():
        for _ in range(6):
            seen["b"].append((g.save(b), open(b, "rb").read(2)))

    th = [threading.Thread(target=tiffs), threading.Thread(target=jpegs)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not any(t.is_alive() for t in th)
    assert seen["a"] == [(True, True)] * 6
    assert seen["b"] == [(True, b"\xff\xd8")] * 6
    g.close()
