"""The JPEG encoder on the GPU (csrc/jpeg_encode.hip) against the host encoder (csrc/jpeg_encode.hpp, itself pinned to libjpeg-turbo's bytes
by tests/test_jpeg_encode.py): byte-equal.  Then its three users: save("x.jpg") of a map and of a sharded map (the collapsed mosaic never
leaves HBM as pixels), and blend_tiles_jpeg (the tiles of a blend launch leave as independent streams)."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

import jpeg_encode_model as model
from helpers import jitter_poses, workloads
from test_jpeg_encode import vectors

pytestmark = pytest.mark.gpu


def on_device(pf, a, q, step=0, stream=None):
    import torch
    h, w = a.shape[:2]
    if step:
        buf = torch.full((h, step), 0x5A, dtype=torch.uint8, device="cuda")
        buf[:, :3 * w] = torch.from_numpy(np.ascontiguousarray(a).reshape(h, 3 * w)).cuda()
    else:
        buf = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return pf.jpeg_encode_device(buf.data_ptr(), h, w, q, step, stream)


def test_device_encode_equals_the_committed_streams(pf):
    for i, (h, w, kind, q, stream) in enumerate(vectors()):
        assert on_device(pf, model.content(h, w, kind, i), q) == stream, (h, w, kind, q)


def test_device_encode_equals_host_encode_sweep(pf):
    import torch
    rng = np.random.default_rng(20261016)
    kinds = ("noise", "smooth", "zero", "white", "steps")
    shapes = [tuple(int(v) for v in rng.integers(1, 71, 2)) for _ in range(60)] + [(256, 256), (480, 640), (768, 1024), (1024, 768), (3000, 4000)]
    side = torch.cuda.Stream()
    for n, (h, w) in enumerate(shapes):
        kind = kinds[n % len(kinds)] if h * w < 10 ** 6 else "noise"
        q = int(rng.choice([1, 25, 50, 75, 95, 100]))
        a = model.content(h, w, kind, n)
        want = pf.jpeg_encode(a, q)
        assert on_device(pf, a, q) == want, (h, w, kind, q)
        if n % 4 == 0:
            assert on_device(pf, a, q, step=3 * w + 1 + n % 29) == want, ("padded step", h, w, kind, q)
        if n % 5 == 0:
            assert on_device(pf, a, q, stream=side.cuda_stream) == want, ("side stream", h, w, kind, q)
    # quality is clamped as jpeg_set_quality clamps it
    a = model.content(33, 47, "noise", 5)
    assert on_device(pf, a, 0) == pf.jpeg_encode(a, 1) and on_device(pf, a, 1000) == pf.jpeg_encode(a, 100)


def test_device_encode_8192_noise_at_quality_100(pf):
    """the worst case for the stream's length and for stuffing: every code length, about one byte in 256 a 0xFF"""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    img = torch.randint(0, 256, (8192, 8192, 3), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    got = pf.jpeg_encode_device(img.data_ptr(), 8192, 8192, 100)
    want = pf.jpeg_encode(img.cpu().numpy(), 100)
    assert len(got) == len(want) and got == want
    assert got.count(b"\xff\x00") > 100000


def test_device_encode_refuses_what_it_cannot_do(pf):
    import torch
    L = pf.lib()
    a = model.content(40, 56, "noise", 1)
    dev = torch.from_numpy(a).cuda()
    want = pf.jpeg_encode(a, 95)
    n = C.c_size_t(0)
    out = np.full(len(want) + 8, 0xA5, np.uint8)
    assert L.pf_jpeg_encode_device(dev.data_ptr(), 40, 56, 0, 95, out.ctypes.data, len(want) - 1, C.byref(n), None) == 0
    assert b"bytes" in L.pf_last_error() and n.value == len(want) and (out == 0xA5).all()          # nothing written, the length reported
    assert L.pf_jpeg_encode_device(dev.data_ptr(), 40, 56, 0, 95, out.ctypes.data, len(want), C.byref(n), None) == 1
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
    assert L.pf_jpeg_encode_device(None, 40, 56, 0, 95, out.ctypes.data, out.size, C.byref(n), None) == 0
    assert L.pf_jpeg_encode_device(dev.data_ptr(), 0, 56, 0, 95, out.ctypes.data, out.size, C.byref(n), None) == 0
    assert L.pf_jpeg_encode_device(dev.data_ptr(), 40, 56, 100, 95, out.ctypes.data, out.size, C.byref(n), None) == 0           # step below a row
    assert L.pf_jpeg_encode_device(a.ctypes.data, 40, 56, 0, 95, out.ctypes.data, out.size, C.byref(n), None) == 0 and b"device memory" in L.pf_last_error()
    assert L.pf_jpeg_encode_device(dev.data_ptr(), 40, 65536, 0, 95, out.ctypes.data, out.size, C.byref(n), None) == 0 and b"65535" in L.pf_last_error()
    assert L.pf_jpeg_encode_device(dev.data_ptr(), 40, 56, 0, 95, None, 0, C.byref(n), None) == 1 and n.value >= len(want)           # the bound


def build_map(pf, orc, ff, bands, bg=0, n=5):
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    poses = jitter_poses(n, seed=12)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=ff, bg_color=bg, band_number=bands)
    o = orc.OracleMap(band_num=bands, force_float=ff, bg_color=bg)
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses) and o.prepare(wl.IDENTITY_PLANE, cam, poses)
    for k, p in enumerate(poses):
        img = wl.smooth_frame(480, 640, k) ^ (wl.noise_frame(480, 640, 300 + k) >> 3)
        assert g.feed(img, p) and o.feed(img, p)
    return g, o


@pytest.mark.parametrize("ff,bands,bg", [(0, 5, 0), (1, 5, 255), (0, 0, 255), (1, 0, 0)])
def test_save_jpg_is_the_host_encoding_of_the_mosaic(pf, orc, tmp_path, ff, bands, bg):
    """save("m.jpg") == pf_jpeg_encode_bgr(save_to_memory, 95); the other extensions and the map itself are as they were"""
    from PIL import Image
    g, o = build_map(pf, orc, ff, bands, bg)
    ref, oorg = o.save()
    mem, org = g.save_to_memory()
    assert org == oorg and np.array_equal(mem, ref)
    g.blend_changed()                                                     # clears Ischanged: what follows must not be touched by the save
    tiles = g.tiles()
    before = g.blend_tiles(tiles)
    for name in ("m.jpg", "m.JPEG"):
        f = str(tmp_path / name)
        assert g.save(f)
        assert open(f, "rb").read() == pf.jpeg_encode(mem, 95), name
    assert np.array_equal(pf.read_image(str(tmp_path / "m.jpg")), np.asarray(Image.open(str(tmp_path / "m.jpg")).convert("RGB"))[:, :, ::-1])
    assert g.blend_changed()[0] == [] and np.array_equal(g.blend_tiles(tiles), before)
    again, org2 = g.save_to_memory()
    assert org2 == org and np.array_equal(again, ref)
    for ext in (".png", ".ppm"):
        f = str(tmp_path / ("m" + ext))
        assert g.save(f)
        assert np.array_equal(np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1], ref)
    assert not g.save(str(tmp_path / "missing" / "x.jpg"))
    g.close()


def test_single_band_map_saves_jpg_through_the_host_encoder(pf, tmp_path):
    wl = workloads()
    cam = [640, 480, 500, 500, 320, 240]
    poses = jitter_poses(4, seed=3)
    g = pf.Map2D.create(pf.TypeCPU, False)
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses)
    for k, p in enumerate(poses):
        assert g.feed(wl.smooth_frame(480, 640, k), p)
    mem, _ = g.save_to_memory()
    f = str(tmp_path / "single.jpg")
    assert g.save(f) and open(f, "rb").read() == pf.jpeg_encode(mem, 95)
    t = g.tiles()[0]
    assert g.blend_tiles_jpeg([t, (t[0] - 50, t[1])], 80) == [pf.jpeg_encode(g.blend_tile(*t), 80), b""]
    g.close()


def test_dist_save_jpg_on_rank_0_equals_the_unsharded_file(pf, orc, tmp_path):
    from test_gpu_dist import Rendezvous, collective, workload
    sh = importlib.import_module("pi_slam_fusion_amd.sharding")
    wl = workloads()
    cam, poses, frames = workload(wl)
    world = 2
    whole = pf.Map2D.create(pf.TypeMultiBandCPU, False, scale=2.0)
    maps = [pf.Map2D.create(pf.TypeMultiBandCPU, False, scale=2.0, shard_rank=r, shard_count=world, shard_block=1) for r in range(world)]
    for m in maps + [whole]:
        assert m.prepare(wl.IDENTITY_PLANE, cam, poses[:2])
        for f, p in zip(frames, poses):
            assert m.feed(f, p)
    rv = Rendezvous(world)
    dms = [sh.DistMap(m, r, world, backend="host", exchange=rv.fn(r)) for r, m in enumerate(maps)]
    names = [str(tmp_path / ("rank%d.jpg" % r)) for r in range(world)]
    assert collective(world, rv, lambda r: dms[r].save(names[r])) == [True] * world
    one = str(tmp_path / "whole.jpg")
    assert whole.save(one)
    import os
    assert open(names[0], "rb").read() == open(one, "rb").read() == pf.jpeg_encode(whole.save_to_memory()[0], 95)
    assert not os.path.exists(names[1])                                   # the other ranks hold no picture
    for d in dms:
        d.close()
    for m in maps + [whole]:
        m.close()


def test_blend_tiles_jpeg_streams_are_the_host_encodings_of_the_tiles(pf, orc):
    g, o = build_map(pf, orc, 0, 5)
    tiles = g.tiles()
    gone = (min(t[0] for t in tiles) - 3, tiles[0][1])
    ask = tiles[:2] + [gone] + tiles[2:] + [gone, tiles[0]]
    px = g.blend_tiles(ask)
    for q in (95, 30):
        streams = g.blend_tiles_jpeg(ask, q)
        assert len(streams) == len(ask)
        for t, s, im in zip(ask, streams, px):
            assert s == (b"" if t == gone else pf.jpeg_encode(im, q)), (t, q)
    assert np.array_equal(px[0], o.blend_tile(*ask[0]))
    # offsets are monotone and end inside the buffer; a buffer one byte short is refused and left alone past its end
    L = pf.lib(); n = len(ask)
    xy = (C.c_int * (2 * n))(*[v for t in ask for v in t])
    total = sum(len(s) for s in streams)
    out = np.full(total + 4, 0xA5, np.uint8); off = (C.c_size_t * (n + 1))()
    assert L.pf_blend_tiles_jpeg(g._h, xy, n, 30, out.ctypes.data, total, off) == 1
    o_ = list(off)
    assert o_[0] == 0 and all(a <= b for a, b in zip(o_, o_[1:])) and o_[n] == total and (out[total:] == 0xA5).all()
    assert out[:total].tobytes() == b"".join(streams)
    out[:] = 0xA5
    assert L.pf_blend_tiles_jpeg(g._h, xy, n, 30, out.ctypes.data, total - 1, off) == 0 and b"buffer" in L.pf_last_error()
    assert (out[total - 1:] == 0xA5).all()
    assert g.blend_changed()[0] != []                                     # Ischanged was left alone, as blend_tiles leaves it
    g.close()


def test_blend_tiles_jpeg_across_the_blend_launch_boundary(pf, orc):
    """more tiles than one blend launch takes (4096): the second launch's streams follow the first's"""
    g, _ = build_map(pf, orc, 0, 5, n=3)
    tiles = g.tiles()
    gone = (min(t[0] for t in tiles) - 3, tiles[0][1])
    ask = [tiles[i % len(tiles)] if i % 97 else gone for i in range(4096 + 37)]
    streams = g.blend_tiles_jpeg(ask, 40)
    assert streams is not None and len(streams) == len(ask)
    want = {t: pf.jpeg_encode(im, 40) for t, im in zip(tiles, g.blend_tiles(tiles))}
    want[gone] = b""
    bad = [i for i, (t, s) in enumerate(zip(ask, streams)) if s != want[t]]
    assert not bad, bad[:10]
    g.close()
