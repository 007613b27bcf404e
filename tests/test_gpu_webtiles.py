"""North-up Web-Mercator map tiles made on the GPU (csrc/webtiles.hip: the sampler, the 2 x 2 reduction, the pyramid driver; the encoder
of jpeg_encode.hip on the tiles where they lie) against the numpy model of tests/webtiles_model.py fed the library's own tables: pixels,
masks, cover classes, the set of tiles and every JPEG stream, byte for byte.  First for images and masks of any size in device memory
(pf_webtiles_device), then the orientation by the OSM formula alone, then the map (pf_webtiles) and the files (pf_save_webtiles,
export_mbtiles)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import jpeg_encode_model as model
import webtiles_model as wm
from helpers import jitter_poses, workloads
from test_gpu_jpeg_encode import build_map
from test_gpu_tiff import transform_of
from test_tiff_mask import KINDS, make_mask

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (40, 56), (257, 255), (300, 520)]
# (latitude, yaw, rows running northwards): near the equator north-up, two yaws, rows to the north, latitude 60
GEOREFS = [(0.3, 0.0, False), (40.0, 30.0, False), (40.0, 205.0, False), (-33.0, 10.0, True), (60.0, 75.0, False)]
SCALES = [0.3, 0.71, 1.0, 1.41, 3.0]          # output pixels per source pixel: minified ... magnified
Z = 20
ORIGIN = (13.405, 52.52, 40.0)


def on_device(pf, a, m, p, zmin, zmax, q=95, bg=0, pixels=True, step=0, mstep=0, stream=None):
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
    return pf.webtiles_device(buf.data_ptr(), h, w, mb.data_ptr(), p, zmin, zmax, q, bg, pixels, step, mstep, stream)


def keyed(recs):
    recs = list(recs)
    out = {(t["z"], t["x"], t["y"]): t for t in recs}
    assert len(out) == len(recs)          # no tile twice
    return out


def model_of(pf, a, m, p, zmin, zmax, bg):
    rg, ux, uy, vx, vy = pf.webtiles_plan(p, a.shape[0], a.shape[1], zmax)
    return wm.pyramid(a, m, rg, ux, uy, vx, vy, zmin, zmax, bg), rg


def check(pf, recs, want, q=None, what=""):
    got = keyed(recs)
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want))[:8])
    for k, (px, cov) in want.items():
        t = got[k]
        assert t["cover"] == wm.cover_class(cov), (what, k)
        assert (t["mask"] is None) == bool(cov.all()) and (t["mask"] is None or np.array_equal(t["mask"], cov)), (what, k)
        if "bgr" in t:
            assert np.array_equal(t["bgr"], px), (what, k, int((t["bgr"] != px).sum()))
        if q is not None:
            assert t["jpeg"] == pf.jpeg_encode(px, q), (what, k)


@pytest.mark.parametrize("si", range(len(SIZES)))
def test_sampled_tiles_equal_the_model(pf, si):
    """zmax alone: every (georeference, scale) pair, every mask kind, both backgrounds, padded steps and a side stream on a third each"""
    import torch
    h, w = SIZES[si]
    side = torch.cuda.Stream()
    emitted = 0
    for ki, kind in enumerate(KINDS):
        n = len(KINDS) * si + ki
        lat, yaw, north = GEOREFS[(n % 25) % 5]; scale = SCALES[(n % 25) // 5]
        bg = (0, 255)[n % 2]
        a = model.content(h, w, ("noise", "smooth")[n % 2], n)
        m = make_mask(h, w, kind, n)
        p = wm.make_px2ll(13.0 + 0.37 * n, lat, h, w, Z, scale, yaw, north)
        want, rg = model_of(pf, a, m, p, Z, Z, bg)
        kw = {}
        if n % 3 == 0:
            kw = dict(step=3 * w + 1 + n % 29, mstep=w + 1 + n % 13)
        if n % 3 == 1:
            kw = dict(stream=side.cuda_stream)
        check(pf, on_device(pf, a, m, p, Z, Z, 95, bg, **kw), want, what=(h, w, kind, lat, yaw, north, scale, bg, sorted(kw)))
        if kind == "none":
            assert not want
        emitted += len(want)
    assert emitted > 0 or (h, w) == (1, 1)


def test_one_pixel_is_found_when_magnified(pf):
    a = np.full((1, 1, 3), 200, np.uint8); m = np.ones((1, 1), np.uint8)
    p = wm.make_px2ll(13.0, 0.3, 1, 1, Z, 3.0)
    want, _ = model_of(pf, a, m, p, Z, Z, 0)
    assert want and 4 <= sum(int(c.sum()) for _, c in want.values()) <= 16          # a pixel of 3 x 3 output pixels, its half-weight rim included
    check(pf, on_device(pf, a, m, p, Z, Z), want)


@pytest.mark.parametrize("case", ["small_q95", "large_q30_batches"])
def test_pyramid_down_to_zoom_0_equals_the_model(pf, case):
    L = pf.lib()
    if case == "small_q95":
        h, w, q, bg = 40, 56, 95, 0
        a = model.content(h, w, "smooth", 3); m = make_mask(h, w, "disc", 1)
        p = wm.make_px2ll(13.405, 52.52, h, w, Z, 1.0, 205.0)
    else:
        h, w, q, bg = 300, 520, 30, 255
        a = model.content(h, w, "noise", 4); m = make_mask(h, w, "disc", 2)
        p = wm.make_px2ll(-70.6, -33.0, h, w, Z, 3.0, 30.0, True)
    want, rg = model_of(pf, a, m, p, 0, Z, bg)
    recs = on_device(pf, a, m, p, 0, Z, q, bg)
    check(pf, recs, want, q, case)
    # low zooms: the image has shrunk to a single covered pixel of the one tile
    assert (0, 0, 0) in want and int(want[(0, 0, 0)][1].sum()) == 1 and keyed(recs)[(0, 0, 0)]["cover"] == 1
    assert all(sum(1 for k in want if k[0] == z) == 1 for z in range(0, 8))
    if case != "small_q95":
        # tiles of the range whose pixels are all uncovered are absent, at zmax and above it
        in_range = (rg[2] - rg[0] + 1) * (rg[3] - rg[1] + 1)
        at_zmax = sum(1 for k in want if k[0] == Z)
        assert in_range >= 30 and 0 < at_zmax < in_range
        # a batch of 2 x 2 tiles: many groups, many ancestors carried on -- and the same result
        assert L.pf_debug_webtiles_batch(2) == 2
        try:
            small = on_device(pf, a, m, p, 0, Z, q, bg)
        finally:
            assert L.pf_debug_webtiles_batch(8) == 8
        a_, b_ = keyed(recs), keyed(small)
        assert set(a_) == set(b_)
        for k in a_:
            assert a_[k]["jpeg"] == b_[k]["jpeg"] and a_[k]["cover"] == b_[k]["cover"] and np.array_equal(a_[k]["bgr"], b_[k]["bgr"]), k
            assert (a_[k]["mask"] is None) == (b_[k]["mask"] is None) and (a_[k]["mask"] is None or np.array_equal(a_[k]["mask"], b_[k]["mask"])), k
        # zmin of its own: the first zoom at which one tile holds the range; zmax of its own: the native zoom
        auto = keyed(on_device(pf, a, m, p, None, None, q, bg, pixels=False))
        nz = pf.webtiles_native_zoom(p, h, w)
        assert nz == Z - 2 and max(k[0] for k in auto) == nz
        rgn = pf.webtiles_plan(p, h, w, nz)[0]
        assert min(k[0] for k in auto) == wm.default_zmin(rgn, nz)


def mosaic_of(recs, z):
    """the tiles of zoom z pasted together: (pixels, covered, global pixel of the top-left corner)"""
    t = {k: v for k, v in keyed(recs).items() if k[0] == z}
    x0, y0 = min(k[1] for k in t), min(k[2] for k in t)
    x1, y1 = max(k[1] for k in t), max(k[2] for k in t)
    px = np.zeros(((y1 - y0 + 1) * 256, (x1 - x0 + 1) * 256, 3), np.uint8); cov = np.zeros(px.shape[:2], bool)
    for (_, x, y), r in t.items():
        px[(y - y0) * 256:(y - y0 + 1) * 256, (x - x0) * 256:(x - x0 + 1) * 256] = r["bgr"]
        cov[(y - y0) * 256:(y - y0 + 1) * 256, (x - x0) * 256:(x - x0 + 1) * 256] = True if r["mask"] is None else r["mask"]
    return px, cov, (256 * x0, 256 * y0)


@pytest.mark.parametrize("lat,yaw", [(40.0, 30.0), (-33.0, 205.0), (60.0, 0.0)])
def test_orientation_by_the_osm_formula_alone(pf, lat, yaw):
    """a bright blob at a known source pixel: where the OSM formula puts its longitude and latitude, the brightest output pixel lies --
    and with the rows of the SAME ground running northwards (image flipped, georeference flipped) the tiles do not mirror"""
    h, w, r0, c0 = 200, 300, 50, 220
    a = np.zeros((h, w, 3), np.uint8)
    a[:, :, 1] = (np.mgrid[0:h, 0:w][1] // 4).astype(np.uint8)          # a gentle ramp to the east of the image, well below the blob
    a[r0 - 1:r0 + 2, c0 - 1:c0 + 2] = 150; a[r0, c0] = 255
    m = np.ones((h, w), np.uint8)
    out = []
    for north in (False, True):
        p = wm.make_px2ll(13.405, lat, h, w, Z, 1.0, yaw, north)
        img = a[::-1] if north else a
        rr = h - 1 - r0 if north else r0
        lng = p[0] + p[1] * (c0 + 0.5) + p[2] * (rr + 0.5); la = p[3] + p[4] * (c0 + 0.5) + p[5] * (rr + 0.5)
        n = 256.0 * 2 ** Z
        gx = (lng + 180.0) / 360.0 * n
        gy = (1.0 - math.log(math.tan(math.radians(la)) + 1.0 / math.cos(math.radians(la))) / math.pi) / 2.0 * n
        px, cov, (ox, oy) = mosaic_of(on_device(pf, img, m, p, Z, Z), Z)
        y, x = np.unravel_index(int(px.astype(np.int64).sum(2).argmax()), px.shape[:2])
        assert abs(ox + x + 0.5 - gx) <= 1.0 and abs(oy + y + 0.5 - gy) <= 1.0, (north, ox + x, oy + y, gx, gy)
        # north is up: the blob lies north-east or north-west of the image centre as the yaw says, never mirrored
        cx, cy = wm.global_pixel(13.405, lat, Z)
        e = (c0 + 0.5 - w / 2.0) * math.cos(math.radians(yaw)) + (r0 + 0.5 - h / 2.0) * math.sin(math.radians(yaw))          # metres east / gsd
        nn = (c0 + 0.5 - w / 2.0) * math.sin(math.radians(yaw)) - (r0 + 0.5 - h / 2.0) * math.cos(math.radians(yaw))         # metres north / gsd
        assert abs((gx - cx) - e) < 1.5 and abs((cy - gy) - nn) < 1.5
        out.append((px, cov, ox, oy))
    (pa, ca, oxa, oya), (pb, cb, oxb, oyb) = out
    assert (oxa, oya, pa.shape) == (oxb, oyb, pb.shape)
    both = ca & cb
    assert both.sum() > 0.95 * max(ca.sum(), cb.sum())
    # the same ground sampled through mirrored fractions: weights differ by at most 1 / 256 per axis, below 3 grey levels with the rounding
    assert int(np.abs(pa.astype(np.int64) - pb.astype(np.int64))[both].max()) <= 3


# ---------------------------------------------------------------- the map
def check_map(pf, g, bg, q=95, recs=None):
    mem, mask, org = g.save_to_memory_mask()
    p, rows, cols = g.webtiles_georef(ORIGIN)
    assert (rows, cols) == mem.shape[:2]
    assert np.allclose(p, pf.webtiles_georef_compose(transform_of(g, org), workloads().IDENTITY_PLANE, ORIGIN), rtol=1e-12, atol=0)
    zmax = pf.webtiles_native_zoom(p, rows, cols)
    rg = pf.webtiles_plan(p, rows, cols, zmax)[0]
    zmin = wm.default_zmin(rg, zmax)
    want, _ = model_of(pf, mem, mask, p, zmin, zmax, bg)
    if recs is None:
        recs = list(g.webtiles(ORIGIN, quality=q, pixels=True))
    check(pf, recs, want, q)
    assert 0 <= zmin <= zmax and sum(1 for k in want if k[0] == zmin) == 1 and len(want) >= 3
    return recs, want


@pytest.mark.parametrize("ff,bg", [(0, 0), (1, 255)])
def test_map_tiles_are_the_model_of_its_mosaic_and_mask(pf, orc, ff, bg):
    g, _ = build_map(pf, orc, ff, 5, bg)
    g.blend_changed()
    tiles = g.tiles(); before = g.blend_tiles(tiles)
    recs, want = check_map(pf, g, bg, (95, 30)[ff])
    assert any(t["cover"] == 1 for t in recs)
    # explicit zooms; the map and its flags are as they were
    zs = sorted({k[0] for k in want})
    sub = keyed(g.webtiles(ORIGIN, zmin=zs[-1] - 1, zmax=zs[-1], quality=(95, 30)[ff]))
    assert set(sub) == {k for k in want if k[0] >= zs[-1] - 1} and all(sub[k]["jpeg"] == keyed(recs)[k]["jpeg"] for k in sub)
    assert g.blend_changed()[0] == [] and np.array_equal(g.blend_tiles(tiles), before)
    g.close()


def test_map_with_holes_leaves_the_absent_slots_uncovered(pf):
    import pyramid_inject as pi
    g, _ = pi.build(pf, 5, 0, "holes", "view", "half", 3)
    mem, mask, org = g.save_to_memory_mask()
    have = {(ix - org[0], iy - org[1]) for ix, iy in g.tiles()}
    assert (mem.shape[0] // 256) * (mem.shape[1] // 256) > len(have)
    check_map(pf, g, pi.BG)
    g.close()


def test_waiting_keyframes_are_in_the_tiles(pf, orc):
    """default lookahead, no sync: the export drains the window under its one hold of the map"""
    g, _ = build_map(pf, orc, 0, 5)
    waiting = list(g.webtiles(ORIGIN, pixels=True))          # nothing read before
    h, _ = build_map(pf, orc, 0, 5)
    assert h.sync()
    synced = keyed(h.webtiles(ORIGIN, pixels=True))
    w = keyed(waiting)
    assert set(w) == set(synced) and all(w[k]["jpeg"] == synced[k]["jpeg"] and np.array_equal(w[k]["bgr"], synced[k]["bgr"]) for k in w)
    check_map(pf, g, 0, recs=waiting)
    g.close(); h.close()


def test_single_band_map_goes_through_its_host_mosaic_and_alpha(pf):
    wl = workloads()
    poses = jitter_poses(4, seed=3)
    g = pf.Map2D.create(pf.TypeCPU, False)
    assert g.prepare(wl.IDENTITY_PLANE, [640, 480, 500, 500, 320, 240], poses)
    for k, p in enumerate(poses):
        assert g.feed(wl.smooth_frame(480, 640, k), p)
    check_map(pf, g, 0)
    g.close()


def test_map_refusals(pf, orc):
    wl = workloads()
    L = pf.lib()
    cam = [640, 480, 500, 500, 320, 240]
    e = pf.Map2D.create(pf.TypeMultiBandCPU, False)
    assert e.prepare(wl.IDENTITY_PLANE, cam, jitter_poses(2, seed=1))
    assert e.webtiles_georef(ORIGIN) is None and b"no content" in L.pf_last_error()
    with pytest.raises(RuntimeError, match="no content"):
        list(e.webtiles(ORIGIN))
    e.close()
    poses = jitter_poses(3, seed=12)
    s = pf.Map2D.create(pf.TypeMultiBandCPU, False, shard_rank=0, shard_count=2, shard_block=1)
    assert s.prepare(wl.IDENTITY_PLANE, cam, poses)
    for k, p in enumerate(poses):
        assert s.feed(wl.smooth_frame(480, 640, k), p)
    assert s.save_to_memory() is not None and s.webtiles_georef(ORIGIN) is None and b"sharded" in L.pf_last_error()
    with pytest.raises(RuntimeError, match="sharded"):
        list(s.webtiles(ORIGIN))
    s.close()
    g, _ = build_map(pf, orc, 0, 5)
    p, rows, cols = g.webtiles_georef(ORIGIN)
    nz = pf.webtiles_native_zoom(p, rows, cols)
    with pytest.raises(RuntimeError, match="zmin"):
        list(g.webtiles(ORIGIN, zmin=nz + 1))
    with pytest.raises(RuntimeError, match="zoom"):
        list(g.webtiles(ORIGIN, zmax=25))
    # a sink that returns 0 stops the export at its first tile, and the call returns 0
    seen = []
    sink = pf.WEBTILE_SINK(lambda user, t: seen.append((t.contents.z, t.contents.x, t.contents.y)) or 0)
    o = (C.c_double * 3)(*ORIGIN)
    assert L.pf_webtiles(g._h, o, -1, -1, 95, 0, sink, None) == 0 and len(seen) == 1 and b"sink" in L.pf_last_error()
    assert len(list(g.webtiles(ORIGIN))) > 1          # ... and the next export is whole
    g.close()


# ---------------------------------------------------------------- files
def test_saved_files_are_the_yielded_records(pf, orc, tmp_path):
    import sqlite3
    g, _ = build_map(pf, orc, 0, 5, 255)
    recs = keyed(g.webtiles(ORIGIN, quality=90))
    d = tmp_path / "tiles"
    assert g.save_webtiles(str(d), ORIGIN, quality=90)
    found = {}
    for root, _, files in os.walk(str(d)):
        for f in files:
            if f != "tiles.json":
                z, x = os.path.relpath(root, str(d)).split(os.sep)
                found[(int(z), int(x), int(f.split(".")[0]), f.split(".")[1])] = open(os.path.join(root, f), "rb").read()
    assert {k[:3] for k in found if k[3] == "jpg"} == set(recs)
    assert {k[:3] for k in found if k[3] == "pbm"} == {k for k, t in recs.items() if t["cover"] == 1} and {k[3] for k in found} == {"jpg", "pbm"}
    for (z, x, y, ext), data in found.items():
        if ext == "jpg":
            assert data == recs[(z, x, y)]["jpeg"] and pf.decode_jpeg(data).shape == (256, 256, 3)
        else:
            assert data == b"P4\n256 256\n" + wm.pack_mask(recs[(z, x, y)]["mask"])
    info = json.load(open(str(d / "tiles.json")))
    zs = sorted({k[0] for k in recs})
    assert info["minzoom"] == zs[0] and info["maxzoom"] == zs[-1] and [e["z"] for e in info["zooms"]] == zs
    for e in info["zooms"]:
        mine = [k for k in recs if k[0] == e["z"]]
        assert e["tiles"] == len(mine) and e["partial"] == sum(1 for k in mine if recs[k]["cover"] == 1)
        assert (e["x0"], e["x1"], e["y0"], e["y1"]) == (min(k[1] for k in mine), max(k[1] for k in mine), min(k[2] for k in mine), max(k[2] for k in mine))
    p, rows, cols = g.webtiles_georef(ORIGIN)
    ll = wm.corners_lnglat(p, rows, cols)
    want = [min(v[0] for v in ll), min(v[1] for v in ll), max(v[0] for v in ll), max(v[1] for v in ll)]
    assert np.allclose(info["bounds"], want, rtol=0, atol=1e-9) and abs(want[0] - ORIGIN[0]) < 0.1 and abs(want[1] - ORIGIN[1]) < 0.1
    # failing halfway: 0, the tile named, what was written left alone
    blocked = tmp_path / "blocked"
    blocked.mkdir(); (blocked / str(zs[0])).write_bytes(b"a file where a directory has to be")
    assert not g.save_webtiles(str(blocked), ORIGIN, quality=90) and b"cannot write tile" in pf.lib().pf_last_error()
    assert any(f != str(zs[0]) for f in os.listdir(str(blocked))) and not os.path.exists(str(blocked / "tiles.json"))
    # MBTiles: the same streams under flipped rows
    mb = str(tmp_path / "m.mbtiles")
    assert g.export_mbtiles(mb, ORIGIN, quality=90) == len(recs)
    db = sqlite3.connect(mb)
    rows_ = db.execute("SELECT zoom_level, tile_column, tile_row, tile_data FROM tiles").fetchall()
    meta = dict(db.execute("SELECT name, value FROM metadata").fetchall())
    db.close()
    assert len(rows_) == len(recs)
    for z, x, ty, blob in rows_:
        assert bytes(blob) == recs[(z, x, (1 << z) - 1 - ty)]["jpeg"]
    assert meta["format"] == "jpg" and int(meta["minzoom"]) == zs[0] and int(meta["maxzoom"]) == zs[-1]
    assert np.allclose([float(v) for v in meta["bounds"].split(",")], want, rtol=0, atol=1e-7)
    g.close()
