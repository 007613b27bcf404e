"""Rendered views on the GPU (csrc/view.hip, map_view.cpp behind pf_render_view*) against their model (view_model.py: the oracle's
orc.warp_linear_const_8u of the mosaic and its coverage, cropped to the plan's rectangle, by the plan's M0), byte for byte over every
pixel: crops, the ring of tiles at 0, 1, 5 and 8 bands, general homographies at every level and awkward sizes, cvRound's ties,
freshness between feeds and across a grid that grows, the three ways out, the refusals, and the helpers that make a V.  Small maps:
camera 160 x 120, 8 jittered keyframes, 5 x 4 tiles, both pyramid types, the default lookahead."""
import ctypes as C

import numpy as np
import pytest

from helpers import workloads
from view_model import BG, CAM, ELE, extent_of, oracle_map, rig_frame, rig_poses, truth, view_model

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SIZES = ((64, 64), (150, 37), (40, 5), (300, 9), (1, 1))          # width x height: see test_general_homographies


def gpu_map(pf, force_float, bands, upto=8, n=8, seed=4, prep=None, thread=False, sync=False, **opt):
    poses = rig_poses(n, seed)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, thread, force_float=force_float, band_number=bands, bg_color=BG, **opt)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:prep] if prep else poses)
    for k in range(upto):
        assert g.feed(rig_frame(k), poses[k])
    if sync:
        assert g.sync()
    return g


def check_view(pf, g, o, V, width, height, level, channels=4, out=None):
    """one view against the model; returns the info.  The plan the map used is the pure plan of the oracle's grid and extent"""
    got, info = g.render_view(V, width, height, level, channels, out)
    dims, geo = o.grid()
    plan = pf.view_plan(V, width, height, level, dims, geo, o.num_levels, extent_of(o.tiles()))
    for key in ("level", "rect", "window", "empty", "tiles"):
        assert info[key] == plan[key], (key, info[key], plan[key])
    assert info["M0"].tobytes() == plan["M0"].tobytes() and info["Minv"].tobytes() == plan["Minv"].tobytes()
    S, Cv, origin = truth(o, info["level"])
    want = view_model(S, Cv, origin, info, width, height, BG, channels)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (width, height, level, channels, info["rect"], int((got != want).any(axis=2).sum()), "pixels differ")
    return info


def crop_view(o, k, ax, ay):
    """V of scale 1 at level k: view pixel (u, v) over level-k pixel (u + ax, v + ay) of the extent"""
    dims, geo = o.grid()
    ex = extent_of(o.tiles())
    s = geo[5] * (1 << k)
    ox, oy = geo[0] + (ex[0] - dims[2]) * geo[4], geo[1] + (ex[1] - dims[3]) * geo[4]
    return np.array([[1 / s, 0, -ox / s - ax], [0, 1 / s, -oy / s - ay], [0, 0, 1.0]])


# ---------------------------------------------------------------- crops
@pytest.mark.parametrize("force_float", [0, 1])
def test_a_crop_is_the_crop_of_the_saved_mosaic_and_its_mask(pf, force_float):
    g, o = gpu_map(pf, force_float, 5), oracle_map(force_float, 5)
    mosaic, mask, origin = g.save_to_memory_mask()
    assert origin == extent_of(o.tiles())[:2]
    rows, cols = mask.shape
    #        ax, ay, width, height: starts on a tile border; ends on one; crosses the extent's edges; wholly outside
    cases = ((ELE, ELE, 200, 100), (ELE - 150, 2 * ELE - 90, 150, 90), (-20, -10, 120, 60), (cols - 50, rows - 30, 100, 70), (cols + 5, 40, 64, 48), (-400, -300, 64, 48))
    for ax, ay, w, h in cases:
        info = check_view(pf, g, o, crop_view(o, 0, ax, ay), w, h, 0)
        got, _ = g.render_view(crop_view(o, 0, ax, ay), w, h, 0)
        want = np.zeros((h, w, 4), np.uint8); want[:, :, :3] = BG
        x0, y0, x1, y1 = max(ax, 0), max(ay, 0), min(ax + w, cols), min(ay + h, rows)
        if x0 < x1 and y0 < y1:
            want[y0 - ay:y1 - ay, x0 - ax:x1 - ax, :3] = mosaic[y0:y1, x0:x1]
            want[y0 - ay:y1 - ay, x0 - ax:x1 - ax, 3] = mask[y0:y1, x0:x1]
        assert np.array_equal(got, want), (ax, ay)
        assert info["empty"] == (not (x0 < x1 and y0 < y1))
        if info["empty"]:
            assert (got[:, :, :3] == BG).all() and (got[:, :, 3] == 0).all() and info["tiles"] == 0
    g.close()


# ---------------------------------------------------------------- the ring
@pytest.mark.parametrize("bands", [0, 1, 5, 8])
def test_one_pixel_views_on_a_tiles_first_and_last_column(pf, bands):
    """one pixel wide and one tile high on a tile's first and last column, one pixel high and one tile wide on its first and last row: at
    eight bands the last column and row need two tiles of ring (tests/test_view_model.py: one is not enough)"""
    g, o = gpu_map(pf, 0, bands), oracle_map(0, bands)
    tiles = set(o.tiles()); ex = extent_of(o.tiles())
    t = sorted(t for t in tiles if (t[0] + 1, t[1]) in tiles and (t[0] + 2, t[1]) in tiles)[0]
    tx, ty = (t[0] - ex[0]) * ELE, (t[1] - ex[1]) * ELE
    last = []
    for ax, ay, w, h in ((tx, ty, 1, ELE), (tx + ELE - 1, ty, 1, ELE), (tx, ty, ELE, 1), (tx, ty + ELE - 1, ELE, 1)):
        info = check_view(pf, g, o, crop_view(o, 0, ax, ay), w, h, 0)
        last.append(info["rect"][0] + info["rect"][2] - 1)
    # the last column: the tile behind it for the second tap, and at eight bands one more -- two tiles of ring
    assert last[1] == t[0] + (2 if bands == 8 else 1), (last, t)
    g.close()


# ---------------------------------------------------------------- general homographies
def seeded_views(g, o, seed):
    """twelve V: rotations, scales 0.3 .. 5 (view pixels per level-0 pixel), mild perspective, centred somewhere on the content; four of
    them what a camera at a fed keyframe's pose sees"""
    rng = np.random.RandomState(seed)
    dims, geo = o.grid()
    ex = extent_of(o.tiles())
    ox, oy = geo[0] + (ex[0] - dims[2]) * geo[4], geo[1] + (ex[1] - dims[3]) * geo[4]
    out = []
    for i in range(8):
        a = rng.uniform(-np.pi, np.pi); s = 0.3 * (5 / 0.3) ** rng.uniform(0, 1) / geo[5]
        V = np.array([[s * np.cos(a), -s * np.sin(a), 0.0], [s * np.sin(a), s * np.cos(a), 0.0], [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]])
        c = np.array([ox + rng.uniform(0.2, 0.8) * ex[2] * geo[4], oy + rng.uniform(0.2, 0.8) * ex[3] * geo[4], 1.0])
        p = V @ c
        V[0, 2] = rng.uniform(10, 60) * p[2] - p[0]; V[1, 2] = rng.uniform(2, 30) * p[2] - p[1]
        out.append(V)
    poses = rig_poses()
    for k in (0, 3, 5, 7):
        V = g.view_from_pose(poses[k])
        assert V is not None
        out.append(V)
    return out


@pytest.mark.parametrize("case", range(12))
def test_general_homographies_at_every_level_and_size(pf, case):
    """sizes: 64 x 64; 150 x 37 (the width is no multiple of the 64-pixel run); 40 x 5 (height < 16, so bw0 = 204 exceeds the width);
    300 x 9 (bw0 = 113 < width: a run boundary inside a row); 1 x 1.  Level -1 and every explicit level; four channels into a packed
    buffer, three into rows with padding, whose bytes stay the caller's"""
    ff = case & 1
    g, o = gpu_map(pf, ff, 5), oracle_map(ff, 5)
    V = seeded_views(g, o, 17)[case]
    levels = set()
    for level in [-1] + list(range(o.num_levels)):
        for w, h in SIZES:
            info = check_view(pf, g, o, V, w, h, level)
            levels.add(info["level"])
            pad = np.full((h, w * 3 + 5), SENTINEL, np.uint8)
            out = pad[:, :w * 3].reshape(h, w, 3)
            check_view(pf, g, o, V, w, h, level, 3, out)
            assert (pad[:, w * 3:] == SENTINEL).all()
    assert levels == set(range(o.num_levels))
    g.close()


# ---------------------------------------------------------------- ties
def tie_view(pf, g, o, ax, ay, w, h):
    """V with which the plan's M0 is EXACTLY the translation by (-ax, -ay): every source coordinate is then x + ax exactly.  lengthPixel
    is 0.5 (the map's resolution option), so M0's scale is exact; the offset is searched among the neighbouring doubles"""
    dims, geo = o.grid()
    assert geo[5] == 0.5
    V = crop_view(o, 0, ax, ay)
    ex = extent_of(o.tiles())
    info = pf.view_plan(V, w, h, 0, dims, geo, o.num_levels, ex)
    ax, ay = ax - (info["rect"][0] - ex[0]) * ELE, ay - (info["rect"][1] - ex[1]) * ELE          # against the rectangle's origin, as M0 is
    for axis, want in ((0, -ax), (1, -ay)):
        base = V[axis, 2]
        for n in range(-8, 9):
            V[axis, 2] = base + n * np.spacing(base)
            got = pf.view_plan(V, w, h, 0, dims, geo, o.num_levels, extent_of(o.tiles()))
            if got["M0"][axis, 2] == want and got["rect"] == info["rect"]:
                break
        else:
            raise AssertionError("no offset puts M0 on the tie")
    got = pf.view_plan(V, w, h, 0, dims, geo, o.num_levels, extent_of(o.tiles()))
    assert got["M0"].tolist() == [[1, 0, -ax], [0, 1, -ay], [0, 0, 1]]
    return V


def test_every_coordinate_on_cvrounds_tie(pf):
    """scale 1 shifted by 1 / 64 pixel in x and in y: 32 (x + ax) ends in .5 at every pixel, and rounds to even; also 1 / 64 + k / 32"""
    opt = dict(resolution=0.5)
    poses = rig_poses()
    from oracle import orc
    o = orc.OracleMap(band_num=5, force_float=0, bg_color=BG, resolution=0.5)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=5, bg_color=BG, **opt)
    for m in (o, g):
        assert m.prepare(workloads().IDENTITY_PLANE, CAM, poses)
        for k in range(4):
            assert m.feed(rig_frame(k), poses[k])
    assert sorted(g.tiles()) == sorted(o.tiles())
    for k in (0, 1, 5, 16, 31):
        sh = 1 / 64 + k / 32
        for ax, ay in ((300 + sh, 200 + sh), (255 + sh, 40.0), (40.0, 255 + sh), (-3 + sh, -2 + sh)):
            V = tie_view(pf, g, o, ax, ay, 150, 37)
            info = check_view(pf, g, o, V, 150, 37, 0)
            assert not info["empty"]
    g.close()


# ---------------------------------------------------------------- freshness
@pytest.mark.parametrize("force_float", [0, 1])
def test_a_view_between_feeds_sees_every_keyframe_fed_so_far(pf, force_float):
    """no pf_sync: keyframes wait for the lookahead and the view renders them first"""
    poses = rig_poses()
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float, band_number=5, bg_color=BG)
    assert g.opt.lookahead > 0
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses)
    V = None
    for upto in (3, 6, 8):
        for k in range(upto - 3 if upto < 8 else 6, upto):
            assert g.feed(rig_frame(k), poses[k])
        o = oracle_map(force_float, 5, upto)
        if V is None:
            V = seeded_views(g, o, 3)[1]
        for level in (-1, 0, 2):
            check_view(pf, g, o, V, 150, 37, level)
        check_view(pf, g, o, g.view_of_extent(96, 80), 96, 80, -1)
    g.close()


def test_a_threaded_map_after_sync(pf):
    g = gpu_map(pf, 0, 5, thread=True, sync=True, max_queue=8)
    log = g.render_log()
    assert log == list(range(8)), log                   # nothing was dropped: the oracle fed all eight is the map
    o = oracle_map(0, 5)
    for V in seeded_views(g, o, 5)[:3]:
        check_view(pf, g, o, V, 64, 64, -1)
    g.close()


def test_the_same_v_before_and_after_the_grid_grows(pf):
    """prepared from the first three poses, so that later keyframes leave the grid (spreadMap): V is in plane metres and stays valid"""
    poses = rig_poses()
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=5, bg_color=BG)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:3])
    for k in range(3):
        assert g.feed(rig_frame(k), poses[k])
    before = oracle_map(0, 5, 3, prep=3)
    grid0 = g.grid()
    assert grid0 == tuple(before.grid()) or list(grid0[0]) == list(before.grid()[0])
    V = g.view_of_extent(120, 100)
    check_view(pf, g, before, V, 120, 100, -1)
    check_view(pf, g, before, V, 120, 100, 0)
    for k in range(3, 8):
        assert g.feed(rig_frame(k), poses[k])
    after = oracle_map(0, 5, 8, prep=3)
    assert g.grid()[0] != grid0[0], "the grid did not grow"
    assert list(g.grid()[0]) == list(after.grid()[0])
    check_view(pf, g, after, V, 120, 100, -1)
    check_view(pf, g, after, V, 120, 100, 0)
    g.close()


# ---------------------------------------------------------------- ways out
def test_ways_out(pf):
    import torch
    g, o = gpu_map(pf, 0, 5), oracle_map(0, 5)
    V = seeded_views(g, o, 9)[2]
    w, h = 150, 37
    # the draw loop's flags are left alone: a twin that is never viewed hands out the same tiles
    twin = gpu_map(pf, 0, 5)
    host4, info = g.render_view(V, w, h, -1, 4)
    host3, _ = g.render_view(V, w, h, -1, 3)
    assert np.array_equal(host3, host4[:, :, :3])
    for channels, host in ((4, host4), (3, host3)):
        dev = torch.full((h, w, channels), SENTINEL, dtype=torch.uint8, device="cuda")
        assert g.render_view_device(V, w, h, dev.data_ptr(), -1, channels)["rect"] == info["rect"]
        assert np.array_equal(dev.cpu().numpy(), host)
        padded = torch.full((h, w * channels + 12), SENTINEL, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            g.render_view_device(V, w, h, padded.data_ptr(), -1, channels, step=w * channels + 12, stream=stream.cuda_stream)
            back = padded.cpu().numpy()                  # queued behind the view on the same stream
        assert np.array_equal(back[:, :w * channels].reshape(h, w, channels), host) and (back[:, w * channels:] == SENTINEL).all()
    for quality in (95, 60):
        stream, jinfo = g.render_view_jpeg(V, w, h, -1, quality)
        assert stream == pf.jpeg_encode(host3, quality) and jinfo["rect"] == info["rect"]
    with pytest.raises(ValueError, match="bytes"):
        g.render_view_jpeg(V, w, h, -1, 95, cap=100)
    pinned = pf.host_array((h, w, 4)); pinned[:] = SENTINEL
    got, _ = g.render_view(V, w, h, -1, 4, pinned)
    assert got is pinned and np.array_equal(pinned, host4)
    a, b = g.blend_changed(cap=32), twin.blend_changed(cap=32)
    assert a[0] == b[0] and len(a[0]) == len(o.tiles()) and np.array_equal(a[1], b[1])
    g.close(); twin.close()


# ---------------------------------------------------------------- refusals
def test_refusals_return_nothing_name_the_reason_and_touch_nothing(pf):
    wl = workloads()
    poses = rig_poses()
    o = oracle_map(0, 5)
    V = crop_view(o, 0, 100, 100)
    L = pf.lib()

    def refused(m, V, word, w=64, h=48):
        out = np.full((48, 64, 4), SENTINEL, np.uint8)
        v = np.ascontiguousarray(V, np.float64).reshape(9)
        pv = v.ctypes.data_as(C.POINTER(C.c_double))
        info = pf.ViewInfo(); info.tiles = 77
        n = C.c_size_t(77)
        assert L.pf_render_view(m._h, pv, w, h, 0, 4, out.ctypes.data, 0, C.byref(info)) == 0
        msg = L.pf_last_error().decode()
        assert msg.startswith("pf_render_view: ") and word in msg, msg
        assert L.pf_render_view_jpeg(m._h, pv, w, h, 0, 95, out.ctypes.data, out.size, C.byref(n), C.byref(info)) == 0
        assert word in L.pf_last_error().decode()
        assert (out == SENTINEL).all() and info.tiles == 77 and n.value == 77
        with pytest.raises(ValueError, match=word):
            m.render_view(V, w, h, 0, 4, out if (h, w) == out.shape[:2] else None)
        assert (out == SENTINEL).all()

    single = pf.Map2D.create(pf.TypeCPU, False)
    sharded = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=5, bg_color=BG, shard_rank=0, shard_count=2, shard_block=1)
    for m, word in ((single, "TypeCPU"), (sharded, "sharded")):
        assert m.prepare(wl.IDENTITY_PLANE, CAM, poses)
        for k in range(4):
            assert m.feed(rig_frame(k), poses[k])
        refused(m, V, word)
        m.close()
    fresh = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=5, bg_color=BG)
    refused(fresh, V, "prepared")
    fresh.close()
    g = gpu_map(pf, 0, 5)
    dims, geo = o.grid()
    ex = extent_of(o.tiles())
    A0 = np.array([[geo[5], 0, geo[0] + (ex[0] - dims[2]) * geo[4]], [0, geo[5], geo[1] + (ex[1] - dims[3]) * geo[4]], [0, 0, 1.0]])
    Minv = np.array([[1.0, 0, 100], [0, 1.0, 100], [-2.0 / 63, 0, 1.0]])          # the denominator runs from 1 to -1 along a row
    refused(g, np.linalg.inv(Minv) @ np.linalg.inv(A0), "horizon")
    refused(g, np.zeros((3, 3)), "singular")
    refused(g, V * np.nan, "finite")
    refused(g, V, "16384", w=0)
    # a map without content is not refused: the background, coverage 0, empty
    empty = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=5, bg_color=BG)
    assert empty.prepare(wl.IDENTITY_PLANE, CAM, poses)
    got, info = empty.render_view(V, 64, 48)
    assert info["empty"] and info["tiles"] == 0 and (got[:, :, :3] == BG).all() and (got[:, :, 3] == 0).all()
    assert empty.view_of_extent(64, 48) is None
    empty.close(); g.close()


# ---------------------------------------------------------------- the helpers that make a V
def test_helpers_make_the_v_they_promise(pf):
    g, o = gpu_map(pf, 0, 5), oracle_map(0, 5)
    dims, geo = g.grid()
    ex = extent_of(o.tiles())
    ox, oy = geo[0] + (ex[0] - dims[2]) * geo[4], geo[1] + (ex[1] - dims[3]) * geo[4]
    lp = geo[5]

    def apply(V, x, y):
        p = V @ np.array([x, y, 1.0])
        return p[:2] / p[2]

    # view_of_extent: pixels are areas; the extent's outer corners (half a pixel before its first pixel's centre, half behind its last)
    # go to the view's where the aspects agree, and the content is centred where they do not
    w, h = ex[2] * 32, ex[3] * 32
    V = g.view_of_extent(w, h)
    x0, y0 = ox - lp / 2, oy - lp / 2
    x1, y1 = x0 + ex[2] * ELE * lp, y0 + ex[3] * ELE * lp
    for (x, y), (u, v) in (((x0, y0), (0, 0)), ((x1, y0), (w, 0)), ((x0, y1), (0, h)), ((x1, y1), (w, h))):
        assert np.allclose(apply(V, x, y) + 0.5, (u, v), atol=1e-9), (x, y)
    V = g.view_of_extent(w + 40, h)
    assert np.allclose(apply(V, x0, y0) + 0.5, (20, 0), atol=1e-9) and np.allclose(apply(V, x1, y1) + 0.5, (w + 20, h), atol=1e-9)
    # view_from_pose: the footprint's four plane points go to the image corners
    poses = rig_poses()
    for k in (0, 4, 7):
        V = g.view_from_pose(poses[k])
        pts = pf.footprint(CAM, pf.se3_mul(pf.se3_inverse(workloads().IDENTITY_PLANE), poses[k]))
        for (x, y), (u, v) in zip(pts, ((0, 0), (CAM[0], 0), (0, CAM[1]), (CAM[0], CAM[1]))):
            assert np.abs(apply(V, x, y) - (u, v)).max() < 1e-6, (k, apply(V, x, y), (u, v))
        cam2 = [320, 200, 300, 280, 150, 90]
        V2 = g.view_from_pose(poses[k], cam2)
        pts2 = pf.footprint(cam2, pf.se3_mul(pf.se3_inverse(workloads().IDENTITY_PLANE), poses[k]))
        for (x, y), (u, v) in zip(pts2, ((0, 0), (320, 0), (0, 200), (320, 200))):
            assert np.abs(apply(V2, x, y) - (u, v)).max() < 1e-6
    oblique = list(poses[0]); oblique[3:] = workloads().quat_axis((1, 0, 0), 1.4)
    assert pf.footprint(CAM, oblique) is None and g.view_from_pose(oblique) is None and not g.feed(rig_frame(0), oblique)
    # view_from_lnglat: where pf_webtiles_georef's px2ll puts the window's corners on the mosaic, the view puts them on its own corners
    gps = (108.9, 34.2, 400.0)
    p, rows, cols = g.webtiles_georef(gps)
    assert abs(p[2]) < 1e-12 * abs(p[1]) + 1e-300 and abs(p[4]) < 1e-12 * abs(p[5]) + 1e-300          # the identity plane: north-up already
    (c0, r0), (c1, r1) = (37.25, 21.5), (700.0, 433.75)                                                  # continuous mosaic coordinates
    lng_w, lat_n, lng_e, lat_s = p[0] + p[1] * c0, p[3] + p[5] * r0, p[0] + p[1] * c1, p[3] + p[5] * r1
    w, h = 300, 200
    V = g.view_from_lnglat(gps, lng_w, lat_n, lng_e, lat_s, w, h)
    for (c, r), (u, v) in (((c0, r0), (0, 0)), ((c1, r0), (w, 0)), ((c0, r1), (0, h)), ((c1, r1), (w, h))):
        # web tiles sample the mosaic at pixel index = continuous - 0.5; that index's plane position under the views' convention:
        x, y = ox + (c - 0.5) * lp, oy + (r - 0.5) * lp
        assert np.abs(apply(V, x, y) + 0.5 - (u, v)).max() < 1e-9, ((c, r), apply(V, x, y) + 0.5, (u, v))
    check_view(pf, g, o, V, w, h, -1)
    g.close()
