"""BGRA keyframes (8UC4, as the live tracker holds them: SURVEY 8 row f1) through every way into the multi-band map.

The channel count selects other code in the warp's tap addressing (cn * ux), the `hisel` permute of the finish stages, the border
path's shifts (8 * cn, and the move-back shift at the end of the buffer), the per-op warp of fused = 0, the LDS patch pitch and the
strips form, and on the host in frame_bytes / upload / stage_frame, the cn a queued keyframe carries through the queue and the lookahead
window, and pf_dist_feed.  The BGR instantiation of all that is pinned from every side; this file runs the same comparisons with
cn = 4.  The frames are tests/bgra.py's: the colour content of the BGR twins with an alpha plane that no colour comes near, so that an
alpha byte in any tap changes the map (tests/test_bgra_model.py shows it for every kind of frame).  Witnesses: the oracle and ModelMap
fed the first three channels, which is what the map takes of a BGRA frame (TrackerOpt.cpp:376-380, cvtColor BGRA2BGR)."""
import functools
import importlib

import numpy as np
import pytest

import bgra
from helpers import HOSTILE_KINDS, compare_maps, compare_with_model, jitter_poses, map_digest, neighbourhoods, workloads
from test_gpu_dist import Rendezvous, collective, shards_equal_the_oracle, workload as dist_workload
from test_gpu_model import BG, CAM, COLS, N, ROWS, check, witnesses

pytestmark = pytest.mark.gpu
CAM_VGA = [640, 480, 500, 500, 320, 240]
# the other paths at 5 bands, in two groups so that a case costs about what its BGR twin (four paths) costs: kernel forms and options / ways in
PATHS_5 = {"forms": ("fused0", "fused2", "fused3", "lookahead0", "nocull"), "ways": ("pad6", "pad90", "device", "device_pad6", "thread")}

def last_error(pf):
    return pf.lib().pf_last_error().decode()


def bgr_of(f):
    return np.ascontiguousarray(f[:, :, :3])


def feed_way(g, way, f, pose, keep):
    """One BGRA keyframe f into the HIP map g: "host" packed, "padN" as a host view whose rows lie N bytes apart (what lies in HBM
    afterwards must be the caller's bytes, padding included), "device" / "device_padN" resident in HBM; "bgr": its colour channels as a
    BGR frame.  keep: what must stay alive until the map has rendered (device frames are read when their turn comes)."""
    rows, cols = f.shape[:2]
    if way == "bgr":
        return g.feed(bgr_of(f), pose)
    if way == "host":
        return g.feed(f, pose)
    if way.startswith("pad"):
        view = bgra.padded(f, int(way[3:]))
        ok = g.feed(view, pose)
        got = g.read_last_frame()
        want = bgra.frame_bytes(view)
        assert got is not None and got.size == want.size and np.array_equal(got, want), (way, "the frame in HBM is not the caller's bytes")
        return ok
    import torch
    if way == "device":
        t, step = torch.from_numpy(np.ascontiguousarray(f)).cuda(), 0
    else:
        t, step = bgra.padded_device(f, int(way[10:]))
    torch.cuda.synchronize()
    keep.append(t)
    return g.feed_device(t.data_ptr(), rows, cols, pose, step=step, channels=4)


# ---------------------------------------------------------------- hostile frames, three witnesses
def run_path(pf, path, poses, prep, four, ff, bands):
    opt = dict(force_float=ff, band_number=bands, bg_color=BG)
    if path.startswith("fused"):
        opt["fused"] = int(path[5:])
    if path == "lookahead0":
        opt["lookahead"] = 0
    if path.startswith("device"):
        opt["lookahead"] = 3                                              # the caller's buffers are read up to three feeds later
    g = pf.Map2D.create(pf.TypeMultiBandCPU, path == "thread", **opt)
    if path == "nocull":
        g.set_cull(False)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, prep)
    way = {"pad6": "pad6", "pad90": "pad90", "device": "device", "device_pad6": "device_pad6", "bgr": "bgr"}.get(path, "host")
    keep = []
    for f, p in zip(four, poses):
        assert feed_way(g, way, f, p, keep), (path, last_error(pf))
    assert g.sync()
    del keep
    if path == "thread":
        assert g.render_log() == list(range(N))                           # nothing dropped: the model holds every keyframe
    if path == "nocull":
        assert g.culled_tiles() + g.culled_cells() == 0
    return g


@pytest.mark.parametrize("bands", [1, 5, 8])
@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_hostile_bgra_frames_hip_equals_model_and_oracle(pf, kind, force_float, bands):
    """test_gpu_model.py's hostile-frame cases with BGRA keyframes, the product path (fused, default lookahead and cull) at 1, 5 and 8
    bands: whole map, blend_tile(_raw) of every tile, blend_tiles and save, bit for bit against the model (which equals the oracle);
    and a HIP map fed the BGR pixels has the same digest."""
    poses, prep, frames, o, m = witnesses(kind, force_float, bands)
    assert compare_with_model(o, m) == []
    assert all(neighbourhoods(m.tiles()))
    four = [bgra.with_alpha(f, k) for k, f in enumerate(frames)]
    assert all(f.shape == (ROWS, COLS, 4) for f in four)
    g = run_path(pf, "product", poses, prep, four, force_float, bands)
    check(g, o, m, (kind, "product"))
    b = run_path(pf, "bgr", poses, prep, four, force_float, bands)
    assert map_digest(b) == map_digest(g)
    g.close(); b.close()


@pytest.mark.parametrize("group", sorted(PATHS_5))
@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_hostile_bgra_frames_every_other_path(pf, kind, force_float, group):
    """... and at 5 bands through fused 0, 2 and 3, no lookahead and no cull ("forms"); host rows padded by 6 and 90 bytes,
    device-resident frames packed and padded by 6 with the lookahead on, and the render thread ("ways"): the same checks."""
    poses, prep, frames, o, m = witnesses(kind, force_float, 5)
    four = [bgra.with_alpha(f, k) for k, f in enumerate(frames)]
    for path in PATHS_5[group]:
        g = run_path(pf, path, poses, prep, four, force_float, 5)
        check(g, o, m, (kind, path))
        g.close()


# ---------------------------------------------------------------- BGRA images given to prepare
@pytest.mark.parametrize("force_float,layout", [(0, "packed"), (1, "packed"), (0, "pad6"), (1, "pad90")])
def test_bgra_prepare_images_on_the_render_thread(pf, orc, force_float, layout):
    """A thread = true map renders the images given to prepare first (map_feed.cpp, Map2D.cpp:42).  The tracker's keyframes are
    BGRA: the first three go in through prepare(images=...), packed or as row-padded views, the rest through feed, and the map equals
    the oracle fed all of them as BGR in that order -- tiles and saved mosaic, as test_wire.py::test_live_wire_cfg4 compares.  (The
    binding used to label every prepare image 8UC3: rows * cols * 3 bytes of BGRA rendered as BGR, without an error.)"""
    wl = workloads()
    poses = jitter_poses(7, seed=52)
    four = [bgra.with_alpha(wl.noise_frame(480, 640, 700 + k), k) for k in range(len(poses))]
    lay = (lambda f: f) if layout == "packed" else (lambda f: bgra.padded(f, int(layout[3:])))
    m = pf.Map2D.create(pf.TypeMultiBandCPU, True, force_float=force_float)
    assert m.prepare(wl.IDENTITY_PLANE, CAM_VGA, poses[:3], images=[lay(f) for f in four[:3]])
    for f, p in zip(four[3:], poses[3:]):
        assert m.feed(lay(f), p)
    assert m.sync() and m.queueSize() == 0
    assert m.stats() == {"rendered": len(poses), "rejected": 0, "dropped": 0}
    o = orc.OracleMap(force_float=force_float)
    assert o.prepare(wl.IDENTITY_PLANE, CAM_VGA, poses[:3])
    for f, p in zip(four, poses):
        assert o.feed(bgr_of(f), p)
    assert compare_maps(m, o) == []
    assert np.array_equal(m.save_to_memory()[0], o.save()[0])
    m.close()


def test_prepare_rejects_what_feed_rejects(pf):
    """an image that is no 8UC3 / 8UC4 frame of the camera's size (another dtype, another size) given to prepare is
    refused by renderFrame's gate (.cpp:319-323) as the threaded feed refuses it: never rendered, and no byte beyond it read"""
    wl = workloads()
    poses = jitter_poses(3, seed=53)
    good = bgra.with_alpha(wl.noise_frame(480, 640, 710), 0)
    bad = [good.astype(np.float32), good[:100, :200], good.astype(np.uint16)]
    m = pf.Map2D.create(pf.TypeMultiBandCPU, True)
    assert m.prepare(wl.IDENTITY_PLANE, CAM_VGA, poses, images=bad)
    assert m.sync() and m.stats()["rendered"] == 0 and m.tiles() == []
    assert m.feed(good, poses[0]) and m.sync() and m.stats()["rendered"] == 1
    m.close()


# ---------------------------------------------------------------- a sortie of mixed keyframes
WAYS = ("bgr", "host", "pad6", "device")


@functools.lru_cache(maxsize=None)
def sortie(force_float):
    """12 tilted keyframes and the oracle fed their BGR pixels (shared by the lookaheads; nobody feeds it again)"""
    from oracle import orc
    wl = workloads()
    poses = jitter_poses(12, seed=61)
    four = [bgra.with_alpha(wl.noise_frame(480, 640, 720 + k), k) for k in range(len(poses))]
    o = orc.OracleMap(force_float=force_float)
    assert o.prepare(wl.IDENTITY_PLANE, CAM_VGA, poses[:2])
    for f, p in zip(four, poses):
        assert o.feed(bgr_of(f), p)
    assert len(o.tiles()) >= 6
    return poses, four, o


@pytest.mark.parametrize("lookahead", [None, 0])
@pytest.mark.parametrize("force_float", [0, 1])
def test_mixed_sortie(pf, force_float, lookahead):
    """BGR, BGRA, row-padded BGRA and device-resident BGRA keyframes in turn, waiting side by side in the lookahead window (the
    default one holds all twelve) and rendered one by one (lookahead 0): each with its own cn and row step."""
    poses, four, o = sortie(force_float)
    opt = {} if lookahead is None else {"lookahead": lookahead}
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float, **opt)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM_VGA, poses[:2])
    keep = []
    for k, (f, p) in enumerate(zip(four, poses)):
        assert feed_way(g, WAYS[k % len(WAYS)], f, p, keep), (k, last_error(pf))
    assert g.sync()
    del keep
    assert g.grid() == o.grid()
    assert compare_maps(g, o) == []
    assert g.stats()["rendered"] == len(poses)
    g.close()


# ---------------------------------------------------------------- frames of a few pixels
def degenerate_case(shape):
    wl = workloads()
    rows, cols = shape
    cam = [cols, rows, 40.0, 40.0, cols / 2.0, rows / 2.0]                # the cameras and poses of test_gpu_parity.test_degenerate_frame_shapes
    poses = [[0.7 * k, 0.3 * k, -100.0] + wl.quat_axis((0, 0, 1), 0.2 * k) for k in range(3)]
    four = [bgra.with_alpha(wl.noise_frame(rows, cols, 500 + k), k) for k in range(3)]
    return cam, poses, four


@pytest.mark.parametrize("layout", ["packed", "pad1"])
@pytest.mark.parametrize("shape", [(1, 2), (2, 1), (1, 64), (2, 48), (40, 1), (3, 3)])
def test_degenerate_bgra_frame_shapes(pf, orc, shape, layout):
    """One row, one column, a few pixels: every canvas pixel takes the border paths, whose last 8-byte load is moved back by 4 bytes
    for BGRA (2 or 5 for BGR).  (1, 2) and (2, 1) are 8 bytes, the smallest frame feed accepts, and exist as BGRA only.  Both pyramid
    types and the single-band map against the oracle."""
    wl = workloads()
    cam, poses, four = degenerate_case(shape)
    way = "host" if layout == "packed" else "pad1"
    for ff in (0, 1):
        g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=ff); o = orc.OracleMap(force_float=ff)
        assert g.prepare(wl.IDENTITY_PLANE, cam, poses) and o.prepare(wl.IDENTITY_PLANE, cam, poses)
        for f, p in zip(four, poses):
            assert feed_way(g, way, f, p, None) == o.feed(bgr_of(f), p) == True, last_error(pf)
        assert g.sync()
        assert compare_maps(g, o) == [] and len(o.tiles()) > 0
        g.close()
    s = pf.Map2D.create(pf.TypeCPU, False); so = orc.OracleMap(single_band=True)
    assert s.prepare(wl.IDENTITY_PLANE, cam, poses) and so.prepare(wl.IDENTITY_PLANE, cam, poses)
    for f, p in zip(four, poses):
        assert feed_way(s, way, f, p, None) == so.feed(bgr_of(f), p) == True, last_error(pf)
    assert s.sync()
    assert s.tiles() == so.tiles() and len(so.tiles()) > 0
    for t in so.tiles():
        assert np.array_equal(s.tile_bgra(*t), so.tile_bgra(*t)), t
    s.close()


@pytest.mark.parametrize("typ", ["TypeMultiBandCPU", "TypeCPU"])
def test_frame_of_four_bytes_is_refused(pf, typ):
    """(1, 1) as BGRA is 4 bytes: the warp loads 8 per source row, so feed says false and why, and the map is the one never fed it"""
    wl = workloads()
    cam, poses, four = degenerate_case((1, 1))
    g = pf.Map2D.create(getattr(pf, typ), False); fresh = pf.Map2D.create(getattr(pf, typ), False)
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses) and fresh.prepare(wl.IDENTITY_PLANE, cam, poses)
    assert g.feed(four[0], poses[0]) is False
    assert "smaller than 8 bytes" in last_error(pf)
    assert g.sync()
    assert g.grid() == fresh.grid() and g.tiles() == fresh.tiles() == [] and g.stats()["rendered"] == 0
    assert map_digest(g) == map_digest(fresh)
    g.close(); fresh.close()


# ---------------------------------------------------------------- the weight plane
@pytest.mark.parametrize("weight_type", [0, 1])
def test_bgra_frame_wider_than_8191_px(pf, orc, weight_type):
    """test_gpu_parity.test_frame_wider_than_8191_px with BGRA keyframes: frames with a side of 8192 px or more gather their weight
    from the plane, a kernel instantiation of its own, here with cn = 4"""
    wl = workloads()
    w, h = 8256, 96
    cam = [w, h, 9000.0, 9000.0, w / 2, h / 2]
    poses = [[k * 7.0, k * 0.3, -100.0] + wl.quat_axis((0, 0, 1), 0.01 * k) for k in range(3)]
    four = [bgra.with_alpha(wl.noise_frame(h, w, 300 + k), k) for k in range(3)]
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, band_number=3, weight_type=weight_type)
    o = orc.OracleMap(band_num=3, weight_type=weight_type)
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses) and o.prepare(wl.IDENTITY_PLANE, cam, poses)
    for f, p in zip(four, poses):
        assert g.feed(f, p) == o.feed(bgr_of(f), p) == True
    assert g.sync() and g.grid() == o.grid()
    assert compare_maps(g, o) == []
    g.close()


# ---------------------------------------------------------------- pf_dist_feed
@functools.lru_cache(maxsize=None)
def dist_witness(force_float):
    from oracle import orc
    wl = workloads()
    cam, poses, frames = dist_workload(wl)
    o = orc.OracleMap(force_float=force_float, scale=2.0)
    assert o.prepare(wl.IDENTITY_PLANE, cam, poses[:2])
    for f, p in zip(frames, poses):
        assert o.feed(f, p)
    return cam, poses, [bgra.with_alpha(f, k) for k, f in enumerate(frames)], o


@pytest.mark.parametrize("root", [0, 2])
@pytest.mark.parametrize("force_float", [0, 1])
def test_dist_feed_bgra_from_one_rank(pf, force_float, root):
    """test_gpu_dist.test_dist_feed_from_one_rank with BGRA keyframes on the host of one of three thread-ranks: the frames travel with
    four bytes a pixel (hashed on both ends) and the shards' tiles -- union and pixels -- are the oracle's"""
    sh = importlib.import_module("pi_slam_fusion_amd.sharding")
    wl = workloads()
    world = 3
    cam, poses, four, o = dist_witness(force_float)
    maps = [pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float, scale=2.0,
                            shard_rank=r, shard_count=world, shard_block=2) for r in range(world)]
    for m in maps:
        assert m.prepare(wl.IDENTITY_PLANE, cam, poses[:2])
    rv = Rendezvous(world)
    dms = [sh.DistMap(m, r, world, backend="host", exchange=rv.fn(r)) for r, m in enumerate(maps)]
    for d in dms:
        d.set_verify(True)

    def rank_main(r):
        moved = 0
        for f, p in zip(four, poses):
            assert dms[r].feed(f if r == root else None, p, root=root, shape=f.shape) is True
            st = dms[r].stats()
            moved += st["bytes_received"] + st["bytes_sent"]
        assert maps[r].sync()
        return moved
    out = collective(world, rv, rank_main)
    shards_equal_the_oracle(pf, maps, o, out, root, four[0].size, len(four))
    assert four[0].size == 480 * 640 * 4
    for d in dms:
        d.close()
    for m in maps:
        m.close()
