"""The single-band map (Map2D::create(TypeCPU | TypeGPU): csrc/single_band.hip and the single-band branches of fusion_map.cpp) against
ModelMapSingleBand (map_model.py), which shares no arithmetic with the kernel or the oracle, and against the oracle as the third
witness; known answers that need neither; and the lookahead and the cull on this path, whose select is the strict `<` of
Map2DCPU.cpp:327 -- the OLDEST keyframe wins among equal alphas, the opposite of the multi-band map.  Every comparison is of bytes.

A case that compares with the model also asserts, from the model's statistics, that it reached both arithmetic paths of k_single2
(64-pixel waves wholly inside the frame, and waves that straddle its edge) and the rim of a footprint, where the stored alpha is
below the weight's floor of 2."""
import functools
import math

import numpy as np
import pytest

import jpeg_enc
from helpers import (HOSTILE_KINDS, compare_single_with_model, feed_single_with_model, hostile_frame, jitter_poses, single_band_pair,
                     workloads)
pytestmark = pytest.mark.gpu

CAMS = {(257, 333): [333, 257, 260, 260, 166.5, 128.5], (480, 640): [640, 480, 500, 500, 320, 240]}
N = 4


def model_pair(cam, poses, prep, frames, wt=0, scale=1.0):
    """the oracle and the model fed the same keyframes, and found equal (a function the cached witnesses() can call: the session's
    `orc` fixture is this module, loaded)"""
    from oracle import orc
    o, m = single_band_pair(orc, cam, poses, frames, prep, wt, scale)
    assert compare_single_with_model(o, m) == []
    return o, m


@functools.lru_cache(maxsize=None)
def witnesses(kind, wt, size):
    """Jittered poses (every sub-pixel phase), the grid prepared from the last one so that spreadMap moves the origin.  Built once per
    (kind, weight type, size) and shared by the cases that differ in the HIP path only: the model is frozen and nobody feeds the oracle
    again (a case with other frames, such as the .jpg one, builds its own pair)."""
    rows, cols = size
    poses = jitter_poses(N, seed=29, step=(30.0, 20.0))
    frames = [hostile_frame(kind, rows, cols, k) for k in range(N)]
    o, m = model_pair(CAMS[size], poses, poses[3:], frames, wt)
    assert o.grid()[0][2] < 0                                              # the origin moved
    return poses, poses[3:], frames, o, m.freeze()


def reached(m):
    assert m.waves_inside > 0 and m.waves_straddling > 0 and m.rim_px > 0, (m.waves_inside, m.waves_straddling, m.rim_px)


def check(g, o, m, label):
    assert g.sync()
    assert g.grid() == o.grid(), label
    assert g.num_levels == 1
    bad = compare_single_with_model(g, m)
    assert bad == [], (label, bad[:8])
    reached(m)


def same_tiles(g, o, label=None):
    """every tile of the HIP map byte for byte the oracle's"""
    assert g.tiles() == o.tiles() and len(o.tiles()) > 0, label
    bad = [t for t in o.tiles() if not np.array_equal(g.tile_bgra(*t), o.tile_bgra(*t))]
    assert bad == [], (label, bad[:6])


# ---------------------------------------------------------------- a. hostile frames, three witnesses
@pytest.mark.parametrize("size", sorted(CAMS))
@pytest.mark.parametrize("typ", ["TypeCPU", "TypeGPU"])
@pytest.mark.parametrize("weight_type", [0, 1])
@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_hostile_frames_hip_equals_model_and_oracle(pf, kind, weight_type, typ, size):
    wl = workloads()
    poses, prep, frames, o, m = witnesses(kind, weight_type, size)
    g = pf.Map2D.create(getattr(pf, typ), False, weight_type=weight_type)
    assert g.prepare(wl.IDENTITY_PLANE, CAMS[size], prep)
    for f, p in zip(frames, poses):
        assert g.feed(f, p)
    check(g, o, m, (kind, weight_type, typ, size))
    g.close()


PATH_KIND = {0: "checker2", 1: "step"}
SIZE = (257, 333)


@pytest.mark.parametrize("weight_type", [0, 1])
@pytest.mark.parametrize("path", ["lookahead0", "lookahead1", "lookahead3", "nocull", "thread", "bgra_padded", "device", "device_bgra", "jpeg"])
def test_other_ways_in_equal_the_model(pf, path, weight_type):
    """The same maps through every other way in: short lookaheads, the cull off, the render thread, BGRA host frames whose rows are
    padded (a view of a wider array: the binding hands its row step over), device-resident BGR and BGRA frames, and .jpg bytes (the
    model is then fed what decode_jpeg makes of the same bytes)."""
    wl = workloads()
    rows, cols = SIZE
    kind = PATH_KIND[weight_type]
    poses, prep, frames, o, m = witnesses(kind, weight_type, SIZE)
    opt = dict(weight_type=weight_type)
    if path.startswith("lookahead"):
        opt["lookahead"] = int(path[9:])
    if path.startswith("device"):
        opt["lookahead"] = 3                                              # the caller's buffers are read up to three feeds later
    g = pf.Map2D.create(pf.TypeCPU, path == "thread", **opt)
    if path == "nocull":
        g.set_cull(False)
    assert g.prepare(wl.IDENTITY_PLANE, CAMS[SIZE], prep)
    keep = []
    if path == "jpeg":
        streams = [jpeg_enc.encode(np.ascontiguousarray(f[:, :, ::-1])) for f in frames]
        decoded = [pf.decode_jpeg(s) for s in streams]
        assert all(d.shape == (rows, cols, 3) for d in decoded) and any(not np.array_equal(d, f) for d, f in zip(decoded, frames))
        o, m = model_pair(CAMS[SIZE], poses, prep, decoded, weight_type)
        for s, p in zip(streams, poses):
            assert g.feed(s, p)
    elif path == "bgra_padded":
        for k, (f, p) in enumerate(zip(frames, poses)):
            wide = np.full((rows, cols + 5, 4), 0xEE, np.uint8)
            view = wide[:, :cols]
            view[:, :, :3] = f; view[:, :, 3] = wl.noise_frame(rows, cols, 70 + k)[:, :, 0]
            assert view.strides[0] == 4 * (cols + 5) and not view.flags["C_CONTIGUOUS"]
            assert g.feed(view, p)
            got = g.read_last_frame()                                     # the bytes as they arrived: rows of the padded step
            assert got is not None and got.size == (rows - 1) * 4 * (cols + 5) + 4 * cols
            assert np.array_equal(got, wide.reshape(-1)[:got.size])
    elif path.startswith("device"):
        import torch
        cn = 4 if path == "device_bgra" else 3
        for k, (f, p) in enumerate(zip(frames, poses)):
            h = f if cn == 3 else np.dstack([f, wl.noise_frame(rows, cols, 80 + k)[:, :, :1]])
            keep.append(torch.from_numpy(np.ascontiguousarray(h)).cuda())
        torch.cuda.synchronize()
        for t, p in zip(keep, poses):
            assert g.feed_device(t.data_ptr(), rows, cols, p, channels=cn)
    else:
        for f, p in zip(frames, poses):
            assert g.feed(f, p)
    assert g.sync()
    if path == "thread":
        assert g.render_log() == list(range(N))                           # nothing dropped: the model holds exactly these keyframes
    if path == "nocull":
        assert g.culled_tiles() + g.culled_cells() == 0
    check(g, o, m, (path, weight_type))
    g.close()
    del keep


# ---------------------------------------------------------------- b. known answers: neither model nor oracle
def fed(pf, cam, prep, seq, **opt):
    wl = workloads()
    g = pf.Map2D.create(pf.TypeCPU, False, **opt)
    assert g.prepare(wl.IDENTITY_PLANE, cam, prep)
    g.set_cull(True)
    for f, p in seq:
        assert g.feed(f, p)
    assert g.sync()
    return g


def assert_same_map(a, b):
    assert a.tiles() == b.tiles() and len(b.tiles()) > 0
    for t in b.tiles():
        assert np.array_equal(a.tile_bgra(*t), b.tile_bgra(*t)), t


@pytest.mark.parametrize("lookahead", [0, 4, 48])
def test_same_pose_twice_equals_the_first_keyframe_alone(pf, lookahead):
    """Keyframe A, then B at the same pose: every alpha ties and the select is `<`, so A keeps every pixel, alpha included -- the
    opposite of the multi-band map (test_gpu_model.py).  With the cull on, at lookaheads where B waits beside A and where it does not."""
    rows, cols = SIZE
    poses = jitter_poses(3, seed=41, step=(30.0, 20.0))
    a_img, b_img = hostile_frame("checker1", rows, cols, 0), hostile_frame("impulse", rows, cols, 1)
    ab = fed(pf, CAMS[SIZE], poses, [(a_img, poses[1]), (b_img, poses[1])], lookahead=lookahead)
    a = fed(pf, CAMS[SIZE], poses, [(a_img, poses[1])], lookahead=lookahead)
    assert_same_map(ab, a)
    assert ab.stats()["rendered"] == 2
    ab.close(); a.close()


def test_a_b_a_at_one_pose_and_b_one_source_pixel_away(pf):
    """A, B, A at one pose: A alone.  A at pose p, then B one source pixel to the side: the alphas tie along lines only, B wins on one
    side of the centre and A keeps the other -- that map equals the model's."""
    rows, cols = SIZE
    cam = CAMS[SIZE]
    p = [5.0, 3.0, -100.0, 0, 0, 0, 1]
    a_img, b_img = hostile_frame("ramp", rows, cols, 0), hostile_frame("checker2", rows, cols, 1)
    aba = fed(pf, cam, [p], [(a_img, p), (b_img, p), (a_img, p)])
    a = fed(pf, cam, [p], [(a_img, p)])
    assert_same_map(aba, a)
    q = list(p); q[0] += 100.0 / cam[2]                                    # one source pixel: height / fx
    o, m = model_pair(cam, [p, q], [p], [a_img, b_img])
    g = fed(pf, cam, [p], [(a_img, p), (b_img, q)])
    check(g, o, m, "one pixel away")
    stored = sum(int((a.tile_bgra(*t)[:, :, 3] > 0).sum()) for t in a.tiles())
    lost = sum(int(((a.tile_bgra(*t)[:, :, 3] > 0) & (g.tile_bgra(*t) != a.tile_bgra(*t)).any(axis=2)).sum()) for t in a.tiles())
    assert m.tie_px > 0 and 0.25 * stored < lost < 0.75 * stored, (m.tie_px, lost, stored)      # B took about half of A's pixels
    for x in (aba, a, g):
        x.close()


@pytest.mark.parametrize("colour", [(255, 0, 37), (255, 255, 255), (0, 0, 0), (1, 254, 128)])
def test_constant_colour_keyframe(pf, colour):
    """One keyframe of one colour (white and black among them: the saturating pack of k_single2).  Where all four taps lay inside the
    frame the tile holds exactly the colour, and the alpha the model interpolates from the weight bytes; where none did, and wherever
    the alpha is 0, all four bytes are 0; every other pixel is on the rim (some taps outside), and the rim is as large as the model's.
    The geometry (which taps lie inside) is the model's; the colour needs no witness: the taps sum to 32768."""
    rows, cols = SIZE
    cam = CAMS[SIZE]
    pose = [3.0, -2.0, -100.0] + workloads().quat_axis((0, 0, 1), 0.2)
    img = np.broadcast_to(np.array(colour, np.uint8), (rows, cols, 3)).copy()
    o, m = model_pair(cam, [pose], [pose], [img])
    g = fed(pf, cam, [pose], [(img, pose)])
    (x0, y0, tx, ty) = m.last[0]
    canvas = np.zeros((ty * 256, tx * 256, 4), np.uint8)
    assert g.tiles() == m.tiles()
    for (ix, iy) in g.tiles():
        canvas[(iy - y0) * 256:(iy - y0 + 1) * 256, (ix - x0) * 256:(ix - x0 + 1) * 256] = g.tile_bgra(ix, iy)
    full, none = m.last_all_taps, m.last_no_tap
    rim = ~full & ~none
    assert full.sum() > 0.5 * rows * cols and rim.sum() > 0 and none.sum() > 0
    assert (canvas[full][:, :3] == np.array(colour, np.uint8)).all()
    assert np.array_equal(canvas[full][:, 3], m.last_dst[full][:, 3]) and canvas[full][:, 3].min() >= 2
    assert not canvas[none].any()
    assert not canvas[canvas[:, :, 3] == 0].any()
    other = ~((canvas[:, :, :3] == np.array(colour, np.uint8)).all(axis=2) & (canvas[:, :, 3] >= 2)) & canvas.any(axis=2)
    assert not (other & ~rim).any()                                        # nothing but colour or 0 off the rim
    assert int((canvas[:, :, 3] == 1).sum()) == m.rim_px > 0
    assert compare_single_with_model(g, m) == []
    g.close()


# ---------------------------------------------------------------- c. the lookahead and the cull, against the oracle (which renders everything)
CAM = CAMS[(480, 640)]


def sortie(wl, seed, n=18, **kw):
    rs = np.random.RandomState(6100 + seed)
    return wl.serpentine(CAM, float(rs.uniform(70, 130)), n, per_row=int(rs.randint(3, 7)), fwd_overlap=float(rs.uniform(0.6, 0.9)),
                         side_overlap=float(rs.uniform(0.4, 0.8)), seed=seed, yaw_jitter_deg=kw.get("yaw", 10.0),
                         tilt_jitter_deg=kw.get("tilt", 3.0), max_rows=3)


def frame(wl, seed, k):
    """noise with flat and checkerboard keyframes mixed in"""
    if k % 4 == 1:
        return hostile_frame("const", 480, 640, k + seed)
    if k % 4 == 3:
        return hostile_frame("checker2", 480, 640, k)
    return wl.noise_frame(480, 640, 100 * seed + k)


def pair(pf, orc, prep, thread=False, wt=0, scale=2.0, **opt):
    wl = workloads()
    g = pf.Map2D.create(pf.TypeCPU, thread, weight_type=wt, scale=scale, **opt)
    o = orc.OracleMap(single_band=1, weight_type=wt, scale=scale)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, prep) == o.prepare(wl.IDENTITY_PLANE, CAM, prep) == True
    return g, o


@pytest.mark.parametrize("lookahead", [0, 1, 2, 4, 9, 40, None])
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_every_lookahead_equals_the_oracle(pf, orc, seed, lookahead):
    """an overlapping serpentine, its start flown again at the end; None is the default lookahead"""
    wl = workloads()
    poses = sortie(wl, seed)
    poses = poses + [list(p) for p in poses[:4]]
    g, o = pair(pf, orc, poses[:8], wt=seed & 1, **({} if lookahead is None else {"lookahead": lookahead}))
    for k, p in enumerate(poses):
        img = frame(wl, seed, k)
        assert g.feed(img, p) == o.feed(img, p) == True
    assert g.sync() and g.grid() == o.grid()
    same_tiles(g, o)
    assert g.stats()["rendered"] == len(poses)
    assert g.culled_tiles() + g.culled_cells() > 0
    g.close()


def test_looking_at_the_map_between_feeds(pf, orc):
    """tile_bgra, blend_changed, save_to_memory and stats between feeds, with keyframes waiting: each sees the map after the keyframes
    fed so far -- the oracle's at that moment.  blend_changed lists the tiles of every canvas since it was last asked."""
    wl = workloads()
    poses = sortie(wl, 21, n=16)
    g, o = pair(pf, orc, poses[:8], lookahead=5)
    due = set()
    for k, p in enumerate(poses):
        img = frame(wl, 21, k)
        assert g.feed(img, p) == o.feed(img, p) == True
        (x0, y0, tx, ty), _ = o.last_canvas()
        due |= {(x, y) for x in range(x0, x0 + tx) for y in range(y0, y0 + ty)}
        if k % 4 == 1:
            assert g.stats() == {"rendered": k + 1, "rejected": 0, "dropped": 0}          # no sync: the reader renders what waits
            assert g.tiles() == o.tiles()
        if k % 5 == 2:
            same_tiles(g, o, k)
        if k % 6 == 3:
            changed, imgs = g.blend_changed()
            assert sorted(changed) == sorted(due), k
            for t, im in zip(changed, imgs):
                assert np.array_equal(im, o.tile_bgra(*t)[:, :, :3]), (k, t)
            due = set()
        if k in (6, 13):
            img_, (sx0, sy0) = g.save_to_memory()
            exp = np.zeros_like(img_)
            for (ix, iy) in o.tiles():
                exp[(iy - sy0) * 256:(iy - sy0 + 1) * 256, (ix - sx0) * 256:(ix - sx0 + 1) * 256] = o.tile_bgra(ix, iy)[:, :, :3]
            assert (sx0, sy0) == (min(t[0] for t in o.tiles()), min(t[1] for t in o.tiles())) and np.array_equal(img_, exp), k
    assert g.sync()
    same_tiles(g, o)
    assert g.culled_tiles() + g.culled_cells() > 0
    g.close()


def test_rejected_keyframes_and_a_moving_grid_among_waiting_keyframes(pf, orc):
    """an oblique keyframe is refused inside its own feed call (Map2DCPU.cpp:179-182) and one far outside the grid moves it at once
    (spreadMap), while accepted keyframes before them still wait"""
    wl = workloads()
    poses = sortie(wl, 31, n=14)
    steep = list(poses[5]); steep[3:] = wl.quat_axis((1, 0, 0), math.radians(75.0))
    far = [poses[0][0] - 900.0, poses[0][1] - 700.0, poses[0][2], 0, 0, 0, 1]
    seq = poses[:6] + [steep, far] + poses[6:] + [far] + poses[2:5]
    g, o = pair(pf, orc, poses[:8], lookahead=4)
    for k, p in enumerate(seq):
        img = frame(wl, 31, k)
        a, b = g.feed(img, p), o.feed(img, p)
        assert a == b, (k, a, b)
        assert g.grid()[0] == o.grid()[0], k
    assert g.sync()
    same_tiles(g, o)
    assert g.stats()["rejected"] == 1 and g.stats()["rendered"] == len(seq) - 1
    g.close()


def test_geometry_only_feed_among_waiting_keyframes(pf, orc):
    """feed(None, pose) -- a keyframe without pixels, as a shard gets it whose tiles the canvas does not touch -- between keyframes that
    wait (lookahead 4): the grid moves at once (spreadMap) and nothing else happens.  The tiles are those of maps that never saw that
    feed: byte for byte an oracle's that was fed a frame at that pose (the same grid history), less the tiles of that far canvas; the
    tile set also an oracle's that skipped the feed; the grid the first oracle's.  A HIP map at lookahead 0 answers the same."""
    wl = workloads()
    poses = sortie(wl, 33, n=14)
    far = [poses[0][0] - 900.0, poses[0][1] - 700.0, poses[0][2], 0, 0, 0, 1]
    g, o_far = pair(pf, orc, poses[:8], lookahead=4)
    g0, o_skip = pair(pf, orc, poses[:8], lookahead=0)
    far_tiles = set()
    for k, p in enumerate(poses[:6] + [far] + poses[6:] + [far] + poses[2:5]):
        if p is far:
            before = g.grid()
            assert g.feed(None, p) == g0.feed(None, p) == True
            assert o_far.feed(frame(wl, 33, k), p)
            (x0, y0, tx, ty), _ = o_far.last_canvas()
            far_tiles |= {(x, y) for x in range(x0, x0 + tx) for y in range(y0, y0 + ty)}
            assert g.grid() == g0.grid() == o_far.grid()                   # inside the feed call, with keyframes waiting
            assert k > 6 or g.grid() != before
            continue
        img = frame(wl, 33, k)
        assert g.feed(img, p) == g0.feed(img, p) == o_far.feed(img, p) == o_skip.feed(img, p) == True
    assert g.sync() and g0.sync()
    assert g.grid() == o_far.grid()
    near = [t for t in o_far.tiles() if t not in far_tiles]
    assert len(near) > 0 and len(far_tiles) > 0 and not far_tiles & set(o_skip.tiles())
    assert g.tiles() == g0.tiles() == near == o_skip.tiles()
    for t in near:
        assert np.array_equal(g.tile_bgra(*t), o_far.tile_bgra(*t)) and np.array_equal(g0.tile_bgra(*t), o_far.tile_bgra(*t)), t
    assert g.stats()["rejected"] == 0 and g.culled_tiles() + g.culled_cells() > 0
    g.close(); g0.close()


def test_prepare_again_with_keyframes_waiting(pf, orc):
    wl = workloads()
    poses = sortie(wl, 41, n=12)
    g, o = pair(pf, orc, poses[:8], lookahead=8)
    for rnd in range(2):
        if rnd:
            assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:8]) == o.prepare(wl.IDENTITY_PLANE, CAM, poses[:8]) == True
        for k, p in enumerate(poses[: 7 + 5 * rnd]):
            img = frame(wl, 41 + rnd, k)
            assert g.feed(img, p) == o.feed(img, p) == True
    assert g.sync() and g.grid() == o.grid()
    same_tiles(g, o)
    g.close()


@pytest.mark.parametrize("lookahead", [0, 48])
def test_threaded_map_with_lookahead(pf, orc, lookahead):
    wl = workloads()
    poses = sortie(wl, 51, n=16)
    g, o = pair(pf, orc, poses[:8], thread=True, lookahead=lookahead)
    imgs = [frame(wl, 51, k) for k in range(len(poses))]
    for k, p in enumerate(poses):
        assert g.feed(imgs[k], p)
    assert g.sync()
    log = g.render_log()
    assert log == sorted(log) and len(log) == g.stats()["rendered"] > 0
    for k in log:                                                          # the keyframes the queue did not drop, in order
        assert o.feed(imgs[k], poses[k])
    same_tiles(g, o)
    g.close()


@pytest.mark.parametrize("block", [1, 8])
@pytest.mark.parametrize("count", [2, 3])
def test_shards_partition_the_unsharded_map(pf, orc, count, block):
    wl = workloads()
    poses = sortie(wl, 61, n=14)
    poses = poses + [list(p) for p in poses[:3]]
    scale = 2.0 if block == 1 else 4.0                                     # (blocks of 8 x 8 tiles: a mosaic that spans several of them)
    g, o = pair(pf, orc, poses[:8], scale=scale)
    shards = []
    for r in range(count):
        s = pf.Map2D.create(pf.TypeCPU, False, scale=scale, shard_count=count, shard_rank=r, shard_block=block)
        assert s.prepare(wl.IDENTITY_PLANE, CAM, poses[:8])
        shards.append(s)
    for k, p in enumerate(poses):
        img = frame(wl, 61, k)
        assert g.feed(img, p) == o.feed(img, p) == True
        for s in shards:
            assert s.feed(img, p)
    assert g.sync()
    same_tiles(g, o)
    got = {}
    for r, s in enumerate(shards):
        assert s.sync()
        for t in s.tiles():
            assert t not in got and pf.tile_owner(s.opt, *t) == r
            got[t] = s.tile_bgra(*t)
    assert sorted(got) == sorted(g.tiles())
    assert sum(1 for s in shards if s.tiles()) >= 2                        # a real partition
    for t in g.tiles():
        assert np.array_equal(got[t], g.tile_bgra(*t)), t
    assert g.culled_tiles() + g.culled_cells() > 0
    for s in shards + [g]:
        s.close()


@pytest.mark.parametrize("scale", [0.5, 3.0])
def test_weight_type_1_at_other_scales(pf, orc, scale):
    wl = workloads()
    poses = wl.serpentine(CAM, 90.0, 16, per_row=4, fwd_overlap=0.85, side_overlap=0.7, seed=78, yaw_jitter_deg=20.0, tilt_jitter_deg=6.0, max_rows=4)
    g, o = pair(pf, orc, poses[:8], wt=1, scale=scale, lookahead=6)
    for k, p in enumerate(poses + poses[:3]):
        img = frame(wl, 78, k)
        assert g.feed(img, p) == o.feed(img, p) == True
    assert g.sync() and g.grid() == o.grid()
    same_tiles(g, o)
    assert g.culled_tiles() + g.culled_cells() > 0
    g.close()


# the margin case: chosen on the CPU by scanning MARGIN_DX with the model for cells in [-6, 0] (several between 20 m and 22.3 m)
MARGIN_DX = 20.75                                                          # metres between the two passes, at one height


def test_cells_in_the_margin_of_the_cull(pf, orc):
    """Two passes at one height, MARGIN_DX to the side of one another, frame axes on the canvas axes.  Over whole 64 x 64 cells of the
    later keyframe's canvas its largest alpha lies 0 to 6 steps below the smallest alpha stored there: it cannot win anywhere in such
    a cell, but only just -- the cull (fusion_map.cpp, sb_gap = 3.2 / 254) may leave a cell out only where its bounds are 3.2 steps
    apart, so cells at -4 and below may go and cells at -3 .. 0 must stay.  Beside them lie cells where the gap is +1 .. +3: there the
    later keyframe wins pixels by the smallest margins there are, and a cull that dropped such a cell would show in the bytes.  The
    model alone shows the case to be there (cells on both sides of the gap, and the small positive ones); then the map, with cells
    culled, is the oracle's and the model's byte for byte.

    One keyframe per pass suffices: the cull decides cell by cell from the bounds of the keyframes whose canvas held the tile, and a
    second keyframe along a pass would only raise the stored bound in cells this one leaves in the margin, moving them out of it.
    (The host's bounds carry 2 source pixels of slack on either side besides sb_gap -- about 2.5 alpha steps at this frame size -- so
    a cull with sb_gap = 0 still drops no cell of this case that it should keep.)"""
    rows, cols = 480, 640
    a_img, b_img = hostile_frame("ramp", rows, cols, 0), hostile_frame("checker2", rows, cols, 1)
    pa, pb = [0.0, 0.0, -100.0, 0, 0, 0, 1], [MARGIN_DX, 0.0, -100.0, 0, 0, 0, 1]
    o, m = model_pair(CAM, [pa], [pa, pb], [a_img])
    before = {t: m.tile_bgra(*t) for t in m.tiles()}
    assert feed_single_with_model(o, m, b_img, pb) and compare_single_with_model(o, m) == []
    x0, y0, tx, ty = m.last[0]
    gaps = []
    for cy in range(4 * ty):
        for cx in range(4 * tx):
            t = before.get((x0 + cx // 4, y0 + cy // 4))
            if t is None:
                continue
            stored = t[(cy % 4) * 64:(cy % 4 + 1) * 64, (cx % 4) * 64:(cx % 4 + 1) * 64, 3]
            new = m.last_dst[cy * 64:(cy + 1) * 64, cx * 64:(cx + 1) * 64, 3]
            if stored.min() > 0 and new.max() > 0:
                gaps.append(int(new.max()) - int(stored.min()))
    margin = sorted(g for g in gaps if -6 <= g <= 0)
    just_over = sorted(g for g in gaps if 1 <= g <= 3)
    assert len(margin) >= 5 and margin[0] <= -4 and margin[-1] >= -1, margin
    assert len(just_over) >= 1, sorted(gaps)
    for lookahead in (0, 48):
        g = fed(pf, CAM, [pa, pb], [(a_img, pa), (b_img, pb)], lookahead=lookahead)
        assert g.culled_tiles() + g.culled_cells() > 0
        check(g, o, m, ("margin", lookahead))
        g.close()
