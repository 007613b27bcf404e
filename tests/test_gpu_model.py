"""The HIP path against the independent model (map_model.py) and the oracle on hostile frames (helpers.hostile_frame): saturated,
flat and pixel-sharp content that drives the int16 level kernel's packed 16-bit stages to the top of their ranges (kernels.hip), the
8U clamp to both ends after a mixed-frame collapse, and sharp edges across 64-px warp blocks and tile borders.  The model is the
witness that shares no arithmetic with either side; the oracle is the third.  Known answers and a float64 collapse at the end need
neither."""
import math

import numpy as np
import pytest

from helpers import HOSTILE_KINDS, compare_with_model, feed_with_model, hostile_frame, jitter_poses, neighbourhoods, workloads
from map_model import ModelMap, np_pyr_up_int

pytestmark = pytest.mark.gpu

CAM = [333, 257, 260, 260, 166.5, 128.5]
ROWS, COLS = 257, 333
N = 4
BG = 201
MIXED = ("const", "checker2", "const", "step")                    # keyframe kinds of a mosaic whose collapse leaves [0, 255]
LATTICE = ((0.0, 0.0), (80.0, 0.0), (0.0, 90.0), (80.0, 90.0))     # 2 x 2 keyframes: 3 x 3 tiles and more, a middle with all nine


def lattice_poses(seed):
    """jitter_poses' rotations and heights (every 32 x 32 sub-pixel phase of the warp) on the LATTICE positions"""
    poses = jitter_poses(N, seed=seed, step=(0.0, 0.0))
    for p, (x, y) in zip(poses, LATTICE):
        p[0] += x; p[1] += y
    return poses


def step_position(o, pose):
    """The frame column whose canvas column is the 64-px block boundary nearest the frame's middle, and the frame row on a tile
    border (identity rotation, so frame axes are canvas axes; the grid must not move in this feed)."""
    _, geo = o.grid()
    pts = o.footprint(pose)
    es, lp = geo[4], geo[5]
    xs = geo[0] + es * math.floor((pts[:, 0].min() - geo[0]) / es)
    ys = geo[1] + es * math.floor((pts[:, 1].min() - geo[1]) / es)
    sx, sy = (pts[1, 0] - pts[0, 0]) / COLS, (pts[2, 1] - pts[0, 1]) / ROWS          # plane units per frame pixel
    X = lambda u: (pts[0, 0] + sx * u - xs) / lp
    Y = lambda v: (pts[0, 1] + sy * v - ys) / lp
    cx = 64 * round(X(COLS / 2) / 64)
    cy = 256 * math.ceil(Y(0) / 256)
    u = int(round((cx * lp + xs - pts[0, 0]) / sx))
    v = int(round((cy * lp + ys - pts[0, 1]) / sy))
    assert 0 < u < COLS and 0 < v < ROWS and abs(X(u) - cx) < 1 and abs(Y(v) - cy) < 1
    return u, v


def witnesses(kind, ff, bands):
    """Oracle and model fed the same keyframes; jittered poses (every sub-pixel phase, spreadMap after a grid from two poses) except
    for "step", whose poses keep the frame axes on the canvas axes so that its edges land where step_position puts them."""
    from oracle import orc
    wl = workloads()
    o = orc.OracleMap(band_num=bands, force_float=ff, bg_color=BG)
    m = ModelMap(band_num=bands, force_float=ff, bg_color=BG)
    if kind == "step":
        poses = [[x + 0.37 * k, y + 0.29 * k, -100.0, 0, 0, 0, 1] for k, (x, y) in enumerate(LATTICE)]
        prep = poses
    else:
        poses = lattice_poses(11 + bands)
        prep = poses[:2]
    assert o.prepare(wl.IDENTITY_PLANE, CAM, prep)
    frames = []
    for k, p in enumerate(poses):
        sc, sr = step_position(o, p) if kind == "step" else (None, None)
        frames.append(hostile_frame(kind, ROWS, COLS, k, sc, sr))
        assert feed_with_model(o, m, frames[-1], p)
    return poses, prep, frames, o, m


def check(g, o, m, label):
    assert g.sync()
    assert g.grid() == o.grid(), label
    bad = compare_with_model(g, m)
    assert bad == [], (label, bad[:8])
    tiles = m.tiles()
    for t, im in zip(tiles, g.blend_tiles(tiles)):
        assert np.array_equal(im, m.blend_tile(*t)), (label, "blend_tiles", t)


def run_path(pf, path, poses, prep, frames, ff, bands):
    wl = workloads()
    opt = dict(force_float=ff, band_number=bands, bg_color=BG)
    if path == "unfused":
        opt["fused"] = 0
    if path == "device":
        opt["lookahead"] = 3
    g = pf.Map2D.create(pf.TypeMultiBandCPU, path == "thread", **opt)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, prep)
    if path == "device":
        import torch
        keep = [torch.from_numpy(f).cuda() for f in frames]
        torch.cuda.synchronize()
        for t, p in zip(keep, poses):
            assert g.feed_device(t.data_ptr(), ROWS, COLS, p)
        assert g.sync()
        del keep
    else:
        for f, p in zip(frames, poses):
            assert g.feed(f, p)
        assert g.sync()
    if path == "thread":
        assert g.render_log() == list(range(N))                       # nothing dropped: the model holds every keyframe
    return g


@pytest.mark.parametrize("bands", [1, 5, 8])
@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_hostile_frames_hip_equals_model_and_oracle(pf, kind, force_float, bands):
    """The product path (fused, default lookahead and cull) at 1, 5 and 8 bands; at 5 bands also fused = 0, device-resident frames
    with the lookahead on, and thread = true.  Whole map, blend_tile(_raw) of every tile, blend_tiles and save, bit for bit."""
    poses, prep, frames, o, m = witnesses(kind, force_float, bands)
    assert compare_with_model(o, m) == []                               # the oracle agrees with the model ...
    full, alone = neighbourhoods(m.tiles())
    assert full and alone
    paths = ["product"] + (["unfused", "device", "thread"] if bands == 5 else [])
    for path in paths:                                                  # ... and so does every HIP path
        g = run_path(pf, path, poses, prep, frames, force_float, bands)
        check(g, o, m, (kind, path))
        g.close()
    if force_float == 0:
        s = m.stats
        if kind in ("white", "const", "step"):
            # the bounds of the packed 16-bit stages, reached: 5-tap 255*16, vertical 65280 (+128 = 65408 in 16 unsigned bits),
            # pyrUp 255*64
            assert (s["h5"], s["v5"], s["up"]) == (4080, 65280, 16320), s
        if kind == "impulse":
            # 239 is the largest |Laplacian| 8-bit content can give (test_model_oracle.py); the warp's phases decide how close
            assert s["lap"] >= 235, s
        if kind in ("checker1", "checker2"):
            assert s["lap"] >= 128, s
        if kind == "noise":
            assert s["v5"] < 65280 and s["lap"] < 239, s                # the control does not get there


@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_single_band_hostile_frames(pf, orc, kind):
    """Map2DCPU (TypeCPU) on the same frames against the oracle, through tile_bgra (the single-band map has its own model,
    ModelMapSingleBand, and its own three-witness cases: test_gpu_single_band_model.py)."""
    wl = workloads()
    poses = jitter_poses(N, seed=29, step=(30.0, 20.0))
    g = pf.Map2D.create(pf.TypeCPU, False)
    o = orc.OracleMap(single_band=1)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2]) and o.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
    for k, p in enumerate(poses):
        img = hostile_frame(kind, ROWS, COLS, k)
        assert g.feed(img, p) == o.feed(img, p) == True
    assert g.sync()
    assert g.grid() == o.grid() and g.tiles() == o.tiles()
    for t in o.tiles():
        assert np.array_equal(g.tile_bgra(*t), o.tile_bgra(*t)), t
    g.close()


# ---------------------------------------------------------------- known answers: neither model nor oracle
@pytest.mark.parametrize("force_float", [0, 1])
def test_same_pose_twice_equals_the_second_keyframe_alone(pf, force_float):
    """Keyframe A, then keyframe B at the same pose: the weights are equal and the select is `>=`, so B wins every pixel of every
    level and the map equals a map fed B alone (with the cull and the lookahead on)."""
    wl = workloads()
    poses = jitter_poses(3, seed=41, step=(30.0, 20.0))
    a_img, b_img = hostile_frame("checker1", ROWS, COLS, 0), hostile_frame("impulse", ROWS, COLS, 1)
    ab = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float, lookahead=4)
    b = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float, lookahead=4)
    for g in (ab, b):
        assert g.prepare(wl.IDENTITY_PLANE, CAM, poses)
        g.set_cull(True)
    assert ab.feed(a_img, poses[1]) and ab.feed(b_img, poses[1]) and b.feed(b_img, poses[1])
    assert ab.sync() and b.sync()
    assert ab.tiles() == b.tiles() and len(b.tiles()) > 0
    for t in b.tiles():
        for lv in range(b.num_levels):
            (la, wa), (lb, wb) = ab.tile_level(*t, lv), b.tile_level(*t, lv)
            assert np.array_equal(la, lb) and np.array_equal(wa, wb), (t, lv)
        assert np.array_equal(ab.blend_tile_raw(*t), b.blend_tile_raw(*t)), t
    ab.close(); b.close()


@pytest.mark.parametrize("force_float", [0, 1])
def test_constant_colour_keyframe(pf, force_float):
    """One constant-colour keyframe (channels 0, 255 and 37): the canvas is that colour everywhere (REFLECT border), so every
    Laplacian level below the top is zero and the top level holds the colour; blend_tile gives the colour on every weight > 0
    pixel of a tile whose nine neighbours all hold it, and 0 elsewhere.  int16 exactly; fp32 levels within a few ulp, its 8U
    view exactly."""
    wl = workloads()
    cam = [800, 800, 400, 400, 400, 400]                               # about 3 x 3 tiles and more: full neighbourhoods
    pose = [3.0, -2.0, -100.0] + wl.quat_axis((0, 0, 1), 0.2)
    colour = np.array([0, 255, 37], np.uint8)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float)
    assert g.prepare(wl.IDENTITY_PLANE, cam, [pose])
    assert g.feed(np.broadcast_to(colour, (800, 800, 3)).copy(), pose) and g.sync()
    full, _ = neighbourhoods(g.tiles())
    assert full
    top = g.num_levels - 1
    c = colour.astype(np.float32) * np.float32(1. / 255.) if force_float else colour.astype(np.int16)
    for t in g.tiles():
        for lv in range(g.num_levels):
            lap, _ = g.tile_level(*t, lv)
            if force_float:
                assert np.abs(lap - (c if lv == top else 0)).max() <= 1e-6, (t, lv)
            else:
                assert (lap == (c if lv == top else 0)).all(), (t, lv)
    for t in full:
        _, w0 = g.tile_level(*t, 0)
        out = g.blend_tile(*t)
        assert (out[w0 > 0] == colour).all() and (out[w0 == 0] == 0).all(), t
    g.close()


# ---------------------------------------------------------------- a collapse done here, in float64 / int64
def _up(a, scale):
    """pyrUp of a float64 array: rows and columns [1 6 1] / [4 4] with index -1 -> 1 and n -> n-1, divided by `scale`; with scale
    None the 16S rule instead, (v + 32) >> 6 cast to int16."""
    if scale is None:
        return np_pyr_up_int(a)

    def ax(a, axis):
        a = np.moveaxis(a, axis, 0); n = a.shape[0]
        prev = a[[1 if n > 1 else 0] + list(range(n - 1))]; nxt = a[list(range(1, n)) + [n - 1]]
        out = np.empty((2 * n,) + a.shape[1:]); out[0::2] = prev + 6 * a + nxt; out[1::2] = 4 * (a + nxt)
        return np.moveaxis(out, 0, axis)
    return ax(ax(a, 1), 0) / scale


@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("kind", ["mixed", "checker2"])
def test_blend_equals_a_collapse_done_here(pf, kind, force_float):
    """Every tile's levels read back (with the 3 x 3 halo of 1 << (nl-1-i) pixels where all nine tiles exist) and collapsed here:
    fp32 in float64, where blend_tile_raw must lie within the rounding bound of the fp32 collapse (per level: pyrUp at most 6u of
    its input's magnitude -- three roundings in each direction, weights summing to 8 -- and the add u of its result, u = 2^-24;
    pyrUp passes earlier errors on with gain 1); int16 in int64 with the 16S casts and saturating adds, where it must be equal, and
    blend_tile must be that collapse clamped to [0, 255].  The keyframes ("mixed": flat, checkerboard and step content side by side)
    make the collapse overshoot both ends of the 8-bit range."""
    wl = workloads()
    poses = lattice_poses(23)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, poses)
    for k, p in enumerate(poses):
        assert g.feed(hostile_frame(MIXED[k] if kind == "mixed" else kind, ROWS, COLS, k), p)
    assert g.sync()
    nl, tiles = g.num_levels, g.tiles()
    assert all(neighbourhoods(tiles))
    have, lv_cache = set(tiles), {}

    def level(t, i):
        if (t, i) not in lv_cache:
            lv_cache[(t, i)] = g.tile_level(*t, i)[0]
        return lv_cache[(t, i)]

    u = 2.0 ** -24
    below = above = 0
    for (ix, iy) in tiles:
        if all((ix + dx, iy + dy) in have for dx in (-1, 0, 1) for dy in (-1, 0, 1)):
            lv = []
            for i in range(nl):
                b, s = 1 << (nl - 1 - i), 256 >> i
                big = np.concatenate([np.concatenate([level((ix + dx, iy + dy), i) for dx in (-1, 0, 1)], axis=1)
                                      for dy in (-1, 0, 1)], axis=0)
                lv.append(big[s - b:2 * s + b, s - b:2 * s + b])
            b0 = 1 << (nl - 1)
        else:
            lv, b0 = [level((ix, iy), i) for i in range(nl)], 0
        raw = g.blend_tile_raw(ix, iy)
        w0 = g.tile_level(ix, iy, 0)[1]
        if force_float:
            G, bound = lv[-1].astype(np.float64), 0.0
            for i in range(nl - 2, -1, -1):
                up = _up(G, 64.0)
                G = up + lv[i]
                bound += 6 * u * np.abs(up).max() * 1.01 + u * np.abs(G).max() * 1.01
            exp = G[b0:b0 + 256, b0:b0 + 256]
            err = np.abs(raw.astype(np.float64) - exp)[w0 > 0]
            assert err.max() <= bound, ((ix, iy), err.max(), bound)
            top = 1.0
        else:
            G = lv[-1].astype(np.int16)
            for i in range(nl - 2, -1, -1):
                G = np.clip(_up(G, None).astype(np.int64) + lv[i], -32768, 32767).astype(np.int16)
            exp = G[b0:b0 + 256, b0:b0 + 256]
            assert np.array_equal(raw[w0 > 0], exp[w0 > 0]), (ix, iy)
            assert np.array_equal(g.blend_tile(ix, iy)[w0 > 0], np.clip(exp, 0, 255)[w0 > 0]), (ix, iy)
            top = 255
        assert (raw[w0 == 0] == 0).all()
        below += int((exp[w0 > 0] < 0).sum()); above += int((exp[w0 > 0] > top).sum())
    assert below > 0 and above > 0, (below, above)                     # the 8U view clamps at both ends
    g.close()
