"""The cull on canvases too large for the kernel arguments, against the oracle: product library, default switches.

By which rule a block of the level kernel decides whether it runs (k_levels' prologue, kernels.hip) follows from the size of the keyframe's
canvas alone, and every other GPU test of the cull stays on canvases of at most 256 tiles, where the tile table travels in the kernel
arguments and the level-0 blocks test themselves against it.  The sorties here cross each threshold with the smallest canvas that does:

  A   17 x 16 to 18 x 18 tiles (272 entries and more > kArgTable): the table is staged and copied, level 0 takes the need rectangles, the upper levels' need
      bitmaps still fit the launch
  B   19 x 18 to 20 x 18: level 1's bitmap fits kNeedWords by itself (at most 90 of 100 words on every canvas of the sortie, asserted), the jobs of
      one launch together do not -- some fall back to the (at most four, merged) rectangles
  C   22 x 22 and 23 x 22: level 1 alone needs more than kNeedWords and takes the rectangles, the levels above keep their bitmaps: one launch, both forms
  D   34 x 6: 4 * tx > 128 cells across, no bitmaps: every upper level of these canvases takes the rectangles (204 entries: level 0 still
      tests itself against the table in the arguments)      D'  its transpose, 6 x 34: the bitmaps stay, the rule is about the width
  E   seven bands on 17 x 16 and 17 x 17: a reach of 382 px (no in-kernel test at any canvas size), cells dilated by 256 px; the plan makes
      rectangles at every level, and the six upper-level jobs of a launch carry their bitmaps all the same (they fit: asserted)
  F   two shards with shard_block = 1 on 12 x 12 tiles: more than 64 hash cells, CellList overflows and every block runs; and a pair of
      shards with 4 x 4-tile cells on shape A, whose rectangles are merged

pf_debug_admission_counts says which rule the launches took; every case asserts the counters of the form it is named after, so that none
passes on a silent fall-back to the small-canvas form.  (The counters are sums over the launches of a sortie: they tell that a form ran,
not in which launch.)

A canvas is the keyframe's footprint, so a camera of W x H pixels at Map2D.Scale 8 gives one of about W / 32 x H / 32 tiles: the frames are
a few hundred pixels a side, and the oracle's render of the canvases is the cost of a case.  Per sortie: six keyframes, forward overlap
0.82, each shifted sideways by a few cells so that the box around its rendered cells stays the whole canvas, yaw drawn from
{0, 45, 180} degrees (the 45-degree ones flown lower, so that their canvases stay as large as the others'), tilt up to 1.5 degrees, noise and
smooth frames alternating, and the first three keyframes fed again at the end.  The oracle's map of a sortie is computed once and shared
by the runs that differ in the lookahead only.  tools/cull_soak.py --large runs the same generator over many seeds."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import compare_maps, workloads

pytestmark = pytest.mark.gpu

F = 500.0          # focal length, pixels
HEIGHT = 100.0     # flight height over the plane, metres
SCALE = 8.0        # Map2D.Scale: canvas pixels per frame pixel at HEIGHT
N_KEY = 6
K_ARG_TABLE, K_NEED_WORDS, BH = 256, 100, 32      # plan_limits.hpp, the level kernel's block rows

# case -> (frame width, frame height, bands, flight axis): footprints of n + 0.25 tiles, i.e. n + 1 or n + 2 tiles of canvas
SHAPES = {
    "A": (520, 488, 5, "y"),
    "B": (584, 520, 5, "y"),
    "C": (680, 648, 5, "y"),
    "D": (1064, 168, 5, "y"),
    "Dt": (168, 1064, 5, "x"),
    "E": (520, 488, 7, "y"),
    "F": (360, 360, 5, "y"),
}


def sortie(case, seed=0):
    """-> (camera, bands, poses, yaws in degrees): N_KEY keyframes and the first three again"""
    wl = workloads()
    w, h, bands, axis = SHAPES[case]
    cam = [w, h, F, F, w // 2, h // 2]
    rs = np.random.RandomState(7100 + 31 * seed + sum(map(ord, case)))
    yaws = [0.0, 45.0, 180.0] + [float(rs.choice([0.0, 45.0, 180.0])) for _ in range(N_KEY - 3)]
    rs.shuffle(yaws)
    along, across = (h, w) if axis == "y" else (w, h)                 # frame pixels along / across the flight
    step = 0.18 * along * HEIGHT / F                                   # forward overlap 0.82
    poses = []
    for k, yaw in enumerate(yaws):
        # sideways by 1.5 - 3 cells of 64 canvas pixels, alternating: every keyframe sticks out of the ones before it along one whole side
        side = (1 if k & 1 else -1) * float(rs.uniform(96, 192)) / SCALE * HEIGHT / F
        # a frame yawed 45 degrees has a canvas (w + h) / sqrt(2) a side: flown lower, so that it stays near the others' tile count
        low = 1.0 if yaw != 45.0 else (0.3 if max(w, h) > 3 * min(w, h) else math.sqrt(2.0) * max(w, h) / (w + h))
        q = wl.quat_mul(wl.quat_axis((0, 0, 1), math.radians(yaw)),
                        wl.quat_mul(wl.quat_axis((0, 1, 0), math.radians(float(rs.uniform(-1.5, 1.5)))), wl.quat_axis((1, 0, 0), math.radians(float(rs.uniform(-1.5, 1.5))))))
        f, s = k * step + float(rs.uniform(-0.3, 0.3)), side
        poses.append(([s, f] if axis == "y" else [f, s]) + [-HEIGHT * low] + q)
    return cam, bands, poses + [list(p) for p in poses[:3]], yaws + yaws[:3]


def frame(cam, seed, k):
    wl = workloads()
    return wl.noise_frame(cam[1], cam[0], 100 * seed + k) if k & 1 else wl.smooth_frame(cam[1], cam[0], k)


def admission():
    from conftest import load_package
    c = (C.c_longlong * 8)()
    load_package().lib().pf_debug_admission_counts(c)
    return np.array(list(c), dtype=np.int64)


def level1_words(tx, ty):
    """words of the level-1 need bitmap when the compute region is the whole canvas (its most)"""
    return ((tx * 128 + 63) // 64 * ((ty * 128 + BH - 1) // BH) + 31) // 32


def joint_words(tx, ty, bands):
    """... and of the bitmaps of levels 1 .. bands - 1 together, as one launch carries them for keyframes of this canvas"""
    return sum((((tx * 256 >> i) + 63) // 64 * (((ty * 256 >> i) + BH - 1) // BH) + 31) // 32 for i in range(1, bands))


_oracle = {}


def oracle_map(orc, case, force_float, weight_type=0, seed=0):
    """The oracle's map of a sortie and the canvas (tile x0, y0, tiles across, tiles down) of each keyframe, made once per (case, pyramid
    type) and kept while the runs that differ in the lookahead alone follow each other; never changed after it is made."""
    key = (case, force_float, weight_type, seed)
    if key not in _oracle:
        for k in [k for k in _oracle if (k[0], k[3]) != ("A", 0)]:      # (shape A's maps of the tests' own seed serve the shard pair as well)
            del _oracle[k]
        wl = workloads()
        cam, bands, poses, _ = sortie(case, seed)
        o = orc.OracleMap(force_float=force_float, scale=SCALE, band_num=bands, weight_type=weight_type)
        assert o.prepare(wl.IDENTITY_PLANE, cam, poses[:N_KEY])
        canvases = []
        for k, p in enumerate(poses):
            assert o.feed(frame(cam, seed, k), p), (case, k)
            canvases.append(tuple(o.last_canvas()[0]))
        _oracle[key] = (o, canvases)
    return _oracle[key]


def compare_tiles(g, o, tiles):
    """compare_maps for the tiles a shard holds"""
    bad = []
    for (ix, iy) in tiles:
        for lv in range(o.num_levels):
            (gl, gw), (ol, ow) = g.tile_level(ix, iy, lv), o.tile_level(ix, iy, lv)
            if not (np.array_equal(gl, ol) and np.array_equal(gw, ow)):
                bad.append("tile (%d,%d) level %d: %d values, %d weights differ" % (ix, iy, lv, int((gl != ol).sum()), int((gw != ow).sum())))
    return bad


def run_gpu(pf, case, force_float, lookahead, weight_type=0, seed=0, canvases=None, flags=True, **shard):
    """One map fed the sortie, one sync at the end; with flags, one more before the last keyframe, where the changed flags are cleared
    (draw()).  -> (map, coordinates and pixels of the tiles flagged by the last keyframe, movement of the admission counters)"""
    wl = workloads()
    cam, bands, poses, _ = sortie(case, seed)
    opt = dict(force_float=force_float, fused=1, scale=SCALE, band_number=bands, weight_type=weight_type, **shard)
    if lookahead is not None:
        opt["lookahead"] = lookahead
    before = admission()
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, **opt)                 # thread = 0
    assert g.prepare(wl.IDENTITY_PLANE, cam, poses[:N_KEY])
    for k, p in enumerate(poses[:-1]):
        assert g.feed(frame(cam, seed, k), p), (case, k)
    if not flags:
        assert g.feed(frame(cam, seed, len(poses) - 1), poses[-1]) and g.sync()
        return g, None, None, admission() - before
    assert g.sync()
    cap = 2 * max(c[2] * c[3] for c in canvases) if canvases else 2048
    g.blend_changed(cap=cap)
    assert g.feed(frame(cam, seed, len(poses) - 1), poses[-1]) and g.sync()
    coords, px = g.blend_changed(cap=cap)
    return g, coords, px, admission() - before


# what the counters must show, per case: (must have moved, must not have moved)
FORMS = {
    "A": ([1, 3, 4], [0]),
    "B": ([1, 3, 4, 5], [0]),
    "C": ([1, 3, 4, 5, 7], [0]),
    "D": ([0, 5], []),               # (204 entries: the table still travels in the arguments; its 45-degree keyframes, 9 x 9 tiles, carry bitmaps)
    "Dt": ([0, 4], [5]),             # the asymmetry: 34 tiles down keep the bitmaps that 34 tiles across lose
    "E": ([1, 3, 4, 7], [0, 5]),
}


def check_shapes(case, bands, canvases, yaws):
    """the canvases of the sortie are on the side of each threshold that the case is named after (geometry alone: the oracle's canvases)"""
    straight = [c for c, y in zip(canvases, yaws) if y != 45.0]
    if case in ("A", "B", "C", "E"):
        assert all(c[2] * c[3] > K_ARG_TABLE for c in canvases), canvases                     # no keyframe's table fits the arguments
        assert all(c[2] <= 32 for c in canvases), canvases                                    # bitmaps are made
    if case == "A":
        assert any(joint_words(c[2], c[3], bands) <= K_NEED_WORDS for c in straight), canvases
    if case == "B":
        # level 1 alone fits on every canvas, so a job that took the rectangles did so because the launch's jobs did not fit together
        assert all(level1_words(c[2], c[3]) <= K_NEED_WORDS for c in canvases), canvases
        assert all(joint_words(c[2], c[3], bands) > K_NEED_WORDS for c in straight), canvases
    if case == "C":
        assert all(level1_words(c[2], c[3]) > K_NEED_WORDS for c in straight), canvases
    if case == "D":
        assert all(c[2] >= 33 and c[3] <= 7 for c in straight), canvases
    if case == "Dt":
        assert all(c[3] >= 33 and c[2] <= 7 for c in straight), canvases
        assert all(c[2] <= 32 for c in canvases), canvases                                    # never too wide: bitmaps on every canvas


@pytest.mark.parametrize("lookahead", [None, 0])
@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("case", ["A", "B", "C", "D", "Dt", "E"])
def test_large_canvas_sortie_equals_oracle(pf, orc, case, force_float, lookahead):
    """(figures: DESIGN.md section 4, "the cull on large canvases")"""
    weight_type = 1 if case == "B" else 0                              # WeightType 1 (.cpp:407-414) on one case
    cam, bands, poses, yaws = sortie(case)
    o, canvases = oracle_map(orc, case, force_float, weight_type)
    check_shapes(case, bands, canvases, yaws)
    g, coords, px, moved = run_gpu(pf, case, force_float, lookahead, weight_type, canvases=canvases)
    miss = compare_maps(g, o)
    assert miss == [], (case, miss[:4])
    # the changed flags after the last keyframe: every tile of its canvas, culled or not (Apply, MultiBandMap2DCPU.cpp:553)
    x0, y0, tx, ty = canvases[-1]
    assert sorted(coords) == sorted((x0 + x, y0 + y) for y in range(ty) for x in range(tx)), (case, canvases[-1], len(coords))
    for (ix, iy), img in list(zip(coords, px))[:: max(1, len(coords) // 6)]:
        assert np.array_equal(img, o.blend_tile(ix, iy)), (ix, iy)
    inner = (x0 + tx // 2, y0 + ty // 2)
    assert np.array_equal(g.blend_tile(*inner), o.blend_tile(*inner)), inner
    (gs, go), (os_, oo) = g.save_to_memory(), o.save()
    assert tuple(go) == tuple(oo) and np.array_equal(gs, os_)
    assert g.culled_tiles() > 0 and g.culled_cells() > 0, (case, g.culled_tiles(), g.culled_cells())
    must, never = FORMS[case]
    print("large canvas %s ff=%d lookahead=%s: canvases %s admission %s culled tiles %d cells %d" %
          (case, force_float, lookahead, [c[2:] for c in canvases], [int(v) for v in moved], g.culled_tiles(), g.culled_cells()))
    for i in must:
        assert moved[i] > 0, (case, i, [int(v) for v in moved])
    for i in never:
        assert moved[i] == 0, (case, i, [int(v) for v in moved])
    st = g.render_stats()
    canvas_px = 65536.0 * sum(c[2] * c[3] for c in canvases)
    rendered_px = canvas_px - 4096.0 * g.culled_cells() - 65536.0 * g.culled_tiles()
    assert rendered_px <= st["level0_px"] <= canvas_px and st["owned_px"] == canvas_px - 65536.0 * g.culled_tiles(), (case, rendered_px, canvas_px, st)
    g.close()


@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("case,block", [("F", 1), ("A", 4)])
def test_two_shards_partition_the_oracle_map(pf, orc, case, block, force_float):
    """Two ranks on one card, each fed every keyframe.  shard_block = 1 on 12 x 12 tiles: a rank's hash cells are its tiles, more than 64 of
    them are rendered, CellList overflows and every block of every level runs (no filter).  4 x 4-tile cells on shape A: a dozen cells a
    rank, merged down to the eight (level 0) / four (above) rectangles a job carries.  Per rank: its tiles against the oracle's, the cull
    statistics, the level-0 pixels that ran, and (4 x 4-tile cells) the blend of a tile in the middle of a cell, whose eight neighbours are
    the rank's own.  A shard's saved mosaic and its changed flags hold its own tiles only and have no counterpart in the oracle; with
    shard_block = 1 no tile has all its neighbours on its rank, and the blend across ranks is tests/test_gpu_sharding.py's."""
    cam, bands, poses, yaws = sortie(case)
    o, canvases = oracle_map(orc, case, force_float)
    assert all(c[2] >= 12 and c[3] >= 12 for c, y in zip(canvases, yaws) if y != 45.0), canvases
    want = set(o.tiles())
    got, moved = set(), np.zeros(8, np.int64)
    for rank in range(2):
        g, _, _, m = run_gpu(pf, case, force_float, None, flags=False, shard_rank=rank, shard_count=2, shard_block=block)
        mine = set(g.tiles())
        assert mine and not (mine & got) and all(pf.tile_owner(g.opt, *t) == rank for t in mine)
        miss = compare_tiles(g, o, sorted(mine))
        assert miss == [], (case, rank, miss[:4])
        if block == 1:
            assert max(sum(pf.tile_owner(g.opt, c[0] + x, c[1] + y) == rank for y in range(c[3]) for x in range(c[2])) for c in canvases) > 64
        assert g.culled_tiles() > 0 and g.culled_cells() > 0, (case, rank, g.culled_tiles(), g.culled_cells())
        st = g.render_stats()
        assert st["owned_px"] - 4096.0 * g.culled_cells() <= st["level0_px"] <= 65536.0 * sum(c[2] * c[3] for c in canvases), (case, rank, st)
        if block == 4:
            inner = [t for t in sorted(mine) if t[0] % 4 in (1, 2) and t[1] % 4 in (1, 2) and all((t[0] + dx, t[1] + dy) in mine for dx in (-1, 0, 1) for dy in (-1, 0, 1))]
            assert inner
            t = inner[len(inner) // 2]
            assert np.array_equal(g.blend_tile(*t), o.blend_tile(*t)), t
        got |= mine; moved += m
        g.close()
    assert got == want
    print("large canvas shards %s block %d ff=%d: admission %s" % (case, block, force_float, [int(v) for v in moved]))
    if block == 1:
        assert moved[2] > 0 and moved[6] > 0, list(moved)      # overflow: launches of a shard (which is never without a plan otherwise) with no filter
    else:
        assert moved[1] > 0 and moved[3] > 0 and moved[7] > 0 and moved[0] == 0, list(moved)
