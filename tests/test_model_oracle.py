"""The CPU oracle (oracle/oracle.c) against an independent numpy model of MultiBandMap2DCPU (map_model.py), whole map, bit for bit.

Every GPU parity test compares the HIP path with the oracle, so a mistake the oracle shared with the kernels would pass them all.
This file pins the oracle above the single-op level of test_oracle_ops.py: Apply (fresh copy, the `>=` select, weight-0 pixels),
the weight pyramid, Ele::blend (halo borders 1 << (nl-1-i), the all-nine rule, blend by self, the weights[0]==0 mask), the
saturating collapse, save (bounding box, zero levels for holes, one whole-mosaic collapse, bg_color) and the 8U views."""
import numpy as np
import pytest

from helpers import HOSTILE_KINDS, compare_with_model, feed_with_model, hostile_frame, jitter_poses, neighbourhoods, workloads
from map_model import ModelMap

CAM = [333, 257, 260, 260, 166.5, 128.5]        # odd frame sizes; a keyframe covers about 2 x 2 tiles


def lattice_poses(wl, seed):
    """A 3 x 3 lattice of keyframes (tiles with all nine neighbours in the middle, tiles on the mosaic border around them) and one
    keyframe far off the diagonal (a hole inside the save bounding box)."""
    rng = np.random.RandomState(seed)
    pos = [(i * 60.0, j * 50.0) for j in range(3) for i in range(3)] + [(420.0, 330.0)]
    poses = []
    for (x, y) in pos:
        q = wl.quat_mul(wl.quat_axis((0, 0, 1), np.radians(rng.uniform(-20, 20))),
                        wl.quat_axis((1, 0, 0), np.radians(rng.uniform(-5, 5))))
        poses.append([x + rng.uniform(-2, 2), y + rng.uniform(-2, 2), -100.0 + rng.uniform(-3, 3)] + q)
    return poses


def build(orc, poses, frames, n_prepare, **opt):
    wl = workloads()
    o = orc.OracleMap(**opt)
    m = ModelMap(**opt)
    assert o.prepare(wl.IDENTITY_PLANE, CAM, poses[:n_prepare])
    dims0 = o.grid()[0]
    m.canvases = []
    for img, p in zip(frames, poses):
        assert feed_with_model(o, m, img, p)
        m.canvases.append(m.last[0])
    return o, m, dims0


def check_save_has_holes(o, m, bg):
    img, _ = m.save()
    assert img.shape[0] * img.shape[1] > len(o.tiles()) * 256 * 256       # the bounding box holds missing tiles
    assert (img == bg).all(axis=2).any()


@pytest.mark.parametrize("bands", [0, 1, 5, 8])
@pytest.mark.parametrize("force_float", [0, 1])
def test_whole_map_equals_the_model(orc, force_float, bands):
    """Both pyramid types, 0-8 bands (at 8 the top level of a tile is 1 x 1, and levels 6-8 of the fp32 weight pyramid end in the
    scalar tail of pyrDown on odd canvas widths), weight types 0 and 1, a nonzero background, spreadMap (the grid is prepared from
    two poses), a hole in the mosaic and both blend paths."""
    wl = workloads()
    poses = lattice_poses(wl, 10 + bands)
    frames = [hostile_frame(HOSTILE_KINDS[(k + bands) % len(HOSTILE_KINDS)], 257, 333, k) for k in range(len(poses))]
    o, m, dims0 = build(orc, poses, frames, 2, band_num=bands, force_float=force_float, weight_type=bands % 2, bg_color=77)
    assert o.grid()[0][:2] != dims0[:2]                            # spreadMap grew the grid
    assert compare_with_model(o, m) == []
    full, alone = neighbourhoods(o.tiles())
    assert full and alone                                           # both blend paths taken
    check_save_has_holes(o, m, 77)
    if bands == 8:
        assert m.tile_level(*full[0], 8)[0].shape == (1, 1, 3)
        assert any(c[2] % 2 for c in m.canvases)                    # an odd canvas width in tiles


@pytest.mark.parametrize("force_float", [0, 1])
def test_low_quality_blend_and_spread_to_negative_tiles(orc, force_float):
    """high_quality_show = 0: every tile collapses alone.  The grid is prepared from the far keyframe alone and the lattice lies
    below and left of it, so spreadMap moves the origin to negative world tiles; the model keys its tiles by world tile."""
    wl = workloads()
    poses = lattice_poses(wl, 3)
    poses = poses[-1:] + poses[:-1]
    frames = [hostile_frame(("step", "checker2", "const", "impulse", "ramp")[k % 5], 257, 333, k) for k in range(len(poses))]
    o, m, _ = build(orc, poses, frames, 1, band_num=5, force_float=force_float, high_quality=0, bg_color=255)
    assert o.grid()[0][2] < 0 and o.grid()[0][3] < 0 and min(t[0] for t in o.tiles()) < 0
    assert compare_with_model(o, m) == []
    check_save_has_holes(o, m, 255)


def test_hostile_frames_reach_the_int16_bounds(orc):
    """The int16 level kernel runs stages B/D in packed 16-bit arithmetic, exact under the bounds stated in kernels.hip: 5-tap sums
    <= 255*16, vertical sums <= 65280 (+128, unsigned 16 bits), pyrUp sums <= 255*64 = 16320, |Laplacian| <= 255.  The hostile
    frames reach the sum bounds through the warp, and the map still equals the model.  |L| cannot pass 239 with 8-bit content: a
    255 pixel adds at least 16/256 of itself to a coarse pixel, so pyrUp gives back at least 16 there; an impulse on an odd/odd
    position reaches exactly that.  Uniform noise, the control, reaches none of these."""
    poses = jitter_poses(4, seed=12, step=(30.0, 20.0))
    seen = {}
    for kind in ("white", "impulse", "noise"):
        o, m, _ = build(orc, poses, [hostile_frame(kind, 257, 333, k) for k in range(4)], 4, band_num=5)
        assert compare_with_model(o, m, blends=False) == []
        seen[kind] = m.stats
    assert seen["white"]["h5"] == 255 * 16 and seen["white"]["v5"] == 65280 and seen["white"]["up"] == 16320
    assert seen["impulse"]["lap"] == 239
    assert seen["noise"]["v5"] < 65280 and seen["noise"]["up"] < 16320 and seen["noise"]["lap"] < 239
