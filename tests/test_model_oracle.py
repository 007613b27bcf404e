"""The CPU oracle (oracle/oracle.c) against independent numpy models of MultiBandMap2DCPU and of Map2DCPU (map_model.py), whole map, bit
for bit.

Every GPU parity test compares the HIP path with the oracle, so a mistake the oracle shared with the kernels would pass them all.
This file pins the oracle above the single-op level of test_oracle_ops.py: Apply (fresh copy, the `>=` select, weight-0 pixels),
the weight pyramid, Ele::blend (halo borders 1 << (nl-1-i), the all-nine rule, blend by self, the weights[0]==0 mask), the
saturating collapse, save (bounding box, zero levels for holes, one whole-mosaic collapse, bg_color) and the 8U views.

The second half does the same for the single-band map (Map2DCPU.cpp:236-334): the weight byte image, OpenCV's 15-bit tap table, the
8-bit LINEAR / BORDER_CONSTANT warp and the strict `<` select, each against ModelMapSingleBand's restatement."""
import itertools

import numpy as np
import pytest

from helpers import (HOSTILE_KINDS, compare_single_with_model, compare_with_model, feed_with_model, hostile_frame, jitter_poses,
                     neighbourhoods, single_band_pair, workloads)
from map_model import (ModelMap, ModelMapSingleBand, _warp_coords, invert3x3, linear_tab_fixpt, warp_linear_const_8u_inv,
                       weight_bytes)

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


# ================================================================ the single-band map (Map2DCPU)
def test_tap_table_of_the_fixed_point_warp():
    """initInterTab2D(INTER_LINEAR, fixpt) as the model writes it out: every entry sums to 32768; entry (0, 0) is [32767, 0, 0, 1]
    (32768 saturates as a short, and the fix-up puts the missing 1 on element (1, 1)); every other entry is the exact product, so the
    fix-up touches entry (0, 0) alone; and that fix-up changes no output byte, whatever the 8-bit taps S (the one at (0, 0)) and T (the
    one at (1, 1)): (S * 32767 + T + 16384) >> 15 == S -- the claim on which both the oracle and the kernel move the 1 about freely."""
    tab = linear_tab_fixpt()
    assert tab.shape == (32, 32, 4)
    assert (tab.sum(axis=2) == 32768).all()
    assert tab[0, 0].tolist() == [32767, 0, 0, 1]
    fy, fx = np.mgrid[0:32, 0:32]
    exact = np.stack([(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32], axis=2)
    rest = np.ones((32, 32), bool); rest[0, 0] = False
    assert np.array_equal(tab[rest], exact[rest])
    assert np.array_equal(linear_tab_fixpt(fixup=False)[rest], exact[rest])        # nothing but (0, 0) needed the fix-up
    assert linear_tab_fixpt(fixup=False)[0, 0].tolist() == [32767, 0, 0, 0]
    assert tab.min() >= 0 and tab.max() <= 32767
    S, T = np.mgrid[0:256, 0:256]
    assert np.array_equal((S * 32767 + T + (1 << 14)) >> 15, S)


SIZES_8U = ((480, 640), (257, 333), (9, 7), (2, 2), (1, 5), (301, 401))             # the last: an odd centre (w/2, h/2 truncate)


@pytest.mark.parametrize("weight_type", [0, 1])
def test_weight_byte_image_equals_the_model(orc, weight_type):
    for rows, cols in SIZES_8U:
        w = orc.weight_image_8uc4(rows, cols, weight_type)
        a = weight_bytes(rows, cols, weight_type)
        assert (w[:, :, :3] == 0).all() and np.array_equal(w[:, :, 3], a), (rows, cols)
        assert a.min() >= 2 and a.max() <= 254
    assert weight_bytes(480, 640, weight_type)[240, 320] == 254
    assert weight_bytes(301, 401, weight_type)[150, 200] == 254 and weight_bytes(301, 401, weight_type)[0, 0] == 2


def _warp_pair(orc, src, M0, drows, dcols):
    """the oracle's warp of src by the forward matrix M0 and the model's; also the phases (Y & 31, X & 31) the model saw"""
    Minv = invert3x3(M0)
    XY = _warp_coords(Minv, drows, dcols, (32.0,))[0]
    return orc.warp_linear_const_8u(src, M0, drows, dcols), warp_linear_const_8u_inv(src, Minv, drows, dcols, XY), XY


@pytest.mark.parametrize("cn", [3, 4])
def test_fixed_point_warp_equals_the_model(orc, cn):
    """orc.warp_linear_const_8u against the model's warp: 24 random homographies onto canvases wider than one 64-column block; pure
    translations by every (fx, fy) / 32; a homography whose W is exactly 0 on a canvas column and changes sign across it; one that
    sends most of the canvas beyond +-32768 source pixels (sat_short of the coordinate).  3- and 4-channel sources with 0 and 255."""
    rng = np.random.RandomState(100 + cn)
    src = rng.randint(0, 256, (37, 45, cn)).astype(np.uint8)
    src[rng.rand(37, 45) < 0.2] = 255; src[rng.rand(37, 45) < 0.2] = 0
    for seed in range(24):
        r = np.random.RandomState(seed)
        a = np.radians(r.uniform(-180, 180)); sc = r.uniform(0.5, 3.0)
        M0 = np.array([[sc * np.cos(a), -sc * np.sin(a), r.uniform(10, 60)], [sc * np.sin(a), sc * np.cos(a), r.uniform(10, 60)],
                       [r.uniform(-2e-3, 2e-3), r.uniform(-2e-3, 2e-3), 1.0]])
        got, exp, _ = _warp_pair(orc, src, M0, 70, 150)
        assert np.array_equal(got, exp), seed
        assert (exp != 0).any() and (exp == 0).all(axis=2).any()                     # the image and the border are both on the canvas
    small = src[:6, :7]
    phases = set()
    for fy, fx in itertools.product(range(32), range(32)):
        M0 = np.array([[1, 0, 1 + fx / 32.0], [0, 1, 1 + fy / 32.0], [0, 0, 1.0]])
        got, exp, (X, Y) = _warp_pair(orc, small, M0, 9, 10)
        assert np.array_equal(got, exp), (fy, fx)
        phases |= set(zip((Y & 31).ravel().tolist(), (X & 31).ravel().tolist()))
    assert len(phases) == 1024
    Minv = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0 / 16, 0, 1.0]])                    # W = 1 - x / 16: 0 at x = 16, negative beyond
    M0 = invert3x3(Minv)
    assert np.array_equal(invert3x3(M0), Minv)
    got, exp, (X, Y) = _warp_pair(orc, src, M0, 40, 48)
    assert np.array_equal(got, exp)
    assert (X[:, 16] == 0).all() and (Y[:, 16] == 0).all() and X[5, 15] > 0 > X[5, 17]
    assert np.array_equal(exp[:, 16], np.broadcast_to(src[0, 0], (40, cn)))            # W == 0: the coordinate is (0, 0)
    M0 = invert3x3(np.array([[3000.0, 0, -68989.7], [0, 2500.0, -59984.6], [0, 0, 1.0]]))
    got, exp, (X, Y) = _warp_pair(orc, src, M0, 40, 130)
    assert np.array_equal(got, exp)
    assert (X >> 5).max() > 32768 and (X >> 5).min() < -32768 and (Y >> 5).max() > 32768 and (Y >> 5).min() < -32768
    assert (exp[24, 23] != 0).any() and not exp[:24].any()                          # canvas (23, 24) lands on source (10.3, 15.4)


SB_CAM = [333, 257, 260, 260, 166.5, 128.5]


@pytest.mark.parametrize("weight_type", [0, 1])
@pytest.mark.parametrize("kind", HOSTILE_KINDS)
def test_single_band_whole_map_equals_the_model(orc, kind, weight_type):
    """Map2DCPU on the hostile frames at Map2D.Scale 1, 0.5 and 2, BGRA input, the grid prepared from the last pose so that
    spreadMap moves the origin when the first ones arrive.  Every case reaches the rim of a footprint (stored alphas below the
    weight's floor of 2) and pixels where two keyframes' alphas are equal."""
    wl = workloads()
    poses = jitter_poses(4, seed=29, step=(30.0, 20.0))
    frames = [np.dstack([hostile_frame(kind, 257, 333, k), wl.noise_frame(257, 333, 900 + k)[:, :, :1]]) for k in range(4)]
    for scale in (1.0, 0.5, 2.0):
        o, m = single_band_pair(orc, SB_CAM, poses, frames, poses[3:], weight_type, scale)
        assert o.grid()[0][2] < 0, "spreadMap did not move the origin"
        assert compare_single_with_model(o, m) == [], scale
        assert m.rim_px > 0 and m.tie_px > 0, (scale, m.rim_px, m.tie_px)
        assert m.waves_inside > 0 and m.waves_straddling > 0 and m.waves_outside > 0


def test_single_band_equal_alphas_keep_the_oldest_keyframe(orc):
    """one pose fed twice with other pixels: every alpha ties, `<` (Map2DCPU.cpp:327) keeps the first keyframe everywhere"""
    pose = jitter_poses(1, seed=3)[0]
    a, b = hostile_frame("checker1", 257, 333, 0), hostile_frame("ramp", 257, 333, 1)
    o, m = single_band_pair(orc, SB_CAM, [pose, pose], [a, b], [pose])
    o1, m1 = single_band_pair(orc, SB_CAM, [pose], [a], [pose])
    assert compare_single_with_model(o, m) == [] and compare_single_with_model(o1, m) == []
    stored = sum(int((m.tile_bgra(*t)[:, :, 3] > 0).sum()) for t in m.tiles())
    assert m.tie_px == stored > 0
    assert any(not np.array_equal(m.tile_bgra(*t), np.zeros((256, 256, 4), np.uint8)) for t in m.tiles())
