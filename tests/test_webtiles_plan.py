"""The host half of the Web-Mercator tile export (csrc/webtiles_plan.hpp behind pf_webtiles_plan, pf_webtiles_native_zoom and
pf_webtiles_georef_compose) and the numpy model the GPU tests hold the kernels against (tests/webtiles_model.py): the model against
hand-computed cases, the plan against an independent statement of the OSM formulas in extended precision, the georeference chain
against pf_lnglat_from_distance, the refusals.  No device."""
import ctypes as C
import math

import numpy as np
import pytest

import webtiles_model as wm

RES0 = 156543.03392804097          # metres per output pixel at zoom 0 on the equator


def ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(3 * x + y) % 251, (x + 5 * y) % 241, (7 * x + 2 * y) % 239], -1).astype(np.uint8)


# ---------------------------------------------------------------- 1. the model
def test_model_integer_tables_shift_the_source_exactly():
    img = ramp(300, 400); mask = np.full((300, 400), 9, np.uint8)
    mask[100:120, 50:90] = 0
    for dx, dy, bg in ((0, 0, 0), (37, 11, 255), (-20, -30, 7), (200, 150, 300)):
        ux = np.arange(256, dtype=np.float64) + dx; vy = np.arange(256, dtype=np.float64) + dy
        px, cov = wm.sample(img, mask, ux, np.zeros(256), np.zeros(256), vy, bg)
        want = np.full((256, 256, 3), min(bg, 255), np.uint8); wcov = np.zeros((256, 256), bool)
        for r in range(256):
            for c in (range(256) if r % 17 == 0 else (0, 1, 127, 254, 255)):
                y, x = r + dy, c + dx
                if 0 <= y < 300 and 0 <= x < 400 and mask[y, x]:
                    want[r, c] = img[y, x]; wcov[r, c] = True
                assert np.array_equal(px[r, c], want[r, c]) and cov[r, c] == wcov[r, c], (dx, dy, r, c)


def test_model_half_pixel_tables_blend_as_computed_by_hand():
    img = np.zeros((4, 4, 3), np.uint8); img[:, 2:] = 200; img[:, :, 1] = 0; img[2:, :, 1] = 100          # channels 0, 2: left 0 / right 200; channel 1: bottom half 100
    mask = np.ones((4, 4), np.uint8)
    ux = np.array([0.5, 1.5, 2.5]); vy = np.array([0.0, 1.5])
    px, cov = wm.sample(img, mask, ux, np.zeros(3), np.zeros(2), vy, 0)
    assert cov.all()
    # row 0 (fy = 0): columns between (0, 1) -> 0, (1, 2) -> (0 * 32768 + 200 * 32768 + 32768) // 65536 = 100, (2, 3) -> 200
    assert px[0, :, 0].tolist() == [0, 100, 200] and px[0, :, 2].tolist() == [0, 100, 200] and px[0, :, 1].tolist() == [0, 0, 0]
    # row 1 (fy = 128, rows 1 and 2): channel 1 is 100 on row 2 only -> (100 * 32768 + 32768) // 65536 = 50; channels 0, 2 as above
    assert px[1, :, 1].tolist() == [50, 50, 50] and px[1, :, 0].tolist() == [0, 100, 200]
    # a quarter pixel: fx = 64 -> (0 * 192 + 200 * 64) * 256 = 3276800, + 32768, // 65536 = 50
    px, _ = wm.sample(img, mask, np.array([1.25]), np.zeros(1), np.zeros(1), np.zeros(1), 0)
    assert px[0, 0].tolist() == [50, 0, 50]


def test_model_renormalises_over_the_valid_taps_and_flips_at_half_weight():
    img = np.full((3, 3, 3), 10, np.uint8); img[:, 2] = 250; img[1, 1] = 90
    mask = np.ones((3, 3), np.uint8)
    one = lambda sx, sy, m=mask: tuple(v[0, 0] for v in wm.sample(img, m, np.array([sx]), np.array([sy]), np.zeros(1), np.zeros(1), 77))
    # past the right edge: column 3 does not exist, column 2 alone counts -- exactly half of the weight, still covered, its own colour
    px, cov = one(2.5, 0.0)
    assert cov and px.tolist() == [250, 250, 250]
    px, cov = one(2.0 + 129 / 256.0, 0.0)          # a 256th further: 127 * 256 * 2 < 65536 -> background, uncovered
    assert not cov and px.tolist() == [77, 77, 77]
    px, cov = one(-0.5, 1.0)                       # before the left edge, the same from the other side: fx = 128 on the valid tap
    assert cov and px.tolist() == [10, 10, 10]
    px, cov = one(-1.0 + 127 / 256.0, 1.0)
    assert not cov and px.tolist() == [77, 77, 77]
    # an uncovered tap is renormalised away like a missing one: the bright column switched off leaves its neighbour's colour
    m = mask.copy(); m[:, 2] = 0
    px, cov = one(1.25, 1.0, m)
    assert cov and px.tolist() == [90, 90, 90]
    px, cov = one(1.25, 1.0)                       # ... and with it on: (90 * 192 + 250 * 64) * 256 + 32768 >> 16 = 130
    assert cov and px.tolist() == [130, 130, 130]
    # a corner: one valid tap of four with a quarter of the weight -> uncovered; NaN and far positions touch nothing
    assert not one(-0.5, -0.5)[1] and not one(float("nan"), 0.0)[1] and not one(1e300, 0.0)[1] and not one(0.0, -2.0)[1]
    # the reduction: the mean over the covered pixels alone, rounded half up; absent children count as uncovered
    a = np.zeros((256, 256, 3), np.uint8); ca = np.zeros((256, 256), bool)
    a[0, 0] = 10; a[0, 1] = 11; a[1, 0] = 13; ca[0, 0] = ca[0, 1] = ca[1, 0] = True          # (34 + 1) // 3 = 11
    a[2, 2] = 200; ca[2, 2] = True
    px, cov = wm.reduce4([[(a, ca), None], [None, None]], 5)
    assert px[0, 0].tolist() == [11, 11, 11] and px[1, 1].tolist() == [200, 200, 200] and cov[0, 0] and cov[1, 1] and cov.sum() == 2
    assert px[0, 1].tolist() == [5, 5, 5] and px[200, 200].tolist() == [5, 5, 5]


# ---------------------------------------------------------------- 2. the plan
def test_plan_fixed_points(pf):
    # z = 0: one tile, wherever the image lies
    for lat in (0.3, 60.0, -33.0):
        p = wm.make_px2ll(13.0, lat, 300, 520, 18, 1.0, 30.0)
        assert pf.webtiles_plan(p, 300, 520, 0)[0] == (0, 0, 0, 0) == wm.tile_range(p, 300, 520, 0)
    # (lng 0, lat 0) is the corner the four tiles of z = 1 share: an image centred there touches all of them
    p = wm.make_px2ll(0.0, 0.0, 100, 100, 18, 1.0)
    assert pf.webtiles_plan(p, 100, 100, 1)[0] == (0, 0, 1, 1)
    # Berlin (13.405 E, 52.52 N) at z = 10: x = floor((13.405 + 180) / 360 * 1024) = floor(550.13) = 550;
    # asinh(tan 52.52 deg) = ln(1.30401 + 1.64330) = 1.08089, y = floor((1 - 1.08089 / pi) / 2 * 1024) = floor(335.84) = 335
    p = wm.make_px2ll(13.405, 52.52, 64, 64, 19, 1.0, 12.0)
    rg, ux, uy, vx, vy = pf.webtiles_plan(p, 64, 64, 10)
    assert rg == (550, 335, 550, 335) and ux.size == uy.size == vx.size == vy.size == 256
    # the native zoom: a source pixel of scale output pixels of zoom z is at least 1 / sqrt 2 of one from zoom z - ceil(log2(scale sqrt 2)) on
    for scale, dz in ((1.0, 0), (1.41, 0), (1.42, -1), (0.71, 0), (0.70, 1), (3.0, -2), (0.3, 2)):
        p = wm.make_px2ll(13.0, 40.0, 300, 520, 18, scale, 205.0, True)
        assert pf.webtiles_native_zoom(p, 300, 520) == 18 + dz == wm.native_zoom(p, 300, 520), (scale, dz)


@pytest.mark.parametrize("z", [18, 22, 24])
def test_plan_tables_against_extended_precision(pf, z):
    """|fp64 table - extended-precision table| <= 1e-5 source pixel: fp64 carries about 1.4e-14 degrees at these longitudes and a 1 cm
    pixel is 1.1e7 px per degree, so a few roundings give some 1e-7; measured worst over these cases 2.4e-7, the bound leaves 40 x"""
    assert np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(20261019 + z)
    worst = 0.0
    for lat in (0.3, 40.0, 60.0, -33.0, 84.0):
        for north in (False, True):
            res = RES0 * math.cos(math.radians(lat)) / 2 ** z
            gsd = max(0.01, float(rng.uniform(0.01, 0.25)))
            scale = gsd / res          # output pixels per source pixel
            cols = int(min(max(2400 / scale, 2), 6000)); rows = int(min(max(1800 / scale, 2), 6000))
            p = wm.make_px2ll(float(rng.uniform(-179, 179)), lat, rows, cols, z, scale, float(rng.uniform(0, 360)), north)
            rg, ux, uy, vx, vy = pf.webtiles_plan(p, rows, cols, z)
            assert rg == wm.tile_range(p, rows, cols, z)
            assert 256 * (rg[2] - rg[0] + 1) <= 6000 and 256 * (rg[3] - rg[1] + 1) <= 6000          # within +-3000 output pixels of the centre
            ref = wm.tables(p, rg, z, np.longdouble)
            for got, want in zip((ux, uy, vx, vy), ref):
                assert got.shape == want.shape
                worst = max(worst, float(np.abs(got.astype(np.longdouble) - want).max()))
            # ... and the numpy model in fp64 gives what the library gives, to the same bound
            for got, want in zip((ux, uy, vx, vy), wm.tables(p, rg, z)):
                assert float(np.abs(got - want).max()) <= 1e-5
    print("worst table error at z = %d: %.3g source pixels" % (z, worst))
    assert worst <= 1e-5


# ---------------------------------------------------------------- 3. the georeference
def test_georef_chain_is_the_map_update_chain(pf):
    rng = np.random.default_rng(7)
    for k in range(12):
        lp = float(rng.uniform(0.01, 0.5))
        flip = -1.0 if k % 3 == 0 else 1.0
        T = [lp, 0, 0, float(rng.uniform(-500, 500)), 0, flip * lp, 0, float(rng.uniform(-500, 500)), 0, 0, 1, 0, 0, 0, 0, 1]
        yaw, tilt = float(rng.uniform(0, 2 * math.pi)), float(rng.uniform(-0.2, 0.2))
        qa = np.array([0, 0, math.sin(yaw / 2), math.cos(yaw / 2)]); qb = np.array([math.sin(tilt / 2), 0, 0, math.cos(tilt / 2)])
        q = pf.se3_mul([0, 0, 0] + list(qa), [0, 0, 0] + list(qb))[3:]
        plane = [float(rng.uniform(-100, 100)), float(rng.uniform(-100, 100)), float(rng.uniform(-5, 5))] + list(q)
        origin = [float(rng.uniform(-179, 179)), (0.3, 40.0, 60.0, -33.0, 84.0)[k % 5], 400.0]
        p = pf.webtiles_georef_compose(T, plane, origin)
        # the same affine from the three steps, in numpy: units of pf_lnglat_from_distance, the plane's rotated axes
        inv_lng = pf.lnglat_from_distance(0.0, origin[1], 1.0, 0.0)[0]
        inv_lat = (pf.lnglat_from_distance(0.0, origin[1], 0.0, 1e7)[1] - origin[1]) / 1e7
        rx, ry = pf.so3_rotate(q, [1, 0, 0]), pf.so3_rotate(q, [0, 1, 0])
        e = lambda x, y: plane[0] + rx[0] * x + ry[0] * y
        n = lambda x, y: plane[1] + rx[1] * x + ry[1] * y
        want = [e(T[3], T[7]) * inv_lng + origin[0], rx[0] * T[0] * inv_lng, ry[0] * T[5] * inv_lng,
                n(T[3], T[7]) * inv_lat + origin[1], rx[1] * T[0] * inv_lat, ry[1] * T[5] * inv_lat]
        assert np.allclose(p, want, rtol=1e-12, atol=0), (k, p, want)
        # the corners of tile (ix, iy) of a mosaic whose origin tile starts at pixel (0, 0): through px2ll and through the chain itself
        for ix, iy in ((0, 0), (3, 1), (7, 12)):
            for cx, cy in ((256 * ix, 256 * iy), (256 * ix + 256, 256 * iy + 256)):
                x, y = T[0] * cx + T[3], T[5] * cy + T[7]
                w = pf.so3_rotate(q, [x, y, 0.0])
                lng, lat = pf.lnglat_from_distance(origin[0], origin[1], plane[0] + w[0], plane[1] + w[1])
                assert abs(p[0] + p[1] * cx + p[2] * cy - lng) < 1e-9 and abs(p[3] + p[4] * cx + p[5] * cy - lat) < 1e-9


# ---------------------------------------------------------------- 4. refusals
def test_plan_refuses_and_touches_nothing(pf):
    L = pf.lib()
    dp = C.POINTER(C.c_double)
    good = wm.make_px2ll(13.0, 40.0, 300, 520, 18, 1.0)

    def call(p, rows, cols, z, cap_c=4096, cap_r=4096):
        a = np.ascontiguousarray(p, np.float64)
        rg = (C.c_int * 4)(-7, -7, -7, -7)
        t = [np.full(4096, 123.25) for _ in range(4)]
        ok = L.pf_webtiles_plan(a.ctypes.data_as(dp), rows, cols, z, rg, *[v.ctypes.data_as(dp) for v in t], cap_c, cap_r)
        return ok, tuple(rg), all((v == 123.25).all() for v in t), L.pf_last_error().decode()

    ok, rg, clean, _ = call(good, 300, 520, 18)
    assert ok == 1 and rg == wm.tile_range(good, 300, 520, 18) and not clean
    singular = good.copy(); singular[4] = singular[1] * 2; singular[5] = singular[2] * 2          # the second row a multiple of the first
    for p, z, word in ((singular, 18, "singular"), (good, 25, "zoom"), (good, -1, "zoom"), (wm.make_px2ll(13.0, 86.0, 300, 520, 18, 1.0), 18, "85.05"),
                       (wm.make_px2ll(13.0, -85.2, 300, 520, 18, 1.0), 18, "85.05")):
        ok, rg, clean, msg = call(p, 300, 520, z)
        assert ok == 0 and rg == (-7, -7, -7, -7) and clean and word in msg, (z, msg)
    assert call(good, 0, 520, 18)[:3] == (0, (-7, -7, -7, -7), True)
    # tables that are too small: the range says what is needed, the tables stay as they were
    need = wm.tile_range(good, 300, 520, 18)
    nc, nr = 256 * (need[2] - need[0] + 1), 256 * (need[3] - need[1] + 1)
    for cc, cr in ((nc - 1, nr), (nc, nr - 1), (0, 0)):          # (tables given: not the question for the range alone)
        ok, rg, clean, msg = call(good, 300, 520, 18, cc, cr)
        assert ok == 0 and rg == need and clean and "room" in msg
    assert call(good, 300, 520, 18, nc, nr)[0] == 1
    assert pf.webtiles_native_zoom(singular, 300, 520) == -1 and pf.webtiles_georef_compose([0.1, 0, 0, 0, 0, 0.1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1],
                                                                                             [0, 0, 0, math.sin(math.pi / 4), 0, 0, math.cos(math.pi / 4)], [13.0, 40.0, 0.0]) is None
    with pytest.raises(ValueError):
        pf.webtiles_plan(good, 300, 520, 25)
