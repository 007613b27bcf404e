"""The cull's bounds over the cell itself plus the pyramid's Lipschitz slack (csrc/frame_plan.hpp, pyramid_slack; FusionMap::render_frame)
against the oracle, which renders every tile of every canvas: 640 x 480 keyframes, every tile level bit-equal.  The cases sit where the
tighter bounds are closest to failing: neighbours a fraction of a cell apart at every yaw, a footprint edge through cells another keyframe
holds the bound of, equal weights, readers and a moving grid among waiting keyframes -- and the dilated rule of the experiments library
(PF_CULL_DILATED) as the twin."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import compare_maps, map_digest, workloads

pytestmark = pytest.mark.gpu
CAM = [640, 480, 500, 500, 320, 240]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = 100.0


def cell_m(scale):
    """one 64-px cell of the canvas in metres (lengthPixel = H / f / Scale)"""
    return 64.0 * H / CAM[2] / scale


def stepped_poses(wl, seed, scale, n=16):
    """n keyframes stepped by 0.25 - 3 cells along and across track, at eight yaws (with a little tilt: real perspective terms)"""
    rs = np.random.RandomState(8800 + seed)
    c = cell_m(scale)
    poses, x, y = [], 0.0, 0.0
    for k in range(n):
        x += float(rs.choice([0.25, 0.5, 1.0, 1.5, 2.0, 3.0])) * c
        y += float(rs.choice([-3.0, -1.0, -0.25, 0.25, 0.5, 2.0])) * c
        yaw = math.radians(45.0 * (k % 8) + float(rs.uniform(-4, 4)))
        q = wl.quat_mul(wl.quat_axis((0, 0, 1), yaw), wl.quat_mul(wl.quat_axis((0, 1, 0), float(rs.uniform(-0.06, 0.06))), wl.quat_axis((1, 0, 0), float(rs.uniform(-0.06, 0.06)))))
        poses.append([x, y, -H] + q)
    return poses


def frame(wl, seed, k):
    return wl.noise_frame(480, 640, 100 * seed + k) if k % 3 else wl.smooth_frame(480, 640, k)


def feed_pair(pf, orc, poses, prep, seed, lookahead, between=None, **opt):
    wl = workloads()
    o_opt = {"force_float": opt.get("force_float", 0), "scale": opt.get("scale", 1.0), "band_num": opt.get("band_number", 5), "weight_type": opt.get("weight_type", 0)}
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, fused=1, lookahead=lookahead, **opt)
    o = orc.OracleMap(**o_opt)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, prep) == o.prepare(wl.IDENTITY_PLANE, CAM, prep)
    for k, p in enumerate(poses):
        img = frame(wl, seed, k)
        a, b = g.feed(img, p), o.feed(img, p)
        assert a == b, (seed, k, a, b)
        if between:
            between(k, g, o)
    assert g.sync()
    return g, o


# (a)
@pytest.mark.parametrize("weight_type", [0, 1])
@pytest.mark.parametrize("bands", [1, 5, 7])
@pytest.mark.parametrize("force_float", [0, 1])
@pytest.mark.parametrize("lookahead", [0, 4])
def test_neighbours_a_fraction_of_a_cell_apart_at_eight_yaws(pf, orc, lookahead, force_float, bands, weight_type):
    wl = workloads()
    scale = 2.0
    seed = 2 * bands + weight_type
    poses = stepped_poses(wl, seed, scale)
    g, o = feed_pair(pf, orc, poses, poses[:8], seed, lookahead, force_float=force_float, band_number=bands, weight_type=weight_type, scale=scale)
    miss = compare_maps(g, o)
    assert miss == [], miss[:4]
    assert g.stats()["rendered"] == len(poses)
    # (seven bands: a slack of ~110 px on a 400-px half diagonal leaves little to cull on so short a walk)
    if bands <= 5:
        assert g.culled_tiles() + g.culled_cells() > 0
    g.close()


# (b)
@pytest.mark.parametrize("lookahead", [0, 4])
@pytest.mark.parametrize("weight_type", [0, 1])
def test_a_footprint_edge_through_cells_whose_bound_another_keyframe_holds(pf, orc, weight_type, lookahead):
    """A holds the bound around its centre.  B .. E lie half a footprint away, so that one of their edges runs through those very cells, at
    sub-cell phases and two yaws: their weights end there, and their lower bound in the cells the edge cuts (and within the pyramid's
    reach of it) must be 0.  A comes again at the end, with other pixels, and must win everything it won before."""
    wl = workloads()
    scale = 2.0
    px = H / CAM[2] / scale
    a = [0.0, 0.0, -H, 0, 0, 0, 1]
    others = []
    for i, (d, yaw_deg) in enumerate([(640 + 5, 0.0), (640 - 37, 0.0), (480 + 70, 90.0), (640 + 21, 30.0), (640 - 64, 180.0), (480 + 1, 270.0)]):
        yaw = math.radians(yaw_deg)
        # the camera's x axis along `yaw`: an offset of d px along it puts the footprint's short edge d - 640 px past A's centre
        others.append([d * px * math.cos(yaw), d * px * math.sin(yaw), -H] + wl.quat_axis((0, 0, 1), yaw))
    seq = [a] + others[:3] + [list(a)] + others[3:] + [list(a)] + [list(p) for p in others[:2]]
    g, o = feed_pair(pf, orc, seq, seq[:6], 40 + weight_type, lookahead, force_float=weight_type, weight_type=weight_type, scale=scale)
    miss = compare_maps(g, o)
    assert miss == [], miss[:4]
    assert g.culled_tiles() + g.culled_cells() > 0
    g.close()


# (c)
@pytest.mark.parametrize("lookahead", [0, 5])
@pytest.mark.parametrize("force_float", [0, 1])
def test_a_repeated_pose_the_newest_keyframe_wins(pf, orc, force_float, lookahead):
    """equal weights everywhere (`>=`, MultiBandMap2DCPU.cpp:521, :542): no bound of one copy may cull the other, ub >= lb of the same geometry"""
    wl = workloads()
    base = stepped_poses(wl, 71, 2.0, n=7)
    poses = [p for q in base for p in (q, list(q))] + [list(p) for p in base[:2]]
    g, o = feed_pair(pf, orc, poses, base, 71, lookahead, force_float=force_float, scale=2.0)
    miss = compare_maps(g, o)
    assert miss == [], miss[:4]
    g.close()


# (d)
def test_a_reader_between_feeds_and_a_moving_grid_among_waiting_keyframes(pf, orc):
    wl = workloads()
    poses = stepped_poses(wl, 81, 2.0, n=14)
    far = [poses[0][0] - 900.0, poses[0][1] - 700.0, -H, 0, 0, 0, 1]
    seq = poses[:6] + [far] + poses[6:] + [far] + [list(p) for p in poses[2:5]]
    seen = []

    def between(k, g, o):
        assert g.grid()[0] == o.grid()[0], k                      # spreadMap inside the feed call
        if k % 4 == 1:
            assert g.stats()["rendered"] == k + 1 and sorted(g.tiles()) == sorted(o.tiles())
        if k in (4, 11):
            assert compare_maps(g, o) == [], k
            seen.append(k)
    g, o = feed_pair(pf, orc, seq, poses[:8], 81, 4, between=between, force_float=1, scale=2.0)
    assert seen == [4, 11]
    miss = compare_maps(g, o)
    assert miss == [], miss[:4]
    assert g.culled_tiles() + g.culled_cells() > 0
    g.close()


# (e)
TWIN = """
import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)
from conftest import load_package
from helpers import map_digest
import test_gpu_cull_slack as T
pf = load_package()
print('TWIN', json.dumps(T.twin_run(pf)))
"""


def twin_run(pf):
    wl = workloads()
    poses = wl.serpentine(CAM, H, 24, per_row=6, fwd_overlap=0.85, side_overlap=0.7, seed=5, yaw_jitter_deg=8.0, tilt_jitter_deg=3.0, max_rows=4)
    out = {}
    for la in (0, 6):
        g = pf.Map2D.create(pf.TypeMultiBandCPU, False, fused=1, force_float=1, scale=2.0, lookahead=la)
        assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:8])
        for k, p in enumerate(poses):
            assert g.feed(frame(wl, 5, k), p)
        assert g.sync()
        out[str(la)] = {"d": {str(k): list(v) for k, v in map_digest(g).items()}, "cells": g.culled_tiles() * 16 + g.culled_cells()}
        g.close()
    return out


def test_the_dilated_rule_of_the_experiments_library_gives_the_same_map_and_culls_no_more(pf):
    exp = os.path.join(ROOT, "pi-slam-fusion_amd", "libpifusion_exp.so")
    assert os.path.exists(exp), "build the experiments library first (__graft_entry__.build())"
    mine = twin_run(pf)
    r = subprocess.run([sys.executable, "-c", TWIN % (HERE, ROOT)], env=dict(os.environ, PF_CULL_DILATED="1", PF_LIB=exp), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    twin = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TWIN ")][-1][5:])
    for la in ("0", "6"):
        assert twin[la]["d"] == mine[la]["d"], la
        print("lookahead", la, "culled cells: dilated rule", twin[la]["cells"], "product", mine[la]["cells"])
        assert 0 < twin[la]["cells"] <= mine[la]["cells"], (la, twin[la]["cells"], mine[la]["cells"])
    assert mine["6"]["cells"] > twin["6"]["cells"]                  # the tighter bounds do cull more where there is something to cull
