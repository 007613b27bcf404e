"""A dataset of decoder dumps: rgb/<name>.nv12 (packed NV12 of the camera's size) replayed through the file drivers equals the same dataset
with the pictures of tests/raw_model.py as .ppm -- the Python driver (pi_slam_fusion_amd.dataset + datatrans.feed_loop, what tools/replay.py
runs) in this process, the C++ one (include/pifusion/TestSystem.h) as the program tests/test_replay.py builds."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import raw_frames as rf
import raw_model as rm
from helpers import jitter_poses, map_digest, workloads
from test_replay import build_replay, write_dataset

pytestmark = pytest.mark.gpu
CAM = [320, 240, 250, 250, 160, 120]
ROWS, COLS, N = 240, 320, 3


def datasets(tmp_path):
    wl = workloads()
    poses = jitter_poses(N, seed=31)
    raws = [rf.smooth_planes(rm.NV12, ROWS, COLS, 40 + k) for k in range(N)]
    pics = [rm.to_bgr(rm.NV12, p, ROWS, COLS) for p in raws]
    a, b = str(tmp_path / "nv12"), str(tmp_path / "ppm")
    write_dataset(a, CAM, poses, [None] * N, wl.IDENTITY_PLANE, ppm=None, extra="PrepareFrameNum = 1\nVideo.fps = 0\n")
    for k, p in enumerate(raws):
        rm.pack(rm.NV12, p).tofile(os.path.join(a, "rgb", "%06d.nv12" % k))
    write_dataset(b, CAM, poses, pics, wl.IDENTITY_PLANE, extra="PrepareFrameNum = 1\nVideo.fps = 0\n")
    return a, b, pics


def replay(pf, path, thread):
    """tools/replay.py's steps"""
    ds = importlib.import_module("pi_slam_fusion_amd.dataset").DroneMapDataset(path)
    dt = importlib.import_module("pi_slam_fusion_amd.datatrans")
    m = pf.Map2D.create(pf.TypeMultiBandCPU, thread, max_queue=N)
    first = [ds.load(0)]
    assert m.prepare(ds.plane, ds.camera, [p for _, p in first], images=[i for i, _ in first] if thread else None)
    it = iter(range(1, len(ds)))
    fed = dt.feed_loop(m, lambda: (lambda k: None if k is None else ds.load(k, encoded=True))(next(it, None)))
    assert fed == N - 1 and m.sync()
    out = (m.grid(), map_digest(m), m.stats())
    m.close()
    return out


@pytest.mark.parametrize("thread", [False, True])
def test_nv12_dataset_equals_the_ppm_dataset(pf, tmp_path, thread):
    a, b, pics = datasets(tmp_path)
    ds = importlib.import_module("pi_slam_fusion_amd.dataset").DroneMapDataset(a)
    img, _ = ds.load(1)
    assert np.array_equal(img, pics[1])                                           # the host conversion of a prepare frame
    raw, _ = ds.load(1, encoded=True)
    assert isinstance(raw, pf.RawImage) and raw.format == pf.RAW_NV12            # ... and the frame as the map takes it
    got, want = replay(pf, a, thread), replay(pf, b, thread)
    assert got == want and len(want[1]) > 0 and want[2]["rendered"] == (N if thread else N - 1)


def test_cpp_driver_feeds_nv12_files(pf, tmp_path):
    from PIL import Image
    a, b, _ = datasets(tmp_path)
    exe = build_replay(str(tmp_path))
    outs = []
    for d in (a, b):
        out = os.path.join(d, "cpp.png")
        r = subprocess.run([exe, d, "Map2D.Thread=1", "Map.File2Save=" + out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode == 0 and b"Loaded 1 frames" in r.stdout and b"Fed 2 frames" in r.stdout, r.stdout.decode()
        outs.append(np.asarray(Image.open(out).convert("RGB")))
    assert np.array_equal(outs[0], outs[1]) and outs[0].std() > 0
