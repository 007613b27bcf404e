"""Keyframe undistortion on the GPU (csrc/undistort.hip, the input camera of map_feed.cpp) against the numpy model of
tests/undistort_model.py, byte for byte.

Kernel level: pf_undistort_bgr / pf_undistort_device on the golden cases (data of the reference's own Undistorter.h), on sizes that are
no multiple of the thread's run of four pixels, on a frame smaller than a wave, on an output wider than one block, on the rules where
the library deviates from the reference (X == 0 valid, taps clamped, uncovered entries black), and on BGRA and row-padded sources.

Map level: a map with an OpenCV input camera of another size than its own camera, fed raw frames, equals on every tile, level and
weight a twin map without input camera that was fed the model's undistorted frames -- through every way in."""
import functools
import importlib

import numpy as np
import pytest

import bgra
import undistort_model as um
from helpers import jitter_poses, map_digest, workloads
from test_gpu_dist import Rendezvous
from test_gpu_model import CAM, lattice_poses
from test_undistort_model import ATAN, OCV, OUT, OUT_WIDE, PIN, PIN_HALF, TANGENTIAL, golden, mean_of_four

pytestmark = pytest.mark.gpu

IN_SMALL = [37, 29, 30, 30, 18.2, 14.1, -0.2, 0.05, 0.001, -0.002, 0.0]
OUT_SMALL = [41, 23, 36, 36, 20.0, 11.2]
IN_TINY = [5, 3, 4, 4, 2.2, 1.3, -0.1, 0.01, 0.0, 0.0, 0.0]
OUT_TINY = [7, 2, 6, 6, 3.1, 0.6]
IN_LONG = [300, 20, 250, 250, 150.2, 9.6, -0.15, 0.03, 0.001, 0.002, 0.0]
OUT_LONG = [523, 9, 400, 400, 261.3, 4.4]             # three blocks of 256 pixels in x, the last one partly filled; width no multiple of 4
KERNEL_CASES = {
    "small": (IN_SMALL, OUT_SMALL), "tiny": (IN_TINY, OUT_TINY), "long": (IN_LONG, OUT_LONG), "identity": (PIN, PIN), "half_shift": (PIN, PIN_HALF),
    "wide": (OCV, OUT_WIDE), "atan_wide": (ATAN, OUT_WIDE), "tangential": (TANGENTIAL, OUT),
}


def last_error(pf):
    return pf.lib().pf_last_error().decode()


def library_table(pf, cam_in, cam_out):
    """the table the kernel reads is the library's own (for ATAN it may differ from the model's by an ulp: test_undistort_model.py)"""
    x, y, _ = pf.undistort_table(cam_in, cam_out)
    return x, y


def on_device(pf, src, cam_in, cam_out, channels=3, src_step=0, dst_pad=0):
    """pf_undistort_device on a source that lies in HBM (src: a uint8 device tensor in the layout the step describes); the destination has
    dst_pad bytes between its rows and a guard behind it, all of which must come back untouched"""
    import torch
    w, h = int(cam_out[0]), int(cam_out[1])
    step = w * 3 + dst_pad
    guard = 64
    dst = torch.full((h * step + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert pf.undistort_device(src.data_ptr(), cam_in, cam_out, dst.data_ptr(), channels=channels, src_step=src_step, dst_step=step if dst_pad else 0), last_error(pf)
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    rows = raw[:h * step].reshape(h, step)
    assert (rows[:, w * 3:] == 0xA5).all() and (raw[h * step:] == 0xA5).all(), "bytes outside the output rows were written"
    return np.ascontiguousarray(rows[:, :w * 3]).reshape(h, w, 3)


# ---------------------------------------------------------------- kernel level
@pytest.mark.parametrize("name", ["ocv", "atan", "tangential", "atan_frac"])
def test_golden_cases(pf, name):
    """the reference's own output, through the library's table and kernel: host to host and on device pointers"""
    import torch
    g = golden(name)
    x, y = library_table(pf, g["camera_in"], g["camera_out"])
    assert np.array_equal(x, g["x"]) and np.array_equal(y, g["y"])          # (these ATAN cases included)
    assert np.array_equal(pf.undistort(g["src"], g["camera_in"], g["camera_out"]), g["out"])
    t = torch.from_numpy(np.ascontiguousarray(g["src"])).cuda()
    assert np.array_equal(on_device(pf, t, g["camera_in"], g["camera_out"]), g["out"])


@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_kernel_equals_the_model(pf, name):
    import torch
    cam_in, cam_out = KERNEL_CASES[name]
    src = um.source_frame(int(cam_in[1]), int(cam_in[0]), 40 + len(name))
    x, y = library_table(pf, cam_in, cam_out)
    want = um.pixels(x, y, src)
    if name == "identity":
        assert np.array_equal(want, src) and (x[:, 0] == 0).all()
    if name == "half_shift":
        assert np.array_equal(want, mean_of_four(src))
    if name.endswith("wide"):
        assert (x < 0).any() and (want[x < 0] == 0).all()
    assert np.array_equal(pf.undistort(src, cam_in, cam_out), want)
    t = torch.from_numpy(src).cuda()
    assert np.array_equal(on_device(pf, t, cam_in, cam_out), want)
    assert np.array_equal(on_device(pf, t, cam_in, cam_out, dst_pad=5), want)           # rows that do not start on a dword: byte stores


@pytest.mark.parametrize("name", ["small", "half_shift", "wide", "long"])
def test_bgra_and_padded_sources(pf, name):
    """BGRA with an alpha plane no colour comes near, packed and with rows 6 bytes apart (rows start at 2 mod 4), on the host and in HBM;
    a BGR source in HBM with a row step"""
    import torch
    cam_in, cam_out = KERNEL_CASES[name]
    rows, cols = int(cam_in[1]), int(cam_in[0])
    src = um.source_frame(rows, cols, 70 + len(name))
    x, y = library_table(pf, cam_in, cam_out)
    want = um.pixels(x, y, src)
    four = bgra.with_alpha(src, 1)
    assert bgra.apart(four) >= bgra.ALPHA_GAP
    assert np.array_equal(pf.undistort(four, cam_in, cam_out), want)
    assert np.array_equal(pf.undistort(bgra.padded(four, 6), cam_in, cam_out), want)
    t = torch.from_numpy(np.ascontiguousarray(four)).cuda()
    assert np.array_equal(on_device(pf, t, cam_in, cam_out, channels=4), want)
    t, step = bgra.padded_device(four, 6)
    assert np.array_equal(on_device(pf, t, cam_in, cam_out, channels=4, src_step=step), want)
    step = cols * 3 + 7
    host = np.full((rows, step), bgra.PAD_BYTE, np.uint8)
    host[:, :cols * 3] = src.reshape(rows, cols * 3)
    t = torch.from_numpy(host).cuda()
    assert np.array_equal(on_device(pf, t, cam_in, cam_out, src_step=step), want)


def test_undistort_refuses_a_frame_of_another_size(pf):
    with pytest.raises(RuntimeError):
        pf.undistort(um.source_frame(48, 63, 1), OCV, OUT)
    assert "input camera's size" in last_error(pf)


# ---------------------------------------------------------------- map level
IN_CAM = [401, 311, 300, 300, 200.3, 155.2, -0.12, 0.03, 0.001, -0.0015, 0.0]          # another size than CAM's 333 x 257
IN_ROWS, IN_COLS = 311, 401
N = 4


@functools.lru_cache(maxsize=None)
def raw_frames(n=N):
    wl = workloads()
    return tuple(wl.noise_frame(IN_ROWS, IN_COLS, 900 + k) for k in range(n))


@functools.lru_cache(maxsize=None)
def undistorted_frames(n=N):
    x, y, unc = um.table(IN_CAM, CAM)
    assert unc == 0
    return tuple(um.pixels(x, y, f) for f in raw_frames(n))


@functools.lru_cache(maxsize=None)
def twin_digest(force_float):
    """the map without input camera fed the model's undistorted frames (computed once; the select is order independent, so one twin
    serves every way in and every lookahead)"""
    from conftest import load_package
    pf = load_package()
    poses = lattice_poses(17)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    for f, p in zip(undistorted_frames(), poses):
        assert g.feed(f, p)
    assert g.sync()
    out = (g.grid(), map_digest(g), g.save_to_memory()[0].copy())
    assert len(out[1]) > 0
    g.close()
    return out


def check_against_twin(g, force_float, label):
    grid, digest, mosaic = twin_digest(force_float)
    assert g.sync(), label
    assert g.grid() == grid, label
    assert map_digest(g) == digest, label
    assert np.array_equal(g.save_to_memory()[0], mosaic), label
    assert g.stats()["rendered"] == N and g.stats()["rejected"] == 0, label


def new_map(pf, force_float, thread=False, **opt):
    g = pf.Map2D.create(pf.TypeMultiBandCPU, thread, force_float=force_float, **opt)
    assert g.input_camera_info() is None
    return g


@pytest.mark.parametrize("way", ["host", "host_lookahead0", "reader", "reader_lookahead0", "bgra_pad6", "device", "device_bgra_pad6", "jpeg", "jpeg_batch", "thread", "prepare"])
@pytest.mark.parametrize("force_float", [0, 1])
def test_map_with_input_camera_equals_the_twin(pf, force_float, way):
    import torch
    wl = workloads()
    poses = lattice_poses(17)
    raws = raw_frames()
    opt = {"lookahead": 0} if way.endswith("lookahead0") else {}
    g = new_map(pf, force_float, thread=way in ("thread", "prepare"), **opt)
    # set before prepare: it survives prepare, and the table is there once both cameras are known
    assert g.set_input_camera(IN_CAM), last_error(pf)
    assert g.input_camera_info() == (IN_ROWS, IN_COLS, -1)
    if way == "jpeg" or way == "jpeg_batch":
        streams = [pf.jpeg_encode(f, 90) for f in raws]
        decoded = [pf.decode_jpeg(s) for s in streams]
        x, y, _ = um.table(IN_CAM, CAM)
        und = [um.pixels(x, y, d) for d in decoded]
        t = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=force_float)
        assert t.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
        for f, p in zip(und, poses):
            assert t.feed(f, p)
        assert t.sync()
        assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
        if way == "jpeg":
            for s, p in zip(streams, poses):
                assert g.feed_jpeg(s, p), last_error(pf)
        else:
            assert g.feed_jpeg_batch(streams, poses) == [True] * N, last_error(pf)
        assert g.sync() and g.grid() == t.grid() and map_digest(g) == map_digest(t) and g.stats()["rendered"] == N
        t.close(); g.close()
        return
    if way == "prepare":
        assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2], images=[raws[0], bgra.padded(bgra.with_alpha(raws[1], 1), 6)])
        rest = list(zip(raws, poses))[2:]
    else:
        assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
        rest = list(zip(raws, poses))
    assert g.input_camera_info() == (IN_ROWS, IN_COLS, 0)
    keep = []
    for k, (f, p) in enumerate(rest):
        if way.startswith("device"):
            if way == "device":
                t, step, cn = torch.from_numpy(np.ascontiguousarray(f)).cuda(), 0, 3
            else:
                (t, step), cn = bgra.padded_device(bgra.with_alpha(f, k), 6), 4
            torch.cuda.synchronize()
            keep.append(t)
            assert g.feed_device(t.data_ptr(), IN_ROWS, IN_COLS, p, step=step, channels=cn), last_error(pf)
        elif way == "bgra_pad6":
            assert g.feed(bgra.padded(bgra.with_alpha(f, k), 6), p), last_error(pf)
        else:
            assert g.feed(f, p), last_error(pf)
        if way.startswith("reader"):
            assert len(g.tiles()) > 0                   # a reader between feeds drains the window
    check_against_twin(g, force_float, way)
    if way in ("thread", "prepare"):
        assert g.render_log() == list(range(len(rest))) and g.queueSize() == 0
    del keep
    g.close()


@pytest.mark.parametrize("thread", [False, True])
@pytest.mark.parametrize("force_float", [0, 1])
def test_more_raw_frames_than_frame_slots(pf, force_float, thread):
    """16 raw keyframes back to back into a map that may hold 7 frame slots (max_queue 1, lookahead 2): scratch slots and frame slots are
    handed out again while the kernels that read them are in flight, and blocking uploads go into them"""
    wl = workloads()
    n = 16
    poses = jitter_poses(n, seed=23, step=(9.0, 4.0))
    raws, und = raw_frames(n), undistorted_frames(n)
    opt = dict(force_float=force_float, max_queue=n if thread else 1, lookahead=2)
    t = pf.Map2D.create(pf.TypeMultiBandCPU, False, **opt)
    g = pf.Map2D.create(pf.TypeMultiBandCPU, thread, **opt)
    assert g.set_input_camera(IN_CAM)
    assert t.prepare(wl.IDENTITY_PLANE, CAM, poses[:2]) and g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
    for f, p in zip(raws, poses):
        assert g.feed(f, p), last_error(pf)
    for f, p in zip(und, poses):
        assert t.feed(f, p)
    assert g.sync() and t.sync()
    assert g.stats()["rendered"] == t.stats()["rendered"] == n
    assert g.grid() == t.grid() and map_digest(g) == map_digest(t)
    g.close(); t.close()


def test_single_band_map_takes_an_input_camera(pf):
    """the input camera sits in front of feed(), which the single-band map shares"""
    wl = workloads()
    poses = lattice_poses(17)
    t = pf.Map2D.create(pf.TypeCPU, False); g = pf.Map2D.create(pf.TypeCPU, False)
    assert t.prepare(wl.IDENTITY_PLANE, CAM, poses[:2]) and g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
    assert g.set_input_camera(IN_CAM)
    for raw, f, p in zip(raw_frames(), undistorted_frames(), poses):
        assert g.feed(raw, p) and t.feed(f, p)
    assert g.sync() and t.sync() and g.tiles() == t.tiles() and len(t.tiles()) > 0
    for ix, iy in t.tiles():
        assert np.array_equal(g.tile_bgra(ix, iy), t.tile_bgra(ix, iy))
    g.close(); t.close()


def test_frame_sizes_and_clearing(pf):
    """with an input camera a frame of the OUTPUT camera's size is rejected as feed rejects any mismatched frame and the input size is
    accepted; set after prepare works like set before; n = 0 restores the map that takes frames of its own camera"""
    wl = workloads()
    poses = lattice_poses(17)
    raws, und = raw_frames(), undistorted_frames()
    g = new_map(pf, 0)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
    assert g.feed(raws[0], poses[0]) is False and g.stats()["rejected"] == 1            # no input camera yet: the raw size is the wrong one
    assert g.set_input_camera(IN_CAM) and g.input_camera_info() == (IN_ROWS, IN_COLS, 0)
    assert g.feed(und[0], poses[0]) is False and g.stats()["rejected"] == 2
    assert g.tiles() == []
    assert g.feed(raws[0], poses[0]) and g.feed(raws[1], poses[1])
    # a camera that is none leaves the map as it was
    assert not g.set_input_camera([401, 311, 300, 300, 200, 155, 0.1, 0.2]) and "6 (PinHole), 7 (ATAN) or 11 (OpenCV)" in last_error(pf)
    assert not g.set_input_camera([401, 311, 0, 300, 200, 155])
    assert g.input_camera_info() == (IN_ROWS, IN_COLS, 0)
    assert g.set_input_camera(None) and g.input_camera_info() is None
    assert g.feed(raws[2], poses[2]) is False and g.stats()["rejected"] == 3
    assert g.feed(und[2], poses[2]) and g.feed(und[3], poses[3])
    grid, digest, _ = twin_digest(0)
    assert g.sync() and g.grid() == grid and map_digest(g) == digest
    # a second prepare keeps the input camera
    assert g.set_input_camera(IN_CAM) and g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
    assert g.input_camera_info() == (IN_ROWS, IN_COLS, 0)
    for f, p in zip(raws, poses):
        assert g.feed(f, p)
    assert g.sync() and map_digest(g) == digest
    g.close()


def test_an_uncovered_output_camera_is_reported(pf):
    wide = [333, 257, 120, 120, 166.5, 128.5]
    g = new_map(pf, 0)
    poses = lattice_poses(17)
    assert g.prepare(workloads().IDENTITY_PLANE, wide, poses[:2]) and g.set_input_camera(IN_CAM)
    unc = um.table(IN_CAM, wide)[2]
    assert unc > 0 and g.input_camera_info() == (IN_ROWS, IN_COLS, unc)
    g.close()


def test_dist_feed_is_refused(pf):
    sh = importlib.import_module("pi_slam_fusion_amd.sharding")
    wl = workloads()
    poses = lattice_poses(17)
    g = new_map(pf, 0)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2]) and g.set_input_camera(IN_CAM)
    rv = Rendezvous(1)
    d = sh.DistMap(g, 0, 1, backend="host", exchange=rv.fn(0))
    with pytest.raises(RuntimeError, match="input camera"):
        d.feed(raw_frames()[0], poses[0], root=0)
    with pytest.raises(RuntimeError, match="input camera"):
        d.feed_jpeg(pf.jpeg_encode(raw_frames()[0], 90), poses[0], (IN_ROWS, IN_COLS), root=0)
    assert g.sync() and g.tiles() == [] and g.stats()["rendered"] == 0
    d.close(); g.close()
