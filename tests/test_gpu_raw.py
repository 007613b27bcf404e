"""Raw frames on the GPU (csrc/raw_convert.hip, FusionMap::feed_raw in map_feed.cpp) against the numpy model of tests/raw_model.py.

Kernel level: pf_raw_to_bgr_device equals pf_raw_to_bgr and the model, byte for byte, for every format at the sizes of raw_frames.SIZES and
at 1032 x 4 (two workgroups in x, no tail), from plane pointers 1, 2 and 4 bytes into their allocations, from planes with odd pitches
(the byte-wise path) and into destinations with row padding and guards, which must stay 0xA5.

Map level: a map fed raw frames equals, on every tile, level and weight, a twin fed the model's BGR pictures through pf_feed -- through
pf_feed_raw and pf_feed_raw_device, with and without lookahead, with a render thread and a queue that drops, mixed with BGR and BGRA
frames, behind an input camera of another size, on both pyramid types and the single-band map."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bgra
import raw_frames as rf
import raw_model as rm
import undistort_model as um
from helpers import map_digest, workloads
from test_gpu_model import lattice_poses

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "pi-slam-fusion_amd", "libpifusion_exp.so")

KERNEL_CASES = rf.cases() + [(f, 4, 1032) for f in rm.FORMATS]


def last_error(pf):
    return pf.lib().pf_last_error().decode()


# ---------------------------------------------------------------- kernel level
@pytest.mark.parametrize("case", KERNEL_CASES, ids=rf.case_id)
def test_kernel_equals_host_and_model(pf, case):
    fmt, rows, cols = case
    rng = np.random.default_rng(1000 * fmt + rows + cols)
    # packed planes (aligned wherever the width allows: the vector path), then odd pitches (rows that start anywhere: the byte path)
    for pad in ((0, 0, 0), (3, 5, 7)):
        views, bufs = rm.random_planes(fmt, rows, cols, rng, pad=pad)
        want = rm.to_bgr(fmt, views, rows, cols)
        assert np.array_equal(rf.convert_host(pf, fmt, views, rows, cols), want)
        for dst_pad in (0, 5, 8):
            got = rf.convert_device(pf, fmt, bufs, rows, cols, dst_pad=dst_pad)
            assert np.array_equal(got, want), (pad, dst_pad, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("case", [(f, r, c) for f in rm.FORMATS for (c, r) in ((530, 6), (1032, 4), (37, 29)) if rm.valid_size(f, r, c)], ids=rf.case_id)
def test_plane_pointers_inside_an_allocation(pf, case):
    """each plane 1, 2 or 4 bytes from the start of its allocation, in turn and all at once; the destination 4 bytes in (4-byte stores) and 3"""
    fmt, rows, cols = case
    rng = np.random.default_rng(7 * fmt + cols)
    views, bufs = rm.random_planes(fmt, rows, cols, rng)
    want = rm.to_bgr(fmt, views, rows, cols)
    for offsets in ((1, 0, 0), (0, 2, 0), (0, 0, 4), (4, 4, 4), (1, 2, 4), (2, 1, 1)):
        got = rf.convert_device(pf, fmt, bufs, rows, cols, offsets=offsets)
        assert np.array_equal(got, want), offsets
    for dst_offset in (4, 3):
        assert np.array_equal(rf.convert_device(pf, fmt, bufs, rows, cols, dst_offset=dst_offset), want), dst_offset


def test_device_entry_refuses_what_the_host_entry_refuses(pf):
    import torch
    y = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.full((8 * 8 * 3,), rf.PAD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = y.data_ptr()
    for args, words in ((([p], [0], 7, 8, 8), "unknown raw format"), (([p], [0], rm.NV12, 8, 8), "is missing"), (([p, p], [0, 0], rm.NV12, 6, 7), "even"),
                        (([p], [7], rm.GREY, 8, 8), "step of plane 0"), (([p], [0], rm.BAYER_RGGB, 2, 8), "3 x 3"), (([p], [1 << 30], rm.GREY, 2, 8), "2 GiB")):
        assert not pf.raw_to_bgr_device(*args, dst.data_ptr()) and words in last_error(pf), (args, last_error(pf))
    assert not pf.raw_to_bgr_device([p], [0], rm.GREY, 8, 8, dst.data_ptr(), 23) and "bgr_step" in last_error(pf)
    host = np.zeros(64, np.uint8)
    assert not pf.raw_to_bgr_device([host.ctypes.data], [0], rm.GREY, 8, 8, dst.data_ptr()) and "plane 0" in last_error(pf)
    assert not pf.raw_to_bgr_device([p], [0], rm.GREY, 8, 8, host.ctypes.data) and "destination" in last_error(pf)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == rf.PAD).all()


# ---------------------------------------------------------------- map level
CAM, ROWS, COLS, N = rf.CAM, rf.ROWS, rf.COLS, rf.N
KINDS = ("i16", "f32", "single")


@functools.lru_cache(maxsize=None)
def raw_frames(fmt, rows=ROWS, cols=COLS):
    return tuple(tuple(rf.smooth_planes(fmt, rows, cols, 300 + i)) for i in range(N))


@functools.lru_cache(maxsize=None)
def pictures(fmt, rows=ROWS, cols=COLS):
    """the model's BGR pictures of raw_frames(fmt): what the twin is fed"""
    out = tuple(rm.to_bgr(fmt, p, rows, cols) for p in raw_frames(fmt, rows, cols))
    for a in out:
        a.setflags(write=False)
    return out


def create(pf, kind, thread=False, **opt):
    if kind == "single":
        return pf.Map2D.create(pf.TypeCPU, thread, **opt)
    return pf.Map2D.create(pf.TypeMultiBandCPU, thread, force_float=int(kind == "f32"), **opt)


def digest(g, kind):
    if kind == "single":
        return {"%d,%d" % t: g.tile_bgra(*t).tobytes() for t in g.tiles()}
    return map_digest(g)


def twin_of(pf, kind, frames, order=range(N)):
    """(grid, digest) of the map fed `frames` (BGR or BGRA host pictures) in `order` through pf_feed"""
    poses = lattice_poses(17)
    t = create(pf, kind)
    assert t.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    for k in order:
        assert t.feed(frames[k], poses[k])
    assert t.sync()
    out = (t.grid(), digest(t, kind))
    assert len(out[1]) > 0
    t.close()
    return out


@functools.lru_cache(maxsize=None)
def twin(kind, fmt):
    """computed once per pyramid type and format: the select is order independent, so one twin serves every way in and every lookahead"""
    from conftest import load_package
    return twin_of(load_package(), kind, pictures(fmt))


def feed_raw_device(g, fmt, planes, pose, keep):
    import torch
    ts = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes]
    torch.cuda.synchronize()
    keep.extend(ts)                  # valid and unchanged until sync()
    return g.feed_raw_device([t.data_ptr() for t in ts], [p.shape[1] for p in planes], fmt, ROWS, COLS, pose)


@pytest.mark.parametrize("way", ["host", "host_lookahead0", "device", "device_lookahead0"])
@pytest.mark.parametrize("fmt", rf.MAP_FORMATS, ids=lambda f: rm.NAMES[f])
@pytest.mark.parametrize("kind", KINDS)
def test_map_fed_raw_frames_equals_the_twin(pf, kind, fmt, way):
    poses = lattice_poses(17)
    g = create(pf, kind, **({"lookahead": 0} if way.endswith("lookahead0") else {}))
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    keep = []
    for planes, p in zip(raw_frames(fmt), poses):
        if way.startswith("device"):
            assert feed_raw_device(g, fmt, planes, p, keep), last_error(pf)
        elif fmt == rm.NV12 and way == "host":
            assert g.feed_raw(rm.pack(fmt, planes).reshape(ROWS * 3 // 2, COLS), fmt, p), last_error(pf)          # the packed layout of a file
        else:
            assert g.feed_raw(planes, fmt, p), last_error(pf)
    assert g.sync(), last_error(pf)
    grid, want = twin(kind, fmt)
    assert g.grid() == grid and digest(g, kind) == want
    assert g.stats() == {"rendered": N, "rejected": 0, "dropped": 0}
    del keep
    g.close()


@pytest.mark.parametrize("fmt", rf.MAP_FORMATS, ids=lambda f: rm.NAMES[f])
@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_render_thread_and_a_queue_that_drops(pf, kind, fmt):
    """thread = 1, a queue of one place: frames are dropped as pf_feed drops them; what the map holds is the twin of the keyframes it rendered"""
    poses = lattice_poses(17)
    g = create(pf, kind, thread=True, max_queue=1)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    planes = raw_frames(fmt)
    n = 3 * N
    for k in range(n):
        assert g.feed_raw(planes[k % N], fmt, poses[k % N]), last_error(pf)
    assert g.sync(), last_error(pf)
    log, st = g.render_log(), g.stats()
    assert st["rendered"] == len(log) >= 1 and st["rendered"] + st["dropped"] == n and st["rejected"] == 0 and g.queueSize() == 0
    grid, want = twin_of(pf, kind, pictures(fmt), [k % N for k in log])
    assert g.grid() == grid and digest(g, kind) == want
    # a queue that holds everything drops nothing
    g2 = create(pf, kind, thread=True, max_queue=n)
    assert g2.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    for k in range(N):
        assert g2.feed_raw(planes[k], fmt, poses[k])
    assert g2.sync() and g2.render_log() == list(range(N)) and digest(g2, kind) == twin(kind, fmt)[1]
    keep = []
    assert not feed_raw_device(g2, fmt, planes[0], poses[0], keep) and "thread=0" in last_error(pf)          # device planes need a thread=0 map
    g.close(); g2.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_sortie_that_mixes_raw_bgr_and_bgra_frames(pf, kind):
    poses = lattice_poses(17)
    fmts = (rm.NV12, None, rm.BAYER_RGGB, rm.GREY)
    bgr = pictures(rm.I420)[1]
    four = bgra.padded(bgra.with_alpha(pictures(rm.BAYER_GBRG)[3], 3), 6)
    fed = [pictures(rm.NV12)[0], bgr, pictures(rm.BAYER_RGGB)[2], pictures(rm.GREY)[3], pictures(rm.BAYER_GBRG)[3]]
    g = create(pf, kind)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    for k, f in enumerate(fmts):
        if f is None:
            assert g.feed(bgr, poses[k])
        else:
            assert g.feed_raw(raw_frames(f)[k], f, poses[k]), last_error(pf)
    assert g.feed(four, poses[3])
    assert g.sync()
    t = create(pf, kind)
    assert t.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    for f, k in zip(fed, (0, 1, 2, 3, 3)):
        assert t.feed(f, poses[k])
    assert t.sync() and g.grid() == t.grid() and digest(g, kind) == digest(t, kind) and len(digest(t, kind)) > 0
    g.close(); t.close()


IN_CAM = [402, 312, 300, 300, 200.3, 155.2, -0.12, 0.03, 0.001, -0.0015, 0.0]          # another size than CAM's, even
IN_ROWS, IN_COLS = 312, 402


@pytest.mark.parametrize("way", ["host", "device", "thread"])
@pytest.mark.parametrize("fmt", rf.MAP_FORMATS, ids=lambda f: rm.NAMES[f])
def test_raw_frames_behind_an_input_camera(pf, fmt, way):
    """raw -> BGR -> undistorted: the twin is fed the model's pictures undistorted by tests/undistort_model.py"""
    import torch
    poses = lattice_poses(17)
    x, y, unc = um.table(IN_CAM, CAM)
    assert unc == 0
    und = [um.pixels(x, y, np.ascontiguousarray(p)) for p in pictures(fmt, IN_ROWS, IN_COLS)]
    g = create(pf, "i16", thread=way == "thread")
    assert g.set_input_camera(IN_CAM) and g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
    # a raw frame of the OUTPUT camera's size is now the wrong size
    assert g.feed_raw(raw_frames(fmt)[0], fmt, poses[0]) is (way == "thread") and g.stats()["rendered"] == 0
    keep = []
    for planes, p in zip(raw_frames(fmt, IN_ROWS, IN_COLS), poses):
        if way == "device":
            ts = [torch.from_numpy(np.ascontiguousarray(q)).cuda() for q in planes]
            torch.cuda.synchronize()
            keep.extend(ts)
            assert g.feed_raw_device([t.data_ptr() for t in ts], [q.shape[1] for q in planes], fmt, IN_ROWS, IN_COLS, p), last_error(pf)
        else:
            assert g.feed_raw(planes, fmt, p), last_error(pf)
    assert g.sync(), last_error(pf)
    grid, want = twin_of(pf, "i16", und)
    assert g.grid() == grid and digest(g, "i16") == want and g.stats()["rendered"] == N
    g.close()


@pytest.mark.parametrize("thread", [False, True])
def test_a_raw_frame_of_the_wrong_size_is_rejected_as_pf_feed_rejects_one(pf, thread, capfd):
    poses = lattice_poses(17)
    wrong = rf.smooth_planes(rm.NV12, ROWS - 2, COLS, 1)
    results = []
    for raw in (False, True):
        g = create(pf, "i16", thread=thread)
        assert g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
        capfd.readouterr()
        if raw:
            r = [g.feed_raw(tuple(wrong), rm.NV12, poses[0]), g.feed_raw(rf.smooth_planes(rm.GREY, ROWS, COLS + 1, 2), rm.GREY, poses[1])]
        else:
            r = [g.feed(np.zeros((ROWS - 2, COLS, 3), np.uint8), poses[0]), g.feed(np.zeros((ROWS, COLS + 1, 3), np.uint8), poses[1])]
        assert g.sync()
        results.append((r, g.stats(), g.tiles(), capfd.readouterr().err.count("renderFrame: frame.first.cols!=p->_camera.w")))
        g.close()
    assert results[0] == results[1]
    assert results[0][0] == [thread, thread] and results[0][1]["rejected"] == (0 if thread else 2) and results[0][1]["rendered"] == 0 and results[0][3] == 2


def test_more_raw_frames_than_frame_slots(pf):
    """16 raw keyframes back to back into a map that may hold 7 frame slots: scratch and frame slots are handed out again while the kernels
    that read them are in flight, and blocking uploads go into them"""
    from helpers import jitter_poses
    n = 16
    poses = jitter_poses(n, seed=23, step=(9.0, 4.0))
    fmt = rm.NV12
    raws = [rf.smooth_planes(fmt, ROWS, COLS, 500 + i) for i in range(n)]
    pics = [rm.to_bgr(fmt, p, ROWS, COLS) for p in raws]
    for thread in (False, True):
        opt = dict(max_queue=n if thread else 1, lookahead=2)
        t = create(pf, "i16", **opt); g = create(pf, "i16", thread=thread, **opt)
        assert t.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2]) and g.prepare(workloads().IDENTITY_PLANE, CAM, poses[:2])
        for planes, pic, p in zip(raws, pics, poses):
            assert g.feed_raw(tuple(planes), fmt, p), last_error(pf)
            assert t.feed(pic, p)
        assert g.sync() and t.sync() and g.stats()["rendered"] == t.stats()["rendered"] == n
        assert g.grid() == t.grid() and map_digest(g) == map_digest(t)
        g.close(); t.close()


CHILD = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import raw_frames\n"
         "print('RESULT ' + json.dumps(raw_frames.alloc_failure_case(json.loads(sys.argv[1]))))\n") % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("kind,fmt", [("i16", rm.NV12), ("f32", rm.BAYER_RGGB), ("single", rm.GREY)], ids=["i16-nv12", "f32-rggb", "single-grey"])
def test_an_allocation_failure_during_a_raw_feed_costs_that_keyframe_alone(kind, fmt):
    """the experiments library (its pf_debug_tile_store refuses a tile slab) in a child process, as tests/alloc_failure.py runs its cases"""
    assert os.path.exists(EXP_LIB), "build the experiments library first (__graft_entry__.build())"
    env = dict(os.environ, PF_LIB=EXP_LIB)
    p = subprocess.run([sys.executable, "-c", CHILD, json.dumps({"format": fmt, "type": kind, "k": 2})], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode(errors="replace")
    lines = [l for l in text.splitlines() if l.startswith("RESULT ")]
    assert p.returncode == 0 and lines, text[-3000:]
    r = json.loads(lines[-1][7:])
    assert r["has_hook"]
    assert r["feeds"] == [True, True, False, True] and "tile store" in r["error"], r
    assert r["failed"] == 1 and r["sync"] == [False, True]
    assert r["equal_without_k"] and r["feed_again"] and r["sync_again"] and r["equal_with_k"]
    assert r["stats"] == {"rendered": N - 1, "rejected": 0, "dropped": 0}
