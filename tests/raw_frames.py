"""What the raw-frame tests share (test_raw_model.py, test_raw_sanitizers.py, test_gpu_raw.py, test_replay_raw.py): the size list, the calls
into pf_raw_to_bgr / pf_raw_to_bgr_device with padded, guarded destinations, and the child-process case of the allocation-failure test."""
import ctypes as C

import numpy as np

import raw_model as rm

# (cols, rows) as the issue lists them: the smallest of each family, widths around a thread's run of 8 pixels, a row longer than one
# wave's 512 pixels with a tail, and an odd size for the formats that take one
SIZES = [(2, 2), (3, 3), (1, 1), (6, 4), (10, 6), (18, 2), (530, 6), (37, 29)]
PAD = 0xA5
GUARD = 64


def cases():
    return [(f, r, c) for f in rm.FORMATS for (c, r) in SIZES if rm.valid_size(f, r, c)]


def case_id(case):
    return "%s-%dx%d" % (rm.NAMES[case[0]], case[2], case[1])


def descriptor(pf, fmt, planes, rows, cols, ptrs=None, steps=None):
    """pf_raw_frame of 2-D uint8 views (or of explicit pointers and steps)"""
    f = pf.RawFrame(int(fmt), int(rows), int(cols))
    for k in range(len(planes) if ptrs is None else len(ptrs)):
        f.plane[k] = planes[k].ctypes.data if ptrs is None else ptrs[k]
        f.step[k] = planes[k].strides[0] if steps is None else steps[k]
    return f


def convert_host(pf, fmt, planes, rows, cols, dst_pad=0):
    """pf_raw_to_bgr into a destination with dst_pad bytes between its rows and a guard behind it, all of which must come back untouched"""
    step = cols * 3 + dst_pad
    dst = np.full(rows * step + GUARD, PAD, np.uint8)
    f = descriptor(pf, fmt, planes, rows, cols)
    assert pf.lib().pf_raw_to_bgr(C.byref(f), dst.ctypes.data, step if dst_pad else 0), pf.lib().pf_last_error().decode()
    body = dst[:rows * step].reshape(rows, step)
    assert (body[:, cols * 3:] == PAD).all() and (dst[rows * step:] == PAD).all(), "bytes outside the output rows were written"
    return np.ascontiguousarray(body[:, :cols * 3]).reshape(rows, cols, 3)


def to_device(buf, offset=0):
    """a host buffer (any shape) as a flat device tensor that starts `offset` bytes into its allocation; returns (tensor, pointer)"""
    import torch
    flat = np.ascontiguousarray(buf).reshape(-1)
    t = torch.empty(flat.size + offset, dtype=torch.uint8, device="cuda")
    t[offset:] = torch.from_numpy(flat).cuda()
    return t, t.data_ptr() + offset


def convert_device(pf, fmt, bufs, rows, cols, dst_pad=0, offsets=(0, 0, 0), dst_offset=0):
    """pf_raw_to_bgr_device.  bufs[k]: plane k's 2-D host buffer, a row of it being the plane's step; the planes go into
    separate device allocations, plane k offsets[k] bytes from its allocation's start; destination padded and guarded as on the host"""
    import torch
    keep, ptrs, steps = [], [], []
    for k, b in enumerate(bufs):
        t, p = to_device(b, offsets[k])
        keep.append(t); ptrs.append(p); steps.append(b.shape[1])
    step = cols * 3 + dst_pad
    dst = torch.full((dst_offset + rows * step + GUARD,), PAD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ok = pf.raw_to_bgr_device(ptrs, steps, fmt, rows, cols, dst.data_ptr() + dst_offset, step if dst_pad else 0)
    assert ok, pf.lib().pf_last_error().decode()
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    body = raw[dst_offset:dst_offset + rows * step].reshape(rows, step)
    assert (raw[:dst_offset] == PAD).all() and (body[:, cols * 3:] == PAD).all() and (raw[dst_offset + rows * step:] == PAD).all(), \
        "bytes outside the output rows were written"
    del keep
    return np.ascontiguousarray(body[:, :cols * 3]).reshape(rows, cols, 3)


# ---- the map-level workload: the small camera of tests/test_gpu_model.py with even sides
CAM = [332, 256, 260, 260, 166.0, 128.0]
ROWS, COLS = 256, 332
N = 4
MAP_FORMATS = (rm.NV12, rm.BAYER_RGGB, rm.GREY)


def smooth_planes(fmt, rows, cols, seed):
    """a raw frame with structure at every scale (noise over gradients), as separate contiguous planes"""
    rng = np.random.default_rng(seed)
    out = []
    for (r, c) in rm.plane_shapes(fmt, rows, cols):
        yy, xx = np.mgrid[0:r, 0:c]
        base = 96 + 64 * np.sin(xx / (7.0 + seed % 5)) * np.cos(yy / (11.0 + seed % 3))
        out.append(np.clip(base + rng.integers(-60, 61, (r, c)), 0, 255).astype(np.uint8))
    return out


def alloc_failure_case(spec):
    """Runs in a child process that loaded the experiments library (PF_LIB): keyframe K of a raw sortie meets a refused tile slab inside its
    own pf_feed_raw.  Returns plain facts; the parent asserts.  spec: {"format", "type", "k"}"""
    import importlib
    from conftest import load_package
    from helpers import map_digest
    from test_gpu_model import lattice_poses
    pf = load_package()
    wl = importlib.import_module("pi_slam_fusion_amd.workloads")
    fmt, k_fail = spec["format"], spec["k"]
    poses = lattice_poses(17)
    raws = [smooth_planes(fmt, ROWS, COLS, 300 + i) for i in range(N)]
    pictures = [rm.to_bgr(fmt, p, ROWS, COLS) for p in raws]

    def create():
        if spec["type"] == "single":
            return pf.Map2D.create(pf.TypeCPU, False, lookahead=0)
        return pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=int(spec["type"] == "f32"), lookahead=0)

    def digest(m):
        if spec["type"] == "single":
            return {"%d,%d" % t: m.tile_bgra(*t).tobytes().hex() for t in m.tiles()}
        return map_digest(m)
    r = {"has_hook": hasattr(pf.lib(), "pf_debug_tile_store"), "feeds": []}
    g = create()
    g.debug_tile_store(4)
    assert g.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
    for i in range(N):
        if i == k_fail:
            g.debug_tile_store(4, 0, 1)          # the next slab the store asks for is refused
        r["feeds"].append(bool(g.feed_raw(tuple(raws[i]), fmt, poses[i])))
        if i == k_fail:
            r["error"] = pf.lib().pf_last_error().decode()
            g.debug_tile_store(4)
    r["failed"] = g.failed()
    r["sync"] = [bool(g.sync()), bool(g.sync())]
    r["stats"] = g.stats()
    # the twin never saw keyframe K
    t = create()
    assert t.prepare(wl.IDENTITY_PLANE, CAM, poses[:2])
    for i in range(N):
        if i != k_fail:
            assert t.feed(pictures[i], poses[i])
    assert t.sync()
    r["equal_without_k"] = digest(g) == digest(t) and len(digest(t)) > 0
    # fed again once memory is back, the keyframe is in
    r["feed_again"] = bool(g.feed_raw(tuple(raws[k_fail]), fmt, poses[k_fail]))
    assert t.feed(pictures[k_fail], poses[k_fail])
    r["sync_again"] = bool(g.sync()) and bool(t.sync())
    r["equal_with_k"] = digest(g) == digest(t)
    g.close(); t.close()
    return r
