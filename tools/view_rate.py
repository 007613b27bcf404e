#!/usr/bin/env python3
"""What a rendered view costs (csrc/view.hip, map_view.cpp behind pf_render_view*) on the bench mosaic, beside what a client needed before
there were views.

  python tools/view_rate.py [--frames 220] [--reps 7] [--float]

bench.py's cfg-2 sortie (4000 x 3000 keyframes, 20 a flight line) is flown into one map.  Four views of it:
  native    1920 x 1080 at the mosaic's own scale, centred on the content
  rotated   the same turned by 30 degrees
  fitted    the whole content in 1920 x 1080, at the level the scale chooses
  camera    what the camera saw at a keyframe's pose (4000 x 3000)
For each, the median over --reps of: the wall time of the view into device memory (nothing crosses PCIe), into page-locked host memory
(width x height x 4 bytes cross) and as a JPEG stream (the stream crosses); the GPU time of the collapse, the coverage pass and the view
kernel between HIP events (pf_debug_view_timing); the tiles collapsed.  Beside them the closest a client could do without views:
pf_blend_tiles_level of the tiles the view touches, at the view's level, into page-locked memory (the client still has to compose, rotate
and scale them), and pf_save_to_memory_level of the whole mosaic at that level.

Prints one JSON line per view and a summary line.  Needs the GPU: there is no CPU path."""
import argparse
import importlib
import importlib.util
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = [4000, 3000, 3000, 3000, 2000, 1500]
HEIGHT = 100.0


def load_package():
    name = "pi_slam_fusion_amd"
    if name in sys.modules:
        return sys.modules[name]
    path = os.path.join(ROOT, "pi-slam-fusion_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--float", action="store_true", help="the fp32 pyramid instead of int16")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("view_rate: no GPU (a rate is measured on the GPU or not at all)")
    pf = load_package()
    wl = importlib.import_module("pi_slam_fusion_amd.workloads")
    poses = wl.serpentine(CAM, HEIGHT, args.frames, max_rows=16)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1234)
    frames = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(8)]
    torch.cuda.synchronize()
    m = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=int(args.float))
    assert m.prepare(wl.IDENTITY_PLANE, CAM, poses)
    for k in range(args.frames):
        assert m.feed_device(frames[k % len(frames)].data_ptr(), 3000, 4000, poses[k])
    assert m.sync()
    dims, geo = m.grid()
    tiles = set(m.tiles())
    xs, ys = [t[0] for t in tiles], [t[1] for t in tiles]
    lp = geo[5]
    cx = geo[0] + ((min(xs) + max(xs) + 1) / 2 - dims[2]) * geo[4]
    cy = geo[1] + ((min(ys) + max(ys) + 1) / 2 - dims[3]) * geo[4]

    def similarity(scale, deg, w, h):          # plane point (cx, cy) to the view's middle
        a = math.radians(deg)
        V = np.array([[scale * math.cos(a), -scale * math.sin(a), 0.0], [scale * math.sin(a), scale * math.cos(a), 0.0], [0, 0, 1.0]])
        p = V @ np.array([cx, cy, 1.0])
        V[0, 2] = w / 2 - p[0]; V[1, 2] = h / 2 - p[1]
        return V

    views = [("native", similarity(1 / lp, 0, 1920, 1080), 1920, 1080), ("rotated", similarity(1 / lp, 30, 1920, 1080), 1920, 1080),
             ("fitted", m.view_of_extent(1920, 1080), 1920, 1080), ("camera", m.view_from_pose(poses[args.frames // 2]), CAM[0], CAM[1])]
    m.view_timing(True)
    summary = {}
    for name, V, w, h in views:
        dev = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        pinned = pf.host_array((h, w, 4))
        info = m.render_view_device(V, w, h, dev.data_ptr())          # warm-up: scratch buffers, code objects
        m.render_view(V, w, h, out=pinned); stream, _ = m.render_view_jpeg(V, w, h)
        gpu = []
        def device_view():
            m.render_view_device(V, w, h, dev.data_ptr()); gpu.append(m.view_timing())
        wall_dev = timed(device_view, args.reps)
        wall_host = timed(lambda: m.render_view(V, w, h, out=pinned), args.reps)
        wall_jpeg = timed(lambda: m.render_view_jpeg(V, w, h), args.reps)
        k = info["level"]; e = 256 >> k
        tx, ty, nx, ny = info["rect"]
        touched = [(x, y) for y in range(ty, ty + ny) for x in range(tx, tx + nx) if (x, y) in tiles]
        tile_buf = pf.host_array((max(len(touched), 1), e, e, 3))
        wall_tiles = timed(lambda: m.blend_tiles(touched, out=tile_buf, level=k), args.reps) if touched else None
        whole = m.save_to_memory(alloc=pf.host_array, level=k)[0]
        wall_save = timed(lambda: m.save_to_memory(alloc=lambda s: whole, level=k), max(args.reps // 2, 1))
        rec = {"what": "view", "view": name, "pyramid": "fp32" if args.float else "int16", "width": w, "height": h, "level": k, "tiles_collapsed": info["tiles"],
               "tiles_held": len(touched), "map_tiles": len(tiles),
               "gpu_ms": {"collapse": statistics.median(g[0] for g in gpu), "coverage": statistics.median(g[1] for g in gpu), "view_kernel": statistics.median(g[2] for g in gpu)},
               "wall_ms": {"device": wall_dev, "host_pinned": wall_host, "jpeg": wall_jpeg},
               "pcie_bytes": {"device": 0, "host_pinned": w * h * 4, "jpeg": len(stream)},
               "before": {"blend_tiles_level_ms": wall_tiles, "blend_tiles_level_bytes": len(touched) * e * e * 3, "save_to_memory_level_ms": wall_save,
                          "save_to_memory_level_bytes": int(whole.size)}}
        print(json.dumps(rec)); sys.stdout.flush()
        summary[name] = {"level": k, "tiles": info["tiles"], "device_ms": round(wall_dev, 3), "host_ms": round(wall_host, 3), "jpeg_ms": round(wall_jpeg, 3),
                         "tiles_route_ms": None if wall_tiles is None else round(wall_tiles, 3), "save_route_ms": round(wall_save, 3)}
        del dev
    print(json.dumps({"summary": summary}))
    m.close()


if __name__ == "__main__":
    main()
