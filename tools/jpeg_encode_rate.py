#!/usr/bin/env python3
"""save("m.jpg") on the bench mosaic (dev tool; the mosaic is tools/blend_save_rate.py's): wall time of save(".jpg"), save(".png") and
save_to_memory on the same map in the same process, interleaved, median of --reps after a warm-up round.
usage: tools/jpeg_encode_rate.py [--int16] [--frames N] [--reps R] [--dir D] [--kernels-only]
  --kernels-only   a few save(".jpg") and nothing else: the run to put under  rocprofv3 --kernel-trace --stats -d OUT -- python tools/...
                   (the k_jenc_* kernels and the scan's; wall times under the profiler mean nothing)
Also prints what the encoder's kernels move (pixels read, coefficients written and read, streams written) for the rate against the roofline,
the time of writing a file of the stream's size alone, and checks the file against the host encoder once (pf_jpeg_encode_bgr)."""
import argparse, importlib, os, statistics, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench
ap = argparse.ArgumentParser(); ap.add_argument("--int16", action="store_true"); ap.add_argument("--frames", type=int, default=120)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--dir", default=None); ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--no-check", action="store_true")
a = ap.parse_args()
import numpy as np, torch
pf = bench.load_package(); wl = importlib.import_module("pi_slam_fusion_amd.workloads")
cam = [4000, 3000, 3000, 3000, 2000, 1500]
poses = wl.serpentine(cam, 100.0, a.frames)
m = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=0 if a.int16 else 1)
assert m.prepare(wl.IDENTITY_PLANE, cam, poses[:20])
fr = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
torch.cuda.synchronize()
for k in range(a.frames):
    m.feed_device(fr[k % 4].data_ptr(), 3000, 4000, poses[k])
m.sync()
with tempfile.TemporaryDirectory(dir=a.dir) as d:
    jpg, png, raw = os.path.join(d, "m.jpg"), os.path.join(d, "m.png"), os.path.join(d, "m.bin")
    if a.kernels_only:
        for _ in range(3):
            assert m.save(jpg)
        print("kernels-only: 3 x save(jpg), file %d bytes" % os.path.getsize(jpg))
        sys.exit(0)
    keep = {}
    def pinned(shape):
        if "p" not in keep: keep["p"] = pf.host_array(shape)
        return keep["p"]
    def t_jpg():
        t0 = time.perf_counter(); assert m.save(jpg); return time.perf_counter() - t0
    def t_png():
        t0 = time.perf_counter(); assert m.save(png); return time.perf_counter() - t0
    def t_mem():
        t0 = time.perf_counter(); r = m.save_to_memory(alloc=pinned); assert r is not None; return time.perf_counter() - t0
    def t_write():
        t0 = time.perf_counter()
        with open(raw, "wb") as f: f.write(keep["stream"])
        return time.perf_counter() - t0
    t_jpg(); t_png(); t_mem()                                   # warm-up: code objects, buffers, page-locked memory
    keep["stream"] = open(jpg, "rb").read()
    t_write()
    times = {"jpg": [], "png": [], "mem": [], "write": []}
    for _ in range(max(a.reps, 5)):
        times["jpg"].append(t_jpg()); times["png"].append(t_png()); times["mem"].append(t_mem()); times["write"].append(t_write())
    med = {k: statistics.median(v) for k, v in times.items()}
    img = keep["p"]
    rows, cols = img.shape[:2]
    px = rows * cols
    nstream = len(keep["stream"])
    print("mosaic %d x %d (%d tiles, %.0f MB of BGR8), %d reps interleaved, medians:" % (cols, rows, len(m.tiles()), px * 3 / 1e6, len(times["jpg"])))
    for k, label in (("jpg", "save(m.jpg)"), ("png", "save(m.png)"), ("mem", "save_to_memory (page-locked buffer)"), ("write", "writing %.1f MB alone" % (nstream / 1e6))):
        print("  %-38s %9.1f ms   (min %.1f, max %.1f)" % (label, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3))
    print("  jpg file %.1f MB, png file %.1f MB" % (nstream / 1e6, os.path.getsize(png) / 1e6))
    print("  jpg / png wall: %.3f;  (jpg - file write) / save_to_memory: %.2f" % (med["jpg"] / med["png"], (med["jpg"] - med["write"]) / med["mem"]))
    # what the encoder's kernels read and write: pixels once, coefficients (int16, 1.5 per pixel) written and read once, the entropy-coded
    # data written (packed), read twice (count, scatter) and written once more (stuffed)
    moved = px * 3 + 2 * px * 3 + 4 * nstream
    print("  encoder kernels move %.0f MB per save (pixels %.0f + coefficients 2 x %.0f + stream 4 x %.1f): at 8 TB/s %.2f ms" %
          (moved / 1e6, px * 3 / 1e6, px * 3 / 1e6, nstream / 1e6, moved / 8e12 * 1e3))
    if not a.no_check:
        ok = pf.jpeg_encode(img, 95) == keep["stream"]
        print("  file == pf_jpeg_encode_bgr(save_to_memory, 95): %s" % ok)
        assert ok
