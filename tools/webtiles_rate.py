#!/usr/bin/env python3
"""Web-Mercator map tiles of the bench mosaic at the native zoom (dev tool; the mosaic is tools/tiff_rate.py's): wall time of pf_webtiles into
a discarding sink beside save_tiff of the same map in the same process, interleaved, median of --reps after a warm-up round; the GPU time of
the sample kernel, the reduce kernel and the encoder of one export by HIP events (pf_debug_webtiles_timing); the sample kernel's bytes read +
written over its time, against the 8 TB/s the other profiles quote.
usage: tools/webtiles_rate.py [--int16] [--frames N] [--reps R] [--dir D] [--yaw DEG] [--kernels-only]
  --yaw DEG        the plane's yaw against north (default 30): the tiles are north-up, the sampler gathers across the mosaic's rows
  --kernels-only   three exports and nothing else: the run to put under rocprofv3 --kernel-trace --stats (k_webtile_sample, k_webtile_reduce,
                   the k_jenc_* kernels; wall times under the profiler mean nothing)"""
import argparse, ctypes as C, importlib, math, os, statistics, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import bench
ap = argparse.ArgumentParser(); ap.add_argument("--int16", action="store_true"); ap.add_argument("--frames", type=int, default=120)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--dir", default=None); ap.add_argument("--yaw", type=float, default=30.0)
ap.add_argument("--kernels-only", action="store_true")
a = ap.parse_args()
import numpy as np, torch
pf = bench.load_package(); wl = importlib.import_module("pi_slam_fusion_amd.workloads")
L = pf.lib()
cam = [4000, 3000, 3000, 3000, 2000, 1500]
poses = wl.serpentine(cam, 100.0, a.frames)
m = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=0 if a.int16 else 1)
assert m.prepare(wl.IDENTITY_PLANE, cam, poses[:20])
fr = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
torch.cuda.synchronize()
for k in range(a.frames):
    m.feed_device(fr[k % 4].data_ptr(), 3000, 4000, poses[k])
m.sync()
# the plane is the identity: a yaw of the whole ground is a yaw of GPS north, i.e. of px2ll -- pf_webtiles takes the map's own georeference,
# so the yawed run goes through pf_webtiles_device on the mosaic and mask of the same map, uploaded once
origin = (13.405, 52.52, 40.0)
p, rows, cols = m.webtiles_georef(origin)
count = [0, 0, 0]
def discard(user, t):
    count[0] += 1; count[1] += t.contents.jpeg_len; count[2] += t.contents.cover == 1
    return 1
sink = pf.WEBTILE_SINK(discard)
og = (C.c_double * 3)(*origin)
def export_map():
    count[:] = [0, 0, 0]
    t0 = time.perf_counter(); assert L.pf_webtiles(m._h, og, -1, -1, 95, 0, sink, None), L.pf_last_error(); return time.perf_counter() - t0
mem, mask, org = m.save_to_memory_mask()
dmem, dmask = torch.from_numpy(mem).cuda(), torch.from_numpy(mask).cuda()
torch.cuda.synchronize()
c, s = math.cos(math.radians(a.yaw)), math.sin(math.radians(a.yaw))
cx, cy = cols / 2.0, rows / 2.0
lat0 = p[3] + p[4] * cx + p[5] * cy; k = math.cos(math.radians(lat0))          # degrees of longitude are shorter by cos(lat): rotate in metres
A = np.array([[p[1] * k, p[2] * k], [p[4], p[5]]]); Rm = np.array([[c, -s], [s, c]]) @ A
py = np.array([0, Rm[0, 0] / k, Rm[0, 1] / k, 0, Rm[1, 0], Rm[1, 1]])
py[0] = p[0] + p[1] * cx + p[2] * cy - py[1] * cx - py[2] * cy; py[3] = lat0 - py[4] * cx - py[5] * cy
pyp = np.ascontiguousarray(py).ctypes.data_as(C.POINTER(C.c_double))
def export_yawed():
    count[:] = [0, 0, 0]
    t0 = time.perf_counter()
    assert L.pf_webtiles_device(dmem.data_ptr(), rows, cols, 0, dmask.data_ptr(), 0, pyp, -1, -1, 95, 0, 0, sink, None, None), L.pf_last_error()
    return time.perf_counter() - t0
if a.kernels_only:
    for _ in range(3):
        export_map(); export_yawed()
    print("kernels-only: 3 x (pf_webtiles, pf_webtiles_device yawed %.0f deg), %d tiles in the last" % (a.yaw, count[0]))
    sys.exit(0)
with tempfile.TemporaryDirectory(dir=a.dir) as d:
    tif = os.path.join(d, "m.tif")
    def t_tif():
        t0 = time.perf_counter(); assert m.save_tiff(tif); return time.perf_counter() - t0
    t_tif(); export_map(); export_yawed()                    # warm-up: code objects, buffers, page-locked memory
    times = {"tif": [], "map": [], "yawed": []}
    for _ in range(max(a.reps, 5)):
        times["tif"].append(t_tif()); times["map"].append(export_map()); n_map = list(count); times["yawed"].append(export_yawed()); n_yaw = list(count)
    import tiff_model as tm
    _, ifds = tm.parse(open(tif, "rb").read())
    n_tif = sum(len(i["tags"][324][1]) for i in ifds)
    nz = pf.webtiles_native_zoom(p, rows, cols)
    print("mosaic %d x %d (%d map tiles, %.0f MB of BGR8, %.1f %% covered), native zoom %d, %d reps interleaved:" %
          (cols, rows, len(m.tiles()), rows * cols * 3 / 1e6, 100.0 * (mask != 0).mean(), nz, len(times["tif"])))
    for key, label in (("tif", "save_tiff(m.tif), %d tiles" % n_tif), ("map", "pf_webtiles, %d tiles (%d partial, %.1f MB)" % (n_map[0], n_map[2], n_map[1] / 1e6)),
                       ("yawed", "pf_webtiles_device yawed %.0f deg, %d tiles (%d partial, %.1f MB)" % (a.yaw, n_yaw[0], n_yaw[2], n_yaw[1] / 1e6))):
        v = times[key]
        print("  %-66s median %8.1f ms  (min %.1f, max %.1f; runs %s)" % (label, statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3, " ".join("%.1f" % (x * 1e3) for x in v)))
    # the parts, by HIP events around their launches (a run of its own: the events are extra work in the stream)
    L.pf_debug_webtiles_timing(1)
    out = (C.c_double * 4)()
    for label, run, georef in (("pf_webtiles", export_map, p), ("yawed %.0f deg" % a.yaw, export_yawed, py)):
        wall = run()
        L.pf_debug_webtiles_timing_read(out)
        sample_ms, reduce_ms, enc_ms, sampled = out[0], out[1], out[2], int(out[3])
        # bytes of the sample kernel: every sampled tile written once (pixels + mask), the tables, and of the source what the tiles' footprint
        # covers -- at most the whole mosaic and mask once (4 bytes a pixel), the part of each tap that is not a cache hit
        written = sampled * (256 * 256 * 3 + 8192)
        read = rows * cols * 4
        print("  %-18s wall %8.1f ms: sample %7.3f ms over %d tiles, reduce %7.3f ms, encoder %8.1f ms (its host waits included)" % (label, wall * 1e3, sample_ms, sampled, reduce_ms, enc_ms))
        if sample_ms > 0:
            print("  %-18s sample kernel: %.0f MB written + %.0f MB read once = %.0f MB over %.3f ms = %.2f TB/s (%.0f %% of 8 TB/s)" %
                  ("", written / 1e6, read / 1e6, (written + read) / 1e6, sample_ms, (written + read) / sample_ms / 1e9, 100.0 * (written + read) / sample_ms / 1e9 / 8.0))
    L.pf_debug_webtiles_timing(0)
