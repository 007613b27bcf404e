#!/usr/bin/env python3
"""save("m.tif") on the bench mosaic (dev tool; the mosaic is tools/blend_save_rate.py's): wall time of save(".tif"), save(".jpg") and of
writing a file of the .tif's size alone, on the same map in the same process, interleaved, median of --reps after a warm-up round.
usage: tools/tiff_rate.py [--int16] [--frames N] [--reps R] [--dir D] [--kernels-only] [--no-check] [--masked]
  --masked         save_tiff_masked beside save_tiff on the same map, interleaved: wall times (median, min, max, every run), the mask tiles
                   of the file by kind, the mask bytes that crossed to the host, the file's size against the unmasked file's, and the file
                   against the host writer once (pf_tiff_write_bgr_masked).  With --kernels-only: a few masked saves for the profiler
                   (k_coverage_tiles, k_mask_overview, k_mask_gather).
  --kernels-only   a few save(".tif") and save(".jpg") and nothing else: the run to put under
                   rocprofv3 --kernel-trace --stats -d OUT -- python tools/tiff_rate.py --kernels-only
                   (k_overview*, the k_jenc_* kernels of the tile encode and of the whole-image encode; wall times under the profiler mean nothing)
Also prints the tile and empty-tile counts of the file, the bytes the overview chain moves (for the rate against the roofline), the device
memory in use after each kind of save, and checks the file against the host writer once (pf_tiff_write_bgr)."""
import argparse, importlib, os, statistics, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import bench
ap = argparse.ArgumentParser(); ap.add_argument("--int16", action="store_true"); ap.add_argument("--frames", type=int, default=120)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--dir", default=None); ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--no-check", action="store_true"); ap.add_argument("--masked", action="store_true")
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
def used_mb():
    free, total = torch.cuda.mem_get_info(); return (total - free) / 1e6
with tempfile.TemporaryDirectory(dir=a.dir) as d:
    tif, jpg, raw = os.path.join(d, "m.tif"), os.path.join(d, "m.jpg"), os.path.join(d, "m.bin")
    base = used_mb()
    if a.kernels_only and a.masked:
        for _ in range(3):
            assert m.save_tiff_masked(tif)
        print("kernels-only: 3 x save_tiff_masked, file %d bytes" % os.path.getsize(tif))
        sys.exit(0)
    if a.masked:
        mt = os.path.join(d, "masked.tif")
        def t_plain():
            t0 = time.perf_counter(); assert m.save_tiff(tif); return time.perf_counter() - t0
        def t_masked():
            t0 = time.perf_counter(); assert m.save_tiff_masked(mt); return time.perf_counter() - t0
        t_plain(); t_masked()                                     # warm-up: code objects, buffers, page-locked memory
        times = {"plain": [], "masked": []}
        for _ in range(max(a.reps, 5)):
            times["plain"].append(t_plain()); times["masked"].append(t_masked())
        import tiff_model as tm, tiff_mask_model as mm
        data = open(mt, "rb").read()
        big, ifds = tm.parse(data)
        kinds = {"zero": 0, "one": 0, "own": 0}
        for i in ifds[1::2]:
            for o in i["tags"][324][1]:
                kinds[mm.kind_of(data[o:o + mm.TILE_BYTES])] += 1
        nt = sum(kinds.values())
        rows, cols = ifds[0]["tags"][257][1][0], ifds[0]["tags"][256][1][0]
        print("mosaic %d x %d (%d map tiles), %d images + %d masks, %d reps interleaved:" % (cols, rows, len(m.tiles()), len(ifds) // 2, len(ifds) // 2, len(times["plain"])))
        for k, label in (("plain", "save_tiff(m.tif)"), ("masked", "save_tiff_masked(m.tif)")):
            v = times[k]
            print("  %-26s median %8.1f ms  (min %.1f, max %.1f; runs %s)" % (label, statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3, " ".join("%.1f" % (x * 1e3) for x in v)))
        print("  masked - plain, medians: %+.1f ms" % ((statistics.median(times["masked"]) - statistics.median(times["plain"])) * 1e3))
        print("  mask tiles %d: %d all zero, %d all one (each kind stored once), %d stored on their own" % (nt, kinds["zero"], kinds["one"], kinds["own"]))
        print("  mask bytes that crossed to the host: %d of tiles + %d of flags (the unmasked save: %d of flags); level-0 plane %d bytes stays in HBM" %
              (kinds["own"] * mm.TILE_BYTES, 3 * nt, nt, rows * cols // 8))
        print("  file %d bytes masked, %d unmasked: %+d (%.3f %%)" % (len(data), os.path.getsize(tif), len(data) - os.path.getsize(tif), 100.0 * (len(data) - os.path.getsize(tif)) / os.path.getsize(tif)))
        if not a.no_check:
            mem, mask, org = m.save_to_memory_mask()
            dims, geo = m.grid()
            xf = [geo[5], 0, 0, geo[0] + (org[0] - dims[2]) * geo[4], 0, geo[5], 0, geo[1] + (org[1] - dims[3]) * geo[4], 0, 0, 1, 0, 0, 0, 0, 1]
            assert pf.tiff_write_masked(raw, mem, mask, 95, 0, xf)
            ok = open(raw, "rb").read() == data
            print("  file == pf_tiff_write_bgr_masked(save_to_memory_mask, 95, 0, transform, 0): %s;  covered %.1f %% of the bounding box" % (ok, 100.0 * (mask != 0).mean()))
            assert ok
        sys.exit(0)
    if a.kernels_only:
        for _ in range(3):
            assert m.save(tif) and m.save(jpg)
        print("kernels-only: 3 x (save(tif), save(jpg)), files %d and %d bytes" % (os.path.getsize(tif), os.path.getsize(jpg)))
        sys.exit(0)
    def t_tif():
        t0 = time.perf_counter(); assert m.save(tif); return time.perf_counter() - t0
    def t_jpg():
        t0 = time.perf_counter(); assert m.save(jpg); return time.perf_counter() - t0
    keep = {}
    def t_write():
        t0 = time.perf_counter()
        with open(raw, "wb") as f: f.write(keep["file"])
        return time.perf_counter() - t0
    t_tif(); after_tif = used_mb()                              # warm-up: code objects, buffers, page-locked memory
    t_jpg(); after_jpg = used_mb()
    keep["file"] = open(tif, "rb").read()
    t_write()
    times = {"tif": [], "jpg": [], "write": []}
    for _ in range(max(a.reps, 5)):
        times["tif"].append(t_tif()); times["jpg"].append(t_jpg()); times["write"].append(t_write())
    med = {k: statistics.median(v) for k, v in times.items()}
    import tiff_model as tm
    big, ifds = tm.parse(keep["file"])
    rows, cols = ifds[0]["tags"][257][1][0], ifds[0]["tags"][256][1][0]
    px = rows * cols
    allpx = sum(i["tags"][257][1][0] * i["tags"][256][1][0] for i in ifds)
    per = [tm.tile_streams(keep["file"], i) for i in ifds]
    counts = {}
    for s in per:
        for o in s: counts[o] = counts.get(o, 0) + 1
    shared = max(counts.items(), key=lambda kv: kv[1])
    n_tiles = sum(len(s) for s in per); n_empty = shared[1] if shared[1] > 1 else 0
    n0_empty = sum(1 for o in per[0] if o == shared[0]) if n_empty else 0
    nfile, njpg = len(keep["file"]), os.path.getsize(jpg)
    print("mosaic %d x %d (%d map tiles, %.0f MB of BGR8), %d images, %d reps interleaved, medians:" % (cols, rows, len(m.tiles()), px * 3 / 1e6, len(ifds), len(times["tif"])))
    for k, label in (("tif", "save(m.tif)"), ("jpg", "save(m.jpg)"), ("write", "writing %.1f MB alone" % (nfile / 1e6))):
        print("  %-38s %9.1f ms   (min %.1f, max %.1f)" % (label, med[k] * 1e3, min(times[k]) * 1e3, max(times[k]) * 1e3))
    print("  tif file %.1f MB (%s), jpg file %.1f MB;  tif - its file write: %.1f ms" % (nfile / 1e6, "BigTIFF" if big else "classic", njpg / 1e6, (med["tif"] - med["write"]) * 1e3))
    print("  tiles %d (image 0: %d), empty %d (image 0: %d): %.1f MB of streams and %d tile encodes not made" %
          (n_tiles, len(per[0]), n_empty, n0_empty, max(n_empty - 1, 0) * shared[0][1] / 1e6, n_empty))
    print("  overview chain moves %.0f MB (image 0 read once %.0f + levels written %.0f): at 8 TB/s %.3f ms" %
          ((px + (allpx - px)) * 3 / 1e6, px * 3 / 1e6, (allpx - px) * 3 / 1e6, allpx * 3 / 8e12 * 1e3))
    print("  device memory in use: %.0f MB before any save, %.0f MB after save(tif), %.0f MB after save(jpg) as well" % (base, after_tif, after_jpg))
    if not a.no_check:
        mem, org = m.save_to_memory()
        dims, geo = m.grid()
        xf = [geo[5], 0, 0, geo[0] + (org[0] - dims[2]) * geo[4], 0, geo[5], 0, geo[1] + (org[1] - dims[3]) * geo[4], 0, 0, 1, 0, 0, 0, 0, 1]
        assert pf.tiff_write(raw, mem, 95, 0, xf)
        ok = open(raw, "rb").read() == keep["file"]
        print("  file == pf_tiff_write_bgr(save_to_memory, 95, 0, transform, 0): %s" % ok)
        assert ok
