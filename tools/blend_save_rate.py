#!/usr/bin/env python3
"""Output side of the path on the bench mosaic (dev tool): Ele::blend of every changed tile and save().
usage: tools/blend_save_rate.py [--int16] [--frames N] [--reps R] [--no-files] [--level K[,K...] [--rounds N]]
Prints wall times into a fresh pageable buffer (first touch included), a touched pageable buffer and a page-locked one, and the
kernels' own time and algorithmic rate from the profile table.
--level: the reduced-resolution views instead (level 0 = the existing path).  Every round measures each listed level in turn on the
same map (interleaved, one process, one box): the kernel by HIP events, blend_tiles and save_to_memory into page-locked buffers by
wall clock; then the slowest / fastest round per level.
The frames are seeded, and every mode prints a sha256 of the blend_tiles buffer and of the save_to_memory buffer (per level): two builds
of the library (PF_LIB) that compute the same print the same lines.  --no-files: without the save() of files at the end."""
import argparse, hashlib, importlib, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench
ap = argparse.ArgumentParser(); ap.add_argument("--int16", action="store_true"); ap.add_argument("--frames", type=int, default=120)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--no-files", action="store_true")
ap.add_argument("--level", default=None, help="comma-separated pyramid levels of the views to measure"); ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
import numpy as np, torch
pf = bench.load_package(); wl = importlib.import_module("pi_slam_fusion_amd.workloads")
cam = [4000, 3000, 3000, 3000, 2000, 1500]
poses = wl.serpentine(cam, 100.0, a.frames)
torch.manual_seed(0)
sha = lambda x: hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
m = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=0 if a.int16 else 1)
assert m.prepare(wl.IDENTITY_PLANE, cam, poses[:20])
fr = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
torch.cuda.synchronize()
for k in range(a.frames):
    m.feed_device(fr[k % 4].data_ptr(), 3000, 4000, poses[k])
m.sync()
nt = len(m.tiles())
m.profile_reset(); m.profile_enable(1)
def level_rounds(levels, rounds):
    tiles = m.tiles()
    kern = lambda name: (lambda v: v["ms"] / max(v["launches"], 1))(m.profile_read()[name])
    bufs = {k: pf.host_array((len(tiles), 256 >> k, 256 >> k, 3)) for k in levels}
    keep = {}
    def alloc(shape):
        if shape not in keep: keep[shape] = pf.host_array(shape)
        return keep[shape]
    for k in levels:                                  # warm-up: buffers, page-locked registrations, first launches
        assert m.blend_tiles(tiles, out=bufs[k], level=k) is not None
        img = m.save_to_memory(alloc=alloc, level=k)
        assert img is not None
        print("sha256 level %d: blend_tiles %s save_to_memory %s" % (k, sha(bufs[k]), sha(img[0])))
    res = {k: [] for k in levels}
    for r in range(rounds):
        for k in levels:
            m.profile_reset()
            t0 = time.perf_counter(); m.blend_tiles(tiles, out=bufs[k], level=k); t1 = time.perf_counter()
            kb = kern("blend_level" if k else "blend_fused"); m.profile_reset()
            t2 = time.perf_counter(); img = m.save_to_memory(alloc=alloc, level=k); t3 = time.perf_counter()
            ks = kern("save_level" if k else "save_fused")
            res[k].append((kb, (t1 - t0) * 1e3, ks, (t3 - t2) * 1e3))
            print("round %d level %d: blend kernel %.3f ms, blend_tiles wall %.2f ms (%d tiles, %.1f MB); save kernel %.3f ms, save_to_memory wall %.2f ms (%d x %d)" %
                  (r, k, kb, (t1 - t0) * 1e3, len(tiles), bufs[k].nbytes / 1e6, ks, (t3 - t2) * 1e3, img[0].shape[1], img[0].shape[0]))
    for k in levels:
        a_ = np.array(res[k])
        print("level %d  min / max over %d rounds: blend kernel %.3f / %.3f ms, blend_tiles wall %.2f / %.2f ms, save kernel %.3f / %.3f ms, save_to_memory wall %.2f / %.2f ms" %
              ((k, rounds) + tuple(v for c in range(4) for v in (a_[:, c].min(), a_[:, c].max()))))
if a.level is not None:
    level_rounds([int(v) for v in a.level.split(",")], a.rounds)
    sys.exit(0)
def dump():
    for n, v in m.profile_read().items():
        if v["launches"]:
            print("    %-14s launches %5d  total %8.2f ms  alg %7.1f GB/s" % (n, v["launches"], v["ms"], v["alg_bytes"] / max(v["ms"], 1e-9) / 1e6))
    m.profile_reset()
t0 = time.perf_counter(); xy, out = m.blend_changed(cap=max(nt, 1)); t1 = time.perf_counter()
print("blend_changed: %d of %d tiles in %.1f ms = %.0f tiles/s (fresh pageable buffer, first touch included)" % (len(xy), nt, (t1 - t0) * 1e3, len(xy) / (t1 - t0)))
dump()
if hasattr(m, "blend_tiles"):
    tiles = list(xy)
    pinned = pf.host_array((len(tiles), 256, 256, 3))
    for name, buf in (("touched pageable", out), ("page-locked", pinned)):
        best = 1e9
        for _ in range(a.reps):
            t0 = time.perf_counter(); r = m.blend_tiles(tiles, out=buf); best = min(best, time.perf_counter() - t0)
        assert r is not None and (name == "touched pageable" or np.array_equal(pinned, out))
        if name == "page-locked": print("sha256 level 0: blend_tiles %s" % sha(pinned))
        print("blend_tiles  : %d tiles into a %s buffer: best of %d %.1f ms = %.0f tiles/s, %.1f GB/s of BGR8" %
              (len(tiles), name, a.reps, best * 1e3, len(tiles) / best, len(tiles) * 196608 / best / 1e9))
    dump()
t0 = time.perf_counter(); img = m.save_to_memory(); t1 = time.perf_counter()
print("save_to_memory: mosaic %dx%d (%d tiles) in %.1f ms (fresh pageable buffer)" % (img[0].shape[1], img[0].shape[0], nt, (t1 - t0) * 1e3))
print("sha256 level 0: save_to_memory %s" % sha(img[0]))
dump()
if hasattr(pf, "host_array"):
    keep = {}
    def alloc_pinned(shape):
        if "p" not in keep: keep["p"] = pf.host_array(shape)
        return keep["p"]
    def alloc_touched(shape):
        return img[0]
    for name, al in (("touched pageable", alloc_touched), ("page-locked", alloc_pinned)):
        best = 1e9
        for _ in range(a.reps + 1):
            t0 = time.perf_counter(); m.save_to_memory(alloc=al); best = min(best, time.perf_counter() - t0)
        print("save_to_memory: into a %s buffer: best %.1f ms = %.1f GB/s of BGR8" % (name, best * 1e3, img[0].nbytes / best / 1e9))
    dump()
if a.no_files: sys.exit(0)
import tempfile
with tempfile.TemporaryDirectory() as d:
    for ext in ("png", "ppm"):
        p = os.path.join(d, "mosaic." + ext)
        t0 = time.perf_counter(); ok = m.save(p); t1 = time.perf_counter()
        print("save(%s): %s in %.2f s, file %.0f MB (collapse + D2H + encode on the host: PNG deflate level 1 in 256-row bands on up to 8 threads)" %
              (ext, "ok" if ok else "FAILED", t1 - t0, os.path.getsize(p) / 1e6))
