#!/usr/bin/env python3
"""save_tiff_lossless on the bench mosaic (dev tool; the mosaic is tools/tiff_rate.py's): wall time of save_tiff_lossless (plain and masked),
save("m.tif") (JPEG tiles), save("m.png") and of writing a file of the lossless file's size alone, on the same map in the same process,
interleaved, median of --reps after a warm-up round; the files' sizes; the file against the host writer once.
usage: tools/tiff_lossless_rate.py [--content noise|smooth] [--int16] [--frames N] [--reps R] [--dir D] [--kernels-only] [--no-png] [--no-check]
  --content        the keyframes: noise (the bench's own: every block comes out stored, the file is the mosaic's size) or smooth
                   (photo-like gradients with a little noise: the blocks come out dynamic)
  --kernels-only   three save_tiff_lossless and nothing else: the run to put under
                   rocprofv3 --kernel-trace --stats -d OUT -- python tools/tiff_lossless_rate.py --kernels-only
                   (k_dfl_plan, k_dfl_join, k_dfl_pack, k_overview*; wall times under the profiler mean nothing)
Prints one JSON line per measurement.  Needs the GPU: there is no CPU path."""
import argparse, importlib, json, os, statistics, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import bench
ap = argparse.ArgumentParser(); ap.add_argument("--content", default="noise", choices=("noise", "smooth")); ap.add_argument("--int16", action="store_true")
ap.add_argument("--frames", type=int, default=120); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--dir", default=None)
ap.add_argument("--kernels-only", action="store_true"); ap.add_argument("--no-png", action="store_true"); ap.add_argument("--no-check", action="store_true")
a = ap.parse_args()
import numpy as np, torch
if not torch.cuda.is_available():
    sys.exit("tiff_lossless_rate: no GPU (a rate is measured on the GPU or not at all)")
pf = bench.load_package(); wl = importlib.import_module("pi_slam_fusion_amd.workloads")
cam = [4000, 3000, 3000, 3000, 2000, 1500]
poses = wl.serpentine(cam, 100.0, a.frames)
m = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=0 if a.int16 else 1)
assert m.prepare(wl.IDENTITY_PLANE, cam, poses[:20])
if a.content == "noise":
    fr = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
else:
    y, x = torch.meshgrid(torch.arange(3000, device="cuda"), torch.arange(4000, device="cuda"), indexing="ij")
    fr = []
    for k in range(4):
        base = torch.stack([(x // (5 + k) + y // 7) % 256, (x // 11 + y // (3 + k)) % 256, ((x + y) // 13 + 40 * k) % 256], -1)
        fr.append(((base + torch.randint(0, 3, (3000, 4000, 3), device="cuda")) % 256).to(torch.uint8).contiguous())
torch.cuda.synchronize()
for k in range(a.frames):
    m.feed_device(fr[k % 4].data_ptr(), 3000, 4000, poses[k])
m.sync()
out = lambda **kw: (print(json.dumps(kw)), sys.stdout.flush())
with tempfile.TemporaryDirectory(dir=a.dir) as d:
    ll, lm, tif, png, raw = (os.path.join(d, n) for n in ("lossless.tif", "lossless_masked.tif", "m.tif", "m.png", "m.bin"))
    if a.kernels_only:
        for _ in range(3):
            assert m.save_tiff_lossless(ll)
        out(what="kernels_only", saves=3, file_bytes=os.path.getsize(ll))
        sys.exit(0)
    keep = {}
    def timed(fn):
        t0 = time.perf_counter(); assert fn(); return time.perf_counter() - t0
    def write_alone():
        with open(raw, "wb") as f: f.write(keep["file"])
        return True
    ways = [("save_tiff_lossless", lambda: m.save_tiff_lossless(ll)), ("save_tiff_lossless_masked", lambda: m.save_tiff_lossless(lm, True)),
            ("save_tif_jpeg_tiles", lambda: m.save(tif)), ("write_alone", write_alone)]
    if not a.no_png:
        ways.append(("save_png", lambda: m.save(png)))
    for name, fn in ways[:3] + ways[4:]:                          # warm-up: code objects, buffers, page-locked memory
        timed(fn)
    keep["file"] = open(ll, "rb").read()
    timed(write_alone)
    times = {name: [] for name, _ in ways}
    for _ in range(max(a.reps, 3)):
        for name, fn in ways:
            times[name].append(timed(fn))
    import tiff_model as tm
    big, ifds = tm.parse(keep["file"])
    rows, cols = ifds[0]["tags"][257][1][0], ifds[0]["tags"][256][1][0]
    out(what="mosaic", rows=rows, cols=cols, map_tiles=len(m.tiles()), bgr8_bytes=rows * cols * 3, images=len(ifds), content=a.content, bigtiff=big)
    for name, _ in ways:
        v = times[name]
        out(what=name, wall_ms_median=round(statistics.median(v) * 1e3, 1), wall_ms_spread=[round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)], reps=len(v))
    sizes = {"lossless_tif": len(keep["file"]), "lossless_masked_tif": os.path.getsize(lm), "jpeg_tif": os.path.getsize(tif)}
    if not a.no_png:
        sizes["png"] = os.path.getsize(png)
    out(what="file_bytes", **sizes)
    streams = [s for i in ifds for s in tm.tile_streams(keep["file"], i)]
    out(what="tiles", tiles=len(streams), distinct_streams=len(set(streams)), stream_bytes=sum(n for _, n in set(streams)),
        stored_size_tiles=sum(1 for _, n in set(streams) if n == 196608 + 86))
    if not a.no_check:
        mem, org = m.save_to_memory()
        dims, geo = m.grid()
        xf = [geo[5], 0, 0, geo[0] + (org[0] - dims[2]) * geo[4], 0, geo[5], 0, geo[1] + (org[1] - dims[3]) * geo[4], 0, 0, 1, 0, 0, 0, 0, 1]
        t0 = time.perf_counter()
        assert pf.tiff_write_lossless(raw, mem, None, 0, xf)
        host_s = time.perf_counter() - t0
        ok = open(raw, "rb").read() == keep["file"]
        out(what="check", file_equals_host_writer=ok, host_writer_ms=round(host_s * 1e3, 1))
        assert ok
