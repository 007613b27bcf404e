#!/usr/bin/env python3
"""save_png on the bench mosaic (dev tool; the mosaic is tools/tiff_rate.py's): wall time of save_png (plain and masked), save("m.png") (the
host writer: filter 0, zlib level 1 on up to eight threads), save_tiff_lossless and of writing a file of the PNG's size alone, on the same
map in the same process, interleaved, median (min .. max) of --reps after a warm-up round; the files' sizes; the file against the host
encoder once.
usage: tools/png_rate.py [--content noise|smooth] [--int16] [--frames N] [--reps R] [--dir D] [--kernels-only] [--no-check]
  --content        the keyframes: noise (the bench's own: every block comes out stored, the file is the mosaic's size) or smooth
                   (photo-like gradients with a little noise: the blocks come out dynamic)
  --kernels-only   three save_png and three masked ones and nothing else: the run to put under
                   rocprofv3 --kernel-trace --stats -d OUT -- python tools/png_rate.py --kernels-only
                   (k_png_plan, k_png_join, k_png_pack, k_png_frame; wall times under the profiler mean nothing)
Prints one JSON line per measurement.  Needs the GPU: there is no CPU path."""
import argparse, importlib, json, os, statistics, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import bench
ap = argparse.ArgumentParser(); ap.add_argument("--content", default="noise", choices=("noise", "smooth")); ap.add_argument("--int16", action="store_true")
ap.add_argument("--frames", type=int, default=120); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--dir", default=None)
ap.add_argument("--kernels-only", action="store_true"); ap.add_argument("--no-check", action="store_true")
a = ap.parse_args()
import numpy as np, torch
if not torch.cuda.is_available():
    sys.exit("png_rate: no GPU (a rate is measured on the GPU or not at all)")
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
    new, newm, old, ll, raw = (os.path.join(d, n) for n in ("new.png", "new_masked.png", "m.png", "lossless.tif", "m.bin"))
    if a.kernels_only:
        for _ in range(3):
            assert m.save_png(new) and m.save_png(newm, True)
        out(what="kernels_only", saves=6, file_bytes=os.path.getsize(new), masked_file_bytes=os.path.getsize(newm))
        sys.exit(0)
    keep = {}
    def timed(fn):
        t0 = time.perf_counter(); assert fn(); return time.perf_counter() - t0
    def write_alone():
        with open(raw, "wb") as f: f.write(keep["file"])
        return True
    ways = [("save_png", lambda: m.save_png(new)), ("save_png_masked", lambda: m.save_png(newm, True)), ("save_m_png_host", lambda: m.save(old)),
            ("save_tiff_lossless", lambda: m.save_tiff_lossless(ll)), ("write_alone", write_alone)]
    for name, fn in ways[:4]:                          # warm-up: code objects, buffers, page-locked memory
        timed(fn)
    keep["file"] = open(new, "rb").read()
    timed(write_alone)
    times = {name: [] for name, _ in ways}
    for _ in range(max(a.reps, 3)):
        for name, fn in ways:
            times[name].append(timed(fn))
    mem, mask, org = m.save_to_memory_mask()
    out(what="mosaic", rows=mem.shape[0], cols=mem.shape[1], map_tiles=len(m.tiles()), bgr8_bytes=mem.size, covered=float((mask != 0).mean()), content=a.content)
    for name, _ in ways:
        v = times[name]
        out(what=name, wall_ms_median=round(statistics.median(v) * 1e3, 1), wall_ms_spread=[round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)], reps=len(v))
    sizes = {"save_png": len(keep["file"]), "save_png_masked": os.path.getsize(newm), "save_m_png_host": os.path.getsize(old), "lossless_tif": os.path.getsize(ll)}
    out(what="file_bytes", ratio_to_host_png=round(sizes["save_png"] / sizes["save_m_png_host"], 4), **sizes)
    import png_model as pm
    chunks = pm.walk(keep["file"])
    out(what="chunks", idat=sum(1 for k, _ in chunks if k == b"IDAT"), idat_bytes=sum(len(dd) for k, dd in chunks if k == b"IDAT"))
    if not a.no_check:
        t0 = time.perf_counter()
        want = pf.png_encode(mem)
        host_s = time.perf_counter() - t0
        ok = want == keep["file"] and open(newm, "rb").read() == pf.png_encode(mem, mask)
        out(what="check", files_equal_host_encoder=ok, host_encoder_ms=round(host_s * 1e3, 1))
        assert ok
