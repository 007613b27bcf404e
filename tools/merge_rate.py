#!/usr/bin/env python3
"""Rate of the map merge (csrc/merge.hip) on the bench mosaic, and what a resumed map culls.

  python tools/merge_rate.py [--frames 220] [--reps 5] [--resume-frames 100] [--resume-scale 0.25]

Merge: bench.py's cfg-2 sortie (4000 x 3000 keyframes, 20 a flight line) is flown as two maps -- the even flight lines into one, the
odd lines into the other, both prepared with every pose -- and the second is merged into the first (pf_merge).  Timed with the HIP
events the library records around the merge's launches (pf_debug_merge_stats), --reps times per pyramid type, the two types
interleaved, on freshly built maps every time (a merge changes its destination).  One more merge per type counts the pixel-levels the
source won, which gives the bytes actually stored.  Bytes moved = slot bytes read (src) + weights read (dst, where dst held the tile) +
bytes stored; beside it the bytes the kernel has to touch (it does not load src's Laplacians where src loses: bytes_of()).  Beside it: the wall time of the only route without the merge kernel -- feeding src's keyframes into dst.

Resume: a map is flown for --resume-frames keyframes at Map2D.Scale --resume-scale (the state file of the full-scale mosaic is several
GB), saved, loaded into a new map, and both fly 40 more keyframes: culled cells of the restored map against the uninterrupted one's.

Prints one JSON line per measurement and a summary line.  Needs the GPU: there is no CPU path."""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = [4000, 3000, 3000, 3000, 2000, 1500]
HEIGHT = 100.0
HBM_PEAK, COPY_CEILING = 8.0e12, (4.7e12, 4.9e12)          # bytes/s: the spec sheet; README's measured copy ceiling (k_collapse_fused)


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


def level_bytes(bands, f32):
    """(bytes of a pixel-level: 3 Laplacian channels + the weight, weight bytes of a whole slot)"""
    px = sum((256 >> i) ** 2 for i in range(bands + 1))
    return 3 * (4 if f32 else 2) + 4, 4 * px


def bytes_of(st, px_bytes, w_bytes):
    """(bytes moved as the figure is defined: src's slot read + dst's weights read + bytes stored; bytes the kernel has to touch: it
    loads src's Laplacians only where src wins, so of a src slot it reads the weights and the Laplacians of the pixel-levels won --
    a lower bound, the loads come in groups of 4 or 8 pixels) of the merge whose statistics are st"""
    held = st["pairs"] - st["fresh"]
    copies = 2 * st["fresh"] * st["slot_bytes"]
    moved = held * (st["slot_bytes"] + w_bytes) + st["won"] * px_bytes + copies
    touched = held * 2 * w_bytes + st["won"] * (px_bytes - 4) + st["won"] * px_bytes + copies
    return moved, touched


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resume-frames", type=int, default=100)
    ap.add_argument("--resume-scale", type=float, default=0.25)
    ap.add_argument("--no-resume", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("merge_rate: no GPU (a rate is measured on the GPU or not at all)")
    pf = load_package()
    wl = importlib.import_module("pi_slam_fusion_amd.workloads")
    poses = wl.serpentine(CAM, HEIGHT, args.frames, max_rows=16)
    line = lambda k: k // 20
    even = [k for k in range(args.frames) if line(k) % 2 == 0]
    odd = [k for k in range(args.frames) if line(k) % 2 == 1]
    gen = torch.Generator(device="cuda"); gen.manual_seed(1234)
    frames = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(8)]
    torch.cuda.synchronize()
    ptrs = [f.data_ptr() for f in frames]

    def fly(m, ks):
        for k in ks:
            assert m.feed_device(ptrs[k % len(ptrs)], 3000, 4000, poses[k])

    def new_map(ff, scale=1.0, prep=None):
        m = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=ff, scale=scale)
        assert m.prepare(wl.IDENTITY_PLANE, CAM, poses if prep is None else prep)
        return m

    def built(ff, ks):
        m = new_map(ff); fly(m, ks); assert m.sync()
        return m

    results = {0: [], 1: []}
    feed_route = {0: [], 1: []}
    stored = {}
    for rep in range(args.reps + 1):                      # rep 0: warm-up (code objects, slabs) and the counting pass
        for ff in (1, 0):
            dst, src = built(ff, even), built(ff, odd)
            if rep == 0:
                dst.merge_stats(count_stores=True)
            t0 = time.perf_counter()
            assert dst.merge(src), pf.lib().pf_last_error()
            wall = time.perf_counter() - t0
            st = dst.merge_stats()
            if rep == 0:
                stored[ff] = st
            else:
                results[ff].append((st["ms"], wall * 1e3))
                # the route without the kernel: src's keyframes fed into a map that holds dst's
                alt = built(ff, even)
                t0 = time.perf_counter()
                fly(alt, odd); assert alt.sync()
                feed_route[ff].append((time.perf_counter() - t0) * 1e3)
                alt.close()
            dst.close(); src.close()
    summary = {}
    for ff in (1, 0):
        st = stored[ff]
        px_bytes, w_bytes = level_bytes(5, ff)
        moved, touched = bytes_of(st, px_bytes, w_bytes)
        ms = [r[0] for r in results[ff]]; wall = [r[1] for r in results[ff]]
        med = statistics.median(ms)
        rec = {"what": "merge", "pyramid": "fp32" if ff else "int16", "frames": args.frames, "pairs": st["pairs"], "fresh_pairs": st["fresh"],
               "pixel_levels_won": st["won"], "bytes_moved": moved, "event_ms": ms, "event_ms_median": med, "event_ms_spread": [min(ms), max(ms)],
               "wall_ms_median": statistics.median(wall), "bytes_per_s": moved / (med * 1e-3), "share_of_8TBps": moved / (med * 1e-3) / HBM_PEAK,
               "share_of_copy_ceiling": [moved / (med * 1e-3) / c for c in COPY_CEILING[::-1]],
               "bytes_touched": touched, "touched_per_s": touched / (med * 1e-3), "touched_share_of_8TBps": touched / (med * 1e-3) / HBM_PEAK,
               "touched_share_of_copy_ceiling": [touched / (med * 1e-3) / c for c in COPY_CEILING[::-1]],
               "feed_route_ms": feed_route[ff], "feed_route_ms_median": statistics.median(feed_route[ff])}
        print(json.dumps(rec)); sys.stdout.flush()
        summary[rec["pyramid"]] = {"TBps": round(rec["bytes_per_s"] / 1e12, 3), "touched_TBps": round(rec["touched_per_s"] / 1e12, 3), "ms": round(med, 3), "feed_route_ms": round(rec["feed_route_ms_median"], 1)}
    if not args.no_resume:
        n = min(args.resume_frames, args.frames - 40)
        more = list(range(n, n + 40))
        for ff in (1, 0):
            u = new_map(ff, args.resume_scale, poses[:n + 40]); fly(u, range(n)); assert u.sync()
            with tempfile.TemporaryDirectory() as d:
                p = os.path.join(d, "resume.pfstate")
                t0 = time.perf_counter(); assert u.save_state(p), pf.lib().pf_last_error(); t_save = time.perf_counter() - t0
                size = os.path.getsize(p)
                r = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=ff, scale=args.resume_scale)
                t0 = time.perf_counter(); assert r.load_state(p), pf.lib().pf_last_error(); t_load = time.perf_counter() - t0
            c0 = [(m.culled_cells(), m.culled_tiles()) for m in (u, r)]
            for m in (u, r):
                fly(m, more); assert m.sync()
            c1 = [(m.culled_cells(), m.culled_tiles()) for m in (u, r)]
            rec = {"what": "resume", "pyramid": "fp32" if ff else "int16", "scale": args.resume_scale, "frames_before": n, "frames_after": 40,
                   "tiles": len(u.tiles()), "file_bytes": size, "save_s": t_save, "load_s": t_load,
                   "culled_cells_uninterrupted": c1[0][0] - c0[0][0], "culled_cells_restored": c1[1][0] - c0[1][0],
                   "culled_tiles_uninterrupted": c1[0][1] - c0[0][1], "culled_tiles_restored": c1[1][1] - c0[1][1]}
            print(json.dumps(rec)); sys.stdout.flush()
            summary["resume_" + rec["pyramid"]] = [rec["culled_cells_uninterrupted"], rec["culled_cells_restored"]]
            u.close(); r.close()
    print(json.dumps({"summary": summary}))


if __name__ == "__main__":
    main()
