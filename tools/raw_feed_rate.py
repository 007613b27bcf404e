#!/usr/bin/env python3
"""What feeding raw frames costs and saves (csrc/raw_convert.hip, pf_feed_raw) at 4000 x 3000 on one GPU.

  python tools/raw_feed_rate.py [--reps 30] [--frames 200] [--rounds 5] [--no-map]

Kernels: NV12, I420, grey and Bayer RGGB frames resident in HBM converted by pf_raw_to_bgr_device, timed by HIP events around each call
on one stream.  Beside the time: the bytes the conversion has to move (the planes read once, 3 B written per pixel) over it, next to
8 TB/s and the copy ceiling.

Map: keyframes/s of one host thread feeding pageable host frames into a map -- pf_feed of the BGR8 pictures (the baseline: 3 B a pixel
over the link) and pf_feed_raw of NV12 (1.5 B), Bayer and grey (1 B) frames of the same pictures -- --rounds times each, interleaved in one
process; every round's rate is printed with the medians, and the ratio to the BGR8 feed of the same round.

Prints one JSON line per measurement.  Needs the GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import bench  # noqa: E402  (package loader)

CAM = [4000, 3000, 3000, 3000, 2000, 1500]
ROWS, COLS = 3000, 4000
HBM_PEAK, COPY_CEILING = 8.0e12, (4.7e12, 4.9e12)          # bytes/s: the spec sheet; README's measured copy ceiling


def plane_shapes(pf, fmt):
    if fmt == pf.RAW_I420:
        return [(ROWS, COLS), (ROWS // 2, COLS // 2), (ROWS // 2, COLS // 2)]
    if fmt in (pf.RAW_NV12, pf.RAW_NV21):
        return [(ROWS, COLS), (ROWS // 2, COLS)]
    return [(ROWS, COLS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-map", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("raw_feed_rate: no GPU (a rate is measured on the GPU or not at all)")
    pf = bench.load_package()
    wl = importlib.import_module("pi_slam_fusion_amd.workloads")
    err = lambda: pf.lib().pf_last_error().decode()
    formats = (("nv12", pf.RAW_NV12), ("i420", pf.RAW_I420), ("grey", pf.RAW_GREY), ("bayer_rggb", pf.RAW_BAYER_RGGB))

    # ---- the kernels
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    dst = torch.empty((ROWS, COLS, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for name, fmt in formats:
        shapes = plane_shapes(pf, fmt)
        sets = [[torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=gen) for s in shapes] for _ in range(4)]
        call = lambda k: pf.raw_to_bgr_device([t.data_ptr() for t in sets[k % 4]], [s[1] for s in shapes], fmt, ROWS, COLS, dst.data_ptr(), stream=st)
        for k in range(4):
            assert call(k), err()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for k, (e0, e1) in enumerate(ev):
            e0.record()
            assert call(k), err()
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        moved = sum(r * c for r, c in shapes) + 3 * ROWS * COLS
        med = statistics.median(ms)
        print(json.dumps({"what": "kernel_" + name, "event_ms_median": med, "event_ms_spread": [min(ms), max(ms)], "reps": a.reps,
                          "bytes_moved": moved, "bytes_per_s": moved / (med * 1e-3), "share_of_8TBps": moved / (med * 1e-3) / HBM_PEAK,
                          "share_of_copy_ceiling": [moved / (med * 1e-3) / c for c in COPY_CEILING[::-1]]}))
        sys.stdout.flush()
        del sets
    if a.no_map:
        return

    # ---- a map fed from the host: BGR8 against raw
    n = a.frames
    poses = wl.serpentine(CAM, 100.0, n + 30)
    rng = __import__("numpy").random.default_rng(3)
    raws = {name: [[rng.integers(0, 256, s, dtype="uint8") for s in plane_shapes(pf, fmt)] for _ in range(4)] for name, fmt in formats if name != "i420"}
    # the BGR8 baseline feeds the same pictures the NV12 frames convert to
    bgr = [pf.raw_to_bgr(tuple(p), pf.RAW_NV12, ROWS, COLS) for p in raws["nv12"]]
    fmt_of = dict(formats)

    def run(way):
        m = pf.Map2D.create(pf.TypeMultiBandCPU, False)
        assert m.prepare(wl.IDENTITY_PLANE, CAM, poses[:20])
        if way == "bgr8":
            feed = lambda k: m.feed(bgr[k % 4], poses[k])
        else:
            frames = [tuple(p) for p in raws[way]]
            feed = lambda k: m.feed_raw(frames[k % 4], fmt_of[way], poses[k])
        for k in range(10):
            assert feed(k), err()
        assert m.sync()
        t0 = time.perf_counter()
        for k in range(10, 10 + n):
            assert feed(k), err()
        assert m.sync()
        dt = time.perf_counter() - t0
        m.close()
        return n / dt

    ways = ("bgr8", "nv12", "bayer_rggb", "grey")
    rates = {w: [] for w in ways}
    for _ in range(a.rounds):
        for w in ways:
            rates[w].append(run(w))
    for w in ways:
        rec = {"what": "host_feed_" + w, "frames": n, "rounds": a.rounds, "bytes_over_the_link_per_frame": {"bgr8": 3.0, "nv12": 1.5}.get(w, 1.0) * ROWS * COLS,
               "kf_per_s": [round(v, 1) for v in rates[w]], "median": round(statistics.median(rates[w]), 1),
               "ratio_to_bgr8_per_round": [round(v / b, 3) for v, b in zip(rates[w], rates["bgr8"])]}
        print(json.dumps(rec)); sys.stdout.flush()


if __name__ == "__main__":
    main()
