#!/usr/bin/env python3
"""Rate of keyframe undistortion (csrc/undistort.hip) and what an input camera costs a map.

  python tools/undistort_rate.py [--reps 30] [--frames 300] [--rounds 5] [--no-map]

Kernel: a 4000 x 3000 OpenCV camera remapped into the bench camera (4000 x 3000 pinhole), frames resident in HBM, timed by HIP events
around each pf_undistort_device call on one stream.  Beside the time: the bytes moved (8 B of table and 3 B out per output pixel, 3 B
per source pixel) over it, next to 8 TB/s and the copy ceiling.

Map: the host_feed- and jpeg_feed-style rates (keyframes/s through pf_feed from pageable host frames, and through pf_feed_jpeg) of one
map with and without an input camera, --rounds times each, interleaved in one process; the spread of the rounds is printed with the
medians.  Also the device-resident rate (pf_feed_device), which has no transfer to hide the kernel behind.

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
IN_CAM = [4000, 3000, 3100, 3100, 1990.5, 1510.2, -0.12, 0.03, 0.0008, -0.0012, 0.0]
HBM_PEAK, COPY_CEILING = 8.0e12, (4.7e12, 4.9e12)          # bytes/s: the spec sheet; README's measured copy ceiling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-map", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("undistort_rate: no GPU (a rate is measured on the GPU or not at all)")
    pf = bench.load_package()
    wl = importlib.import_module("pi_slam_fusion_amd.workloads")
    err = lambda: pf.lib().pf_last_error().decode()

    # ---- the kernel
    t0 = time.perf_counter()
    unc = pf.undistort_table(IN_CAM, CAM)[2]
    t_table = time.perf_counter() - t0
    gen = torch.Generator(device="cuda"); gen.manual_seed(99)
    srcs = [torch.randint(0, 256, (3000, 4000, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(4)]
    dst = torch.empty((3000, 4000, 3), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for k in range(3):                                      # the first call builds and uploads the table
        assert pf.undistort_device(srcs[k % 4].data_ptr(), IN_CAM, CAM, dst.data_ptr(), stream=st), err()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for k, (e0, e1) in enumerate(ev):
        e0.record()
        assert pf.undistort_device(srcs[k % 4].data_ptr(), IN_CAM, CAM, dst.data_ptr(), stream=st), err()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    n_out, n_in = CAM[0] * CAM[1], IN_CAM[0] * IN_CAM[1]
    moved = 8 * n_out + 3 * n_out + 3 * n_in
    med = statistics.median(ms)
    print(json.dumps({"what": "k_undistort", "camera_in": IN_CAM, "camera_out": CAM, "uncovered": unc, "host_table_s": round(t_table, 3),
                      "event_ms_median": med, "event_ms_spread": [min(ms), max(ms)], "reps": a.reps, "bytes_moved": moved,
                      "bytes_per_s": moved / (med * 1e-3), "share_of_8TBps": moved / (med * 1e-3) / HBM_PEAK,
                      "share_of_copy_ceiling": [moved / (med * 1e-3) / c for c in COPY_CEILING[::-1]]}))
    sys.stdout.flush()
    if a.no_map:
        return

    # ---- a map with and without the input camera
    n = a.frames
    poses = wl.serpentine(CAM, 100.0, n + 30)
    host = [s.cpu().numpy() for s in srcs]
    smooth = [wl.smooth_frame(3000, 4000, k) for k in range(2)]
    jpgs = [pf.jpeg_encode(f, 90) for f in smooth]

    def run(way, with_camera):
        m = pf.Map2D.create(pf.TypeMultiBandCPU, False)
        if with_camera:
            assert m.set_input_camera(IN_CAM), err()
        assert m.prepare(wl.IDENTITY_PLANE, CAM, poses[:20])

        def feed(k):
            if way == "host_feed":
                return m.feed(host[k % 4], poses[k])
            if way == "jpeg_feed":
                return m.feed_jpeg(jpgs[k % 2], poses[k])
            return m.feed_device(srcs[k % 4].data_ptr(), 3000, 4000, poses[k])
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

    for way in ("device_feed", "host_feed", "jpeg_feed"):
        rates = {False: [], True: []}
        for _ in range(a.rounds):
            for with_camera in (False, True):
                rates[with_camera].append(run(way, with_camera))
        rec = {"what": way, "frames": n, "rounds": a.rounds}
        for with_camera, key in ((False, "plain"), (True, "input_camera")):
            r = rates[with_camera]
            rec[key + "_kf_per_s"] = [round(v, 1) for v in r]
            rec[key + "_median"] = round(statistics.median(r), 1)
        rec["ms_per_frame_added"] = round(1e3 / rec["input_camera_median"] - 1e3 / rec["plain_median"], 3)
        print(json.dumps(rec)); sys.stdout.flush()


if __name__ == "__main__":
    main()
