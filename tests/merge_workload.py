"""The workload of the map-merge tests (test_merge_model.py, test_gpu_merge.py): three short sorties over one site at 640 x 480,
19 tiles, and the oracle maps fed them in a given order -- made once per process and left unchanged.
  A  4 poses of jitter_poses(seed 1)
  B  4 poses of jitter_poses(seed 2) shifted by (20, -30), with B[1] = A[2]: one pose shared, so whole tiles tie in weight
  C  4 poses of jitter_poses(seed 3) shifted by (45, 25): fed after a merge ("life goes on")
  F  B shifted by (700, -600): leaves the grid prepared from A alone, and shares no tile with A
Frames: noise_frame(480, 640, k), k = 0..3 for A, 10..13 for B and F, 20..23 for C."""
import functools

from helpers import jitter_poses, workloads

CAM = [640, 480, 500, 500, 320, 240]


def _shift(poses, dx, dy):
    return [[p[0] + dx, p[1] + dy] + list(p[2:]) for p in poses]


@functools.lru_cache(maxsize=None)
def sorties():
    """{name: (poses, frames)}"""
    wl = workloads()
    A = [list(p) for p in jitter_poses(4, 1)]
    B = _shift(jitter_poses(4, 2), 20.0, -30.0)
    B[1] = list(A[2])
    C = _shift(jitter_poses(4, 3), 45.0, 25.0)
    F = _shift(B, 700.0, -600.0)
    fr = lambda k0: [wl.noise_frame(480, 640, k0 + k) for k in range(4)]
    fb = fr(10)
    return {"A": (A, fr(0)), "B": (B, fb), "C": (C, fr(20)), "F": (F, fb)}


def poses_of(names):
    return [p for n in names for p in sorties()[n][0]]


def feed(m, names):
    """feeds the sorties `names` (a string such as "AB") into map m, oracle or HIP; every keyframe must be accepted"""
    for n in names:
        poses, frames = sorties()[n]
        for img, p in zip(frames, poses):
            assert m.feed(img, p), (n, p)


@functools.lru_cache(maxsize=None)
def oracle_fed(order, prep, force_float=0, bands=5, single_band=0):
    """the OracleMap prepared with the poses of sorties `prep` and fed the sorties `order`; shared, never modified by a test"""
    from oracle import orc
    o = orc.OracleMap(force_float=force_float, band_num=bands, single_band=single_band)
    assert o.prepare(workloads().IDENTITY_PLANE, CAM, poses_of(prep))
    feed(o, order)
    return o
