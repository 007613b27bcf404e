"""What tests/test_gpu_alloc_failure.py shares with its child processes: the workload, the oracle's maps on their way to another process,
and the cases themselves (run_cases: a map of the experiments library -- PF_LIB -- whose allocations fail where a case says so, through
pf_debug_tile_store / pf_debug_fail_workspace; what it observes goes back as plain facts, the parent asserts)."""
import numpy as np

CAM = [640, 480, 500, 500, 320, 240]
N_KEYFRAMES, K = 9, 4                  # keyframe K is the one whose allocation fails: 0 .. 3 are in when it arrives, 5 .. 8 follow
SEED, STEP = 13, (28.0, 18.0)          # ~0.55 x 0.35 tiles a keyframe on canvases of 12 to 16 tiles: consecutive canvases share more than half
SLAB = 4                               # tiles a slab (pf_debug_tile_store): a canvas of 12 tiles crosses several slab allocations
WITHOUT = [k for k in range(N_KEYFRAMES) if k != K]
TYPES = ("i16", "f32", "single")


def poses():
    from helpers import jitter_poses
    return jitter_poses(N_KEYFRAMES, seed=SEED, step=STEP)


def frame(k):
    from helpers import workloads
    return workloads().noise_frame(480, 640, 700 + k)


def store_oracle(path, o, single):
    """an OracleMap's tiles as the .npz that warp_ties.StoredMap reads"""
    out = {"num_levels": np.int64(o.num_levels), "tiles": np.array(o.tiles(), np.int64).reshape(-1, 2)}
    for (ix, iy) in o.tiles():
        if single:
            out["b_%d_%d" % (ix, iy)] = o.tile_bgra(ix, iy)
        else:
            for lv in range(o.num_levels):
                out["l_%d_%d_%d" % (ix, iy, lv)], out["w_%d_%d_%d" % (ix, iy, lv)] = o.tile_level(ix, iy, lv)
    np.savez(path, **out)


def compare(g, path, single):
    """mismatch strings of map g against a stored oracle map: the tile set, every level's Laplacian and weight of every tile (single band:
    every tile's BGRA), and Ischanged -- nothing here has cleared it, so every tile with a pyramid carries it (.cpp:553)"""
    from helpers import compare_maps
    from warp_ties import StoredMap
    m = StoredMap(path)
    if single:
        bad = ["tile sets differ: gpu %d oracle %d" % (len(g.tiles()), len(m.tiles()))] if g.tiles() != m.tiles() else []
        for t in (m.tiles() if not bad else []):
            d = g.tile_bgra(*t) != m.tile_bgra(*t)
            if d.any():
                bad.append("tile_bgra %s: %d px differ (%d in alpha)" % (t, int(d.any(axis=2).sum()), int(d[:, :, 3].sum())))
    else:
        bad = compare_maps(g, m)
    return bad


def changed_differs(g, path):
    """the Ischanged set against the stored map's tiles (reading it clears it: last thing a case does)"""
    from warp_ties import StoredMap
    got, want = sorted(g.blend_changed()[0]), sorted(StoredMap(path).tiles())
    return [] if got == want else ["changed flags: %d tiles, %d expected" % (len(got), len(want))]


def create(pf, c):
    kw = dict(lookahead=c.get("lookahead", 0))
    if c.get("thread"):
        kw["max_queue"] = 64               # nothing drops
    if c["type"] == "single":
        return pf.Map2D.create(pf.TypeCPU, bool(c.get("thread")), **kw)
    return pf.Map2D.create(pf.TypeMultiBandCPU, bool(c.get("thread")), force_float=int(c["type"] == "f32"), band_number=5, **kw)


def last_error(pf):
    return pf.lib().pf_last_error().decode()


def arm_store(g, geo, where):
    """the next new tile is number 0 of keyframe K's new tiles; its tile number j (first: 0, middle, last: n_new - 1) is the one whose slab is
    refused -- j = 0: slabs of SLAB tiles, slab 0 fails; j > 0: a slab of j tiles, then slab 1 fails.  One failure: the window has passed after it"""
    j = {"first": 0, "middle": geo["n_new"] // 2, "last": geo["n_new"] - 1}[where]
    if j == 0:
        g.debug_tile_store(SLAB, 0, 1)
    else:
        g.debug_tile_store(j, 1, 1)
    return j


def run_store_case(pf, c, spec):
    """a, b, c: thread = 0; keyframe K meets a refused tile slab inside its own feed"""
    P, geo, ref = poses(), spec["geometry"], spec["oracles"][c["type"]]
    single = c["type"] == "single"
    g = create(pf, c)
    g.debug_tile_store(SLAB)
    assert g.prepare(pf.workloads.IDENTITY_PLANE, CAM, P)
    r = {"feeds": {}}
    for k in range(K):
        r["feeds"][k] = g.feed(frame(k), P[k])
    r["tiles_before"] = g.render_stats()["tiles_held"] if c.get("lookahead", 0) == 0 else None       # (a reader: only where nothing waits anyway)
    r["failing_tile"] = arm_store(g, geo, c["where"])
    r["feed_k"] = g.feed(frame(K), P[K]); r["error_k"] = last_error(pf)
    g.debug_tile_store(SLAB)
    if c.get("refeed") == "at once":
        r["feed_k_again"] = g.feed(frame(K), P[K])
    for k in range(K + 1, N_KEYFRAMES):
        r["feeds"][k] = g.feed(frame(k), P[k])
    r["failed"] = g.failed()
    r["sync"] = [g.sync(), last_error(pf), g.sync()]
    r["culled"] = g.culled_tiles() + g.culled_cells()
    if c.get("refeed") == "at once":
        r["map"] = compare(g, ref["all"], single)
        r["log"] = g.render_log()
        r["changed"] = changed_differs(g, ref["all"])
    else:
        r["map_without_k"] = compare(g, ref["without"], single)
        r["log_without_k"] = g.render_log()
        r["feed_k_again"] = g.feed(frame(K), P[K])
        r["sync_again"] = g.sync()
        r["map"] = compare(g, ref["without_then_k"], single)
        r["log"] = g.render_log()
        r["changed"] = changed_differs(g, ref["without_then_k"])
    r["failed_end"] = g.failed()
    r["stats"] = g.stats()
    g.close()
    return r


def run_thread_case(pf, c, spec):
    """d: thread = 1.  The hook is armed before the first feed: the render thread takes the keyframes when it gets to them.  Tiles are created
    in feed order, SLAB to a slab, so slab number ceil(tiles before K / SLAB) is opened by a new tile of K (the parent has checked that)"""
    P, geo, ref = poses(), spec["geometry"], spec["oracles"][c["type"]]
    g = create(pf, c)
    g.debug_tile_store(SLAB, geo["slab_in_k"], 1)
    assert g.prepare(pf.workloads.IDENTITY_PLANE, CAM, P)
    r = {"feeds": {k: g.feed(frame(k), P[k]) for k in range(N_KEYFRAMES)}}
    r["sync"] = [g.sync(), last_error(pf), g.sync()]
    r["failed"] = g.failed()
    r["log"] = g.render_log()
    r["map"] = compare(g, ref["without"], False)
    r["changed"] = changed_differs(g, ref["without"])
    r["stats"] = g.stats()
    g.close()
    return r


def run_workspace_case(pf, c, spec):
    """e: the frame workspace cannot grow.  `when` = admission: armed right before keyframe K is fed (thread = 1: after a pf_sync, so that the
    render thread has taken 0 .. 3) -- the first call that sizes the workspace is K's; `when` = reader: armed while keyframes 2 and 3 wait for
    their lookahead and a reader (pf_stats) renders them -- the failure meets keyframe 2 AFTER its admission"""
    P, ref = poses(), spec["oracles"][c["type"]]
    g = create(pf, c)
    g.debug_tile_store(SLAB)
    assert g.prepare(pf.workloads.IDENTITY_PLANE, CAM, P)
    r = {"feeds": {}}
    for k in range(K):
        r["feeds"][k] = g.feed(frame(k), P[k])
    if c.get("thread"):
        r["sync_before"] = g.sync()
    g.debug_fail_workspace(1)
    if c["when"] == "reader":
        r["reader"] = g.stats(); r["failed_after_reader"] = g.failed()
    for k in range(K, N_KEYFRAMES):
        r["feeds"][k] = g.feed(frame(k), P[k])
        if k == K:
            r["error_k"] = last_error(pf)
    r["sync"] = [g.sync(), last_error(pf), g.sync()]
    r["failed"] = g.failed()
    r["log"] = g.render_log()
    if c["when"] == "admission":
        r["map"] = compare(g, ref["without"], False)
        r["changed"] = changed_differs(g, ref["without"])
    r["stats"] = g.stats()
    g.close()
    return r


def hip_state_calls(pf, torch, dev_small, dev_img, dev_mask, px2ll):
    jpg = pf.jpeg_encode_device(dev_small.data_ptr(), dev_small.shape[0], dev_small.shape[1], 90)
    tiles = pf.webtiles_device(dev_img.data_ptr(), dev_img.shape[0], dev_img.shape[1], dev_mask.data_ptr(), px2ll, 20, 20, 95, 0, False)
    return jpg.hex(), sorted((t["z"], t["x"], t["y"], t["cover"], t["jpeg"].hex()) for t in tiles)


def run_hip_state_case(pf, c, spec):
    """f: right after a feed that a refused hipMalloc failed, the same host thread saves the map as JPEG, encodes a small image and makes map
    tiles of a 40 x 56 one -- all three check hipGetLastError() behind their launches -- and gets the bytes of the same calls made without
    any failure: before it (the two stateless calls) and on a map fed the same keyframes 0 .. 3 (the file)"""
    import os
    import torch
    import webtiles_model as wm
    P = poses()
    rs = np.random.RandomState(5)
    small = torch.from_numpy(rs.randint(0, 256, (24, 40, 3)).astype(np.uint8)).cuda()
    img = torch.from_numpy(rs.randint(0, 256, (40, 56, 3)).astype(np.uint8)).cuda()
    mask = torch.from_numpy(np.full((40, 56), 255, np.uint8)).cuda()
    torch.cuda.synchronize()
    px2ll = wm.make_px2ll(13.405, 40.0, 40, 56, 20, 1.0, 30.0, False)
    r = {"feeds": {}}
    want = hip_state_calls(pf, torch, small, img, mask, px2ll)
    files = {}
    for which in ("clean", "failed"):
        g = create(pf, c)
        g.debug_tile_store(SLAB)
        assert g.prepare(pf.workloads.IDENTITY_PLANE, CAM, P)
        for k in range(K):
            assert g.feed(frame(k), P[k])
        name = os.path.join(spec["tmp"], "m_%s.jpg" % which)
        if which == "failed":
            arm_store(g, spec["geometry"], "first")
            r["feed_k"] = g.feed(frame(K), P[K]); r["error_k"] = last_error(pf)
            r["save"] = g.save(name); r["save_error"] = "" if r["save"] else last_error(pf)
            try:
                got = hip_state_calls(pf, torch, small, img, mask, px2ll)
                r["stateless_calls_equal"] = got == want
            except (ValueError, RuntimeError) as e:
                r["stateless_calls_equal"] = False; r["stateless_error"] = str(e)
            r["failed"] = g.failed()
        else:
            assert g.save(name)
        files[which] = open(name, "rb").read() if os.path.exists(name) else b""
        g.close()
    r["file_bytes"] = len(files["clean"])
    r["file_equal"] = files["clean"] == files["failed"]
    return r


def run_parity_case(pf, c, spec):
    """g: a run that never calls the hooks -- the digest of the map, the culled counts and the forms that ran, in whichever library this
    process loaded"""
    import ctypes as C
    from helpers import map_digest
    P = poses()
    g = pf.Map2D.create(pf.TypeMultiBandCPU, False, force_float=0)          # default options: lookahead 48
    assert g.prepare(pf.workloads.IDENTITY_PLANE, CAM, P)
    for k in range(N_KEYFRAMES):
        assert g.feed(frame(k), P[k])
    assert g.sync()
    cnt = (C.c_longlong * 8)(); pf.lib().pf_debug_form_counts(cnt)
    r = {"digest": map_digest(g), "culled": [g.culled_tiles(), g.culled_cells()], "forms": list(cnt), "stats": g.stats(), "failed": g.failed(),
         "has_hook": hasattr(pf.lib(), "pf_debug_tile_store"), "map": compare(g, spec["oracles"]["i16"]["all"], False)}
    g.close()
    return r


RUNNERS = {"store": run_store_case, "thread": run_thread_case, "workspace": run_workspace_case, "hip_state": run_hip_state_case, "parity": run_parity_case}


def run_cases(spec):
    """the child process: {case id: what the case observed}"""
    import importlib
    from conftest import load_package
    pf = load_package()
    pf.workloads = importlib.import_module("pi_slam_fusion_amd.workloads")
    out = {}
    for c in spec["cases"]:
        out[c["id"]] = RUNNERS[c["kind"]](pf, c, spec)
    return out
