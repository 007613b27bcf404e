"""The feed-side select -- level3_block stage D and select_store (csrc/kernels.hip), k_lap_select (fused = 0), the strip form
(strips.inc), k_single / k_single2 (csrc/single_band.hip) -- on slot images that no keyframe leaves behind (feed_slots.py), product
library.  A map fed the keyframe alone gives the keyframe's own pyramid on every tile of its canvas; stored weights built around it
(one ulp either side pixel by pixel, the 16 win patterns of the 2 x 2 quad, NaN, +-inf, -0.0, denormals, FLT_MAX, the kernels' own
sentinels NaN and -1) go into a second map through tile_import with padding 0x3C, beside a tile that stays fresh and one off the
canvas; the keyframe is fed, and every tile is exported whole and compared with the byte-level rule (tests/test_feed_slots.py ties
that rule to the model), padding included.  Pinned here and nowhere else: `>=` on a per-pixel mix of ties and single ulps at every
level and band count, stored NaN / -1 / denormals under the select, every win pattern of the quad, the levels of 2 x 2 and 1 x 1
pixels, every byte the keyframe did not win, fresh and stored tiles in one launch, the cull bounds tile_import has to forget, and
the kernel forms of the experiments library over injected state.  Every comparison is on bytes and exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import feed_slots as fs
import merge_slots as ms
import pyramid_inject as pi
from helpers import workloads

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BG = pi.BG
WAYS = ("fused0", "lookahead0", "default", "thread", "device")


def by_row(tiles):
    return sorted(tiles, key=lambda t: t[::-1])


def to_device(a):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()                                             # the map works on a stream of its own: the upload comes first
    return dev


def new_map(pf, bands, ff, way="default", **opt):
    from test_gpu_model import CAM
    if way == "fused0":
        opt["fused"] = 0
    if way == "lookahead0":
        opt["lookahead"] = 0
    g = pf.Map2D.create(pf.TypeMultiBandCPU, way == "thread", force_float=ff, band_number=bands, bg_color=BG, **opt)
    assert g.prepare(workloads().IDENTITY_PLANE, CAM, fs.rig(bands)[0])
    return g


def feed(g, way, frame, pose):
    if way == "device":
        dev = to_device(frame)
        assert g.feed_device(dev.data_ptr(), frame.shape[0], frame.shape[1], pose) and g.sync()
        del dev
    else:
        assert g.feed(frame, pose) and g.sync()


def levels_of(g, t):
    lw = [g.tile_level(t[0], t[1], i) for i in range(g.num_levels)]
    return [l for l, _ in lw], [w for _, w in lw]


@functools.lru_cache(maxsize=None)
def keyframe_alone(pf, bands, ff, k=0):
    """{t: (lap, w)} of a map fed keyframe k of the rig alone: on fresh tiles every pixel wins, so this is the keyframe's own pyramid"""
    _, poses, frames = fs.rig(bands)
    g = new_map(pf, bands, ff)
    feed(g, "default", frames[k], poses[k])
    out = {t: levels_of(g, t) for t in g.tiles()}
    g.close()
    assert len(out) >= 4
    return out


def import_tiles(g, stored):
    packed = {}
    for t, (lap, w) in stored.items():
        packed[t] = pi.pack(lap, w, pad=fs.PAD)
        dev = to_device(packed[t])
        assert g.tile_import(t[0], t[1], dev.data_ptr()), t
        del dev
    return packed


def export_all(g):
    """{t: the tile's slot image, exported whole}; the guard bytes behind every image must come back untouched"""
    import torch
    tiles, total = g.tiles(), g.tile_bytes()
    buf = torch.full((len(tiles), total + ms.GUARD), ms.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k, t in enumerate(tiles):
        assert g.tile_export(t[0], t[1], buf[k].data_ptr()), t
    got = buf.cpu().numpy()
    assert (got[:, total:] == ms.GUARD_BYTE).all()
    return {t: got[k, :total] for k, t in enumerate(tiles)}


def assert_image(got, want, bands, ff, label, padded=True):
    """a whole slot image against (lap, w): every level on bits, and the padding where the image was imported with it"""
    img = pi.pack(want[0], want[1], pad=fs.PAD)
    if padded and np.array_equal(got, img):
        return
    gl, gw = pi.unpack(got, bands, ff)
    bad = []
    for i in range(len(gw)):
        dl = (gl[i].view(np.uint8) != want[0][i].view(np.uint8)).reshape(gw[i].shape + (-1,)).any(axis=2)
        dw = gw[i].view(np.uint32) != want[1][i].view(np.uint32)
        if dl.any() or dw.any():
            y, x = np.argwhere(dl | dw)[0]
            bad.append("level %d: %d lap px, %d weights, first at (%d, %d): got w %r, want %r" % (i, dl.sum(), dw.sum(), y, x, gw[i][y, x], want[1][i][y, x]))
    if padded:
        n = int((pi.padding_of(got, bands, ff) != fs.PAD).sum())
        if n:
            bad.append("%d padding bytes" % n)
    assert not bad, (label, bad[:6])


def run_rounds(pf, bands, ff, way="default", second=False):
    """The case of one band count and type through one way in; second: a second keyframe, at the rig's other pose with the cull on, over
    the result.  Returns the exported images of every round."""
    prep, poses, frames = fs.rig(bands)
    kf = keyframe_alone(pf, bands, ff)
    rounds = fs.make_rounds(kf, bands, ff)
    fs.check_bite(rounds, kf)                                            # the conditions of tests/test_feed_slots.py, on what was read back
    out = []
    for r, rd in enumerate(rounds):
        g = new_map(pf, bands, ff, way)
        assert g.tile_bytes() == pi.slot_layout(bands, ff)["total"]
        packed = import_tiles(g, rd["stored"])
        assert g.tiles() == by_row(rd["stored"])
        feed(g, way, frames[0], poses[0])
        want, won = fs.expected_round(rd, kf)
        assert won > 0
        assert g.tiles() == by_row(set(kf) | {rd["outside"]})
        got = export_all(g)
        for t in g.tiles():
            assert_image(got[t], want[t], bands, ff, (way, r, t, rd["kinds"].get(t, "fresh")), padded=t != rd["fresh"])
        assert got[rd["outside"]].tobytes() == packed[rd["outside"]].tobytes()
        if way == "thread":
            assert g.render_log() == [0]
        if second:
            kf2 = keyframe_alone(pf, bands, ff, 1)
            assert set(kf2) & set(rd["stored"])
            g.set_cull(True)
            feed(g, way, frames[1], poses[1])
            want2 = fs.feed_tiles(want, kf2)
            assert g.tiles() == by_row(want2)
            got = export_all(g)
            for t in g.tiles():
                assert_image(got[t], want2[t], bands, ff, ("second", r, t), padded=t in rd["stored"])
        out.append(got)
        g.close()
    return out


# ---------------------------------------------------------------- every band count and type
@pytest.mark.parametrize("bands,ff", ms.COMBOS)
def test_every_kind_at_every_band_count(pf, bands, ff):
    run_rounds(pf, bands, ff)


@pytest.mark.parametrize("ff", [0, 1])
def test_every_way_in_at_five_bands(pf, ff):
    """fused = 0 (k_lap_select), lookahead = 0, the default lookahead, thread = True followed by sync(), and feed_device: each against
    the rule, and so the same bytes from all of them"""
    ref = None
    for way in WAYS:
        got = run_rounds(pf, 5, ff, way)
        kf = keyframe_alone(pf, 5, ff)
        held = [{t: im.tobytes() for t, im in rd.items()} for rd in got]
        # a fresh tile's padding is nobody's: compare it by its levels
        for rd, h in zip(fs.make_rounds(kf, 5, ff), held):
            h[rd["fresh"]] = b"".join(a.tobytes() for lw in pi.unpack(np.frombuffer(h[rd["fresh"]], np.uint8), 5, ff) for a in lw)
        if ref is None:
            ref = held
        assert held == ref, way


@pytest.mark.parametrize("ff", [0, 1])
@pytest.mark.parametrize("bands", [2, 5, 8])
def test_second_keyframe_over_the_result(pf, bands, ff):
    """After the first feed the imported tiles' bounds say "nothing known" but for what the first keyframe raised; those are true
    lower bounds of the hostile content only where that keyframe won -- a stored NaN or FLT_MAX lies outside them, and is not the
    second keyframe's to win either.  With the cull on the result is still the rule applied twice."""
    run_rounds(pf, bands, ff, second=True)


# ---------------------------------------------------------------- tile_import forgets the cull bounds
CULL_CAM = [640, 480, 500, 500, 320, 240]


@pytest.mark.parametrize("lookahead", [0, None])
@pytest.mark.parametrize("ff", [0, 1])
def test_import_forgets_the_cull_bounds(pf, ff, lookahead):
    """test_gpu_cull_slack.py's rig, where the cull bites: A at the origin, B half a footprint along x, so that its low-weight short
    edge lies 5 px past A's centre.  Control: fed A then B, cells of B are culled.  Under test: A is fed, `view` pyramids with all-zero
    weights are imported over every tile of B's canvas -- those over A's tiles replace bounds A raised -- and B is fed: it wins every
    pixel, which a tile_import that kept A's bounds would have culled."""
    bands, scale, H = 5, 2.0, 100.0
    px = H / CULL_CAM[2] / scale
    a, b = [0.0, 0.0, -H, 0, 0, 0, 1], [645 * px, 0.0, -H, 0, 0, 0, 1]
    wl = workloads()
    fa, fb = wl.noise_frame(480, 640, 71), wl.noise_frame(480, 640, 72)
    opt = dict(force_float=ff, band_number=bands, scale=scale, bg_color=BG)
    if lookahead is not None:
        opt["lookahead"] = lookahead

    def fresh_map():
        g = pf.Map2D.create(pf.TypeMultiBandCPU, False, **opt)
        assert g.prepare(wl.IDENTITY_PLANE, CULL_CAM, [a, b])
        g.set_cull(True)
        return g

    control = fresh_map()
    assert control.feed(fa, a) and control.sync()
    tiles_a = control.tiles()
    before = control.culled_cells() + control.culled_tiles()
    assert control.feed(fb, b) and control.sync()
    assert control.culled_cells() + control.culled_tiles() > before       # the teeth: B is culled under A's bounds
    control.close()

    alone = fresh_map()
    assert alone.feed(fb, b) and alone.sync()
    canvas_b = alone.tiles()
    assert set(canvas_b) & set(tiles_a)

    g = fresh_map()
    assert g.feed(fa, a) and g.sync()
    assert any((g.tile_bounds(*t) > 0).any() for t in set(canvas_b) & set(tiles_a))      # A left bounds on tiles the import overwrites
    zeros = [np.zeros((256 >> i, 256 >> i), np.float32) for i in range(bands + 1)]
    images = [to_device(pi.pack(pi.make_lap("view", ff, bands, np.random.default_rng([320, j, bands, ff])), zeros, pad=fs.PAD)) for j in range(3)]
    for j, t in enumerate(canvas_b):
        assert g.tile_import(t[0], t[1], images[j % 3].data_ptr()), t
        assert g.tile_bounds(*t).tobytes() == np.full(16, -1.0, np.float32).tobytes(), t
    before = g.culled_cells() + g.culled_tiles()
    assert g.feed(fb, b) and g.sync()
    assert g.culled_cells() + g.culled_tiles() == before
    got = export_all(g)
    for t in canvas_b:
        assert_image(got[t], levels_of(alone, t), bands, ff, ("import", t))
    g.close(); alone.close()


# ---------------------------------------------------------------- single band
def test_single_band_kinds(pf):
    """k_single / k_single2: stored alphas at the keyframe's own, one above and one below it, 0, 255 and both sides of a byte's sign
    bit; `<` alone moves a pixel, so an equal alpha keeps its colours; a fresh tile takes the keyframe where its alpha is not 0"""
    from helpers import hostile_frame
    from test_gpu_model import COLS, ROWS, lattice_poses
    frame, pose = hostile_frame("noise", ROWS, COLS, 0), lattice_poses(11)[0]
    alone = ms.new_single_band_map(pf)
    assert alone.feed(frame, pose) and alone.sync()
    kf = {t: alone.tile_bgra(*t) for t in alone.tiles()}
    alone.close()
    stored = fs.make_bgra_case(kf)
    fs.check_bite_bgra(stored, kf)
    g = ms.new_single_band_map(pf)
    assert g.tile_bytes() == 256 * 256 * 4
    for t, s in stored.items():
        if s is not None:
            dev = to_device(s.reshape(-1))
            assert g.tile_import(t[0], t[1], dev.data_ptr()), t
            del dev
    assert g.feed(frame, pose) and g.sync()
    want = fs.expected_bgra(stored, kf)
    assert g.tiles() == by_row(want)
    got = export_all(g)
    for t, w in want.items():
        assert np.array_equal(g.tile_bgra(*t), w), (t, int((g.tile_bgra(*t) != w).any(axis=2).sum()))
        assert got[t].tobytes() == w.tobytes(), t
        if stored[t] is not None and t in kf:
            eq = (stored[t][:, :, 3] == kf[t][:, :, 3]) & (kf[t][:, :, 3] > 0)
            assert eq.any() and np.array_equal(w[eq], stored[t][eq])
    g.close()


# ---------------------------------------------------------------- the kernel forms the product does not take
CHILD = """
import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)
import ctypes as C
from conftest import load_package
import test_gpu_feed_slots as T
pf = load_package()
for bands in (5, 8):
    for ff in (0, 1):
        T.run_rounds(pf, bands, ff)
c = (C.c_longlong * 8)(); pf.lib().pf_debug_form_counts(c)
print("forms", list(c))
"""


@pytest.mark.parametrize("switch", ["PF_STRIPS", "PF_BLOCK24", "PF_BLOCK28", "PF_A_ILP=0"])
def test_other_kernel_forms(switch):
    """the forms of the experiments library that carry their own copy of the select, each in a child process (the switches are read
    once per process): test_every_kind_at_every_band_count's case at 5 and 8 bands, both types, and the form counter that
    test_gpu_variants.FORM names for the switch, so that a silent fall-back to the default form fails"""
    from test_gpu_variants import EXP_LIB, FORM
    assert os.path.exists(EXP_LIB), "build the experiments library first (__graft_entry__.build())"
    name, _, val = switch.partition("=")
    env = dict(os.environ, **{name: val or "1", "PF_LIB": EXP_LIB})
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=ROOT)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    line = [ln for ln in out.splitlines() if ln.startswith("forms ")][-1]
    c = [int(v) for v in line[len("forms ["):-1].split(",")]
    assert eval(FORM[switch], {"c": c}), (switch, c)
