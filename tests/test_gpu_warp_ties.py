"""The HIP kernels' own coordinate code on cvRound's ties: maps fed keyframes whose homography a test chose (tests/warp_ties.py, through
pf_debug_next_homography) against the numpy models (map_model.py), every tile, every level, Laplacian and weight, byte for byte.

Each of k_levels (fused = 1), k_level3 (3), k_level (2), k_warp (0) and k_single / k_single2 (TypeCPU) carries its own copy of the chain
-- fp64 block-relative terms, rcp_mid_range / rcp_seeded, the magic-number cvRound -- and with the homography of a pose a parity test
lands on a tie only by accident (tests/test_warp_ties.py shows it on the CPU).  Here thousands of pixels per keyframe sit on one or a few
ulps next to one (warp_ties.FEEDS says which matrix is there for which link of the chain, and how many stored pixels each altered link
would change); the last keyframe is fed twice, so every weight ties and the newest must win.

The hook exists in the experiments library alone, so these cases load libpifusion_exp.so (PF_LIB) in child processes -- the switches are
read once per process -- and never the product library: its kernels are the same source and flags as the experiments library's default
instantiations, which is what the `product forms` child runs.  The parent computes the models once per pyramid type and hands them over
as .npz; all children run side by side, each under its own time limit.
Reference: OpenCV 2.4.9 imgwarp.cpp warpPerspectiveInvoker (SURVEY 8c rule 2); Map2DFusion/MultiBandMap2DCPU.cpp:427-474."""
import json
import os
import subprocess
import sys

import pytest

import warp_ties as wt
from helpers import workloads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "pi-slam-fusion_amd", "libpifusion_exp.so")
CHILD = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import warp_ties\n"
         "spec = json.load(open(sys.argv[1]))\n"
         "json.dump(warp_ties.run_cases(spec), open(sys.argv[2], 'w'))\n"
         "print('cases done')\n") % (ROOT, os.path.join(ROOT, "tests"))

TYPES = ("i16", "f32")
# the product's forms, one process: every level-kernel shape for both pyramid types, the single-band map, fused = 1 without the cull and
# without the lookahead, and the same poses WITHOUT the injected matrices (which must not give the model's map: the hook is alive)
PRODUCT = ([{"id": "%s-fused%d" % (t, f), "type": t, "options": {"fused": f}} for t in TYPES for f in (1, 3, 2, 0)]
           + [{"id": "single", "type": "single"}, {"id": "single-nocull", "type": "single", "cull": False}]
           + [{"id": "%s-nocull" % t, "type": t, "cull": False} for t in TYPES]
           + [{"id": "%s-lookahead0" % t, "type": t, "options": {"lookahead": 0}} for t in TYPES]
           + [{"id": "%s-nocull-lookahead0" % t, "type": t, "cull": False, "options": {"lookahead": 0}} for t in TYPES]
           + [{"id": "i16-not-injected", "type": "i16", "inject": False}, {"id": "single-not-injected", "type": "single", "inject": False}]
           # the same keyframes as BGRA (tests/bgra.py: an alpha plane no colour comes near): cn = 4 in the tap addresses of every level-kernel shape
           + [{"id": "%s-fused%d-bgra" % (t, f), "type": t, "options": {"fused": f}, "bgra": True} for t in TYPES for f in (1, 3, 2, 0)]
           + [{"id": "single-bgra", "type": "single", "bgra": True}])
BOTH = [{"id": t, "type": t} for t in TYPES]
BOTH_BGRA = [{"id": "%s-bgra" % t, "type": t, "bgra": True} for t in TYPES]
# experiment forms that change the chain or the taps: (environment, cases, what pf_debug_form_counts must show -- kernels.hip, g_form_counts:
# 0 block form with the computed weight, 1 with the weight plane, 2 LDS patch, 3 strips; the single-band kernels have no counter)
VARIANTS = {
    "PF_SEED=1": (BOTH, "c[0] > 0"),
    "PF_FORCE_GENERAL=1": (BOTH + [{"id": "%s-fused0" % t, "type": t, "options": {"fused": 0}} for t in TYPES] + [{"id": "single", "type": "single"}]
                           + BOTH_BGRA + [{"id": "%s-fused0-bgra" % t, "type": t, "options": {"fused": 0}, "bgra": True} for t in TYPES]
                           + [{"id": "single-bgra", "type": "single", "bgra": True}], "c[0] > 0"),
    "PF_A_ILP=0": (BOTH + BOTH_BGRA, "c[0] > 0"),
    "PF_A_ILP=2": (BOTH, "c[0] > 0"),
    "PF_A_ILP=3": (BOTH, "c[0] > 0"),
    "PF_PATCH=1": (BOTH + BOTH_BGRA, "c[2] > 0"),                       # the plan takes the scale-1 keyframes (the shears); the others run the block form
    "PF_STRIPS=1": (BOTH + BOTH_BGRA, "c[3] > 0 and c[0] == 0"),
    "PF_WEIGHT_PLANE=1": (BOTH + BOTH_BGRA, "c[1] > 0 and c[0] == 0"),
    "PF_SINGLE_OLD=1": ([{"id": "single", "type": "single"}], "True"),
}


def build_models(orc, tmp):
    """{pyramid type: .npz}: ModelMap (16S, 32F) and ModelMapSingleBand fed FEEDS with the geometry of an oracle map at the same poses"""
    from map_model import ModelMap, ModelMapSingleBand
    wl = workloads()
    o = orc.OracleMap()
    assert o.prepare(wl.IDENTITY_PLANE, wt.CAM, wt.POSES)
    models = {"i16": ModelMap(force_float=0), "f32": ModelMap(force_float=1), "single": ModelMapSingleBand()}
    for k, (name, p) in enumerate(wt.FEEDS):
        img = wt.feed_frame(k)
        assert o.feed(img, wt.POSES[p])
        dims, _ = o.last_canvas()
        assert dims[2] == 3 and dims[3] == 3, dims            # 768 x 768: the border ties of the exact matrices lie on the canvas
        for m in models.values():
            m.feed(img, o.grid(), o.footprint(wt.POSES[p]), wt.matrix(name), check_M=False)
            assert m.last[0] == dims
    paths = {}
    for t, m in models.items():
        paths[t] = os.path.join(tmp, "model_%s.npz" % t)
        wt.StoredMap.save(paths[t], m)
    return paths


def run_children(models, tmp, exp_lib):
    """{child name: (return code, output, {case id: mismatches, "forms": counts})}: every child started at once (10 processes with the
    GPU open), each waited for under its own time limit"""
    jobs = {"product": ({}, PRODUCT)}
    for sw, (cases, _) in VARIANTS.items():
        name, _, val = sw.partition("=")
        jobs[sw] = ({name: val}, cases)
    procs = {}
    for j, (env, cases) in jobs.items():
        stem = os.path.join(tmp, j.replace("=", "_"))
        with open(stem + ".spec.json", "w") as f:
            json.dump({"models": models, "cases": cases}, f)
        procs[j] = (subprocess.Popen([sys.executable, "-c", CHILD, stem + ".spec.json", stem + ".out.json"], cwd=ROOT,
                                     env=dict(os.environ, PF_LIB=exp_lib, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT), stem)
    out = {}
    for j, (p, stem) in procs.items():
        try:
            txt = p.communicate(timeout=120)[0].decode()
        except subprocess.TimeoutExpired:
            p.kill()
            txt = "TIMEOUT\n" + p.communicate()[0].decode()
        res = None
        if p.returncode == 0 and os.path.exists(stem + ".out.json"):
            with open(stem + ".out.json") as f:
                res = json.load(f)
        out[j] = (p.returncode, txt, res)
    return out


@pytest.fixture(scope="module")
def results(orc, tmp_path_factory):
    assert os.path.exists(EXP_LIB), "build the experiments library first (__graft_entry__.build())"
    tmp = str(tmp_path_factory.mktemp("warp_ties"))
    out = run_children(build_models(orc, tmp), tmp, EXP_LIB)
    print("\nwarp-ties children, seconds:", {j: round(r[2]["seconds"], 1) for j, r in out.items() if r[2]})
    return out


def case_result(results, job, cid):
    rc, txt, res = results[job]
    assert rc == 0 and res is not None, "%s: exit %s\n%s" % (job, rc, txt[-3000:])
    return res[cid]


@pytest.mark.parametrize("cid", [c["id"] for c in PRODUCT if c.get("inject", True)])
def test_product_forms_on_ties(results, cid):
    assert case_result(results, "product", cid) == []


@pytest.mark.parametrize("cid", [c["id"] for c in PRODUCT if not c.get("inject", True)])
def test_the_hook_is_alive(results, cid):
    """the same poses without the injected matrices give another map: the comparisons above are not fed by the poses' own homographies"""
    assert case_result(results, "product", cid) != []


@pytest.mark.parametrize("switch", list(VARIANTS))
def test_experiment_forms_on_ties(results, switch):
    cases, form = VARIANTS[switch]
    c = case_result(results, switch, "forms")
    assert eval(form), (switch, c)                             # the requested form ran
    for case in cases:
        assert case_result(results, switch, case["id"]) == [], case["id"]
