"""The state file's parser on the host (pi-slam-fusion_amd/csrc/state_file.hpp): tiny files written here -- a header and two fake
records -- and hostile variants of them (truncated at every section boundary, bad magic, wrong slot size, 2^60 tiles, a tile twice ...).
pf_state_info, which is that parser behind the C ABI, refuses each hostile file and returns the good one's fields exactly; and a
stand-alone program that includes nothing but state_file.hpp, built with AddressSanitizer and UndefinedBehaviorSanitizer, reads the same
files and says the same (tests/cpp/state_file_check.cpp).  No GPU and no HIP code runs here."""
import os
import subprocess

import numpy as np
import pytest

import state_files as sf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = {"int16_band0": dict(), "fp32_band2": dict(pyramid_type=sf.T32FC3, band_number=2, weight_type=1),
         "single_band": dict(map_type=sf.TYPE_SINGLE, pyramid_type=sf.T8UC4)}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{name: (path, should be accepted)}, written once"""
    d = tmp_path_factory.mktemp("state")
    out = {}

    def put(name, data, good):
        p = str(d / (name + ".pfstate"))
        with open(p, "wb") as f:
            f.write(data)
        out[name] = (p, good)

    for kind, over in KINDS.items():
        put("good_" + kind, sf.state_file(**over), True)
    put("good_no_tiles", sf.state_file(tiles=()), True)
    wl = np.full((2, 16), 0.25, np.float32); wl[0, 3] = np.nan; wl[1, 0] = np.inf; wl[1, 15] = -np.inf
    put("good_nan_bounds", sf.state_file(wlbs=wl), True)
    for name, data in sf.hostile_files().items():
        put(name, data, False)
    for name in ("header_only", "first_record", "wrong_slot_bytes", "duplicate_tile"):
        put("single_" + name, sf.hostile_files(**KINDS["single_band"])[name], False)
    return out


def test_state_info_accepts_the_good_files_and_returns_their_fields(pf, files):
    for kind, over in KINDS.items():
        f = dict(sf.DEFAULT); f.update(over)
        info = pf.state_info(files["good_" + kind][0])
        assert info is not None, (kind, pf.lib().pf_last_error())
        assert (info["type"], info["pyramid_type"], info["band_number"], info["weight_type"]) == (f["map_type"], f["pyramid_type"], f["band_number"], f["weight_type"])
        assert (info["tiles"], info["w"], info["h"], info["version"]) == (2, 3, 2, 1)
        assert info["plane"] == [float(v) for v in f["plane"]] and info["cam"] == [float(v) for v in f["cam"]]
        assert info["geo"] == [f["min"][0], f["min"][1], f["max"][0], f["max"][1], f["ele_size"], f["length_pixel"]]
    assert pf.state_info(files["good_no_tiles"][0])["tiles"] == 0
    assert pf.state_info(files["good_nan_bounds"][0])["tiles"] == 2          # a bound that is not finite is no reason to refuse: it reads as -1


def test_state_info_refuses_every_hostile_file(pf, files):
    hostile = [n for n, (_, good) in files.items() if not good]
    assert len(hostile) >= 28
    for name in hostile:
        assert pf.state_info(files[name][0]) is None, name
        assert pf.lib().pf_last_error().decode().startswith("pf_state_info: "), name
    assert pf.state_info(os.path.join(os.path.dirname(files[hostile[0]][0]), "no_such_file")) is None
    assert "slot_bytes" in (pf.state_info(files["wrong_slot_bytes"][0]) or pf.lib().pf_last_error().decode())
    assert "length" in (pf.state_info(files["tiles_2_60"][0]) or pf.lib().pf_last_error().decode())


def test_parser_alone_under_sanitizers_says_the_same(pf, files, tmp_path):
    exe = str(tmp_path / "state_file_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "pi-slam-fusion_amd", "csrc"), os.path.join(HERE, "cpp", "state_file_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    names = sorted(files)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe] + [files[n][0] for n in names], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]
    lines = text.splitlines()
    assert len(lines) == len(names), text[-2000:]
    for name, line in zip(names, lines):
        assert line.startswith("ok " if files[name][1] else "refused "), (name, line)
        assert (pf.state_info(files[name][0]) is not None) == files[name][1], name
    w = dict(zip(names, lines))["good_nan_bounds"].split()
    assert int(w[9]) == 3, w                               # the three bounds that were not finite, and no other, were replaced
    data = open(files["good_int16_band0"][0], "rb").read()
    body = sum(sum(data[sf.HEADER_BYTES + k * (sf.HEAD_BYTES + 655360) + sf.HEAD_BYTES:sf.HEADER_BYTES + (k + 1) * (sf.HEAD_BYTES + 655360)]) for k in range(2))
    assert dict(zip(names, lines))["good_int16_band0"].split()[-1] == str(body)      # read_slot reads the slot images, all of them and nothing else
