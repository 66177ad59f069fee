"""The shim's multi-object tracker (dynamic_vins::DeepSORT in dynamic_vins_amd/host/dvins_shim.hpp) through tests/host/mot_shim_test.cpp, built with plain g++ against
include/dvins.h and the library as tests/test_solo_head_ref.py builds its driver.  Without a device: it compiles under -Wall -Werror and refuses a bad parameter set.
With one (`-m gpu`): AddInstancesByTracking over a scenario with integer rectangles, embeddings alternately in host and pinned memory, leaves per frame exactly the
detections and ids tests/mot_ref.py's float64 run gives."""
import os
import subprocess

import numpy as np
import pytest

from tests import mot_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}


def build(tmp_path_factory):
    if "exe" not in _EXE:
        exe, lib = str(tmp_path_factory.mktemp("mot_shim") / "mot_shim_test"), os.path.join(ROOT, "dynamic_vins_amd", "lib")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
               os.path.join(ROOT, "tests", "host", "mot_shim_test.cpp"), "-o", exe, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE["exe"] = exe
    return _EXE["exe"]


def scenario():
    """the small scenario with its rectangles rounded to the integers a dv_inst_det holds; the conditions are asserted on the rounded one"""
    frames = [(np.round(r), f, w) for r, f, w in mc.small_scenario(empty=(5,))]
    r64, _ = mc.conditions(frames, mc.SMALL, ("confirmation", "tentative_death", "ring_wrap"))
    return frames, r64


def test_shim_compiles_and_refuses_bad_parameters(tmp_path_factory):
    exe = build(tmp_path_factory)
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and "refused: DeepSORT" in r.stdout and "budget" in r.stdout, r.stdout + r.stderr
    scenario()


@pytest.mark.gpu
def test_shim_tracking_equals_the_reference(tmp_path_factory, tmp_path):
    exe = build(tmp_path_factory)
    frames, r64 = scenario()
    p = mc.SMALL
    path = str(tmp_path / "scenario.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([p["n_init"], p["max_age"], p["budget"], p["feat_dim"], p["max_tracks"], len(frames)], np.int32).tobytes())
        for r, f, _ in frames:
            fh.write(np.int32(len(r)).tobytes() + r.astype(np.int32).tobytes() + f.astype(np.float32).tobytes())
    out = subprocess.run([exe, "run", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(frames) + 2
    nt = nc = 0
    for k, (ln, ref) in enumerate(zip(lines, r64)):
        if ref["info"]["n"]:      # an empty frame does not reach the tracker: the counters stay
            nt, nc = len(ref["table"]), sum(t["state"] == 1 for t in ref["table"])
        want = [str(k), str(nt), str(nc)] + [f"{j}:{int(i)}" for j, i in enumerate(ref["ids"]) if i >= 0]
        assert ln.split() == want, f"frame {k}: {ln!r}, reference {want}"
    assert lines[-2] == f"tracks {len(r64[-1]['table'])}" and lines[-1] == "after reset 0"
