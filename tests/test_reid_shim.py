"""The shim's ReID extractor (dynamic_vins::Extractor and DeepSORT's image-taking overloads in dynamic_vins_amd/host/dvins_shim.hpp) through tests/host/reid_shim_test.cpp,
built with plain g++ against include/dvins.h and the library.  Without a device: it compiles under -Wall -Werror and load_form refuses a file of the wrong length by
name.  With one (`-m gpu`): Extractor::extract returns bit for bit what Context.reid_extract returns, and DeepSORT::AddInstancesByTracking(dets, planes, image) leaves
the detections and ids Context.mot_update gives on those embeddings."""
import os
import subprocess

import numpy as np
import pytest

from tests import reid_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
W, H, N_INIT, MAX_AGE = 96, 64, 1, 3


def build(tmp_path_factory):
    if "exe" not in _EXE:
        exe, lib = str(tmp_path_factory.mktemp("reid_shim") / "reid_shim_test"), os.path.join(ROOT, "dynamic_vins_amd", "lib")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
               os.path.join(ROOT, "tests", "host", "reid_shim_test.cpp"), "-o", exe, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE["exe"] = exe
    return _EXE["exe"]


def test_shim_compiles_and_refuses_a_short_file(tmp_path_factory, tmp_path):
    exe = build(tmp_path_factory)
    path = str(tmp_path / "short.bin")
    np.zeros(1000, np.float32).tofile(path)
    r = subprocess.run([exe, "check", path], capture_output=True, text=True)
    assert r.returncode == 0 and "refused: Extractor::load_form" in r.stdout and "11178496" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_shim_extractor_and_tracker_equal_the_python_surface(tmp_path_factory, tmp_path):
    from dynamic_vins_amd.frontend import Context, make_cam
    exe = build(tmp_path_factory)
    wpath = rc.write_file(str(tmp_path / "reid.bin"), seed=0)
    # three objects drifting by a pixel per frame; integer rectangles, as a dv_inst_det holds them
    base = np.array([[5, 4, 30, 50], [40, 8, 24, 40], [70, 2, 20, 60]], np.int32)
    frames = []
    for k in range(5):
        r = base.copy()
        r[:, 0] += k
        frames.append((r if k != 3 else r[:2], np.ascontiguousarray(rc.image(W, H, seed=20 + k))))
    spath, opath = str(tmp_path / "scene.bin"), str(tmp_path / "feats.bin")
    with open(spath, "wb") as fh:
        fh.write(np.array([W, H, len(frames), N_INIT, MAX_AGE], np.int32).tobytes())
        for r, img in frames:
            fh.write(np.int32(len(r)).tobytes() + r.tobytes() + img.tobytes())
    out = subprocess.run([exe, "run", wpath, spath, opath], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(frames) + 1 and lines[-1] == "empty 0 0"
    cam = make_cam(100.0, 100.0, W / 2, H / 2, 0, 0, 0, 0)
    ctx = Context(width=W, height=H, max_cnt=30, min_dist=10, cam0=cam, cam1=cam)
    ctx.reid_load(wpath)
    ctx.mot_config(n_init=N_INIT, max_age=MAX_AGE, budget=100, feat_dim=512, max_tracks=128)
    got = np.fromfile(opath, np.float32).reshape(-1, 512)
    off, confirmed = 0, 0
    for k, (r, img) in enumerate(frames):
        e = ctx.reid_extract(img, r.astype(np.float32))
        assert np.array_equal(got[off: off + len(r)].view(np.uint32), e.view(np.uint32)), f"frame {k}: embeddings differ"
        off += len(r)
        ids, nt, nc = ctx.mot_update(r.astype(np.float32), e)
        want = [str(k), str(nt), str(nc)] + [f"{j}:{int(i)}" for j, i in enumerate(ids) if i >= 0]
        assert lines[k].split() == want, f"frame {k}: {lines[k]!r}, python surface {want}"
        confirmed = max(confirmed, nc)
    assert off == len(got) and confirmed >= 2
    ctx.close()
