"""The C++ host shim (dynamic_vins_amd/host/dvins_shim.hpp) with undistort_input: 1 — cfg::is_undistort_input as InitOneCamera sets it up (utils/camera_model.cpp:479-504).
CPU: ReadConfig computes the new intrinsics (Config::cam0 / cam1) with dv_optimal_new_camera and leaves a file that says 0 alone.
GPU: a FeatureTracker built from the file reports them (dv_undistort_setup), an Estimator built from the same file reports the same, and the first distorted frame's rows
equal the Python tracker's after Context.undistort_setup()."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_node import CAM, CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM0 = dict(fx=78.07, fy=91.46, cx=62.5, cy=49.7, k1=-0.28340811, k2=0.07395907, p1=0.00019359, p2=1.76187114e-05)          # EuRoC cam0 scaled to the golden frames (128 x 96)
CAM1 = dict(fx=77.89, fy=91.23, cx=64.7, cy=51.0, k1=-0.28368365, k2=0.07451284, p1=-0.00010473, p2=-3.555907e-05)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shim_undistort") / "shim_undistort_test")
    lib = os.path.join(ROOT, "dynamic_vins_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
           os.path.join(ROOT, "tests", "host", "shim_undistort_test.cpp"), "-o", out, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def write_config(d, w, h, undistort):
    text = CFG.format(w=w, h=h).replace("undistort_input: 0", "undistort_input: %d" % undistort).replace('cam1_calib: "cam.yaml"', 'cam1_calib: "cam1.yaml"')
    text = text.replace("max_cnt: 150", "max_cnt: 30").replace("min_dist: 20", "min_dist: 10")
    assert "undistort_input: %d" % undistort in text and "cam1.yaml" in text and "max_cnt: 30" in text
    open(d / "shim.yaml", "w").write(text)
    open(d / "cam.yaml", "w").write(CAM.format(w=w, h=h, **CAM0))
    open(d / "cam1.yaml", "w").write(CAM.format(w=w, h=h, **CAM1))
    return str(d / "shim.yaml")


def cams_of(lines, tag):
    return [tuple(float(v) for v in ln.split()[1:]) for ln in lines if ln.startswith(tag)]


def test_shim_config_carries_the_new_intrinsics(exe, tmp_path):
    from dynamic_vins_amd import sim
    from dynamic_vins_amd.frontend import optimal_new_camera
    w, h = 128, 96
    out = subprocess.run([exe, "parse", write_config(tmp_path, w, h, 1)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0] == "undistort_input 1"
    assert cams_of(out, "file") == [sim.cam_tuple(CAM0), sim.cam_tuple(CAM1)]
    assert cams_of(out, "cam") == [optimal_new_camera(sim.cam_tuple(c), w, h, 0.0) + (0.0,) * 4 for c in (CAM0, CAM1)]
    out = subprocess.run([exe, "parse", write_config(tmp_path, w, h, 0)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0] == "undistort_input 0"
    assert cams_of(out, "cam") == cams_of(out, "file") == [sim.cam_tuple(CAM0), sim.cam_tuple(CAM1)]


@pytest.mark.gpu
def test_shim_tracker_from_an_undistort_config_matches_the_python_tracker(exe, tmp_path, gpu_ctx_factory):
    from dynamic_vins_amd import sim
    from dynamic_vins_amd.frontend import DV_MODE_NAIVE, cam_tuple, make_cam
    g = np.load(os.path.join(ROOT, "tests", "golden", "front_kat.npz"))
    n, h, w = g["left"].shape
    raw = tmp_path / "frame.raw"
    with open(raw, "wb") as f:
        f.write(g["left"][0].tobytes()); f.write(g["right"][0].tobytes())
    r = subprocess.run([exe, "track", write_config(tmp_path, w, h, 1), str(raw), str(w), str(h)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    ctx = gpu_ctx_factory(width=w, height=h, max_cnt=30, min_dist=10, cam0=make_cam(*sim.cam_tuple(CAM0)), cam1=make_cam(*sim.cam_tuple(CAM1)))
    n0, n1 = ctx.undistort_setup()
    assert cams_of(out, "tracker") == [cam_tuple(n0), cam_tuple(n1)]
    assert cams_of(out, "estimator") == [cam_tuple(n0), cam_tuple(n1)]
    rows = ctx.track_stereo(g["left"][0], g["right"][0], 1.0)
    _compare(out, rows)
    # with an inverse instance mask: the shim remaps it as SemanticImage::SetMask does (basic/semantic_image.cpp:84-92): inv' = ~remap(~inv) with camera 0's maps
    r = subprocess.run([exe, "mask", write_config(tmp_path, w, h, 1), str(raw), str(w), str(h)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    inv = np.full((h, w), 255, np.uint8); inv[h // 4: h // 2, w // 3: 2 * w // 3] = 0
    inv_un = ~ctx.remap(~inv, *ctx.undistort_maps(0))
    assert (inv_un != inv).any()
    ctx.reset()
    rows_m = ctx.track_stereo(g["left"][0], g["right"][0], 1.0, inv_un, DV_MODE_NAIVE)
    _compare(r.stdout.splitlines(), rows_m)
    ctx.reset()
    rows_raw_mask = ctx.track_stereo(g["left"][0], g["right"][0], 1.0, inv, DV_MODE_NAIVE)
    assert len(rows_raw_mask) != len(rows_m) or not np.array_equal(rows_raw_mask["left"], rows_m["left"])      # the unremapped mask gives other rows: the remap matters here


def _compare(out, rows):
    got = [ln.split()[1:] for ln in out if ln.startswith("row ")]
    assert len(got) == len(rows) > 10 and out[[ln.startswith("rows ") for ln in out].index(True)] == "rows %d" % len(rows)
    for tok, q in zip(got, rows):
        assert (int(tok[0]), int(tok[1]), int(tok[2])) == (int(q["id"]), int(q["track_cnt"]), int(q["has_right"]))
        assert [float(v) for v in tok[3:10]] == list(q["left"])
        assert [float(v) for v in tok[10:17]] == (list(q["right"]) if q["has_right"] else [0.0] * 7)
