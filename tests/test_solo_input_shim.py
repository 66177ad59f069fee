"""The shim's detector input (dynamic_vins::Pipeline and Detector2D::ForwardTensor in dynamic_vins_amd/host/dvins_shim.hpp) through tests/host/solo_input_shim_test.cpp,
built with plain g++ against include/dvins.h and the library.  Without a device: it compiles under -Wall -Werror and the construction throws by name.  With one
(`-m gpu`): Pipeline::ProcessInput leaves bit for bit what Context.solo_input leaves, on both alternating buffers, image_info is GetXYWHS's, and ForwardTensor with a
stand-in network equals ForwardHead on the same outputs."""
import os
import subprocess

import numpy as np
import pytest

from tests import solo_input_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
(W, H), (MW, MH) = sr.CASES["pad_rows"]


def build(tmp_path_factory):
    if "exe" not in _EXE:
        exe, lib = str(tmp_path_factory.mktemp("solo_input_shim") / "solo_input_shim_test"), os.path.join(ROOT, "dynamic_vins_amd", "lib")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
               os.path.join(ROOT, "tests", "host", "solo_input_shim_test.cpp"), "-o", exe, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread", "-ldl"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE["exe"] = exe
    return _EXE["exe"]


def test_shim_compiles_and_construction_throws_without_a_ctx(tmp_path_factory):
    exe = build(tmp_path_factory)
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and "refused: Pipeline: a ctx is required" in r.stdout, r.stdout + r.stderr


def head_tensors():
    """one level of 2 x 2 cells over a 16 x 8 mask feature: channel j = +1 inside region j, -1 outside, the last channel 1; cell j selects channel j with bias 1/8 and
    scores class j -> two planes (the recipe of tests/test_solo_head.py's scene_head)"""
    nk, g, fh, fw = 2, 2, MH // 4, MW // 4
    kern, cate = np.zeros((nk + 1, g, g), np.float32), np.full((nk, g, g), 0.01, np.float32)
    for j in range(nk):
        kern[j].reshape(-1)[j] = 1.0; kern[nk].reshape(-1)[j] = 0.125; cate[j].reshape(-1)[j] = 0.9 - 0.05 * j
    feat = -np.ones((nk + 1, fh, fw), np.float32)
    feat[0, 2:6, 1:7] = 1.0; feat[1, 3:7, 9:15] = 1.0; feat[nk] = 1.0
    return (nk + 1, nk, g, fh, fw), kern, cate, feat


@pytest.mark.gpu
def test_shim_pipeline_equals_the_python_surface(tmp_path_factory, tmp_path):
    from dynamic_vins_amd.frontend import Context, make_cam
    exe = build(tmp_path_factory)
    frames = [np.ascontiguousarray(sr.image(W, H, seed=50 + k)[1]) for k in range(3)]
    dims, kern, cate, feat = head_tensors()
    spath, opath = str(tmp_path / "scene.bin"), str(tmp_path / "tensors.bin")
    with open(spath, "wb") as fh:
        fh.write(np.array([W, H, MW, MH, len(frames)] + list(dims), np.int32).tobytes() + kern.tobytes() + cate.tobytes() + feat.tobytes())
        for img in frames:
            fh.write(img.tobytes())
    out = subprocess.run([exe, "run", spath, opath], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(frames) + 2
    got = np.fromfile(opath, np.float32).reshape(2 * len(frames) + 1, 3, MH, MW)
    cam = make_cam(100.0, 100.0, W / 2, H / 2)
    ctx = Context(width=W, height=H, max_cnt=30, min_dist=10, cam0=cam, cam1=cam)
    try:
        for k, img in enumerate(frames):
            t, rect = ctx.solo_input(img, MW, MH)
            want = t.cpu().numpy()
            assert float(np.abs(want.astype(np.float64) - sr.solo_input(img, MW, MH)["out"]).max()) <= sr.BAR
            for j in (0, 1):
                assert np.array_equal(got[2 * k + j].view(np.uint32), want.view(np.uint32)), f"frame {k}, call {j}: the shim's tensor differs"
            assert lines[k].split() == [str(k), "rect"] + [str(v) for v in rect + (W, H)] + ["other", "1"], lines[k]
        assert np.array_equal(got[-1].view(np.uint32), want.view(np.uint32)), "the stand-in network was handed another tensor"
    finally:
        ctx.close()
    a, b = lines[-2].split(), lines[-1].split()
    assert a[0] == "tensor" and b[0] == "head" and a[1:] == b[1:], lines[-2:]
    assert a[1] == "1" and len([v for v in a if v.startswith("[")]) == 2 and len([v for v in a if ":" in v]) == 2, a
