"""The shim's LBD half (LineDetector::Describe / DescribeEnqueue / DescribeCollect and FeatureTracker::TrackImageLine's overload for undescribed LSD output in
dynamic_vins_amd/host/dvins_shim.hpp) through tests/host/lbd_shim_test.cpp, built with plain g++ against include/dvins.h and the library.  Without a device: it compiles
under -Wall -Werror and refuses bad arguments.  With one (`-m gpu`): Describe leaves the rows of tests/lbd_ref.py and the selection's src, the tracker fed the device
frames leaves what Context.line_track leaves for the host copies of the same rows (src composed back to the LSD arrays), and TrackImageLine hands the same rows on as
FeatureBackground::lines with no descriptor row on the host."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import lbd_cases as lc
from tests import lbd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
W, H = 752, 480
CAM = (460.0, 458.0, 367.0, 248.0, -0.28, 0.07)          # the driver's cameras


def build(tmp_path_factory):
    if "exe" not in _EXE:
        exe, lib = str(tmp_path_factory.mktemp("lbd_shim") / "lbd_shim_test"), os.path.join(ROOT, "dynamic_vins_amd", "lib")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
               os.path.join(ROOT, "tests", "host", "lbd_shim_test.cpp"), "-o", exe, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE["exe"] = exe
    return _EXE["exe"]


def test_shim_compiles_and_refuses_bad_arguments(tmp_path_factory):
    exe = build(tmp_path_factory)
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("refused: LineDetector") == 8 and "accepted" in r.stdout, r.stdout + r.stderr
    for why in ("cam must be 0 or 1", "a gray image is required", "one num_pixels per key line", "the image's size and memory kind", "nothing enqueued", "or neither"):
        assert why in r.stdout, why


@functools.lru_cache(None)
def scenario():
    """three stereo frames of a 752 x 480 texture that moves one pixel per frame under lines that move with it; one line is shorter than Detect's 60"""
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (H, W), dtype=np.uint8)
    L0 = np.array([lc.line(100, 100, 300, 140), lc.line(400, 50, 420, 300), lc.line(50, 400, 700, 380), lc.line(200, 200, 230, 210), lc.line(600, 100, 500, 250),
                   lc.line(10, 20, 90, 20), lc.line(350, 240, 351, 420)], np.float32)
    frames = []
    for k in range(3):
        left, right = np.ascontiguousarray(np.roll(base, k, axis=1)), np.ascontiguousarray(np.roll(base, k - 3, axis=1))
        Ll, Lr = L0.copy(), L0[:6].copy()
        Ll[:, [0, 2]] += k
        Lr[:, [0, 2]] += k - 3
        frames.append((left, right, Ll, Lr))
    return frames


def write_scenario(path, frames):
    with open(path, "wb") as fh:
        fh.write(np.array([W, H, len(frames)], np.int32).tobytes())
        for left, right, Ll, Lr in frames:
            fh.write(left.tobytes() + right.tobytes())
            fh.write(np.int32(len(Ll)).tobytes() + Ll.tobytes() + np.int32(len(Lr)).tobytes() + Lr.tobytes())


def make_ctx():
    from dynamic_vins_amd.frontend import Context, make_cam
    return Context(width=W, height=H, max_cnt=30, min_dist=10, cam0=make_cam(*CAM), cam1=make_cam(*CAM))


@pytest.mark.gpu
def test_describe_and_track_equal_the_reference_and_the_host_path(tmp_path_factory, tmp_path):
    exe = build(tmp_path_factory)
    frames = scenario()
    path = str(tmp_path / "scenario.bin")
    write_scenario(path, frames)
    out = subprocess.run([exe, "run", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().splitlines()
    assert len(got) == len(frames)
    ctx = make_ctx()
    try:
        ctx.line_track_reset()
        matched = 0
        for k, (ln, (left, right, Ll, Lr)) in enumerate(zip(got, frames)):
            sides = []
            for img, lines, cam in ((left, Ll, 0), (right, Lr, 1)):
                d = ctx.lbd_describe(img, lines, cam=cam)
                keep = lbd_ref.select(lines, 60.0)
                _, rows = lbd_ref.describe(*lbd_ref.gradients(img), lines)
                assert np.array_equal(d["src"], keep) and np.array_equal(d["desc"], rows[keep]) and 0 < len(keep) < len(lines)
                sides.append(d)
            a, b = sides
            want = ctx.line_track(a["lines"], a["desc"], b["lines"], b["desc"])
            described = lambda d: " ".join(str(s) + (":" + bytes(r).hex() if k % 2 == 0 else "") for s, r in zip(d["src"], d["desc"]))
            left_s = " ".join(f"{i}:{a['src'][s]}:{c}" for i, s, c in zip(want["left_ids"], want["left_src"], want["left_cnt"]))
            right_s = " ".join(f"{i}:{b['src'][s]}" for i, s in zip(want["right_ids"], want["right_src"]))
            rows_s = " ".join(f"{int(r['id'])}:{int(r['has_right'])}" for r in want["rows"])
            expect = f"{k} | dl {described(a)} | dr {described(b)} | left {left_s} | right {right_s} | rows {rows_s}"
            assert ln.split() == expect.split(), f"frame {k}:\n{ln}\n{expect}"
            matched += int((want["left_cnt"] > 0).sum()) + len(want["right_ids"])
        assert matched > 0, "no line was ever matched: the tracker half was not exercised"
    finally:
        ctx.close()


@pytest.mark.gpu
def test_track_image_line_from_undescribed_lines(tmp_path_factory, tmp_path):
    exe = build(tmp_path_factory)
    frames = scenario()
    path = str(tmp_path / "scenario.bin")
    write_scenario(path, frames)
    out = subprocess.run([exe, "image", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().splitlines()
    assert len(got) == len(frames)
    ctx = make_ctx()
    try:
        ctx.line_track_reset()
        for k, (ln, (left, right, Ll, Lr)) in enumerate(zip(got, frames)):
            r = ctx.lbd_track(left, Ll, right, Lr)
            head, _, body = ln.partition(" | lines")
            assert head == f"{k} | kept {len(r['left_ids'])} {len(r['right_ids'])}", ln[:80]
            toks = body.split()
            assert len(toks) == len(r["rows"]) > 0
            for tok, row in zip(toks, r["rows"]):
                parts = tok.split(":")
                want = [float(v) for v in row["left"]] + ([float(v) for v in row["right"]] if row["has_right"] else [])
                assert (int(parts[0]), int(parts[1])) == (int(row["id"]), 2 if row["has_right"] else 1), f"frame {k}: {tok}"
                assert [float.fromhex(v) for v in parts[2:]] == want, f"frame {k}: {tok}"
    finally:
        ctx.close()
