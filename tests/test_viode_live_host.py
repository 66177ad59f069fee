"""CPU checks of the label-image path (dv_runner_set_viode and the key-image entries).
  * the detection-building rule of dv_viode_frame_collect (csrc/viode_host.h) and the runner's scheduling of thread T1's per-frame stage (csrc/runner.hip as plain C++) in a
    stand-alone program — tests/host/runner_viode_host.cpp on the stand-in C ABI (stub_abi.cpp + stub_viode.cpp) — run directly as an AddressSanitizer + UBSan build and as
    a ThreadSanitizer build: the rule on hand-made boxes, every host layout (one-thread order, T2 beside T3, runs cut into several calls, static feedback, every 2nd
    frame to the back end) leaving the one-thread loop's logs, a grouped sequence refused with the documented message.  (The stand-in's contexts live as long as the
    process, as in the other harnesses: the leak check of the ASan build is off.)
  * the C rule against viode.detections, the Python statement of the same rule, through a small C program."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_sanitizers import HOST, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    r = subprocess.run(["make", "-s", "-C", HOST, "-f", "viode.mk", "viode"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(_lib("libasan.so") is None, reason="no libasan in this toolchain")
def test_label_image_host_code_under_asan_ubsan():
    _build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(HOST, "_build", "runner_viode_asan")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "runner_viode_host: ok" in r.stdout and "DIFFERENT" not in r.stdout and "BROKEN" not in r.stdout, r.stdout


@pytest.mark.skipif(_lib("libtsan.so") is None, reason="no libtsan in this toolchain")
def test_label_image_host_code_under_tsan():
    _build()
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66:second_deadlock_stack=1")
    r = subprocess.run([os.path.join(HOST, "_build", "runner_viode_tsan")], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "unexpected memory mapping" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory on this kernel")
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "runner_viode_host: ok" in r.stdout and "DIFFERENT" not in r.stdout and "BROKEN" not in r.stdout, r.stdout


def test_c_rule_equals_the_python_rule(tmp_path):
    """dv_viode_build_dets (what dv_viode_frame_collect runs) against viode.detections on random boxes: same keys, same rectangles, same order"""
    from dynamic_vins_amd import viode
    rng = np.random.default_rng(5)
    nk = 64
    keys = np.sort(rng.choice(10 ** 8, nk, replace=False)).astype(np.uint32)
    boxes = np.zeros((nk, 4), np.int32)
    for k in range(nk):
        r0, c0 = int(rng.integers(0, 300)), int(rng.integers(0, 600))
        boxes[k] = (-1, -1, -1, -1) if k % 7 == 0 else (r0, r0 + int(rng.integers(0, 40)), c0, c0 + int(rng.integers(0, 40)))
    src = ('#include <cstdio>\n#include "viode_host.h"\nint main() { unsigned keys[64]; int b[256]; for (int k = 0; k < 64; ++k) { if (std::scanf("%u %d %d %d %d", &keys[k], &b[4 * k], &b[4 * k + 1], &b[4 * k + 2], &b[4 * k + 3]) != 5) return 2; }\n'
           ' dv_inst_det d[64]; const int n = dv_viode_build_dets(b, keys, 64, 8, d, 64); for (int i = 0; i < n; ++i) std::printf("%u %d %d %d %d\\n", d[i].track_id, d[i].x, d[i].y, d[i].w, d[i].h); return n < 0; }\n')
    open(tmp_path / "t.cpp", "w").write(src)
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "dynamic_vins_amd", "csrc"), str(tmp_path / "t.cpp"), "-o", exe], check=True)
    text = "".join("%d %d %d %d %d\n" % (keys[k], *boxes[k]) for k in range(nk))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    kimg = np.zeros((360, 640), np.uint32)
    want = [(d["track_id"],) + tuple(d["rect"]) for d in viode.detections(kimg, boxes, keys, 8)]
    assert got == want and len(got) > 10
