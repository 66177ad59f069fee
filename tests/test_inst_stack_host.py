"""CPU checks of the mask-stack path (dv_inst_stack_frame_*, dv_inst_track_enqueue_planes, dv_track_unmask_static_planes).
  * its host code (csrc/inst_stack_host.h: the membership rule, BuildBoxes2D's detection list from per-plane boxes, the descriptor / rectangle / plane checks) in a
    stand-alone program — tests/host/inst_stack_host.cpp — and the runner's scheduling of the stage (csrc/runner.hip as plain C++, dv_runner_set_inst_stack) on the
    stand-in C ABI — tests/host/runner_stack_host.cpp, stub_abi.cpp + stub_stack.cpp: every host layout leaving the one-thread loop's logs, dropped planes, a grouped
    sequence refused — both run directly as AddressSanitizer + UBSan builds and as ThreadSanitizer builds;
  * the C membership rule against mask_tensor.to(kInt8).abs().clamp(0, 1) of the installed CPU torch, over all 256 byte values and over floats around a threshold;
  * the Python descriptor (frontend.mask_stack) against the C struct."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_sanitizers import HOST, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    r = subprocess.run(["make", "-s", "-C", HOST, "-f", "inst_stack.mk", "inst_stack"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(_lib("libasan.so") is None, reason="no libasan in this toolchain")
def test_mask_stack_host_code_under_asan_ubsan():
    _build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(HOST, "_build", "inst_stack_asan")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "inst_stack_host: ok" in r.stdout and "BROKEN" not in r.stdout, r.stdout
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"          # (the stand-in's contexts live as long as the process, as in the other runner harnesses)
    r = subprocess.run([os.path.join(HOST, "_build", "runner_stack_asan")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "runner_stack_host: ok" in r.stdout and "DIFFERENT" not in r.stdout and "BROKEN" not in r.stdout, r.stdout


def _tsan_runs(tmp_path):
    """a trivial ThreadSanitizer program, run once BEFORE the work: on kernels where the sanitizer cannot map its shadow memory nothing built with it starts"""
    src = tmp_path / "probe.cpp"
    src.write_text("#include <thread>\nint main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }\n")
    exe = str(tmp_path / "probe")
    if subprocess.run(["g++", "-std=c++17", "-fsanitize=thread", str(src), "-o", exe, "-lpthread"], capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True).returncode == 0


@pytest.mark.skipif(_lib("libtsan.so") is None, reason="no libtsan in this toolchain")
def test_mask_stack_host_code_under_tsan(tmp_path):
    if not _tsan_runs(tmp_path):
        pytest.skip("ThreadSanitizer programs do not start on this kernel")
    _build()
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    r = subprocess.run([os.path.join(HOST, "_build", "inst_stack_tsan")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "inst_stack_host: ok" in r.stdout and "BROKEN" not in r.stdout, r.stdout
    r = subprocess.run([os.path.join(HOST, "_build", "runner_stack_tsan")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "runner_stack_host: ok" in r.stdout and "DIFFERENT" not in r.stdout and "BROKEN" not in r.stdout, r.stdout


def test_c_rule_equals_the_torch_rule(tmp_path):
    """dv_stack_u8_has / dv_stack_f32_has (the expressions the kernels carry) against the reference's tensor expression on this machine's CPU torch: byte 128 is no object
    pixel (abs of int8 -128 wraps), every other non-zero byte is; floats are members strictly above the threshold, NaN never — a naive `!= 0` differs at 128"""
    import torch
    src = ('#include <cstdio>\n#include "inst_stack_host.h"\nint main() { for (int b = 0; b < 256; ++b) std::printf("%d", (int)dv_stack_u8_has((unsigned char)b)); std::printf("\\n");\n'
           ' float v; while (std::scanf("%a", &v) == 1) std::printf("%d", (int)dv_stack_f32_has(v, 0.5f)); std::printf("\\n"); return 0; }\n')
    open(tmp_path / "t.cpp", "w").write(src)
    exe = str(tmp_path / "t")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "dynamic_vins_amd", "csrc"), str(tmp_path / "t.cpp"), "-o", exe], check=True)
    thr = np.float32(0.5)
    fl = np.array([thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0)), np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1e-45], np.float32)
    out = subprocess.run([exe], input=" ".join(float(v).hex() if np.isfinite(v) else str(v) for v in fl), capture_output=True, text=True, check=True).stdout.split()
    want_u8 = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(torch.int8).abs().clamp(0, 1)
    assert int(want_u8[128]) == 0 and int(want_u8[1]) == int(want_u8[127]) == int(want_u8[129]) == int(want_u8[255]) == 1          # what this machine's torch does
    assert out[0] == "".join(str(int(v)) for v in want_u8)
    assert out[0] != "".join(str(int(b != 0)) for b in range(256))
    want_f = (torch.from_numpy(fl) > 0.5).to(torch.int8).abs().clamp(0, 1)
    assert out[1] == "".join(str(int(v)) for v in want_f) == "0100100010"


def test_python_descriptor_matches_the_header():
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_STACK_F32, DV_STACK_U8, dv_mask_stack, mask_stack
    assert C.sizeof(dv_mask_stack) == 40 and dv_mask_stack.plane_stride.offset == 24 and dv_mask_stack.threshold.offset == 32
    hdr = open(os.path.join(ROOT, "include", "dvins.h")).read()
    assert "#define DV_STACK_U8  0" in hdr and "#define DV_STACK_F32 1" in hdr and "#define DV_STACK_REMAP_MERGED 1" in hdr
    a = np.zeros((3, 5, 71), np.float32)[:, :, :67]
    s = mask_stack(a, threshold=0.25)
    assert (s.data, s.n_planes, s.kind, s.mem, s.row_stride, s.plane_stride, s.threshold) == (a.ctypes.data, 3, DV_STACK_F32, DV_MEM_HOST, 284, 1420, 0.25)
    s = mask_stack(np.zeros((2, 4, 64), bool))
    assert (s.kind, s.row_stride, s.plane_stride) == (DV_STACK_U8, 64, 256)
    s = mask_stack(4096, mem=DV_MEM_DEVICE, n_planes=8, row_stride=1242, plane_stride=1242 * 375)
    assert (s.data, s.mem, s.n_planes, s.plane_stride) == (4096, DV_MEM_DEVICE, 8, 465750)
