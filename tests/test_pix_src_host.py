"""CPU check of the dynamic front end's membership rule (csrc/pix_src.h, dv_pix_has): its host side in a stand-alone program — tests/host/pix_src_host.cpp — over all 256
byte values of both byte kinds, the float cases around a threshold and the key comparison, against literal expectations; built with AddressSanitizer + UBSan and run
directly.  The device side of the same function is tests/test_pix_src.py."""
import os
import subprocess

import pytest

from tests.test_sanitizers import HOST, _lib


@pytest.mark.skipif(_lib("libasan.so") is None, reason="no libasan in this toolchain")
def test_membership_rule_host_side_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", HOST, "-f", "pix_src.mk", "pix_src"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(HOST, "_build", "pix_src_asan")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "pix_src_host: ok" in r.stdout and "BROKEN" not in r.stdout, r.stdout
