"""csrc/stereo_sgm_host.h as a stand-alone program (tests/host/sgm_host.cpp, built by tests/host/sgm.mk) under -fsanitize=address,undefined: the census at clamped
borders, the cost rule, the path step, the uniqueness test, the floored division and every refusal.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_rules_under_the_sanitizers():
    host = os.path.join(ROOT, "tests", "host")
    b = subprocess.run(["make", "-s", "-C", host, "-f", "sgm.mk", "sgm"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(host, "_build", "sgm_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "sgm_host ok" in r.stdout, r.stdout + r.stderr
