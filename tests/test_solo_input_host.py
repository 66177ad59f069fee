"""csrc/solo_input_host.h as a stand-alone program (tests/host/solo_input_host.cpp, built by tests/host/solo_input.mk) under -fsanitize=address,undefined: every refusal,
the rectangle, and the per-axis index and weight rule over whole axes.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_rules_under_the_sanitizers():
    host = os.path.join(ROOT, "tests", "host")
    b = subprocess.run(["make", "-s", "-C", host, "-f", "solo_input.mk", "solo_input"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(host, "_build", "solo_input_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "solo_input_host ok" in r.stdout, r.stdout + r.stderr
