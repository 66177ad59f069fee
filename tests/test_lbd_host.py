"""csrc/lbd_host.h as a stand-alone program (tests/host/lbd_host.cpp, built by tests/host/lbd.mk) under -fsanitize=address,undefined: the weight tables, the band-pair
rule, the roundings, the pixel count, computeLBD's tail, the selection and every refusal.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_rules_under_the_sanitizers():
    host = os.path.join(ROOT, "tests", "host")
    b = subprocess.run(["make", "-s", "-C", host, "-f", "lbd.mk", "lbd"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(host, "_build", "lbd_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "lbd_host ok" in r.stdout, r.stdout + r.stderr
