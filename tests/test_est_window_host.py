"""csrc/est_window.h as a stand-alone program (tests/host/est_window_host.cpp, built by tests/host/est.mk) under -fsanitize=address,undefined.
`walk` drives the feature manager, triangulation, the PnP seed, the factor tables, the host outlier rule and every slide over a synthetic track and checks the invariants
the header states.  `preint` pushes sample streams through the pre-integration (two of them through the second-new merge) and prints every quantity with %.17g; the same
streams go through the oracle's IntegrationBase restatement and the two must be the same bits (both are built with contraction off; est_window.h claims the sums over the
structural non-zeros equal the dense loops').  Nothing loaded into Python runs under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
EXE = os.path.join(HOST, "_build", "est_window_asan")
NOISE = np.array([0.08, 0.004, 4e-4, 2e-5])


@pytest.fixture(scope="module")
def program():
    b = subprocess.run(["make", "-s", "-C", HOST, "-f", "est.mk", "est"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return EXE


def test_window_walk_under_the_sanitizers(program):
    r = subprocess.run([program, "walk"], capture_output=True, text=True)
    assert r.returncode == 0 and "est_window_host ok" in r.stdout, r.stdout + r.stderr


def _stream(rng, n, dt, zero_at=None):
    """n samples [dt, acc, gyr] of a body that turns and accelerates; zero_at: index of one sample with dt = 0"""
    s = np.empty((n, 7))
    s[:, 0] = dt
    if zero_at is not None:
        s[zero_at, 0] = 0.0
    s[:, 1:4] = np.array([0.3, -0.2, 9.81]) + rng.normal(0, 0.5, (n, 3))
    s[:, 4:7] = np.array([0.05, -0.1, 0.2]) + rng.normal(0, 0.05, (n, 3))
    return s


def _cases():
    rng = np.random.default_rng(7)
    return {"one_sample": (_stream(rng, 1, 0.005), None), "ten_at_5ms": (_stream(rng, 10, 0.005), None), "one_zero_dt": (_stream(rng, 12, 0.005, zero_at=5), None),
            "two_hundred": (_stream(rng, 200, 0.0025), None), "second_new_merge": (_stream(rng, 10, 0.005), _stream(rng, 9, 0.005))}


CASES = _cases()


def _oracle_preint(lib, a0, g0, ba, bg, samples, rba, rbg):
    lib.dvo_preint_create.restype = C.c_void_p
    lib.dvo_preint_create.argtypes = [C.c_void_p] * 5
    lib.dvo_preint_push.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.dvo_preint_repropagate.argtypes = [C.c_void_p] * 3
    lib.dvo_preint_get.argtypes = [C.c_void_p] * 7
    lib.dvo_preint_destroy.argtypes = [C.c_void_p]
    h = lib.dvo_preint_create(a0.ctypes.data, g0.ctypes.data, ba.ctypes.data, bg.ctypes.data, NOISE.ctypes.data)

    def get():
        sum_dt = C.c_double()
        dp, dq, dv, jac, cov = np.zeros(3), np.zeros(4), np.zeros(3), np.zeros(225), np.zeros(225)
        lib.dvo_preint_get(h, C.addressof(sum_dt), dp.ctypes.data, dq.ctypes.data, dv.ctypes.data, jac.ctypes.data, cov.ctypes.data)
        return np.concatenate([[sum_dt.value], dp, dq, dv, jac, cov])
    for row in samples:
        a, g = np.ascontiguousarray(row[1:4]), np.ascontiguousarray(row[4:7])
        lib.dvo_preint_push(h, float(row[0]), a.ctypes.data, g.ctypes.data)
    first = get()
    lib.dvo_preint_repropagate(h, rba.ctypes.data, rbg.ctypes.data)
    second = get()
    lib.dvo_preint_destroy(h)
    return first, second


@pytest.mark.parametrize("name", list(CASES))
def test_preintegration_is_the_oracles_bits(program, oracle, name):
    first_stream, merged = CASES[name]
    a0, g0 = np.array([0.25, -0.15, 9.7]), np.array([0.04, -0.12, 0.18])
    ba, bg = np.array([0.02, -0.01, 0.03]), np.array([0.001, 0.002, -0.003])
    rba, rbg = np.array([0.0, 0.0, 0.0]), np.array([0.004, -0.001, 0.002])
    nums = list(a0) + list(g0) + list(ba) + list(bg) + list(NOISE) + [len(first_stream)] + list(first_stream.ravel())
    nums += [0 if merged is None else len(merged)] + ([] if merged is None else list(merged.ravel())) + list(rba) + list(rbg)
    r = subprocess.run([program, "preint"], input="\n".join(repr(float(v)) for v in nums) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = np.array([float(v) for v in r.stdout.split()])
    assert got.size == 2 * 461
    samples = first_stream if merged is None else np.vstack([first_stream, merged])
    want = np.concatenate(_oracle_preint(oracle.lib, a0, g0, ba, bg, samples, rba, rbg))
    print(name, "largest difference", np.abs(got - want).max())
    assert np.array_equal(got, want)
