"""The C++ runner's order of ABI calls, pinned (CPU only).  tests/host/calls.mk builds the three runner harnesses (runner_tsan.cpp, runner_group_tsan.cpp,
runner_viode_host.cpp) unsanitized from the tree's runner.hip, compiled as plain C++ against the stand-in C ABI of tests/host/stub_abi.cpp + stub_viode.cpp.  Run with
--calls, a harness prints per (run, context, domain — tracker, estimator, IMU buffer — and per dv_batch) the count of entries called and the FNV-1a of their records:
name, time argument, counts and modes, the unmask entries' id lists, and of every pointer only whether it is null.  Every line must equal
tests/golden/runner_calls_{raw,dynamic,group,viode}.txt, which were generated with the runner.hip of the commit BEFORE the frame schedule was unified (same stubs, same
harnesses, plain -O1): in every layout — one thread, a thread per group, teams, tracker thread, shared or own tracking launches, masks, ba_stride 2, static feedback,
label images, runs cut into several calls — each context sees the calls, arguments and order it saw then.  `--calls-full` prints the records, to diff two builds.
Measured: the build takes about 10 s, the four runs 1 - 2 s each."""
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def harnesses():
    r = subprocess.run(["make", "-s", "-C", HOST, "-f", "calls.mk", "calls"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(HOST, "_build")


@pytest.mark.parametrize("golden, cmd", [("raw", ["runner_calls", "raw"]), ("dynamic", ["runner_calls", "dynamic"]),
                                         ("group", ["runner_group_calls", "layouts"]), ("viode", ["runner_viode_calls"])])
def test_call_order_equals_the_recorded_one(harnesses, golden, cmd):
    r = subprocess.run([os.path.join(harnesses, cmd[0])] + cmd[1:] + ["--calls"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert "DIFFERENT" not in r.stdout and "BROKEN" not in r.stdout, r.stdout
    got = [l for l in r.stdout.splitlines() if l.startswith("calls ")]
    with open(os.path.join(GOLDEN, "runner_calls_%s.txt" % golden)) as f:
        want = f.read().splitlines()
    assert len(want) > 100 and len(got) == len(want), (len(got), len(want))
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d of %d digests differ; the first: got %r, recorded %r" % (len(wrong), len(want), wrong[0][0], wrong[0][1])
