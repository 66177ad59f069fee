"""ThreadSanitizer on the C++ runner's host machinery for dv_batch groups WITH DYNAMIC MEMBERS (CPU only; tests/host/runner_group_tsan.cpp: runner.hip compiled as plain C++
against the stand-in C ABI of tests/host/stub_abi.cpp, the recipe of tests/test_sanitizers.py).  A dynamic member runs begin_ego / enqueue tracking / attach on its group's
host thread or team thread, the group enqueues once, and the member's collect follows behind that enqueue: every layout — one thread, a thread per group, teams, own or
shared tracking launches, runs cut into several calls — must leave each sequence's own one-thread logs, without a data race, and a member's failure must end the run."""
import os
import subprocess

import pytest

from tests.test_sanitizers import HOST, _lib


@pytest.mark.skipif(_lib("libtsan.so") is None, reason="no libtsan in this toolchain")
def test_groups_with_dynamic_members_under_tsan():
    r = subprocess.run(["make", "-s", "-C", HOST, "-f", "group.mk", "tsan_group"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ)
    env["TSAN_OPTIONS"] = "halt_on_error=1:exitcode=66:second_deadlock_stack=1"
    exe = os.path.join(HOST, "_build", "runner_group_tsan")
    for cmd, extra in [([exe, "layouts"], {}), ([exe, "fail"], {"DVSTUB_FAIL": "1:12"}), ([exe, "fail"], {"DVSTUB_FAIL": "4:9"})]:          # contexts 1 and 4 are dynamic members
        e = dict(env); e.update(extra)
        r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
        if r.returncode != 0 and "unexpected memory mapping" in r.stderr:
            pytest.skip("ThreadSanitizer cannot map its shadow memory on this kernel")
        assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (cmd, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        assert "DIFFERENT" not in r.stdout and "BROKEN" not in r.stdout, r.stdout
