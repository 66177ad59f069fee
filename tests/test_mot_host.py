"""The tracker's host half (CPU): dv_mot_check's refusals through ctypes, and dynamic_vins_amd/csrc/mot_host.h — validation, table layout, rect(), IoU, gates, ring and
miss rules, the copies the association kernel shares — driven by tests/host/mot_host.cpp under AddressSanitizer and UBSan as a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mot_check_refusals():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import mot_check, mot_params
    mot_check(mot_params())
    mot_check(mot_params(n_init=0, max_age=0, budget=1, feat_dim=1, max_tracks=1))
    for bad, why in [(dict(budget=0), "budget"), (dict(budget=101), "budget"), (dict(feat_dim=0), "feat_dim"), (dict(feat_dim=513), "feat_dim"),
                     (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=129), "max_tracks"), (dict(n_init=-1), "n_init"), (dict(max_age=-1), "max_age")]:
        with pytest.raises(DvinsError, match=why):
            mot_check(mot_params(**bad))
    with pytest.raises(DvinsError, match="null"):
        mot_check(None)


def test_mot_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mot_host")
    src = os.path.join(ROOT, "tests", "host", "mot_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe, src], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "mot_host: ok" in r.stdout, r.stdout + r.stderr
