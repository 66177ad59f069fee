"""The line tracker without a device: the literal restatement of the Mihasher path (tests/line_track_ref.py (a)) against the closed form the kernel evaluates (b) — the
proof of the tie rule —, the scenario builders' required conditions on the reference run, dv_line_track_check's refusals, and dynamic_vins_amd/csrc/line_track_host.h
(checks, layouts and the rules the kernel shares) driven by tests/host/line_track_host.cpp under AddressSanitizer and UBSan as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

from tests import line_track_cases as lc
from tests import line_track_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def agree(query, train):
    """(a) == (b) wherever (a) finds a row nearer than 30; (b) reports no match everywhere else"""
    lit = lr.match_literal(query, train)
    idx_b, dist_b = lr.nearest_closed_form(query, train)
    if lit is None:
        assert (idx_b == -1).all()
        return 0
    idx_a, dist_a = lit
    near = (dist_a >= 0) & (dist_a < lr.MATCH_DIST)
    assert np.array_equal(idx_a[near], idx_b[near]) and np.array_equal(dist_a[near], dist_b[near])
    assert (idx_b[~near] == -1).all() and (dist_b[~near] == 0).all()
    return int(near.sum())


def test_literal_restatement_has_the_crafted_conditions_and_equals_the_closed_form():
    query, train, tags = lc.match_case()
    idx, dist = lr.match_literal(query, train)
    lc.match_conditions(query, train, tags, idx, dist)
    assert agree(query, train) >= 7
    assert lr.match_literal(query[:0], train) is None and lr.match_literal(query, train[:0]) is None


def test_literal_equals_closed_form_on_seeded_near_duplicates():
    n_near = 0
    ties = 0
    for q, train in lc.near_pairs(3000, seed=7):
        n_near += agree(q[None, :], train)
        d = np.unpackbits(np.bitwise_xor(train, q[None, :]), axis=1).sum(1)
        ties += int(d.min() < lr.MATCH_DIST and (d == d.min()).sum() > 1)
    assert n_near > 2000 and ties > 300          # the set does exercise the tie rule


def test_bucket_order_is_ascending_train_index():
    """the claim the closed form rests on: a bucket hands its rows back in insertion order, whatever the order in which the 32 sub-buckets of a group were first touched"""
    rng = np.random.default_rng(3)
    H = lr.SparseHashtable(8)
    keys = rng.integers(0, 256, 600)
    for i, k in enumerate(keys):
        H.insert(int(k), i)
    for k in range(256):
        assert H.query(k) == [i for i in range(600) if keys[i] == k]


@pytest.mark.parametrize("name", ["small", "wave63", "wave64", "wave65"])
def test_scenarios_literal_equals_closed_form(name):
    frames = lc.small_scenario() if name == "small" else lc.wave_scenario(int(name[4:]))
    a, b = lc.run_ref(frames, literal=True), lc.run_ref(frames, literal=False)
    for ra, rb in zip(a, b):
        for key in ("left_ids", "left_src", "left_cnt", "right_ids", "right_src"):
            assert np.array_equal(ra[key], rb[key])
        assert ra["rows"] == rb["rows"]


def test_small_scenario_conditions():
    frames = lc.small_scenario()
    assert all(len(f[0]) <= 80 for f in frames) and 6 <= len(frames) <= 10
    lc.conditions(frames, lc.run_ref(frames))


def test_wave_and_cap_scenarios_track_everything():
    for n in (63, 64, 65):
        res = lc.run_ref(lc.wave_scenario(n))
        assert all(len(r["left_ids"]) == n and len(r["right_ids"]) == n for r in res) and (res[2]["left_cnt"] == 2).all()
    frames = lc.cap_scenario()
    res = lc.run_ref(frames)
    assert len(frames[0][0]) == len(frames[0][2]) == lc.DV_LINE_MAX
    assert all(len(r["left_ids"]) == lc.DV_LINE_MAX and len(r["right_ids"]) == lc.DV_LINE_MAX for r in res) and (res[1]["left_cnt"] == 1).all()


def test_line_track_check_refusals():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import DV_LINE_MAX, DV_MEM_DEVICE, DV_MEM_HOST, line_track_check
    L, D = np.zeros((DV_LINE_MAX + 1, 6), np.float32), np.zeros((DV_LINE_MAX + 1, 32), np.uint8)
    line_track_check(L, D, DV_LINE_MAX)
    line_track_check(L, D, DV_LINE_MAX, L, D, DV_LINE_MAX, DV_MEM_DEVICE)
    line_track_check(None, None, 0)                       # an empty frame is an ordinary frame
    line_track_check(L, D, 3, None, None, 0)              # no right image
    line_track_check(L, D, 3, L, D, 0)                    # an empty right image
    for args, why in [((L, D, DV_LINE_MAX + 1), "DV_LINE_MAX"), ((L, D, 3, L, D, DV_LINE_MAX + 1), "DV_LINE_MAX"), ((L, D, -1), "negative"), ((None, D, 3), "null"),
                      ((L, None, 3), "null"), ((L, D, 3, None, D, 2), "null"), ((L, D, 3, L, None, 2), "null"), ((L, D, 3, None, None, 2), "null"),
                      ((L.ctypes.data + 2, D, 3), "aligned"), ((L, D.ctypes.data + 1, 3), "aligned"), ((L, D, 3, None, None, 0, 7), "memory kind")]:
        with pytest.raises(DvinsError, match=why):
            line_track_check(*args)
    assert DV_MEM_HOST == 0


def test_line_track_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "line_track_host")
    src = os.path.join(ROOT, "tests", "host", "line_track_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe, src], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "line_track_host: ok" in r.stdout, r.stdout + r.stderr
