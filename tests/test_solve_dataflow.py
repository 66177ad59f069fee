"""The window solve's factorisation loop on LDS flags instead of workgroup barriers (`-m gpu`; be_mf16.h, ldlt_mf16<DF>): the hand-off changes WHEN a wave may proceed,
never what it computes, so every solve must give the bits it gave before the change.  No tolerance anywhere in this file.

tests/golden/solve_dataflow/<case>.npy / .json hold the solved state and the summary of dv_ba_solve on each case below, recorded with the library of the commit BEFORE the
dataflow form (barrier loop only) by tests/tools/solve_dataflow_golden.py; the problems are regenerated here from their seeds (tests/ba_gen.py) and the recorded digest of
the problem's inputs is compared first, so a mismatch of the generator is not mistaken for one of the solve.

  case          n    what it exercises
  vo2           12   one tile, no panel phase (ba_gen gives a two-frame window no landmark — one needs four observations — so this is the prior alone, at its minimum:
                     the tile is factored, no step is taken; vio1 is the one-tile case that moves)
  vio1          15   one frame, IMU states under a prior: one tile with the right-hand-side row in it, two steps
  vio3          45   three tiles, the last one partial (IMU factors only, for the same reason)
  vio5          75
  vo11          66
  vio11         165  the shipped shape
  free11        178  free extrinsics + td: the generic 4-wide form, which must be unaffected
  reject11      165  a window that passes through rejected steps (successful < iterations: the kept factorisation is reused, the radius shrinks)
  short11       165  vio11 with dv_debug_set "short_first_pass": the spare-slot continuation runs

A/B: every MF16 case is also solved with dv_debug_set "ldl_barriers" (the barrier loop, kept as a second instantiation of the single-window kernel) in the same process.
Batched solve (be_solve_batch_kernel shares the body): dv_batch drives estimators, not bare problems, so the two-member case runs two estimators in a group against the
same two alone — with an IMU every solved window is the full one (n = 165), without one the window grows through n = 12, 18, ... 66 (one to five tiles, partial last tiles);
a three-frame IMU window (n = 45) is never solved by an estimator and is covered by the single-window cases only.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import ba_gen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_dataflow")
FREE = dict(with_prior=True, feat_vel=True, td_true=0.01, ex_noise=(0.01, 0.005), prior_ex_scale=1.0, prior_ex_offset=0.01)
# name -> (make_window arguments, debug switches of the solving context, state size n)
CASES = {
    "vo2": (dict(seed=501, nframes=2, use_imu=0, nlm=20, with_prior=True), (), 12),
    "vio1": (dict(seed=501, nframes=1, nlm=0, with_prior=True, prior_x0_noise=0.1), (), 15),
    "vio3": (dict(seed=502, nframes=3, nlm=24), (), 45),
    "vio5": (dict(seed=503, nframes=5, nlm=30), (), 75),
    "vo11": (dict(seed=504, nframes=11, use_imu=0, nlm=40), (), 66),
    "vio11": (dict(seed=505, nframes=11, nlm=40), (), 165),
    "free11": (dict(seed=506, nframes=11, nlm=40, free_blocks=3, **FREE), (), 178),
    "reject11": (dict(seed=407, nframes=11, nlm=30, pose_noise=(0.3, 0.1), depth_noise=0.5, max_iters=10), (), 165),
    "short11": (dict(seed=505, nframes=11, nlm=40), ("short_first_pass",), 165),
}
MF16_CASES = [c for c, (_, _, n) in CASES.items() if n <= 175]


def make_problem(oracle, name):
    return ba_gen.make_window(oracle, **CASES[name][0])


def state_vector(prob):
    return np.concatenate([prob.pose.ravel(), prob.speed_bias.ravel(), prob.ex_pose.ravel(), prob.td.ravel(), prob.inv_depth.ravel()])


def input_digest(prob):
    h = hashlib.sha1()
    for a in (state_vector(prob), prob.factors, prob.landmarks, prob.imu) + ((prob.prior_A, prob.prior_b) if prob.prior is not None else ()):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def summary_dict(s):
    return dict(iterations=int(s.iterations), successful=int(s.successful), termination=int(s.termination),
                initial_cost=float(s.initial_cost).hex(), final_cost=float(s.final_cost).hex())


def solve_case(ctx_factory, oracle, name, extra=()):
    """a fresh context per call (the debug switches stay with their context); returns (input digest, solved state, summary)"""
    from dynamic_vins_amd.backend import ba_solve
    ctx = ctx_factory(width=64, height=48)
    for key in tuple(CASES[name][1]) + tuple(extra):
        assert ctx.lib.dv_debug_set(ctx.h, key.encode(), 1) == 0, key
    prob = make_problem(oracle, name)
    dig = input_digest(prob)
    s = ba_solve(ctx, prob)
    return dig, state_vector(prob), summary_dict(s)


@pytest.fixture(scope="module")
def solved(gpu_ctx_factory, oracle):
    """every case solved once with the default (dataflow) form"""
    return {name: solve_case(gpu_ctx_factory, oracle, name) for name in CASES}


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npy")), json.load(open(os.path.join(GOLDEN, name + ".json")))


@pytest.mark.parametrize("name", list(CASES))
def test_solve_gives_the_recorded_bits(solved, name):
    dig, x, s = solved[name]
    gx, gj = golden(name)
    assert dig == gj["input_sha1"], "the generated problem differs from the one the golden file was recorded on"
    print(name, s, "max |dx| against the record", float(np.abs(x - gx).max()))
    assert {k: gj[k] for k in s} == s
    assert np.array_equal(x.view(np.uint64), gx.view(np.uint64))


def test_cases_exercise_what_they_claim():
    """the records themselves: the rejected-step case does reject, and the short first pass of short11 cannot hold the solve (iterations > max_iters - 2)"""
    rj, sh = golden("reject11")[1], golden("short11")[1]
    assert rj["successful"] < rj["iterations"] - 1, rj       # (the converging iteration also counts as not successful: more than that one)
    assert sh["iterations"] > 8 - 2, sh


@pytest.mark.parametrize("name", MF16_CASES)
def test_barrier_form_and_dataflow_form_agree(gpu_ctx_factory, oracle, solved, name):
    dig, x, s = solve_case(gpu_ctx_factory, oracle, name, extra=("ldl_barriers",))
    assert dig == solved[name][0]
    assert s == solved[name][2]
    assert np.array_equal(x.view(np.uint64), solved[name][1].view(np.uint64))


@pytest.mark.parametrize("use_imu", [1, 0])
def test_two_member_batch_equals_single_windows(gpu_ctx_factory, use_imu):
    from tests import test_batch as tb
    frames = 20
    info = tb.run_group_against_singles(gpu_ctx_factory, use_imu, 2, frames)
    assert info["batched_rounds"] >= frames - 14, info
