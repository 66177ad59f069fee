"""tests/bd_ref.py — the plain float64 restatement of the block-diagonal dogleg solve that tests/test_bd_reference_gpu.py holds bd_solve.h to — checked without a
GPU against the oracle (dvo_obj_solve, dvo_line_solve), and the SWEEP of named problems both files run, with what the sweep must exercise asserted from the
reference's own per-iteration record and every decision of every case at least 100 units (a relative cost error of 1e-9, bd_ref.solve) away from its threshold.

Branches the CPU search did not reach, and why they are unreachable while J^T J is positive semidefinite (none is forced with non-finite inputs):
  * the `c <= 0` form of the interpolated step's beta.  c = a.(b - a) with a = -alpha g the Cauchy point and b the Gauss-Newton point; in the dogleg's coordinates
    b = -(H + mu I)^-1 g, and Cauchy-Schwarz gives g.(H)^-1 g >= |g|^4 / g.H g, that is a.b >= |a|^2, with equality only where g is an eigenvector of H, where a = b
    and the interpolation is not entered.  mu = 1e-8 .. 1 moves that by a relative 1e-8 at the most while no step is invalid.  (The two forms are the same number:
    (d - c)(d + c) = |b - a|^2 (radius^2 - |a|^2); they differ in rounding only.)
  * a failed factorisation of a 6x6 block with its mu escalation: every pivot of S H S + mu D^2 is >= mu D^2 >= 1e-14.
  * an invalid step (model decrease <= 0), hence `termination == 2` (five in a row): the model decrease of any point on the dogleg path is positive.
  * the trust region radius below 1e-32: 150 rejections in a row."""
import math

import numpy as np
import pytest

from tests import bd_ref
from tests import obj_gen as G

BOX = dict(pts_per_obj=0)                                                      # detections only: box-only pose blocks (zero position columns), every step accepted
SWEEP = {
    # ---- objects (dv_obj_solve): V = 12 n_obj, n_obj <= 10 with the working set in LDS
    "o_box": ("obj", dict(seed=2, n_obj=3, max_iters=10, **BOX)),                                        # accepted steps, radius halved on acceptance
    "o_it0": ("obj", dict(seed=3, n_obj=5, max_iters=0, **BOX)),                                         # max_iters = 0
    "o_dims_out": ("obj", dict(seed=12, n_obj=3, dims_noise=3.0, max_iters=12, **BOX)),                  # Huber outliers of the dims factor
    "o_pts_only": ("obj", dict(seed=6, n_obj=2, pts_per_obj=20, box_prob=0.0, max_iters=12)),            # points-only objects: no dims block, no body pose in |x|
    "o_opt": ("obj", dict(seed=100, n_obj=1, box_prob=0.0, dims_noise=0.0, pose_noise=(0.0, 0.0), outside=0.0, pts_per_obj=3, max_iters=5)),      # at its optimum
    "o_grad_step": ("obj", dict(seed=102, n_obj=1, box_prob=0.0, dims_noise=0.0, pose_noise=(0.0, 0.0), outside=0.0, pts_per_obj=3, max_iters=5)),      # ... after one step
    # boxes and points, accepted.  8 iterations: the dims factor's Jacobian is not its derivative, every step gains 2.7 % where the model promises all of it, and what
    # separates two float64 implementations (this reference and the oracle: 4e-16 after the first step) grows about fourfold per step: 2e-10 after 8, 5e-7 after 12
    "o_accept": ("obj", dict(seed=107, n_obj=2, pts_per_obj=6, pose_noise=(0.02, 0.2), outside=0.0, max_iters=8)),
    # points per block against the 8 evaluation lanes (0: box-only, 1, 7, 8, 9: a second stride pass), every step accepted: H and g of those blocks reach the states
    "o_counts": ("obj", dict(seed=107, n_obj=2, pts_per_obj=9, pts_per_block=(0, 1, 7, 8, 9), pose_noise=(0.0, 0.1), outside=0.0, max_iters=6)),
    # nine rejections bring the radius down to the Cauchy point: the Cauchy-limited step (kind 1) is ACCEPTED in iteration 10 and two more steps start from it
    "o_cauchy": ("obj", dict(seed=126, n_obj=2, pose_noise=(0.4, 1.5), dims_noise=3.0, max_iters=12, **BOX)),
    "o_plane1": ("obj", dict(seed=107, n_obj=2, pts_per_obj=6, pose_noise=(0.02, 0.2), outside=0.0, max_iters=6, plane_kind=1)),
    "o_plane2": ("obj", dict(seed=2, n_obj=3, max_iters=4, plane_kind=2, **BOX)),
    "o_xnorm": ("obj", dict(seed=100, n_obj=1, pose_noise=(0.4, 0.002), dims_noise=0.05, max_iters=12, body_shift=1e6, **BOX)),      # parameter tolerance through xnorm2_const
    "o10": ("obj", dict(seed=61, n_obj=10, max_iters=6, **BOX)),                                         # the last size in LDS
    "o11": ("obj", dict(seed=62, n_obj=11, max_iters=6, **BOX)),                                         # the first size in HBM
    "o43": ("obj", dict(seed=35, n_obj=43, pts_per_obj=4, pose_noise=(0.02, 0.2), outside=0.0, max_iters=3)),      # V = 516 with a few points per block: every step rejected
    "o43_box": ("obj", dict(seed=63, n_obj=43, max_iters=3, **BOX)),                                     # V = 516, every step accepted: the dims blocks straddle thread 512 and move
    # ---- lines (dv_line_solve): V = n_lines, working set in HBM
    "l63": ("line", dict(seed=41, n_lines=63, max_iters=6)),
    "l64": ("line", dict(seed=1, n_lines=64, max_iters=6)),
    "l65": ("line", dict(seed=42, n_lines=65, max_iters=6)),
    "l512": ("line", dict(seed=43, n_lines=512, max_iters=3)),
    "l513": ("line", dict(seed=44, n_lines=513, max_iters=3)),
    "l_zero": ("line", dict(seed=3, sqrt_info=(0, 0, 0, 0))),                                            # the reference as shipped: gradient stop at iteration 0
    "l_counts": ("line", dict(seed=5, n_lines=12, obs_counts=(1, 7, 8, 9), max_iters=8)),                # observations per line vs 8 lanes
    "l_func": ("line", dict(seed=100, n_lines=8, orth_noise=0.003, pix_sigma=0.001, max_iters=12, empty_lines=1)),      # function tolerance
    "l_dogleg": ("line", dict(seed=107, n_lines=20, orth_noise=0.5, max_iters=12)),                      # interpolated steps accepted, radius growth
    # iterations 10 and 11 are accepted with rel < 0.25: the radius they halve is what makes iteration 12 a Cauchy-limited step (kind 1), and it is accepted
    "l_cauchy": ("line", dict(seed=101, n_lines=30, orth_noise=0.5, max_iters=12)),
    # iteration 10 is accepted with rel = 0.78 .. 0.9 and grows the radius: the 0.75 threshold decides what iterations 11 and 12 are
    "l_grow": ("line", dict(seed=109, n_lines=20, orth_noise=1.0, max_iters=12)),
    "l_info": ("line", dict(seed=8, sqrt_info=(300.0, 20.0, -10.0, 280.0), max_iters=8)),
}
# (b) of tests/test_bd_reference_gpu.py needs an accepted Gauss-Newton step in the first iteration: these have none (stopped before it, or rejected: the point factor's
# Jacobian is not its derivative), and none of the others may have a condition number above 1e6.  At most a quarter of the sweep.
NO_FORWARD = ["o_pts_only", "o_opt", "o_cauchy", "o43", "l_zero", "l_cauchy", "l_grow"]


GROUP = ("o43_box", "o_grad_step")          # (d) of the GPU test: n_obj = 43 and n_obj = 1 in one launch, both moving


def make(name, **kw):
    kind, args = SWEEP[name]
    return (G.make_obj_scene if kind == "obj" else G.make_line_scene)(**dict(args, **kw))


def ref_problem(oracle, prob):
    return bd_ref.ObjRef(oracle, prob) if hasattr(prob, "dims") else bd_ref.LineRef(oracle, prob)


_SOL = {}


def reference(oracle, name):
    """(problem at entry, bd_ref problem, bd_ref.solve of it at the case's own max_iters): computed once per case, shared, never modified"""
    if name not in _SOL:
        prob = make(name)
        P = ref_problem(oracle, prob)
        _SOL[name] = (prob, P, bd_ref.solve(P, prob.max_iters))
    return _SOL[name]


def first_step(oracle, name):
    """(record, bd_ref.Linear) of the first iteration of the case run with max_iters = 1, or (None, None) where the solve stops before it"""
    prob, P, sol = reference(oracle, name)
    if prob.max_iters == 0 and sol["stop"] == "iterations":
        if (name, 1) not in _SOL:
            _SOL[(name, 1)] = bd_ref.solve(P, 1)
        sol = _SOL[(name, 1)]
    return (sol["records"][0], sol["first"]) if sol["records"] else (None, None)


def blank_active(P, prob):
    """copies of prob's state arrays with the blocks of P.keys zeroed: what is left are the blocks no residual touches"""
    q = prob.clone()
    P.store({k: 0.0 for k in P.keys}, q)
    return (q.state, q.dims) if hasattr(q, "dims") else (q.orth,)


def check_against(prob, P, sol, k, summary, where):
    """the bars of tests/test_obj_solve.py / tests/test_line_solve.py, held against the reference's state after k iterations; prob holds the solver's states"""
    its, succ, term, cost, x = bd_ref.after(sol, k)
    assert (summary.iterations, summary.successful, summary.termination) == (its, succ, term), (where, k)
    c0 = sol["initial_cost"]
    assert abs(summary.initial_cost - c0) <= 1e-9 * max(1.0, c0), (where, k)
    assert abs(summary.final_cost - cost) <= 1e-9 * max(1.0, c0), (where, k, summary.final_cost, cost)
    # blocks without a residual are not in the program: whatever the active ones did, these keep the bits they came with
    rest, entry = blank_active(P, prob), blank_active(P, P.prob)
    assert all(np.array_equal(a, b) for a, b in zip(rest, entry)), (where, k)
    if not P.keys:
        return
    got, want = P.load(prob), (x if x is not None else P.x0())
    d = np.concatenate([np.abs(got[key] - want[key]) for key in P.keys])
    if hasattr(prob, "dims"):
        assert d.max() <= 1e-8, (where, k, d.max())
    else:
        assert np.median(d) <= 1e-10 and d.max() <= 1e-6, (where, k, np.median(d), d.max())


@pytest.mark.parametrize("name", list(SWEEP))
def test_reference_agrees_with_the_oracle(oracle, name):
    prob, P, sol = reference(oracle, name)
    q = prob.clone()
    untouched = (q.state.copy(), q.dims.copy()) if hasattr(q, "dims") else (q.orth.copy(),)
    s = (G.o_obj_solve if hasattr(q, "dims") else G.o_line_solve)(oracle.lib, q)
    check_against(q, P, sol, prob.max_iters, s, "oracle")
    assert len(sol["records"]) <= 12
    # blocks without a residual are not in the program: nobody moves them
    after = (q.state, q.dims) if hasattr(q, "dims") else (q.orth,)
    x = P.load(q)
    P.store({k: P.x0()[k] for k in P.keys}, q)
    assert all(np.array_equal(a, b) for a, b in zip(after, untouched))
    P.store(x, q)


@pytest.mark.parametrize("name", list(SWEEP))
def test_every_decision_is_far_from_its_threshold(oracle, name):
    """a condition on the INPUTS: no case asks the solver for a knife-edge decision (margin in units of a 1e-9 relative cost error, bd_ref.solve)"""
    sol = reference(oracle, name)[2]
    assert sol["margin"] >= 100.0, sol["margin"]


def test_sweep_exercises_what_it_claims(oracle):
    sols = {n: reference(oracle, n) for n in SWEEP}
    recs = [r for _, _, s in sols.values() for r in s["records"]]
    assert {r["kind"] for r in recs} == {0, 1, 2}
    assert {r["beta_branch"] for r in recs if r["kind"] == 2} == {"c>0"}                  # `c <= 0`: unreachable, see the module docstring
    assert any(r["kind"] == 2 and r["accepted"] for r in recs)
    for n in ("o_cauchy", "l_cauchy"):          # an ACCEPTED Cauchy-limited step, in the object and in the line solve: a rejected one leaves no trace in any state
        assert any(r["kind"] == 1 and r["accepted"] for r in sols[n][2]["records"]), n
    last = sols["l_cauchy"][2]["records"]
    assert [r["radius_move"] for r in last[9:11]] == ["shrink_accept"] * 2 and last[11]["kind"] == 1          # the radius halved on acceptance decides a later step's kind
    assert any(r["radius_move"] == "grow" and 0.75 < r["rel"] < 0.9 for r in sols["l_grow"][2]["records"][:-1])
    for n in ("o_counts",) + GROUP:
        assert sols[n][2]["successful"] > 0, n
    assert any(r["accepted"] for r in recs) and any(r["rel"] is not None and not r["accepted"] for r in recs)
    assert {r["radius_move"] for r in recs} >= {"grow", "shrink_accept", "shrink_reject"}
    stops = {(s["stop"], s["iterations"] == 0, hasattr(p, "dims")) for p, _, s in sols.values()}
    assert {s for s, _, _ in stops} == {"iterations", "gradient", "function", "parameter"}      # (radius, invalid: unreachable, see the module docstring)
    assert ("gradient", True, True) in stops and ("gradient", True, False) in stops            # at iteration 0: an object problem at its optimum, the zero-weight lines
    assert ("gradient", False, True) in stops                                                   # and after a step
    assert sols["o_it0"][2]["stop"] == "iterations" and sols["o_it0"][2]["iterations"] == 0 and sols["o_it0"][0].max_iters == 0
    br = {}
    for _, _, s in sols.values():
        for k, v in s["branches"].items():
            br[k] = br.get(k, 0) + v
    assert br["dims_outlier"] > 0 and br["dims_inlier"] > 0 and br["point_outlier"] > 0 and br["point_inlier"] > 0 and br["point_zero"] > 0
    assert sols["o_dims_out"][2]["branches"].get("dims_outlier", 0) > 0
    # shapes: residual blocks per variable block against the 8 lanes that stride over them (points of a pose block: its box is lane 0's; observations of a line)
    P = sols["o_counts"][1]
    boxes = {(int(b["obj"]), int(b["frame"])) for b in sols["o_counts"][0].boxes}
    pts = {P.factors[k] - ((k[1], k[2]) in boxes) for k in P.keys if k[0] == "pose"}
    assert pts >= {0, 1, 7, 8, 9}, pts
    assert set(sols["l_counts"][1].factors.values()) >= {1, 7, 8, 9} and len(sols["l_counts"][1].keys) < len(sols["l_counts"][0].orth)      # (0: the unobserved lines)
    assert [len(sols[n][0].orth) for n in ("l63", "l64", "l65", "l512", "l513")] == [63, 64, 65, 512, 513]
    assert {len(sols[n][0].dims) for n in SWEEP if SWEEP[n][0] == "obj"} >= {1, 10, 11, 43}
    p43 = sols["o43"][0]
    for n in ("o43", "o43_box"):          # dims blocks on both sides of thread 512 (kernel block 473 + o), moving in o43_box
        assert 11 * len(sols[n][0].dims) < 512 < 12 * len(sols[n][0].dims) and {("dims", o) for o in (38, 39)} <= set(sols[n][1].keys), n
    x0, x1 = sols["o43_box"][1].x0(), sols["o43_box"][2]["x"]
    assert all(np.abs(x1[("dims", o)] - x0[("dims", o)]).max() > 1e-6 for o in (38, 39))
    assert 0 < len(p43.points) / (11 * 43) < 10                                                                               # "a few points per block"
    box_only = [k for k in sols["o_box"][1].keys if k[0] == "pose"]
    assert box_only and len(sols["o_box"][0].points) == 0
    assert len(sols["o_pts_only"][0].boxes) == 0 and not any(k[0] == "dims" for k in sols["o_pts_only"][1].keys) and sols["o_pts_only"][1].xnorm2_const == 0.0
    assert {sols[n][0].plane_kind for n in ("o_plane1", "o_plane2")} == {1, 2}
    # (b) of the GPU test: an accepted Gauss-Newton first step everywhere but on NO_FORWARD, and a well-conditioned system there
    assert len(NO_FORWARD) <= len(SWEEP) // 4
    for n, (_, _, s) in sols.items():
        first, lin = first_step(oracle, n)
        good = first is not None and first["kind"] == 0 and first["accepted"]
        assert good == (n not in NO_FORWARD), n
        if good:
            assert lin.cond() <= 1e6, (n, lin.cond())


def test_xnorm2_const_decides_the_parameter_tolerance_stop(oracle):
    """the body poses of the frames that carry a detection are parameter blocks of the reference's program that never move (their Jacobian is left at zero): they count in
    |x|, and only there.  o_xnorm stops by parameter tolerance in iteration 2 because of them; without them it runs on."""
    prob, P, sol = reference(oracle, "o_xnorm")
    assert P.xnorm2_const > 1e11 and sol["stop"] == "parameter" and sol["iterations"] == 2
    without = bd_ref.solve(P, prob.max_iters, count_const=False)
    assert without["iterations"] > sol["iterations"] and without["stop"] != "parameter"
    # frames without a detection do not count: exactly the frames of the boxes
    frames = sorted({int(b["frame"]) for b in prob.boxes})
    assert 0 < len(frames) < 11 and P.xnorm2_const == float(sum(prob.body_pose[f] @ prob.body_pose[f] for f in frames))


def test_blockwise_least_squares_is_the_stacked_one(oracle):
    """bd_ref solves the stacked system [J S; sqrt(mu) D] y = [-r; 0] block by block: the dense stacked solve gives the same step, the same backward error ~ eps"""
    for name in ("o_accept", "l_counts"):
        lin = reference(oracle, name)[2]["first"]
        A, b, at = lin.dense()
        y = np.linalg.lstsq(A, -b, rcond=None)[0]
        yb = np.concatenate([lin.y[k] for k in lin.keys])
        assert [at[k] for k in lin.keys] == list(np.cumsum([0] + [len(lin.y[k]) for k in lin.keys])[:-1])
        assert np.linalg.norm(y - yb) <= 1e-10 * np.linalg.norm(y)
        assert lin.backward_error(lin.y) <= 1e-13
        assert abs(np.linalg.norm(A, 2) - max(np.linalg.norm(lin.A[k], 2) for k in lin.keys)) <= 1e-12 * np.linalg.norm(A, 2)


def test_retractions_and_their_inverses(oracle):
    rng = np.random.default_rng(5)
    d = G.make_batch(5, 10)
    for k in range(10):
        assert np.allclose(bd_ref.line_plus(d["orth"][k], d["delta"][k]), G.o_line_plus(oracle.lib, d["orth"][k], d["delta"][k]), rtol=0, atol=1e-13)
        assert np.allclose(bd_ref.line_minus(bd_ref.line_plus(d["orth"][k], d["delta"][k]), d["orth"][k]), d["delta"][k], rtol=0, atol=1e-13)
        dd = rng.normal(0, 0.05, 6)
        x1 = bd_ref.plus(("pose", 0, 0), d["pose_obj"][k], dd)
        assert np.allclose(x1, G.pose_plus(d["pose_obj"][k], dd), rtol=0, atol=1e-14)
        assert np.allclose(bd_ref.minus(("pose", 0, 0), x1, d["pose_obj"][k]), dd, rtol=0, atol=1e-13)
        from tests import line_geometry_np as LG          # the same U and W as the Plücker conversion's
        U, phi = bd_ref._orth_R(d["orth"][k]), d["orth"][k][3]
        assert np.allclose(LG.orth_to_plk(d["orth"][k]), np.concatenate([math.cos(phi) * U[:, 0], math.sin(phi) * U[:, 1]]), rtol=0, atol=1e-15)
    assert math.isinf(bd_ref._dist(0.0, 1e-10, 0.0))
