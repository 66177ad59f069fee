"""The HIP block-diagonal dogleg solver (bd_solve.h: dv_obj_solve and dv_batch_obj_solve of be_objsolve.hip, dv_line_solve of be_linesolve.hip; SURVEY 8(a) rows I4
and L1) against the dense float64 reference of tests/bd_ref.py (validated without a GPU by tests/test_bd_reference.py), over the SWEEP of that file: every dogleg
branch a positive semidefinite problem reaches (each of kinds 0, 1, 2 in an ACCEPTED step, so that its content shows in the states), every stopping rule, both Huber branches of the dims and point factors, residual blocks per variable block around the
8 evaluation lanes, V around the 64 blocks of an evaluation pass and the 512 solve threads, working sets in LDS (n_obj <= 10) and in HBM.
  (a) max_iters = 0: nothing moves, and initial_cost lies within K_EVAL = 1e3 eps of the reference's magnitude accumulation 0.5 sum |rho|.
  (b) max_iters = 1: the scaled step recovered from the states with the inverse retractions solves the reference's stacked regularised system [J S; sqrt(mu) D] y =
      [-r; 0] with a normwise backward error <= 1e-11 (bd_ref.Linear.backward_error) and equals the reference step to 1e-8 (condition numbers <= 1e6: asserted on the
      CPU); directions whose Jacobian column is identically zero do not move.  The cases of NO_FORWARD have no accepted first step: there nothing may move.
  (c) the k-th iterate, k = 1 .. K (max_iters = k: the kernel is deterministic), against the reference's record: same iterations / successful / termination, cost to
      1e-9 max(1, c0), object states and dims to 1e-8, line parameters median 1e-10 and maximum 1e-6: the bars of tests/test_obj_solve.py and tests/test_line_solve.py; blocks without a residual keep their bits.
  (d) n_obj = 43 (o43_box: V = 516, three accepted steps) and n_obj = 1 through Batch.obj_solve in ONE launch: the end states meet (c).
Branches no case reaches (unreachable while J^T J is positive semidefinite, tests/test_bd_reference.py): the `c <= 0` form of beta, the failed 6x6 factorisation
with its mu escalation, the invalid step and with it termination == 2, the radius below 1e-32.
Measured on the MI355X (V: the kernel's block count; cost: |initial_cost - ref| in eps of the magnitude; backward error; |y - y_ref| / |y_ref|):
    o_box(V=36, 10 active) cost 0 | cond 1.41e+05 be 5.43e-16 dy 1.41e-10; o_it0(V=60, 29 active) cost 0.548 | cond 35.5 be 3.6e-16 dy 5.2e-15
    o_dims_out(V=36, 18 active) cost 0.959 | cond 94.9 be 7.76e-17 dy 2.14e-13; o_pts_only(V=24, 12 active) cost 0.57 | no first step
    o_opt(V=12, 2 active) cost 0 | no first step; o_grad_step(V=12, 5 active) cost 0 | cond 1.27 be 8.35e-15 dy 1.66e-14
    o_accept(V=24, 13 active) cost 0 | cond 10.5 be 2.33e-16 dy 1.55e-15; o_counts(V=24, 13 active) cost 0.582 | cond 15.5 be 7.27e-16 dy 2.98e-15
    o_cauchy(V=24, 14 active) cost 0.707 | no first step; o_plane1(V=24, 13 active) cost 0 | cond 10.5 be 2.33e-16 dy 1.65e-15
    o_plane2(V=36, 10 active) cost 0 | cond 1.41e+05 be 5.43e-16 dy 1.41e-10; o_xnorm(V=12, 4 active) cost 0 | cond 27.5 be 2.95e-16 dy 3.74e-14
    o10(V=120, 53 active) cost 0.542 | cond 3.08e+04 be 2.71e-16 dy 9.73e-12; o11(V=132, 72 active) cost 0 | cond 3.73e+04 be 3.2e-16 dy 3.84e-12
    o43(V=516, 299 active) cost 0.829 | no first step; o43_box(V=516, 268 active) cost 0 | cond 7.56e+04 be 3.35e-16 dy 3.88e-11
    l63(V=63, 61 active) cost 0.661 | cond 2.45e+03 be 2.32e-15 dy 5.21e-12; l64(V=64, 62 active) cost 0 | cond 568 be 2.21e-15 dy 6.94e-13
    l65(V=65, 63 active) cost 0 | cond 474 be 8.29e-15 dy 5.45e-13; l512(V=512, 510 active) cost 0 | cond 1.28e+03 be 1.53e-14 dy 4.92e-12
    l513(V=513, 511 active) cost 0 | cond 1.69e+03 be 4.59e-15 dy 1.4e-12; l_zero(V=40, 38 active) cost 0 | no first step
    l_counts(V=12, 10 active) cost 0 | cond 2.55e+04 be 1.7e-14 dy 2.26e-09; l_func(V=8, 7 active) cost 0.792 | cond 192 be 1.04e-14 dy 1.07e-12
    l_dogleg(V=20, 18 active) cost 0.873 | cond 463 be 1.8e-15 dy 2.74e-12; l_cauchy(V=30, 28 active) cost 0.625 | no first step
    l_grow(V=20, 18 active) cost 0.513 | no first step; l_info(V=40, 38 active) cost 0 | cond 562 be 1.46e-15 dy 9.17e-13
"""
import numpy as np
import pytest

from tests import bd_ref
from tests.test_bd_reference import GROUP, NO_FORWARD, SWEEP, check_against, first_step, make, reference

pytestmark = pytest.mark.gpu
K_EVAL = 1e3


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=64, height=48)


def dev_solve(ctx, prob):
    from dynamic_vins_amd.backend import line_solve, obj_solve
    return (obj_solve if hasattr(prob, "dims") else line_solve)(ctx, prob)


def kernel_V(prob):
    """the kernel's count of variable blocks (BdArgs::V): 11 pose blocks and one dims block per object, or one block per line, with or without residuals"""
    return 12 * len(prob.dims) if hasattr(prob, "dims") else len(prob.orth)


def arrays(prob):
    return (prob.state, prob.dims) if hasattr(prob, "dims") else (prob.orth,)


@pytest.mark.parametrize("name", list(SWEEP))
def test_initial_cost_matches_reference(ctx, oracle, name):
    """(a)"""
    _, _, sol = reference(oracle, name)
    dev = make(name, max_iters=0)
    entry = [a.copy() for a in arrays(dev)]
    s = dev_solve(ctx, dev)
    assert (s.iterations, s.successful, s.termination) == bd_ref.after(sol, 0)[:3]
    assert all(np.array_equal(a, b) for a, b in zip(arrays(dev), entry))
    assert s.final_cost == s.initial_cost
    err, mag = abs(s.initial_cost - sol["initial_cost"]), sol["cost_mag"]
    ratio = err / (bd_ref.EPS * mag) if mag > 0 else (0.0 if err == 0 else np.inf)
    print(f"\n[cost] {name} V={kernel_V(dev)} active={len(reference(oracle, name)[1].keys)} cost {sol['initial_cost']:.6g} ratio {ratio:.3g}")
    assert ratio <= K_EVAL, ratio


@pytest.mark.parametrize("name", list(SWEEP))
def test_first_step_solves_the_reference_system(ctx, oracle, name):
    """(b)"""
    prob, P, _ = reference(oracle, name)
    rec, lin = first_step(oracle, name)
    dev = make(name, max_iters=1)
    s = dev_solve(ctx, dev)
    if name in NO_FORWARD:
        assert rec is None or not rec["accepted"]
        assert s.successful == 0 and s.iterations == (0 if rec is None else 1)
        assert all(np.array_equal(a, b) for a, b in zip(arrays(dev), arrays(prob)))
        return
    assert (s.iterations, s.successful) == (1, 1)
    new, old = P.load(dev), P.x0()
    y = {k: bd_ref.minus(k, new[k], old[k], near=lin.S[k] * lin.y[k]) / lin.S[k] for k in P.keys}          # (near: a line's rotation angles are known up to 2 pi)
    drop = {1: 2, 2: 1}.get(P.plane_kind)          # the translation component a plane constraint drops is not in the states: the value that minimises the residual
    keep = {k: np.array([c for c in range(len(y[k])) if not (k[0] == "pose" and c == drop)]) for k in P.keys}
    if drop is not None:
        for k in P.keys:
            if k[0] == "pose":
                A, b = lin.A[k], lin.b[k]
                y[k][drop] = np.linalg.lstsq(A[:, [drop]], -(A[:, keep[k]] @ y[k][keep[k]] + b), rcond=None)[0][0]
    be = lin.backward_error(y)
    num = np.sqrt(sum(float(np.sum((y[k][keep[k]] - lin.y[k][keep[k]]) ** 2)) for k in P.keys))
    dy = num / np.sqrt(sum(float(np.sum(lin.y[k][keep[k]] ** 2)) for k in P.keys))
    print(f"\n[step] {name} V={kernel_V(dev)} cond {lin.cond():.3g} backward {be:.3g} |y - y_ref| / |y_ref| {dy:.3g}")
    assert be <= 1e-11, be
    assert dy <= 1e-8, dy
    # a direction whose Jacobian column is identically zero does not move: positions and dims bit-equal, quaternions equal to the rounding of one normalisation
    nzero = 0
    for k, cols in lin.zero_columns().items():
        cols = set(cols.tolist())
        nzero += len(cols)
        if k[0] == "pose":
            for c in cols & {0, 1, 2}:
                assert new[k][c] == old[k][c], (k, c)
            if cols >= {3, 4, 5}:
                assert np.abs(new[k][3:] - old[k][3:]).max() <= 4 * bd_ref.EPS, k
        else:
            for c in cols:
                assert new[k][c] == old[k][c], (k, c)
    if hasattr(prob, "dims") and (len(prob.points) == 0 or len(prob.boxes) == 0):
        assert nzero >= 3          # box-only pose blocks have no position column, points-only ones no rotation column


@pytest.mark.parametrize("name", list(SWEEP))
def test_every_iterate_matches_reference(ctx, oracle, name):
    """(c)"""
    prob, P, sol = reference(oracle, name)
    for k in range(1, prob.max_iters + 1):
        dev = make(name, max_iters=k)
        s = dev_solve(ctx, dev)
        check_against(dev, P, sol, k, s, "kernel")


def test_group_launch_matches_reference(gpu_ctx_factory, oracle):
    """(d)"""
    from dynamic_vins_amd.backend import Batch
    b = Batch([gpu_ctx_factory(width=64, height=48) for _ in GROUP])
    try:
        probs = [make(n) for n in GROUP]
        before = b.obj_info()
        out = b.obj_solve([0, 1], probs)
        after = b.obj_info()
        assert (after["launches"] - before["launches"], after["jobs"] - before["jobs"]) == (1, 2), (before, after)
        for n, p, s in zip(GROUP, probs, out):
            _, P, sol = reference(oracle, n)
            check_against(p, P, sol, p.max_iters, s, "group " + n)
    finally:
        b.close()
