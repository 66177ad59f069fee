"""dv_batch_obj_solve (`-m gpu`): the object solves (InstanceManager::Optimization, estimator_insts.cpp:772-807) of several dv_batch members in ONE launch —
bd_solve_group_kernel, one workgroup per problem behind a job table (bd_solve.h) — against dv_obj_solve of the same problem on the same ctx.  The group kernel runs
the single kernel's body on the same data, so states, dims and all five summary fields must be EQUAL, bit for bit, whatever shares the launch: problems of other
sizes and fates (workgroups end at different iteration counts), working sets in LDS beside working sets in HBM, more variable blocks than threads, any member order.
CPU (`-m "not gpu"`): the new entries are declared, exported and mirrored."""
import os

import numpy as np
import pytest

from tests.test_obj_solve import _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 5          # members of the group


def test_group_entries_are_declared_exported_and_mirrored():
    from dynamic_vins_amd import _abi
    from tests.test_abi import exported_symbols, header_functions
    names, exp = header_functions(), exported_symbols()
    for fn in ("dv_batch_obj_solve", "dv_batch_obj_info", "dv_runner_get_batches"):
        assert fn in names, f"{fn} is not declared in include/dvins.h"
        assert fn in exp, f"{fn} is not exported by libdvins_hip.so"
        assert fn in _abi.SIGNATURES, f"{fn} is not mirrored in _abi.SIGNATURES"
        assert getattr(_abi.load(), fn) is not None
    hdr = open(os.path.join(ROOT, "include", "dvins.h")).read()
    i = hdr.index("int dv_batch_obj_solve(")
    assert "estimator_insts.cpp:772-807" in hdr[hdr.rindex("/*", 0, i):i]      # cited like its neighbours


@pytest.fixture(scope="module")
def group(gpu_ctx_factory):
    from dynamic_vins_amd.backend import Batch
    ctxs = [gpu_ctx_factory(width=64, height=48) for _ in range(S)]
    b = Batch(ctxs)
    yield b
    b.close()


_REF = {}


def reference(group, member, kw):
    """dv_obj_solve of the scene on the member's own ctx, computed once per (member, scene) and never touched again -> (state, dims, summary tuple)"""
    from dynamic_vins_amd.backend import obj_solve
    key = (member, tuple(sorted(kw.items())))
    if key not in _REF:
        p = _scene(**kw)
        s = obj_solve(group.ctxs[member], p)
        _REF[key] = (p.state.copy(), p.dims.copy(), fields(s))
    return _REF[key]


def fields(s):
    return (s.iterations, s.successful, s.termination, np.float64(s.initial_cost).tobytes(), np.float64(s.final_cost).tobytes())


def solve_together(group, members, scenes):
    """one dv_batch_obj_solve over the scenes; every job must carry the bits of its dv_obj_solve -> the summaries"""
    probs = [_scene(**kw) for kw in scenes]
    before = group.obj_info()
    out = group.obj_solve(members, probs)
    after = group.obj_info()
    if len(members) > 1:
        assert (after["launches"] - before["launches"], after["jobs"] - before["jobs"]) == (1, len(members)), (before, after)      # ONE launch held them all
    else:
        assert after["launches"] == before["launches"] and after["single"] == before["single"] + 1, (before, after)
    for m, kw, p, s in zip(members, scenes, probs, out):
        state, dims, summ = reference(group, m, kw)
        assert fields(s) == summ, f"member {m}, scene {kw}: summary {fields(s)[:3]} vs {summ[:3]}"
        assert np.array_equal(p.state.view(np.uint64), state.view(np.uint64)), f"member {m}, scene {kw}: states"
        assert np.array_equal(p.dims.view(np.uint64), dims.view(np.uint64)), f"member {m}, scene {kw}: dims"
    return out


FOUR = [dict(seed=1, n_obj=4),                                          # every step rejected
        dict(seed=3, n_obj=5, pts_per_obj=0, max_iters=40),             # runs to convergence
        dict(seed=9, n_obj=1, pts_per_obj=3, max_iters=8),              # the smallest
        dict(seed=6, n_obj=2, box_prob=0.0)]                            # no dims block active


@pytest.mark.gpu
def test_four_jobs_of_different_sizes_and_fates_in_one_launch(group):
    out = solve_together(group, [0, 1, 2, 3], FOUR)
    its = [s.iterations for s in out]
    print("iterations per job:", its, "terminations:", [s.termination for s in out], "successful:", [s.successful for s in out])
    assert len(set(its)) >= 2, its          # the workgroups really ended at different iteration counts
    assert out[0].successful == 0 and out[1].successful > 0, [s.successful for s in out]


@pytest.mark.gpu
def test_working_sets_in_lds_and_in_hbm_share_a_launch(group):
    """n_obj = 11 -> V = 132 > 125: the first size whose working set stays in HBM (a.lds == 0), beside the last size in LDS (n_obj = 10, 96 000 B: the launch's dynamic LDS) and the smallest"""
    solve_together(group, [0, 1, 2], [dict(seed=21, n_obj=11, pts_per_obj=20, max_iters=12), dict(seed=22, n_obj=10, pts_per_obj=20, max_iters=12), dict(seed=9, n_obj=1, pts_per_obj=3, max_iters=8)])
    # and a launch in which NO job lives in LDS (zero dynamic LDS)
    solve_together(group, [3, 4], [dict(seed=21, n_obj=11, pts_per_obj=20, max_iters=12), dict(seed=23, n_obj=12, pts_per_obj=10, max_iters=6)])


@pytest.mark.gpu
def test_more_variable_blocks_than_threads_beside_a_small_job(group):
    solve_together(group, [4, 0], [dict(seed=10, n_obj=70, pts_per_obj=40, pose_noise=(0.05, 0.01), max_iters=15), dict(seed=9, n_obj=1, pts_per_obj=3, max_iters=8)])


@pytest.mark.gpu
def test_one_job_and_one_job_per_member(group):
    solve_together(group, [2], [FOUR[1]])
    solve_together(group, list(range(S)), FOUR + [dict(seed=4, n_obj=4, pose_noise=(0.05, 0.01), max_iters=30)])


@pytest.mark.gpu
def test_member_order_does_not_matter(group):
    solve_together(group, [0, 1, 2, 3], FOUR)
    solve_together(group, [3, 0, 2, 1], [FOUR[3], FOUR[0], FOUR[2], FOUR[1]])          # the same (member, job) pairs in another table order
    solve_together(group, [1, 3, 0, 2], FOUR)                                        # the same jobs on other members


@pytest.mark.gpu
def test_problems_of_a_real_sequence(group):
    """three object-solve problems the escort sequence produced (tests/golden/obj_sequence_problems.npz), one of them from the stagnating regime, in one launch"""
    from dynamic_vins_amd.backend import obj_solve
    from tests.test_obj_sequence_problems import problems
    picked = [p for _, p, _, _ in problems()][:: 4][:3]
    solo = [p.clone() for p in picked]
    ref = [fields(obj_solve(group.ctxs[i], p)) for i, p in enumerate(solo)]
    out = group.obj_solve([0, 1, 2], picked)
    for i in range(3):
        assert fields(out[i]) == ref[i] and np.array_equal(picked[i].state.view(np.uint64), solo[i].state.view(np.uint64)) and np.array_equal(picked[i].dims.view(np.uint64), solo[i].dims.view(np.uint64)), i


@pytest.mark.gpu
def test_argument_errors(group):
    from dynamic_vins_amd.backend import DvinsError, obj_solve
    good = lambda: _scene(**FOUR[2])
    before = group.obj_info()
    with pytest.raises(DvinsError, match="member index out of range"):
        group.obj_solve([0, S], [good(), good()])
    with pytest.raises(DvinsError, match="member index out of range"):
        group.obj_solve([-1], [good()])
    with pytest.raises(DvinsError, match="listed twice"):
        group.obj_solve([1, 2, 1], [good(), good(), good()])
    with pytest.raises(DvinsError, match="dv_obj_solve: null argument"):
        group.obj_solve([0, 1], [good(), None])
    # one bad problem among good ones: dv_obj_solve's message, on the member and on the first member; nothing is launched and no problem is touched
    for spoil, msg in [(lambda q: q.points["frame"].__setitem__(0, 11), "dv_obj_solve: point index out of range"), (lambda q: setattr(q, "plane_kind", 3), "dv_obj_solve: bad plane_kind"),
                       (lambda q: setattr(q, "boxes", np.concatenate([q.boxes, q.boxes[:1]])), "dv_obj_solve: more than one box")]:
        probs = [_scene(**FOUR[0]), _scene(seed=2, n_obj=2), _scene(**FOUR[2])]
        spoil(probs[1])
        kept = [(p.state.copy(), p.dims.copy()) for p in probs]
        with pytest.raises(DvinsError) as e:
            group.obj_solve([0, 3, 2], probs)
        assert msg in str(e.value)
        assert msg in group.lib.dv_last_error(group.ctxs[3].h).decode() and msg in group.lib.dv_last_error(group.ctxs[0].h).decode()
        with pytest.raises(DvinsError) as e1:          # the text IS dv_obj_solve's
            obj_solve(group.ctxs[3], probs[1])
        assert str(e1.value) == group.lib.dv_last_error(group.ctxs[0].h).decode()
        for p, (s0, d0) in zip(probs, kept):
            assert np.array_equal(p.state, s0) and np.array_equal(p.dims, d0)
    assert group.obj_info() == before          # no launch, shared or single, came out of any of these calls
    solve_together(group, [0, 3, 2], [FOUR[0], FOUR[1], FOUR[2]])          # and the members are as usable as before
