"""Dynamic sequences as members of a dv_batch group (`-m gpu`): three dynamic members (escort boxes; default boxes with the static-instance feedback; every 2nd frame to
the back end) and one raw member in ONE group of the C++ runner — window solves in the group's shared slots, the object solves of the round in one
bd_solve_group_kernel launch, every member's own tracking launches — against each member's twin run alone (group_size 0, the one-thread loop): window state,
trajectory, iteration totals, row log, object states, static report and object-branch statistics must be EQUAL, bit for bit, in every host layout and for a run cut
into several calls.  And the sharing must really have happened: more than one object solve per shared launch."""
import numpy as np
import pytest

from dynamic_vins_amd import sim

pytestmark = pytest.mark.gpu

W, H, FRAMES = 640, 360, 30
KW = dict(max_cnt=150, min_dist=20, max_iters=8, use_det3d=1)
_CACHE = {}


def sequences():
    if "seqs" not in _CACHE:
        from dynamic_vins_amd.pipeline import DynamicSequence, SyntheticSequence
        cam = sim.scaled_cam(sim.ZED, W, H, 1280, 720)
        _CACHE["seqs"] = (DynamicSequence(W, H, cam, FRAMES, rate=20.0, boxes=("escort", 4)), DynamicSequence(W, H, cam, FRAMES, rate=20.0),
                          SyntheticSequence(W, H, cam, FRAMES, rate=20.0, phase=1.3))
    return _CACHE["seqs"]


def make_pipes():
    from dynamic_vins_amd.pipeline import DynamicPipeline, Pipeline
    escort, default, raw = sequences()
    return [DynamicPipeline(escort, **KW), DynamicPipeline(default, static_as_background=True, **KW), DynamicPipeline(escort, ba_stride=2, **KW),
            Pipeline(raw, max_cnt=150, min_dist=20, max_iters=8)]


def record(runner, i, pipe):
    st, poses, iters, fr = runner.get(i)
    out = dict(window=np.ctypeslib.as_array(st.window).copy().tobytes(), state=(st.frame, st.nonlinear), poses=poses.tobytes(), n_poses=len(poses), iterations=iters, frames=fr,
               row_log=runner.row_log(i).tobytes(), frames9=runner.frames(i).tobytes())
    if getattr(pipe, "mode", 0) != 0:
        I, S = pipe.est.instances()
        out.update(instances=I.tobytes(), n_instances=len(I), inst_summary=np.asarray(S).tobytes(), static=np.asarray(pipe.est.static_instances()).tobytes(), stats=runner.dynamic_stats(i))
    return out


def twins():
    """every member alone: Runner([twin], group_size=0) with the one-thread loop — computed once, shared by all cases"""
    if "twins" not in _CACHE:
        from dynamic_vins_amd.backend import Runner
        out = []
        for i, p in enumerate(make_pipes()):
            r = Runner([p], group_size=0, threads=1)
            r.set("tracker_thread", 0)
            r.run(FRAMES - 1)
            out.append(record(r, 0, p))
            r.close(); p.ctx.close()
        _CACHE["twins"] = out
    return _CACHE["twins"]


def run_group(calls, threads=1, batch_front=1, teams=0, tracker_thread=None):
    from dynamic_vins_amd.backend import Runner
    pipes = make_pipes()
    r = Runner(pipes, group_size=4, threads=threads)          # (dv_runner_set_dynamic used to refuse a sequence inside a dv_batch group)
    r.set("batch_front", batch_front)
    r.set("teams", teams)
    if tracker_thread is not None:
        r.set("tracker_thread", tracker_thread)
    for n in calls:
        r.run(n)
    got = [record(r, i, p) for i, p in enumerate(pipes)]
    obj, rounds = r.obj_rounds(), r.batch_rounds()
    r.close()
    for p in pipes:
        p.ctx.close()
    return got, obj, rounds


def check(got, obj, rounds):
    ref = twins()
    assert ref[0]["n_poses"] >= FRAMES - 14 and ref[0]["n_instances"] >= 3 and ref[0]["stats"]["object_features"] > 20 * FRAMES, "the twin run must exercise the object branch"
    for i, (g, t) in enumerate(zip(got, ref)):
        for key in t:
            assert g[key] == t[key], f"member {i}: {key} differs from the member's own run"
    print("object-solve launches:", obj, "window rounds (batched, single):", rounds)
    assert obj["launches"] > 0 and obj["jobs"] / obj["launches"] > 1.0, obj          # the three dynamic members really shared launches
    assert rounds[0] >= FRAMES - 14, rounds                                            # and the window solves of the group did too


@pytest.mark.parametrize("batch_front,threads,teams", [(0, 1, 0), (1, 1, 0), (1, 2, 1)])
def test_dynamic_members_of_a_group_equal_their_own_runs(batch_front, threads, teams):
    check(*run_group((FRAMES - 1,), threads=threads, batch_front=batch_front, teams=teams))


def test_tracker_thread_switch_does_not_reach_group_members():
    """a dynamic member of a group runs the one-thread order whatever "tracker_thread" says (the default is 1, as in the cases above; here it is set explicitly, to 0)"""
    check(*run_group((FRAMES - 1,), tracker_thread=0))


def test_a_run_cut_into_several_calls_equals_the_single_call():
    assert sum((7, 1, 13, 8)) == FRAMES - 1
    check(*run_group((7, 1, 13, 8)))
