"""The background tracking of a dv_batch group's DYNAMIC members in the group's shared launches (`-m gpu`), on the scenes of tests/test_runner_dynamic_group.py:
four dynamic sequences — escort boxes; default boxes with the static-instance feedback (dv_track_unmask_static staged per member, applied by the round's one launch);
every 2nd frame to the back end; default boxes — in ONE group of the C++ runner.  Per round the group enqueues the window and object solves once, then ONE
dv_batch_track_enqueue for the members' next frames, then every member's InstsTrack on its own stream.  Every member must equal its own run alone (group_size 0, the
one-thread loop) bit for bit — window, trajectory, iterations, row log, object states, static report — in every host layout and for a run cut into several calls, and
dv_runner_track_info must show every frame of every member in the shared launches."""
import pytest

from tests.test_runner_dynamic_group import FRAMES, KW, record, sequences

pytestmark = pytest.mark.gpu

_CACHE = {}


def make_pipes():
    from dynamic_vins_amd.pipeline import DynamicPipeline
    escort, default, _ = sequences()
    return [DynamicPipeline(escort, **KW), DynamicPipeline(default, static_as_background=True, **KW), DynamicPipeline(escort, ba_stride=2, **KW), DynamicPipeline(default, **KW)]


def twins():
    """every member alone: Runner([twin], group_size=0) with the one-thread loop — computed once, shared by all cases"""
    if "twins" not in _CACHE:
        from dynamic_vins_amd.backend import Runner
        out = []
        for p in make_pipes():
            r = Runner([p], group_size=0, threads=1)
            r.set("tracker_thread", 0)
            r.run(FRAMES - 1)
            out.append(record(r, 0, p))
            r.close(); p.ctx.close()
        _CACHE["twins"] = out
    return _CACHE["twins"]


def run_group(calls, threads=1, batch_front=1, teams=0):
    from dynamic_vins_amd.backend import Runner
    pipes = make_pipes()
    r = Runner(pipes, group_size=4, threads=threads)
    r.set("batch_front", batch_front)
    r.set("teams", teams)
    for n in calls:
        r.run(n)
    got = [record(r, i, p) for i, p in enumerate(pipes)]
    info, obj = r.track_info(), r.obj_rounds()
    r.close()
    for p in pipes:
        p.ctx.close()
    return got, info, obj


def check(got):
    ref = twins()
    assert ref[0]["n_poses"] >= FRAMES - 14 and ref[0]["n_instances"] >= 3 and ref[0]["stats"]["object_features"] > 20 * FRAMES, "the twin run must exercise the object branch"
    for i, (g, t) in enumerate(zip(got, ref)):
        for key in t:
            assert g[key] == t[key], f"member {i}: {key} differs from the member's own run"


@pytest.mark.parametrize("calls,threads,teams", [((FRAMES - 1,), 1, 0), ((FRAMES - 1,), 2, 1), ((7, 1, 13, 8), 1, 0)])
def test_dynamic_members_track_in_the_groups_shared_launches(calls, threads, teams):
    """one thread | a team of two | a run cut into four calls: frames 0 .. FRAMES - 1 of all four members go through dv_batch_track_enqueue's shared launches (the
    first round enqueues two frames), none through a member's own"""
    assert sum(calls) == FRAMES - 1
    got, info, obj = run_group(calls, threads=threads, teams=teams)
    check(got)
    print("tracking launches:", info, "object-solve launches:", obj)
    assert info == dict(rounds=FRAMES, members_batched=4 * FRAMES, members_single=0), info
    assert obj["launches"] > 0 and obj["jobs"] / obj["launches"] > 1.0, obj


def test_own_tracking_launches_still_equal_the_twins():
    """batch_front 0: every member enqueues its tracking inside its own begin phase, as before; the group's tracking entry is never called"""
    got, info, _ = run_group((FRAMES - 1,), batch_front=0)
    check(got)
    assert info == dict(rounds=0, members_batched=0, members_single=0), info
