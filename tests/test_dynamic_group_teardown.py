"""Leaving a dv_batch group with an object solve on the way (`-m gpu`): a dynamic member destroyed, or the whole group closed, while a member's object solve is
DEFERRED (packed and uploaded on the group's object stream, not launched: between dv_est_process_dynamic_attach and dv_batch_enqueue) or IN FLIGHT (inside the
group's shared launch, not collected).  dv_destroy / dv_batch_destroy drain the group's streams first; a solve that was never launched is launched alone when its
member collects it.  Every call succeeds, the remaining members' next rounds run — grouped or, after the group is gone, alone — and no error is left behind.
Ordinary API calls only."""
import numpy as np
import pytest

from dynamic_vins_amd import sim

pytestmark = pytest.mark.gpu

W, H, FRAMES, WARM = 640, 360, 24, 18          # the window is full after 11 frames; by round WARM every member's object branch solves every frame
_CACHE = {}


def group_of_three():
    from dynamic_vins_amd.backend import Batch
    from dynamic_vins_amd.pipeline import DynamicPipeline, DynamicSequence
    if "seq" not in _CACHE:
        _CACHE["seq"] = DynamicSequence(W, H, sim.scaled_cam(sim.ZED, W, H, 1280, 720), FRAMES, rate=20.0, boxes=("escort", 4))
    pipes = [DynamicPipeline(_CACHE["seq"], max_cnt=150, min_dist=20, max_iters=8, use_det3d=1) for _ in range(3)]
    batch = Batch([p.ctx for p in pipes])
    for _ in range(WARM):
        round_of(pipes, batch)
    info = batch.obj_info()
    assert info["launches"] >= 3 and info["jobs"] == 3 * info["launches"], info          # the object solves of the three members share one launch per round
    return pipes, batch


def round_of(pipes, batch=None):
    for p in pipes:
        p.step_begin()
    if batch is not None:
        batch.enqueue()
    return [p.step_end() for p in pipes]


def clean(pipes, lib, global_before):
    for p in pipes:
        assert lib.dv_last_error(p.ctx.h) == b"", lib.dv_last_error(p.ctx.h)
    assert lib.dv_last_error(None) == global_before


@pytest.mark.parametrize("when", ["deferred", "in_flight"])
def test_member_destroyed_with_an_object_solve_on_the_way(when):
    pipes, batch = group_of_three()
    lib = pipes[0].ctx.lib
    err0 = lib.dv_last_error(None)
    before = batch.obj_info()
    for p in pipes:
        p.step_begin()                      # window + object solve of every member uploaded, nothing launched
    if when == "in_flight":
        batch.enqueue()
        assert batch.obj_info()["jobs"] == before["jobs"] + 3
    pipes[1].ctx.close()                    # dv_destroy: leaves the group; its uploaded / running solve is drained first
    rest = [pipes[0], pipes[2]]
    if when == "deferred":
        batch.enqueue()                     # the two remaining members' solves, one launch
        assert batch.obj_info()["jobs"] == before["jobs"] + 2
    for p in rest:
        st = p.step_end()
        assert st.nonlinear and np.isfinite(p.est.window()).all()
    twin = [p.est.instances()[0].tobytes() for p in rest]
    assert twin[0] == twin[1]               # same sequence, same calls: the two survivors agree bit for bit, as they did before
    for _ in range(2):                      # and the next rounds of the group run
        sts = round_of(rest, batch)
        assert all(s.nonlinear for s in sts)
    assert rest[0].est.window().tobytes() == rest[1].est.window().tobytes()
    assert batch.obj_info()["jobs"] == before["jobs"] + (3 if when == "in_flight" else 2) + 4
    clean(rest, lib, err0)
    batch.close()
    for p in rest:
        p.ctx.close()


@pytest.mark.parametrize("when", ["deferred", "in_flight"])
def test_group_closed_with_object_solves_on_the_way(when):
    pipes, batch = group_of_three()
    lib = pipes[0].ctx.lib
    err0 = lib.dv_last_error(None)
    before = batch.obj_info()
    for p in pipes:
        p.step_begin()
    if when == "in_flight":
        batch.enqueue()
        assert batch.obj_info()["launches"] == before["launches"] + 1
    batch.close()                           # dv_batch_destroy: the members stay valid; what was not launched is launched by each member's collect, alone
    for p in pipes:
        st = p.step_end()
        assert st.nonlinear and np.isfinite(p.est.window()).all()
    for _ in range(2):                      # the members go on, each on its own streams
        sts = round_of(pipes)
        assert all(s.nonlinear for s in sts)
    assert pipes[0].est.window().tobytes() == pipes[1].est.window().tobytes() == pipes[2].est.window().tobytes()
    assert pipes[0].est.instances()[0].tobytes() == pipes[2].est.instances()[0].tobytes()
    clean(pipes, lib, err0)
    for p in pipes:
        p.ctx.close()
