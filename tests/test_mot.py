"""The multi-object tracker on the device (`-m gpu`): dv_mot_* against tests/mot_ref.py, the reference's own lines in numpy.
  dv_mot_assign      equals mot_ref.munkres EXACTLY (ties included) on every shape and kind of matrix below
  scenarios          per frame the ids per detection, the track count and each track's state / id / hits / time_since_update / stored embeddings equal the float64
                     reference exactly; tests/mot_cases.py conditions() asserts on the reference alone that this is a fair demand of a float32 device
  filter values      within 4 delta of the float64 reference, delta = the largest deviation between the float32 and the float64 reference over the scenario, per
                     quantity (4: another float32 evaluation order of the same products and a different 4 x 4 solve).  Both are printed.
  uninitialised rows dv_mot_config fills the galleries with NaN, so every scenario here runs over poisoned ring rows; test_stale_and_poisoned_ring_rows runs one over
                     the finite rows a first run left behind a mot_reset: those would show in a minimum
The scenario conditions themselves are checked without a device (test_scenario_conditions)."""
import numpy as np
import pytest

from tests import mot_cases as mc
from tests import mot_ref
from tests.test_inst_stack import stage_ctx

_REF = {}


def ref_of(name):
    """frames, parameters, float64 run and delta of a scenario: computed once, shared, never changed"""
    if name not in _REF:
        if name == "yaml":
            frames, par, need = mc.yaml_scenario(), mc.YAML, mc.YAML_NEED
        elif name == "small":
            frames, par, need = mc.small_scenario(), mc.SMALL, ("ring_wrap",)
        elif name == "wide":
            frames, par, need = mc.wide_scenario(), mc.WIDE, ()
        elif name == "kinds":
            frames, par, need = mc.small_scenario(empty=(0, 5, 11, 12)), mc.SMALL, ("ring_wrap",)
        r64, delta = mc.conditions(frames, par, need)
        _REF[name] = (frames, par, r64, delta)
    return _REF[name]


@pytest.mark.parametrize("name", ["yaml", "small", "wide", "kinds"])
def test_scenario_conditions(name):
    frames, par, r64, delta = ref_of(name)
    if name == "wide":
        assert max(len(r["table"]) for r in r64) > 64 and max(len(f[0]) for f in frames) == 64
    if name == "kinds":
        assert any(len(f[0]) == 0 for f in frames)


def ctx_of(gpu_ctx_factory):
    return stage_ctx(gpu_ctx_factory, 64, 48)


def assert_table(dev, ref, k):
    assert len(dev) == len(ref), f"frame {k}: {len(dev)} tracks, reference {len(ref)}"
    for i, t in enumerate(ref):
        got = (int(dev["state"][i]), int(dev["id"][i]), int(dev["hits"][i]), int(dev["time_since_update"][i]), int(dev["n_feats"][i]))
        assert got == (t["state"], t["id"], t["hits"], t["time_since_update"], t["n_feats"]), f"frame {k} track {i}: {got}"


def deviation(dev, ref, worst):
    for i, t in enumerate(ref):
        for q in worst:
            worst[q] = max(worst[q], float(np.abs(dev[q][i].astype(np.float64) - t[q]).max()))


def feed(ctx, rects, feats, mem, keep):
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED
    if mem == "host" or len(rects) == 0:
        return ctx.mot_update(rects, feats)
    put = (lambda a: torch.from_numpy(a.copy()).cuda()) if mem == "device" else (lambda a: torch.from_numpy(a.copy()).pin_memory())
    r, f = put(rects), put(feats)
    keep += [r, f]
    return ctx.mot_update(r.data_ptr(), f.data_ptr(), n=len(rects), mem=DV_MEM_DEVICE if mem == "device" else DV_MEM_PINNED)


def run_scenario(ctx, name, kinds=("host",), config=True):
    frames, par, r64, delta = ref_of(name)
    if config:
        ctx.mot_config(**par)
    worst, keep = dict(x=0.0, p_diag=0.0, rect=0.0), []
    for k, ((rects, feats, _), ref) in enumerate(zip(frames, r64)):
        ids, nt, nc = feed(ctx, rects, feats, kinds[k % len(kinds)], keep)
        assert np.array_equal(ids, ref["ids"]), f"frame {k}: ids {ids}, reference {ref['ids']}"
        assert nt == len(ref["table"]) and nc == sum(t["state"] == mot_ref.CONFIRMED for t in ref["table"]), f"frame {k}"
        dev = ctx.mot_tracks()
        assert_table(dev, ref["table"], k)
        deviation(dev, ref["table"], worst)
    print(f"{name}: delta (float32 vs float64 reference) {delta}, device vs float64 {worst}")
    for q in worst:
        assert worst[q] <= 4 * delta[q], f"{q}: device {worst[q]:.3e} from float64, delta {delta[q]:.3e}"


RNG_SHAPES = [(1, 1), (1, 64), (128, 1), (33, 64), (65, 64), (128, 64), (64, 64)]


def assign_matrices():
    rng = np.random.default_rng(1)
    for R, C in RNG_SHAPES:
        yield f"random {R}x{C}", rng.random((R, C)).astype(np.float32)
        yield f"ties {R}x{C}", rng.integers(0, 4, (R, C)).astype(np.float32)
        m = np.full((R, C), 1000.0, np.float32)
        hit = rng.random((R, C)) < 0.03
        m[hit] = rng.random(int(hit.sum())).astype(np.float32) * 0.2
        yield f"stage-1-like {R}x{C}", m
        yield f"all equal {R}x{C}", np.full((R, C), 7.0, np.float32)
        z = rng.random((R, C)).astype(np.float32)
        z[np.arange(R), rng.integers(0, C, R)] = 0.0
        yield f"zero row minimum {R}x{C}", z
    yield "all 1000 40x30", np.full((40, 30), 1000.0, np.float32)
    yield "no columns", np.zeros((5, 0), np.float32)


@pytest.mark.gpu
def test_assign_equals_the_reference_munkres(gpu_ctx_factory):
    ctx = ctx_of(gpu_ctx_factory)
    for name, m in assign_matrices():
        assert np.array_equal(ctx.mot_assign(m), mot_ref.munkres(m)), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["yaml", "small", "wide"])
def test_scenario(gpu_ctx_factory, name):
    run_scenario(ctx_of(gpu_ctx_factory), name)


@pytest.mark.gpu
def test_memory_kinds_and_empty_frames(gpu_ctx_factory):
    run_scenario(ctx_of(gpu_ctx_factory), "kinds", kinds=("host", "device", "pinned"))


@pytest.mark.gpu
def test_stale_and_poisoned_ring_rows(gpu_ctx_factory):
    """a first run fills and wraps the rings with finite rows; mot_reset (no reconfiguration, so the galleries keep them) and the same scenario again: a ring row at or
    past a track's count, stale and finite, would lower a minimum and show — the NaN fill of dv_mot_config alone would not, since a minimum by `<` skips a NaN.  Then once
    more behind a reconfiguration (rows NaN again)"""
    ctx = ctx_of(gpu_ctx_factory)
    run_scenario(ctx, "small")
    ctx.mot_reset()
    assert len(ctx.mot_tracks()) == 0
    run_scenario(ctx, "small", config=False)
    run_scenario(ctx, "small")


@pytest.mark.gpu
def test_nan_removal(gpu_ctx_factory):
    frames, par = mc.collapse_scenario()
    r32 = mc.run_ref(frames, par, np.float32)
    r64 = mc.run_ref(frames, par, np.float64)
    hit = [k for k, r in enumerate(r64) if "nan_removed" in r["info"]["events"]]
    assert hit and hit[0] < 10 and all(mc.discrete(a["table"]) == mc.discrete(b["table"]) for a, b in zip(r32, r64))
    ctx = ctx_of(gpu_ctx_factory)
    ctx.mot_config(**par)
    for k, ((rects, feats, _), ref) in enumerate(zip(frames[: hit[0] + 1], r64)):
        ids, nt, _ = ctx.mot_update(rects, feats)
        assert np.array_equal(ids, ref["ids"]) and nt == len(ref["table"]), f"frame {k}"
        assert_table(ctx.mot_tracks(), ref["table"], k)
    dev = ctx.mot_tracks()      # the two standing tracks keep their order around the one that left; the shrunken box starts again as a birth at the end
    assert [int(v) for v in dev["id"]] == [t["id"] for t in r64[hit[0]]["table"]] and dev["id"][0] == 1 and dev["id"][1] == 3 and dev["state"][2] == mot_ref.TENTATIVE


@pytest.mark.gpu
def test_capacity(gpu_ctx_factory):
    from dynamic_vins_amd._abi import DvinsError
    ctx = ctx_of(gpu_ctx_factory)
    ctx.mot_config(n_init=1, max_age=3, budget=2, feat_dim=8, max_tracks=5)
    f = np.eye(8, dtype=np.float32)
    boxes = np.array([[100.0 * i, 10, 40, 50] for i in range(8)], np.float32)
    ctx.mot_update(boxes[:4], f[:4])
    ctx.mot_update(boxes[:4], f[:4])
    before = ctx.mot_tracks()
    with pytest.raises(DvinsError, match="max_tracks"):
        ctx.mot_update(boxes[:6], f[:6])
    after = ctx.mot_tracks()
    assert before.tobytes() == after.tobytes()
    ids, nt, nc = ctx.mot_update(boxes[:5], f[:5])
    assert nt == 5 and nc == 4 and list(ids) == [1, 2, 3, 4, -1]
    assert list(ctx.mot_tracks()["hits"]) == [2, 2, 2, 2, 0]


@pytest.mark.gpu
def test_refusals_on_the_device(gpu_ctx_factory):
    from dynamic_vins_amd._abi import DvinsError
    ctx = ctx_of(gpu_ctx_factory)
    ctx.mot_config(n_init=1, max_age=3, budget=2, feat_dim=8, max_tracks=5)
    with pytest.raises(DvinsError, match="0..64"):
        ctx.mot_update(np.zeros((65, 4), np.float32), np.zeros((65, 8), np.float32))
    with pytest.raises(DvinsError, match="finite"):
        ctx.mot_assign(np.array([[np.nan, 1.0]], np.float32))
    ctx.mot_update_enqueue(np.zeros((0, 4), np.float32), np.zeros((0, 8), np.float32), n=0)
    with pytest.raises(DvinsError, match="not collected"):
        ctx.mot_update_enqueue(np.zeros((0, 4), np.float32), np.zeros((0, 8), np.float32), n=0)
    ids, nt, nc = ctx.mot_update_collect()
    assert len(ids) == 0 and nt == 0 and nc == 0
