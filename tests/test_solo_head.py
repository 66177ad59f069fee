"""The detector head on the device (`-m gpu`): dv_solo_head_enqueue / _collect against tests/solo_ref.py, the reference's own lines in CPU torch.  For every case the test
computes from the reference alone: the float64 result (the yardstick) and delta, the largest deviation between the float32 and the float64 reference's resampled values.
  n, labels, plane order      equal float64 exactly
  scores                      within 1e-4 relative of float64: float32 tree sums of <= 27 648 terms in [0.5, 1] and a few-ulp expf give about 1e-6, two orders of margin; the
                              generator's 1e-3 spacing keeps the order independent of it
  plane pixels                equal float64 wherever its resampled value is at least 4 delta from mask_thr (4: a second float32 evaluation order of the same two lerps); no
                              plane may have more than 1 % of its pixels inside that band
  padding bytes               zero
  the stack                   fed to dv_inst_stack_frame_enqueue / _collect gives what tests/test_inst_stack.py's torch_reference / expected_dets give for the head's planes
What this module reaches: random blob masks (every IoU, decay chains of many candidates) from solo_ref.make_case, channels 128 / 12, feature 24 x 72 (whole waves, whole
words) / 7 x 13 (word, wave and row tails), grids 5 4 3 2 2 against num_grids 2 2 3 4 5 (boundaries inside a level) with a flat and a position-dependent stride table,
80 / 3 classes, three origins, both rect branches, candidate counts 1 / 63 / 65 / nms_pre + 4 / 72, survivors 1 / max_per_img / max_per_img + 3, both NMS kernels, three
memory kinds, two frames back to back, the three empty outcomes, one over-capacity frame, and the stack handed on to the stack stage and the pipeline.
What it does NOT reach, because make_case's random search finds no spaced scores beyond some 70 candidates: a second workgroup of cells or a second scan iteration (58
cells), more than 1024 candidates in the sort, more than 64 mask words, more than 80 sorted candidates or 2 NMS waves, an odd channel count or 256 channels, an origin wider
than 256, an upsampling second interpolation, a NaN, an exact tie, or the reference's own configuration.  Those are tests/test_solo_head_limits.py, on the constructed
inputs of tests/solo_cases.py, through the same check_against."""
import numpy as np
import pytest

from tests import solo_ref
from tests.test_inst_stack import expected_dets, stage_ctx, torch_reference
from tests.test_viode_live import download

pytestmark = pytest.mark.gpu

GRIDS = (5, 4, 3, 2, 2)
FLAT, BY_POS = (8, 8, 8, 8, 8), (4, 8, 16, 32, 32)
# channels, (fh, fw), classes, origin (w, h), model (w, h), strides, candidates, survivors asked, NMS kernel, memory
CASES = [
    (128, (24, 72), 80, (70, 23), (288, 96), FLAT, 63, 8, "gaussian", "device"),
    (12, (7, 13), 3, (64, 4), (52, 28), BY_POS, 65, 11, "linear", "host"),
    (12, (24, 72), 3, (67, 5), (288, 96), BY_POS, 52, 1, "gaussian", "pinned"),
    (128, (7, 13), 80, (70, 23), (50, 14), FLAT, 72, 8, "linear", "device"),
    (12, (7, 13), 3, (67, 5), (52, 28), FLAT, 1, 1, "gaussian", "host"),
    (12, (24, 72), 80, (64, 4), (288, 10), BY_POS, 65, 11, "gaussian", "device"),
]
_REF = {}


def case_ref(case):
    """inputs, parameters, float64 reference and delta of a case — computed once, shared, never changed"""
    if case not in _REF:
        import torch
        from dynamic_vins_amd.frontend import solo_rect
        ch, (fh, fw), ncls, origin, model, strides, n_cand, n_surv, kern, _ = case
        par = solo_ref.params(strides=strides, nms_kernel=kern, rect=solo_rect(model[0], model[1], origin[0], origin[1]), origin=origin)
        inp, par, _ = solo_ref.make_case(ch, fh, fw, GRIDS, ncls, n_cand, n_surv, par, seed=CASES.index(case) + 1)
        r64, r32 = solo_ref.reference(inp, par, torch.float64), solo_ref.reference(inp, par, torch.float32)
        assert r64["n"] == r32["n"] > 0 and np.array_equal(r64["survivors"], r32["survivors"])
        delta = float(np.abs(r64["values"] - r32["values"].astype(np.float64)).max())
        if n_cand == par["nms_pre"] + 4:
            assert r64["n_floor"] > par["nms_pre"], "the first sort cuts nothing"
        _REF[case] = (inp, par, r64, delta)
    return _REF[case]


def device_outputs(inp, mem, keep):
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_PINNED, solo_outputs
    if mem == "host":
        return solo_outputs(inp["kernels"], inp["cates"], inp["feature"])
    put = (lambda a: torch.from_numpy(a).cuda()) if mem == "device" else (lambda a: torch.from_numpy(a).pin_memory())
    ks, cs, f = [put(k) for k in inp["kernels"]], [put(c) for c in inp["cates"]], put(inp["feature"])
    torch.cuda.synchronize()
    keep += ks + cs + [f]
    shapes = (f.shape[0], cs[0].shape[0], [k.shape[1] for k in ks], f.shape[1], f.shape[2])
    return solo_outputs([k.data_ptr() for k in ks], [c.data_ptr() for c in cs], f.data_ptr(), mem=DV_MEM_DEVICE if mem == "device" else DV_MEM_PINNED, shapes=shapes)


def to_params(par):
    from dynamic_vins_amd.frontend import solo_params
    return solo_params(**par)


def planes_of(st, n, w, h):
    pitch = (w + 3) // 4 * 4
    assert st.row_stride == pitch and st.plane_stride == pitch * h and st.n_planes == min(n, 64)
    raw = download(st.data, n * h * pitch).reshape(n, h, pitch)
    assert not raw[:, :, w:].any(), "padding bytes of the output rows are not zero"
    return raw[:, :, :w]


def check_frame(ctx, case, mem, keep):
    inp, par, r64, delta = case_ref(case)
    return check_against(ctx, inp, par, r64, delta, mem, keep, f"case {CASES.index(case)}")[:2]


def check_against(ctx, inp, par, r64, delta, mem, keep, tag):
    """one frame on the device against a float64 reference and its delta: THE checks of this stage (tests/test_solo_head_limits.py runs its cases through them too)"""
    w, h = par["origin"]
    labels, scores, st, n_pass = ctx.solo_head(device_outputs(inp, mem, keep), to_params(par))
    print(f"{tag} {mem}: n {len(labels)} (ref {r64['n']}), cells over score_thr {n_pass}, delta {delta:.3g}")
    assert n_pass == r64["n_pass"] and len(labels) == r64["n"] and np.array_equal(labels, r64["labels"])
    rel = np.abs(scores.astype(np.float64) - r64["scores"]) / r64["scores"]
    print("  largest relative score deviation", rel.max())
    assert rel.max() <= 1e-4
    planes = planes_of(st, r64["n"], w, h)
    assert set(np.unique(planes)) <= {0, 1}
    band = np.abs(r64["values"] - par["mask_thr"]) < 4 * delta
    frac = band.reshape(len(band), -1).mean(1)
    print("  pixels in the band per plane (max)", frac.max(), "differing outside the band", int(((planes != 0) != r64["planes"])[~band].sum()))
    assert frac.max() <= 0.01, "more than 1 % of a plane's pixels lie within 4 delta of mask_thr"
    assert np.array_equal((planes != 0)[~band], r64["planes"][~band])
    return planes, st, labels, scores


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"c{c[0]}_f{c[1][0]}x{c[1][1]}_k{c[2]}_o{c[3][0]}x{c[3][1]}_n{c[6]}_{c[8]}_{c[9]}")
def test_head_equals_the_reference(gpu_ctx_factory, case):
    """one frame of each case, then the head's own stack through the existing stack stage: bit equality with the reference's formulas on the head's planes"""
    w, h = case[3]
    ctx, keep = stage_ctx(gpu_ctx_factory, w, h), []
    planes, st = check_frame(ctx, case, case[9], keep)
    ctx.inst_stack_frame_enqueue(st)
    dets, inv_p, mrg_p = ctx.inst_stack_frame_collect(min_inst_size=2)
    _, merged, inv, boxes = torch_reference(planes, "u8")
    assert np.array_equal(download(mrg_p, w * h).reshape(h, w), merged) and np.array_equal(download(inv_p, w * h).reshape(h, w), inv)
    assert [(d["plane"], d["track_id"], d["rect"]) for d in dets] == expected_dets(boxes, 2)


def test_two_frames_back_to_back_and_memory_kinds(gpu_ctx_factory):
    """frame k's planes stay intact while frame k + 1 is enqueued and collected (the alternating sets); the three memory kinds give the same planes"""
    a, b = CASES[0], CASES[3]                                                   # both 70 x 23
    ctx, keep = stage_ctx(gpu_ctx_factory, 70, 23), []
    pa, st_a = check_frame(ctx, a, "device", keep)
    pb, st_b = check_frame(ctx, b, "pinned", keep)
    assert st_a.data != st_b.data
    assert np.array_equal(planes_of(st_a, len(pa), 70, 23), pa), "frame k's planes changed when frame k + 1 ran"
    for mem in ("host", "pinned"):
        pc, _ = check_frame(ctx, a, mem, keep)
        assert np.array_equal(pc, pa)


def test_empty_outcomes_and_over_capacity(gpu_ctx_factory):
    """the reference's three early returns give zero planes, not an error; more cells over score_thr than max_candidates fail loudly at collect, with no planes"""
    from dynamic_vins_amd._abi import DvinsError
    case = CASES[1]
    inp, par, r64, _ = case_ref(case)
    ctx, keep = stage_ctx(gpu_ctx_factory, *case[3]), []
    import torch
    for change, stage in ((dict(score_thr=5.0), "n_pass"), (dict(strides=(1e6,) * 5), "n_floor"), (dict(update_thr=10.0), "n")):
        p = dict(par, **change)
        ref = solo_ref.reference(inp, p, torch.float64)
        assert ref["n"] == 0 and ref[stage] == 0 and (stage == "n_pass" or ref["n_pass"] > 0)
        labels, scores, st, n_pass = ctx.solo_head(device_outputs(inp, "host", keep), to_params(p))
        assert len(labels) == 0 and st.n_planes == 0 and n_pass == ref["n_pass"]
    with pytest.raises(DvinsError, match="max_candidates"):
        ctx.solo_head(device_outputs(inp, "host", keep), to_params(dict(par, max_candidates=r64["n_pass"] - 1)))
    labels, _, _, _ = ctx.solo_head(device_outputs(inp, "host", keep), to_params(par))          # the ctx goes on with the next frame
    assert np.array_equal(labels, r64["labels"])


def test_more_survivors_than_the_stack_names(gpu_ctx_factory):
    """max_per_img 70 and 72 candidates of distinct labels (no decay): collect reports all n = 70 survivors with labels and scores, the stack names the first 64 planes"""
    import torch
    from dynamic_vins_amd.frontend import solo_rect
    par = solo_ref.params(max_per_img=70, nms_pre=72, rect=solo_rect(52, 28, 70, 23), origin=(70, 23))
    inp, par, _ = solo_ref.make_case(12, 7, 13, GRIDS, 80, 72, 0, par, seed=79)
    par["update_thr"] = 1e-6
    r64 = solo_ref.reference(inp, par, torch.float64)
    assert r64["n"] == 70 and r64["n_floor"] > 70 and solo_ref.relative_gaps(r64["scores"]) >= solo_ref.SPACING
    ctx, keep = stage_ctx(gpu_ctx_factory, 70, 23), []
    labels, scores, st, _ = ctx.solo_head(device_outputs(inp, "device", keep), to_params(par))
    assert len(labels) == 70 and st.n_planes == 64 and np.array_equal(labels, r64["labels"])
    assert (np.abs(scores.astype(np.float64) - r64["scores"]) / r64["scores"]).max() <= 1e-4
    raw = download(st.data, 70 * 23 * 72).reshape(70, 23, 72)                   # all 70 planes are in memory behind the 64 the stack names
    delta = float(np.abs(r64["values"] - solo_ref.reference(inp, par, torch.float32)["values"].astype(np.float64)).max())
    band = np.abs(r64["values"] - par["mask_thr"]) < 4 * delta
    assert band.reshape(70, -1).mean(1).max() <= 0.01 and np.array_equal((raw[:, :, :70] != 0)[~band], r64["planes"][~band]) and not raw[:, :, 70:].any()


# ------------------------------------------------------------------ the pipeline ------------------------------------------------------------------
def scene_head(seq, log):
    """network outputs that make the head reproduce a rendered scene's instances: feature channel j = +1 inside dynamic key j's pixels (every 4th pixel), -1 outside, the
    last channel the constant 1; cell j of the one level selects channel j with bias 1/8 (logit 9/8 or -7/8) and scores class j with 0.9 - 0.05 j -> one plane per key
    present, track id = the key.  `log` receives (k, planes as a device tensor, track ids) from the ids call: what DynamicPipeline(mask_stack=True) is fed afterwards"""
    import torch
    from dynamic_vins_amd import viode
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, solo_outputs, solo_params
    keys = [int(v) for v in seq.dyn_keys]
    nk, g = len(keys), int(np.ceil(np.sqrt(len(keys))))
    w, h = seq.w, seq.h
    assert w % 4 == 0 and h % 4 == 0 and nk <= 16
    kern = np.zeros((nk + 1, g, g), np.float32); cate = np.full((nk, g, g), 0.01, np.float32)
    for j in range(nk):
        kern[j].reshape(-1)[j] = 1.0; kern[nk].reshape(-1)[j] = 0.125; cate[j].reshape(-1)[j] = 0.9 - 0.05 * j
    kern_d, cate_d = torch.from_numpy(kern).cuda(), torch.from_numpy(cate).cuda()
    par = solo_params(score_thr=0.1, mask_thr=0.5, update_thr=0.05, nms_pre=16, max_per_img=16, num_grids=(g,), strides=(8.0,), max_candidates=16, rect=(0, 0, w, h), origin=(w, h))
    feats = {}

    def source(k):
        if k not in feats:
            sg = seq.seg0[k]
            kimg = viode.pixel_to_key(sg[..., 2], sg[..., 1], sg[..., 0])[::4, ::4]
            f = np.stack([np.where(kimg == key, 1.0, -1.0) for key in keys] + [np.ones_like(kimg, np.float64)]).astype(np.float32)
            feats[k] = torch.from_numpy(np.ascontiguousarray(f)).cuda()
            torch.cuda.synchronize()
        out = solo_outputs([kern_d.data_ptr()], [cate_d.data_ptr()], feats[k].data_ptr(), mem=DV_MEM_DEVICE, shapes=(nk + 1, nk, [g], h // 4, w // 4))

        def ids(labels, scores, st):
            tid = np.array([keys[int(l)] for l in labels], np.int64)
            planes = torch.from_numpy(download(st.data, len(labels) * h * w).reshape(len(labels), h, w).copy()).cuda()
            log.append((k, planes, tid))
            return tid, np.zeros(len(labels), np.int32)
        return out, par, ids
    return source


def test_pipeline_head_equals_mask_stack_fed_the_same_planes():
    """DynamicPipeline(solo_head=...) over a short rendered sequence against DynamicPipeline(mask_stack=True) fed the head's own planes and ids: background and object rows of every step, trajectory, object
    states and statistics bit for bit — the head's stack goes through dv_inst_stack_frame_*, dv_track_unmask_static_planes and dv_inst_track_enqueue_planes unchanged.  solo_head is
    refused together with live_masks"""
    import copy
    from dynamic_vins_amd.pipeline import DynamicPipeline
    from tests.test_inst_stack import KW, runner_sequence
    seq, log, steps = runner_sequence(), [], 12
    with pytest.raises(ValueError, match="solo_head"):
        DynamicPipeline(seq, live_masks=True, solo_head=lambda k: None, **KW)
    out = []
    p = DynamicPipeline(seq, solo_head=scene_head(seq, log), **KW)
    rows = []
    for _ in range(steps):
        p.step()
        rows.append((p.rows.tobytes(), np.asarray(p.ifeats).tobytes()))
    I, S = p.est.instances()
    out.append((rows, np.asarray(p.poses).tobytes(), I.tobytes(), np.asarray(S).tobytes(), dict(p.stat)))
    p.ctx.close()
    assert [k for k, _, _ in log] == list(range(len(log))) and len(log) > steps and all(len(t) >= 1 for _, _, t in log)
    fed = copy.copy(seq)
    n = len(seq.frames)
    pad = [log[-1][1]] * (n - len(log))
    fed.mask_stacks = [pl for _, pl, _ in log] + pad
    fed.stack_track_ids = [t for _, _, t in log] + [log[-1][2]] * len(pad)
    fed.stack_class_ids = [np.zeros(len(t), np.int32) for t in fed.stack_track_ids]
    q = DynamicPipeline(fed, mask_stack=True, **KW)
    rows = []
    for _ in range(steps):
        q.step()
        rows.append((q.rows.tobytes(), np.asarray(q.ifeats).tobytes()))
    I, S = q.est.instances()
    out.append((rows, np.asarray(q.poses).tobytes(), I.tobytes(), np.asarray(S).tobytes(), dict(q.stat)))
    q.ctx.close()
    assert out[0][4]["object_features"] > 50, out[0][4]
    assert out[0] == out[1]
