"""DynamicPipeline(mask_stack=True, mot=...) (`-m gpu` but for the refusals): the device tracker between the stack stage and the plane entries, on the rendered escort
scene of the mask-stack tests with embeddings that are one-hot per true object.  The comparison run is the existing track_id path fed the ground truth: every plane
carries its object's id from the frame at which the tracker confirms it — n_init + 2 consecutive detections, ids by first appearance, computed here from the planes
present per frame alone — and -1 (absent) before, as the reference leaves an unconfirmed object out.  Background rows, object rows and features of every step,
trajectory, object states and statistics are then bit-identical.  With mot=None the run equals one without the keyword."""
import numpy as np
import pytest

PAR = dict(n_init=1, max_age=3, budget=8, feat_dim=16, max_tracks=32)
STEPS = 12


def test_mot_refusals():
    from dynamic_vins_amd.pipeline import DynamicPipeline
    f = (lambda k, dets, stack: None, dict(PAR))
    for kw in (dict(), dict(live_masks=True)):
        with pytest.raises(ValueError, match="mot"):
            DynamicPipeline(None, mot=f, **kw)
    for bad in (lambda k, d, s: None, (None, dict(PAR)), (f[0], None)):
        with pytest.raises(ValueError, match="mot must be"):
            DynamicPipeline(None, mask_stack=True, mot=bad)


def run(seq, track_ids=None, steps=STEPS, **kw):
    from dynamic_vins_amd.pipeline import DynamicPipeline
    from tests.test_inst_stack import KW
    p = DynamicPipeline(seq, mask_stack=True, **KW, **kw)
    if track_ids is not None:
        p.stack_input()["track_ids"] = track_ids
    per_step = []
    for _ in range(steps):
        p.step()
        per_step.append((np.asarray(p.rows).tobytes(), np.asarray(p.insts).tobytes(), np.asarray(p.ifeats).tobytes()))
    I, S = p.est.instances()
    out = dict(per_step=per_step, poses=np.asarray(p.poses).tobytes(), inst=I.tobytes(), states=np.asarray(S).tobytes(), stat=dict(p.stat), ids=sorted(set(int(v) for v in I["id"])) if len(I) else [])
    p.ctx.close()
    return out


@pytest.mark.gpu
def test_pipeline_with_the_device_tracker_equals_the_ground_truth_ids():
    import torch
    from tests.test_inst_stack import runner_sequence
    seq, log = runner_sequence(), {}

    def feats(k, dets, stack):
        e = np.zeros((len(dets), PAR["feat_dim"]), np.float32)
        for i, d in enumerate(dets):
            e[i, d["plane"]] = 1.0
        log[k] = [d["plane"] for d in dets]
        return torch.from_numpy(e).cuda()

    got = run(seq, mot=(feats, dict(PAR)))
    frames = sorted(log)
    n_planes = len(seq.dyn_keys)
    assert frames == list(range(frames[-1] + 1)) and frames[-1] >= STEPS - 1 and n_planes <= PAR["feat_dim"]
    # the ground truth's answer: a plane present without a break is confirmed at its (n_init + 2)-th detection; ids in that order, planes ascending within a frame
    first = {}
    for k in frames:
        for pl in log[k]:
            first.setdefault(pl, k)
    for pl, f0 in first.items():
        assert all(pl in log[k] for k in frames if k >= f0), "the scene hides an object: the simple confirmation rule of this test does not cover it"
    conf = {pl: f0 + PAR["n_init"] + 1 for pl, f0 in first.items()}
    order = sorted(conf, key=lambda pl: (conf[pl], pl))
    ident = {pl: 1 + i for i, pl in enumerate(order)}
    assert len(order) >= 2 and min(conf.values()) < STEPS - 4
    n_frames = len(seq.frames)
    tids = [np.array([ident[pl] if pl in conf and k >= conf[pl] else -1 for pl in range(n_planes)], np.int32) for k in range(n_frames)]
    ref = run(seq, track_ids=tids, mot=None)
    assert ref["stat"]["object_features"] > 50 and ref["stat"]["frames_with_objects"] >= STEPS - min(conf.values()) - 1 and ref["ids"], ref["stat"]
    for k, (a, b) in enumerate(zip(got["per_step"], ref["per_step"])):
        assert a == b, f"step {k}: rows differ"
    for name in ("poses", "inst", "states", "stat", "ids"):
        assert got[name] == ref[name], name
    # mot=None changes nothing: the same run without the keyword
    plain = run(seq, track_ids=tids, steps=6)
    assert plain["per_step"] == ref["per_step"][:6]
