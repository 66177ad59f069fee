"""DynamicPipeline(mask_stack=True, mot=("device", params)) (`-m gpu`): the device extractor between the stack stage and the device tracker, on the rendered 640 x 360
scene of tests/test_mot_pipeline.py.  The comparison run is the callable form, its callable returning Context.reid_extract of the same image (downloaded, so it takes
the staged path) and the same rectangles: track ids, background rows, object rows and features of every step, trajectory, object states and statistics are equal bit
for bit.  This checks the hand-over of the device pointer; it makes no claim about what random weights can tell apart (pairwise cosine distances of crops under them are
near 1e-3, far inside the 0.2 gate: the IoU gates do the separating here)."""
import numpy as np
import pytest

from tests import reid_cases as rc

PAR = dict(n_init=1, max_age=3, budget=8, feat_dim=512, max_tracks=32)
STEPS = 12


def run(seq, device_form):
    import torch
    from dynamic_vins_amd.pipeline import DynamicPipeline
    from tests.test_inst_stack import KW
    box, log = {}, {}

    def feats(k, dets, stack):
        p = box["p"]
        if "loaded" not in box:
            p.ctx.reid_load(rc.weights(0))
            box["loaded"] = True
        img = p.reid_image(k).cpu().numpy()
        e = p.ctx.reid_extract(img, np.array([d["rect"] for d in dets], np.float32))
        log[k] = e
        return torch.from_numpy(e).cuda()

    mot = ("device", dict(PAR, reid_weights=rc.weights(0))) if device_form else (feats, dict(PAR))
    p = box["p"] = DynamicPipeline(seq, mask_stack=True, mot=mot, **KW)
    per_step = []
    for _ in range(STEPS):
        p.step()
        per_step.append((np.asarray(p.rows).tobytes(), np.asarray(p.insts).tobytes(), np.asarray(p.ifeats).tobytes()))
    I, S = p.est.instances()
    tracks = p.ctx.mot_tracks()
    out = dict(per_step=per_step, poses=np.asarray(p.poses).tobytes(), inst=I.tobytes(), states=np.asarray(S).tobytes(), stat=dict(p.stat),
               ids=sorted(set(int(v) for v in I["id"])) if len(I) else [], tracks=tracks.tobytes(), n_conf=int((tracks["state"] == 1).sum()), log=log)
    p.ctx.close()
    return out


@pytest.mark.gpu
def test_device_form_equals_the_callable_form():
    from tests.test_inst_stack import runner_sequence
    seq = runner_sequence()
    got, ref = run(seq, True), run(seq, False)
    assert len(ref["log"]) >= STEPS - 2 and all(np.isfinite(e).all() and e.shape[1] == 512 for e in ref["log"].values())
    assert ref["n_conf"] >= 2 and ref["stat"]["object_features"] > 50 and ref["ids"], ref["stat"]
    for k, (a, b) in enumerate(zip(got["per_step"], ref["per_step"])):
        assert a == b, f"step {k}: rows differ"
    for name in ("poses", "inst", "states", "stat", "ids", "tracks"):
        assert got[name] == ref[name], name
