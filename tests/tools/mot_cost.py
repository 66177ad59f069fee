"""Cost of the multi-object tracker stage, measured not asserted: enqueue -> collect at 20 detections / 40 tracks and at 64 / 128 with budget 100 and feat_dim 512
(the reference's YAML).  The stage's kernels are timed by the ctx's HIP events ("mot": mot_feat_kernel + mot_assoc_kernel); the wall time of enqueue + collect,
which adds the launch, the copy of the ids and the wait, is given beside it.  Writes profiles/mot_cost.json.

    python tests/tools/mot_cost.py [--frames 60] [--out profiles/mot_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def case(ctx, n_det, n_trk, frames):
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE
    import torch
    rng = np.random.default_rng(0)
    ctx.mot_config(n_init=3, max_age=1 << 20, budget=100, feat_dim=512, max_tracks=128)
    proto = rng.standard_normal((n_trk, 512))
    proto /= np.linalg.norm(proto, axis=1, keepdims=True)
    boxes = np.array([[(i % 16) * 120.0, (i // 16) * 110.0, 60, 80] for i in range(n_trk)], np.float32)

    groups = max(1, n_trk // n_det)

    def frame(k):
        # every group of n_det objects is shown 5 frames in a row first (a Tentative track dies on its first miss), then the groups take turns
        g = (k // 5) % groups if k < 5 * groups else k % groups
        shown = np.arange(n_det) + g * n_det
        f = proto[shown] + 0.004 * rng.standard_normal((n_det, 512))
        return boxes[shown] + rng.uniform(-0.5, 0.5, (n_det, 4)).astype(np.float32), (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)

    warm = 5 * groups + 104 * groups      # every track Confirmed and its ring of 100 rows full
    for k in range(warm):
        ctx.mot_update(*frame(k))
    ctx.timing_enable(1)
    ctx.timing_reset()
    wall = []
    for k in range(frames):
        r, f = frame(warm + k)
        rd, fd = torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids, nt, nc = ctx.mot_update(rd.data_ptr(), fd.data_ptr(), n=n_det, mem=DV_MEM_DEVICE)
        wall.append((time.perf_counter() - t0) * 1e3)
    ms, cnt = ctx.timing_get("mot")
    ctx.timing_enable(0)
    return dict(detections=n_det, tracks=int(nt), confirmed=int(nc), matched=int((ids >= 0).sum()), frames=frames, kernels_ms_mean=ms / max(cnt, 1),
                wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mot_cost.json"))
    a = ap.parse_args()
    import torch
    torch.zeros(1).cuda()      # the tensor library takes the device first, as in the suite
    from dynamic_vins_amd.frontend import Context, make_cam
    ctx = Context(width=64, height=48, cam0=make_cam(100, 100, 32, 24), cam1=make_cam(100, 100, 32, 24))
    res = dict(tool="tests/tools/mot_cost.py", budget=100, feat_dim=512, cases=[case(ctx, 20, 40, a.frames), case(ctx, 64, 128, a.frames)])
    print(json.dumps(res))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
