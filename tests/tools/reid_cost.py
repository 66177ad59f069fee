"""Cost of the ReID extractor stage, measured not asserted: dv_reid_extract_enqueue -> _collect (crops, network, tail; image and rectangles already on the device) on the
host clock, median of 20 with min and max, at 128 x 64 for 8, 20 and 64 crops out of a 1242 x 375 image.  In the same process and alternating with it, the same network
run by torch in float32 on the same GPU from the same prepared input, after its own warm-up (its library's first-call tuning stays outside the timed calls).  The
achieved share of the 157 TFLOP/s float32 matrix peak follows from the network's multiply-adds as arithmetic.  Writes profiles/reid_cost.json.

    python tests/tools/reid_cost.py [--reps 20] [--out profiles/reid_cost.json]
    python tests/tools/reid_cost.py --one 64        # five frames of 64 crops and nothing else: the run to put under a kernel trace"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 1242, 375
PEAK_TFLOPS = 157.3


def flops_per_crop(in_w=64, in_h=128):
    """2 x multiply-adds of every convolution at the maps' sizes"""
    from tests import reid_ref as rr
    half = lambda n: (n + 1) // 2
    f = 2 * 27 * 64 * in_w * in_h
    h, w = half(in_h), half(in_w)
    for ci, co, down in rr.BLOCKS:
        if down:
            h, w = half(h), half(w)
            f += 2 * ci * co * h * w
        f += 2 * 9 * ci * co * h * w + 2 * 9 * co * co * h * w
    return f


def torch_net(flat):
    import torch
    import torch.nn.functional as F
    from tests import reid_ref as rr
    P = {k: torch.from_numpy(v.copy()).cuda() for k, v in rr.split(flat).items()}
    bn = lambda t, name: F.batch_norm(t, P[name + ".running_mean"], P[name + ".running_var"], P[name + ".weight"], P[name + ".bias"], False, 0.0, rr.EPS)

    def forward(t):
        with torch.no_grad():
            t = torch.relu(bn(F.conv2d(t, P["conv1.0.weight"], P["conv1.0.bias"], stride=1, padding=1), "conv1.1"))
            t = F.max_pool2d(t, 3, 2, 1)
            for i, (ci, co, down) in enumerate(rr.BLOCKS):
                p = f"conv2.{i}."
                y = torch.relu(bn(F.conv2d(t, P[p + "conv.0.weight"], stride=2 if down else 1, padding=1), p + "conv.1"))
                y = bn(F.conv2d(y, P[p + "conv.3.weight"], stride=1, padding=1), p + "conv.4")
                if down:
                    t = bn(F.conv2d(t, P[p + "downsample.0.weight"], stride=2), p + "downsample.1")
                t = torch.relu(t + y)
            t = F.avg_pool2d(t, (8, 4), 1).flatten(1)
            return t / t.norm(2, 1, True)
    return forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reid_cost.json"))
    a = ap.parse_args()
    import torch
    torch.zeros(1).cuda()
    from dynamic_vins_amd.frontend import Context, make_cam, DV_MEM_DEVICE
    from tests import reid_cases as rc
    ctx = Context(width=W, height=H, cam0=make_cam(700, 700, W / 2, H / 2), cam1=make_cam(700, 700, W / 2, H / 2))
    ctx.reid_load(rc.weights(0))
    img = torch.from_numpy(np.ascontiguousarray(rc.image(W, H, seed=9))).cuda()
    torch.cuda.synchronize()

    def ours(rects):
        t0 = time.perf_counter()
        ctx.reid_extract_enqueue(img.data_ptr(), rects, n=len(rects), mem=DV_MEM_DEVICE, stride=3 * W)
        ctx.reid_extract_collect()
        return (time.perf_counter() - t0) * 1e3

    if a.one:
        rects = rc.rects(a.one, W, H, min_w=30, min_h=60)
        for _ in range(5):
            ours(rects)
        ctx.close()
        return
    net, gflop = torch_net(rc.weights(0)), flops_per_crop() / 1e9
    cases = []
    for n in (8, 20, 64):
        rects = rc.rects(n, W, H, min_w=30, min_h=60)
        for _ in range(3):
            ours(rects)
        x = torch.from_numpy(ctx.reid_input(n).copy()).cuda()
        for _ in range(5):      # the tensor library's warm-up at this batch size
            e = net(x)
        torch.cuda.synchronize()
        dev = np.abs(e.cpu().numpy() - ctx.reid_feats(n)).max()
        mine, theirs = [], []
        for _ in range(a.reps):
            mine.append(ours(rects))
            t0 = time.perf_counter()
            net(x)
            torch.cuda.synchronize()
            theirs.append((time.perf_counter() - t0) * 1e3)
        s = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
        cases.append(dict(crops=n, reps=a.reps, device_ms=s(mine), torch_ms=s(theirs), largest_difference_to_torch=float(dev), gflop=gflop * n,
                          share_of_f32_matrix_peak=gflop * n / np.median(mine) / PEAK_TFLOPS))
    res = dict(tool="tests/tools/reid_cost.py", image=[W, H], input=[64, 128], gflop_per_crop=gflop, peak_tflops=PEAK_TFLOPS,
               note="device_ms: enqueue -> collect on the host clock, crops included; torch_ms: the network alone on the prepared input", cases=cases)
    print(json.dumps(res))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
