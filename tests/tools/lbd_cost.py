"""Cost of the LBD stage on one GPU: 752 x 480 stereo, 200 lines of 60 - 400 pixels per image, images in device memory, lines in host memory; both images enqueued
(cam 0 / 1), then both collected.  10 untimed frames, then the host clock around enqueue -> collect: median of 20 with min and max -> profiles/lbd_cost.json.  No bar is
set and there is nothing to race: the numbers are reported as measured.  The kernels' own times (profiles/lbd_cost_kernel_stats.csv) are the statistics of one kernel
trace of this very tool, `rocprofv3 --kernel-trace --stats -- python tests/tools/lbd_cost.py --out <scratch file>`, a run of its own with no counters (dispatches are
serialised under the profiler, so its wall clock is not recorded); their resources are the compiler's -Rpass-analysis=kernel-resource-usage remarks.
    python tests/tools/lbd_cost.py [--frames 20] [--out profiles/lbd_cost.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dynamic_vins_amd.frontend import Context, DV_MEM_DEVICE, DV_MEM_HOST

W, H, N = 752, 480, 200


def make_lines(rng):
    L = np.zeros((N, 6), np.float32)
    for i in range(N):
        n, a = int(rng.integers(60, 401)), float(rng.uniform(-math.pi, math.pi))
        c, s = math.cos(a), math.sin(a)
        half = (n - 1) / (2 * max(abs(c), abs(s)))
        cx, cy = float(rng.uniform(0, W)), float(rng.uniform(0, H))
        L[i] = (cx - half * c, cy - half * s, cx + half * c, cy + half * s, a, 2 * half)
    return L


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbd_cost.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(5)
    imgs = [torch.from_numpy(rng.integers(0, 256, (H, W), dtype=np.uint8)).cuda() for _ in range(2)]
    lines = [make_lines(rng), make_lines(rng)]
    torch.cuda.synchronize()
    ctx = Context(width=W, height=H)

    def frame():
        t0 = time.perf_counter()
        for cam in (0, 1):
            ctx.lbd_describe_enqueue(cam, imgs[cam].data_ptr(), lines[cam], min_length=60.0, size=(W, H), stride=W, mem=DV_MEM_DEVICE, lines_mem=DV_MEM_HOST)
        kept = [ctx.lbd_describe_collect(cam, host=False)["n"] for cam in (0, 1)]
        return (time.perf_counter() - t0) * 1e3, kept

    for _ in range(10):
        frame()
    ms = []
    for _ in range(args.frames):
        dt, kept = frame()
        ms.append(dt)
    ctx.close()
    px = sum(int(np.sum(np.maximum(np.abs(np.rint(l[:, 2]) - np.rint(l[:, 0])), np.abs(np.rint(l[:, 3]) - np.rint(l[:, 1]))) + 1)) for l in lines)
    rec = {"shape": [W, H], "lines_per_image": N, "line_pixels": [60, 400], "frames": args.frames, "kept": kept,
           "enqueue_to_collect_ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))},
           "bytes_per_frame_arithmetic": {"gradients_in": 2 * W * H, "gradients_out": 2 * 4 * W * H, "describe_gathers": 63 * px * 4, "upload_avoided": 2 * N * 32}}
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
