"""Aggregate frames/s of a dv_runner group of 16 EuRoC-size sequences (752x480, stereo) whose members track in shared launches (dv_batch_track_enqueue), in three
variants:
    n  every member in DV_MODE_NAIVE with a per-frame instance mask (dv_runner_set_mask: TrackImageNaive over the sequence; device masks next to the device frames);
    h  members 0, 2, 4, ... naive with masks, the others raw;
    r  every member raw (gray frames, no mask).
One process alternates n, h, r, n, h, r, ... for `--reps` repetitions each (default 5); a repetition builds fresh pipelines over the same rendered frames and masks,
runs 20 warm-up frames and times the next 100 with dv_runner_run's own wall clock.  Every repetition, the medians and the spread (min - max) go to the output file.
Uses nothing newer than dv_runner_set_mask, so the same file measures the commits before and after the naive members joined the group's launches.
    python tests/tools/group_naive_cost.py [--out profiles/group_naive_cost.json] [--reps 5] [--only n] [--frames 100]      (--only: one variant, for a run under a profiler)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                                       # noqa: E402
import torch                                                             # noqa: E402

from dynamic_vins_amd import sim                                         # noqa: E402
from dynamic_vins_amd.backend import DvinsError, Runner                  # noqa: E402
from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MODE_NAIVE       # noqa: E402
from dynamic_vins_amd.pipeline import Pipeline, SyntheticSequence        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_naive_cost.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="", help="run only this variant (n, h or r)")
ap.add_argument("--frames", type=int, default=100)
args = ap.parse_args()

S, W, H, WARM, FRAMES = 16, 752, 480, 20, args.frames
CAM1 = dict(fx=457.587, fy=456.134, cx=379.999, cy=255.238, k1=-0.28368365, k2=0.07451284, p1=-0.00010473, p2=-3.555907e-05)
NF = WARM + FRAMES + 2
seqs = [SyntheticSequence(W, H, sim.EUROC, NF, rate=20.0, phase=0.7 * i, cam1=CAM1) for i in range(S)]


def mask(i, k):
    """member i's inverse instance mask of frame k (0 = object): one object a quarter of the image wide that moves 6 px per frame"""
    m = np.full((H, W), 255, np.uint8)
    x0 = (37 * i + 6 * k) % (W - W // 4)
    m[H // 6: H - H // 6, x0: x0 + W // 4] = 0
    return m


masks = [[torch.from_numpy(mask(i, k)).cuda() for k in range(NF)] for i in range(S)]
mask_ptrs = [(C.c_void_p * NF)(*[m.data_ptr() for m in masks[i]]) for i in range(S)]


def one(variant):
    pipes = [Pipeline(q, max_cnt=150, min_dist=30, max_iters=8, use_imu=1) for q in seqs]
    r = Runner(pipes, group_size=S, threads=1)
    for i in range(S):
        if variant == "n" or (variant == "h" and i % 2 == 0):
            if r.lib.dv_runner_set_mask(r.h, i, C.cast(mask_ptrs[i], C.c_void_p), DV_MEM_DEVICE, DV_MODE_NAIVE) != 0:
                raise DvinsError(r.lib.dv_runner_error(r.h).decode())
    r.run(WARM)
    wall = r.run(FRAMES)
    info = r.track_info()
    r.close()
    for p in pipes:
        p.ctx.close()
    return S * FRAMES / wall, info


variants = [v for v in "nhr" if not args.only or v == args.only]
reps = {v: [] for v in variants}
infos = {}
for k in range(args.reps):
    for v in variants:
        fps, infos[v] = one(v)
        reps[v].append(round(fps, 2))
        print("repetition %d variant %s: %.1f frames/s %s" % (k, v, fps, infos[v]), flush=True)
res = {"what": "aggregate frames/s of Runner(group_size=16) over 16 sequences at 752x480, %d frames timed after %d warm-up frames; n: every member naive with a "
               "mask, h: every second member naive with a mask, r: every member raw" % (FRAMES, WARM),
       "sequences": S, "size": [W, H], "repetitions": args.reps, "variants": {}}
for v in variants:
    res["variants"][v] = dict(frames_per_s=reps[v], median=round(statistics.median(reps[v]), 2), min=min(reps[v]), max=max(reps[v]), track_info=infos[v])
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(res, open(args.out, "w"), indent=1)
