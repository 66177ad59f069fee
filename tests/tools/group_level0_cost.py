"""Aggregate frames/s of a dv_runner group of 16 EuRoC-size sequences (752x480, stereo, EuRoC's distortion) whose members track in shared launches
(dv_batch_track_enqueue), in three variants:
    a  every member with undistort_input (maps installed by dv_undistort_setup, distorted frames remapped into pyramid level 0);
    b  every member plain (gray frames, no maps);
    c  as a, with the runner's "batch_front" switch off: one set of tracking launches per sequence.
One process alternates a, b, c, a, b, c, ... for `--reps` repetitions each (default 5); a repetition builds fresh pipelines over the same rendered frames, runs 20
warm-up frames and times the next 100 with dv_runner_run's own wall clock.  Every repetition, the medians and the spread (max - min) go to the output file.  Uses
nothing newer than Pipeline(undistort_input=...) and Runner.set("batch_front", ...), so the same file measures the commits before and after the group's level-0 stage.
    python tests/tools/group_level0_cost.py [--out profiles/group_level0_cost.json] [--reps 5] [--only a]      (--only: one variant, for a run under a profiler)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dynamic_vins_amd import sim                                         # noqa: E402
from dynamic_vins_amd.backend import Runner                              # noqa: E402
from dynamic_vins_amd.pipeline import Pipeline, SyntheticSequence        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_level0_cost.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="", help="run only this variant (a, b or c)")
args = ap.parse_args()

S, W, H, WARM, FRAMES = 16, 752, 480, 20, 100
CAM1 = dict(fx=457.587, fy=456.134, cx=379.999, cy=255.238, k1=-0.28368365, k2=0.07451284, p1=-0.00010473, p2=-3.555907e-05)
seqs = [SyntheticSequence(W, H, sim.EUROC, WARM + FRAMES + 2, rate=20.0, phase=0.7 * i, cam1=CAM1) for i in range(S)]


def one(variant):
    pipes = [Pipeline(q, max_cnt=150, min_dist=30, max_iters=8, use_imu=1, undistort_input=(variant != "b")) for q in seqs]
    r = Runner(pipes, group_size=S, threads=1)
    if variant == "c":
        r.set("batch_front", 0)
    r.run(WARM)
    wall = r.run(FRAMES)
    info = r.track_info()
    r.close()
    for p in pipes:
        p.ctx.close()
    return S * FRAMES / wall, info


variants = [v for v in "abc" if not args.only or v == args.only]
reps = {v: [] for v in variants}
infos = {}
for k in range(args.reps):
    for v in variants:
        fps, infos[v] = one(v)
        reps[v].append(round(fps, 2))
        print("repetition %d variant %s: %.1f frames/s %s" % (k, v, fps, infos[v]), flush=True)
res = {"what": "aggregate frames/s of Runner(group_size=16) over 16 sequences at 752x480, %d frames timed after %d warm-up frames; a: undistort_input on every member, "
               "b: plain members, c: a with batch_front 0" % (FRAMES, WARM),
       "sequences": S, "size": [W, H], "repetitions": args.reps, "variants": {}}
for v in variants:
    res["variants"][v] = dict(frames_per_s=reps[v], median=round(statistics.median(reps[v]), 2), spread=round(max(reps[v]) - min(reps[v]), 2), track_info=infos[v])
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(res, open(args.out, "w"), indent=1)
