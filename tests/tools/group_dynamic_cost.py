"""Aggregate frames/s of 16 DYNAMIC sequences (752x480, escort scene, objects in every frame) on one GPU under the C++ runner, in two variants:
    a  group_size 0, one host thread per sequence (16 independent launch chains; every sequence's tracker on its own thread beside it: the runner's defaults);
    b  group_size 16: ONE dv_batch group on one host thread — window solves in the group's shared slots, the object solves of a round in one
       bd_solve_group_kernel launch, every member's own tracking launches.
One process alternates a, b, a, b, ... for `--reps` repetitions each (default 5); a repetition builds fresh pipelines over the same rendered frames, runs 20 warm-up
frames and times the next 100 with dv_runner_run's own wall clock.  Every repetition, the medians and the spread (max - min) go to the output file, with the object-solve
launch counters of variant b.  Variant a uses nothing newer than Runner(group_size=0), so `--only a` measures the commit before dynamic members could join a group.
The 16 members run over 4 rendered sequences (3 - 6 boxes), four members each: rendering is not what is measured, and the members do not share a context or a buffer.
Every repetition runs under its own time limit (--rep-timeout, default 120 s).
    python tests/tools/group_dynamic_cost.py [--out profiles/group_dynamic_cost.json] [--reps 5] [--only a]      (--only: one variant, e.g. for a run under a profiler)"""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dynamic_vins_amd import sim                                                # noqa: E402
from dynamic_vins_amd.backend import Runner                                     # noqa: E402
from dynamic_vins_amd.pipeline import DynamicPipeline, DynamicSequence          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_dynamic_cost.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", default="", help="run only this variant (a or b)")
ap.add_argument("--rep-timeout", type=int, default=120, help="seconds one repetition of one variant may take: the process ends (SIGALRM) when one overruns")
args = ap.parse_args()

S, W, H, WARM, FRAMES = 16, 752, 480, 20, 100
cam = sim.scaled_cam(sim.ZED, W, H, 1280, 720)
seqs = [DynamicSequence(W, H, cam, WARM + FRAMES + 2, rate=20.0, boxes=("escort", 3 + i)) for i in range(4)]


def one(variant):
    pipes = [DynamicPipeline(seqs[i % 4], max_cnt=150, min_dist=20, max_iters=8, use_det3d=1, mask_morphology_size=5) for i in range(S)]
    r = Runner(pipes, group_size=0, threads=S) if variant == "a" else Runner(pipes, group_size=S, threads=1)
    r.run(WARM)
    wall = r.run(FRAMES)
    info = r.obj_rounds() if variant == "b" else {}
    feats = sum(r.dynamic_stats(i)["object_features"] for i in range(S))
    r.close()
    for p in pipes:
        p.ctx.close()
    return S * FRAMES / wall, dict(info, object_features=feats)


variants = [v for v in "ab" if not args.only or v == args.only]
reps = {v: [] for v in variants}
infos = {}
for k in range(args.reps):
    for v in variants:
        signal.alarm(args.rep_timeout)          # every repetition under its own time limit: a hung one ends the process instead of holding the GPU
        fps, infos[v] = one(v)
        signal.alarm(0)
        reps[v].append(round(fps, 2))
        print("repetition %d variant %s: %.1f frames/s %s" % (k, v, fps, infos[v]), flush=True)
res = {"what": "aggregate frames/s of 16 dynamic sequences at 752x480 under dv_runner, %d frames timed after %d warm-up frames; a: group_size 0, one host thread per sequence, "
               "b: group_size 16 on one host thread (shared window slots, one object-solve launch per round)" % (FRAMES, WARM),
       "sequences": S, "size": [W, H], "repetitions": args.reps, "variants": {}}
for v in variants:
    res["variants"][v] = dict(frames_per_s=reps[v], median=round(statistics.median(reps[v]), 2), spread=round(max(reps[v]) - min(reps[v]), 2), info=infos[v])
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(res, open(args.out, "w"), indent=1)
