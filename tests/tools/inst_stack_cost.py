"""Cost of thread T1's stage from a mask stack, in isolation: dv_inst_stack_frame_enqueue -> _collect, wall clock, median of 20, at 1242 x 375 (a KITTI frame) with 8 and
with 32 DV_STACK_U8 planes in device memory.  Writes profiles/inst_stack_cost.json with the algorithmic traffic — (n_planes + 2) bytes per pixel: every plane read once,
two masks written once — and the bandwidth it implies.  Each configuration runs in a child process under its own time limit; the first that fails or runs out of time
ends the tool (nothing is started behind it).

    python tests/tools/inst_stack_cost.py            # both configurations -> profiles/inst_stack_cost.json
    python tests/tools/inst_stack_cost.py --one 8    # one configuration, prints its JSON record (what the children run)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H, REPS, WARM, LIMIT_S = 1242, 375, 20, 5, 120


def one(n_planes):
    import numpy as np
    import torch
    from dynamic_vins_amd.frontend import Context, DV_MEM_DEVICE, make_cam
    ctx = Context(width=W, height=H, max_cnt=150, min_dist=30, cam0=make_cam(721.5, 721.5, 609.6, 172.9), cam1=make_cam(721.5, 721.5, 609.6, 172.9))
    rng = np.random.default_rng(1)
    stack = np.zeros((n_planes, H, W), np.uint8)
    for p in range(n_planes):                              # one car-sized blob per plane
        x, y = int(rng.integers(0, W - 200)), int(rng.integers(100, H - 120))
        stack[p, y:y + int(rng.integers(40, 120)), x:x + int(rng.integers(60, 200))] = 1
    t = torch.from_numpy(stack).cuda()
    torch.cuda.synchronize()
    kw = dict(mem=DV_MEM_DEVICE, n_planes=n_planes)
    times = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        ctx.inst_stack_frame_enqueue(t.data_ptr(), **kw)
        dets, _, _ = ctx.inst_stack_frame_collect(8)
        times.append(time.perf_counter() - t0)
    ctx.close()
    times = sorted(times[WARM:])
    med = 0.5 * (times[REPS // 2 - 1] + times[REPS // 2])
    traffic = (n_planes + 2) * W * H
    return dict(n_planes=n_planes, width=W, height=H, detections=len(dets), reps=REPS, median_ms=1e3 * med, min_ms=1e3 * times[0], max_ms=1e3 * times[-1],
                algorithmic_bytes=traffic, implied_gb_per_s=traffic / med / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inst_stack_cost.json"))
    a = ap.parse_args()
    if a.one:
        print("RECORD " + json.dumps(one(a.one)))
        return 0
    recs = []
    for n in (8, 32):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n)], capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{n} planes: no result within {LIMIT_S} s; stopping", file=sys.stderr)
            return 3
        if r.returncode != 0:
            print(f"{n} planes: exit {r.returncode}; stopping\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}", file=sys.stderr)
            return 2
        recs.append(json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RECORD "))[7:]))
        print(recs[-1])
    out = dict(what="dv_inst_stack_frame_enqueue -> _collect, wall clock per frame (launches, the 16 B x n_planes box copy and the host's wait included), DV_STACK_U8, device memory",
               unit="ms", records=recs,
               avoided_host_round_trip_arithmetic=dict(note="byte counts per frame, arithmetic, not measured", stack_download_bytes={str(n): n * W * H for n in (8, 32)},
                                                      roi_mask_upload="the sum of the rectangles' areas, twice (object tracker, static unmasking)"))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
