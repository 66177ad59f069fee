"""Cost of the stereo matcher: dv_stereo_sgm_enqueue -> _collect, wall clock, median of 20 with min and max, the pair in device memory, one process, at
752 x 480 and 1242 x 375 with n_disp = 128 and 752 x 480 with n_disp = 64.  Beside each time the algorithmic traffic the one-volume uint16 layout of S implies
(csrc/stereo_sgm.hip's header) and the bandwidth that would mean if the time were all traffic.  Writes profiles/sgm_cost.json.

    python tests/tools/sgm_cost.py             # -> profiles/sgm_cost.json
    python tests/tools/sgm_cost.py --frames 3  # a short run that writes nothing (the command for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SHAPES, REPS, WARM = [(752, 480, 128), (1242, 375, 128), (752, 480, 64)], 20, 3


def median(v):
    v = sorted(v)
    return 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def traffic(w, h, d):
    """bytes per frame, arithmetic: S written once and read + written seven times, read once by the decision and gathered once more for dR (an upper bound: only
    valid winners gather); per direction the left code once and the right codes n_disp times per pixel; census reads both images and writes both code maps"""
    px = w * h
    return dict(S=px * d * 2 * (1 + 2 * 7 + 2), codes=8 * px * 8 * (d + 1), census=2 * px * (1 + 8), map_out=4 * px)


def run(w, h, d, reps):
    import numpy as np
    import torch
    from dynamic_vins_amd.frontend import Context, DV_MEM_DEVICE, make_cam, sgm_params
    rng = np.random.default_rng(0)
    tex = rng.integers(0, 256, (h, w + 40), dtype=np.uint8)
    l, r = torch.from_numpy(np.ascontiguousarray(tex[:, :w])).cuda(), torch.from_numpy(np.ascontiguousarray(tex[:, 23:23 + w])).cuda()
    torch.cuda.synchronize()
    cam = make_cam(400.0, 400.0, w / 2, h / 2)
    ctx = Context(width=w, height=h, max_cnt=50, min_dist=30, cam0=cam, cam1=cam)
    par, t = sgm_params(n_disp=d), []
    for _ in range(WARM + reps):
        t0 = time.perf_counter()
        ctx.stereo_sgm_enqueue(l.data_ptr(), r.data_ptr(), par, mem=DV_MEM_DEVICE, stride=w)
        ctx.stereo_sgm_collect()
        t.append(time.perf_counter() - t0)
    ctx.close()
    t = t[WARM:]
    tr = traffic(w, h, d)
    return dict(shape=[w, h], n_disp=d, reps=reps, ms=dict(median=1e3 * median(t), min=1e3 * min(t), max=1e3 * max(t)), traffic_bytes=tr,
                implied_GBps=sum(tr.values()) / median(t) / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm_cost.json"))
    a = ap.parse_args()
    recs = [run(w, h, d, a.frames or REPS) for w, h, d in SHAPES]
    for r in recs:
        print(r)
    if a.frames:
        return 0
    out = dict(what="dv_stereo_sgm_enqueue -> _collect, wall clock per frame, the pair in device memory, one process on one GPU; traffic_bytes is arithmetic from the "
                    "S layout (one uint16 volume accumulated in place), not measured; implied_GBps = that traffic over the median time", unit="ms", records=recs)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
