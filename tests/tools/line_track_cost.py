"""Cost of the line tracker stage on one GPU: dv_line_track_enqueue -> _collect at 64, 256 and DV_LINE_MAX lines per image on both sides, every line tracked, input in
pinned memory; 30 untimed frames, then 300 timed: the ctx's event timer "line_track" (kernel + the copy of the result block) and the host clock around the pair.
    python tests/tools/line_track_cost.py"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dynamic_vins_amd.frontend import Context, make_cam, DV_MEM_PINNED
from tests import line_track_cases as lc
ctx = Context(width=752, height=480, cam0=make_cam(460.0, 458.0, 367.0, 248.0, -0.28, 0.07, 2e-4, 1e-5), cam1=make_cam(457.0, 456.0, 379.0, 255.0, -0.28, 0.07, -1e-4, -2e-4))
pin = [ctx.lib.dv_pinned_alloc(512 * s) for s in (24, 32, 24, 32)]
for n in (64, 256, 512):
    sc = lc.Scene(n, 100 + n)
    ids = list(range(n))
    frames = [sc.frame(ids, right=ids) for _ in range(8)]
    def run(k):
        L, Ld, R, Rd = frames[k % 8]
        for p, a in zip(pin, (L, Ld, R, Rd)):
            C.memmove(p, a.ctypes.data, a.nbytes)
        t0 = time.perf_counter()
        ctx.line_track_enqueue(int(pin[0]), int(pin[1]), int(pin[2]), int(pin[3]), n_left=n, n_right=n, mem=DV_MEM_PINNED)
        r = ctx.line_track_collect()
        return time.perf_counter() - t0, r
    ctx.line_track_reset()
    for k in range(30):
        run(k)
    ctx.timing_enable(1); ctx.timing_reset()
    host = []
    for k in range(300):
        dt, r = run(k)
        host.append(dt)
    ms, cnt = ctx.timing_get("line_track")
    ctx.timing_enable(0)
    host = np.array(host) * 1e3
    print(f"n={n}: device events {ms / cnt * 1e3:.1f} us per frame over {cnt} frames; host enqueue-to-collect median {np.median(host) * 1e3:.1f} us, p90 {np.percentile(host, 90) * 1e3:.1f} us; tracked {len(r['left_ids'])} left {len(r['right_ids'])} right rows {len(r['rows'])}", flush=True)
ctx.close()
