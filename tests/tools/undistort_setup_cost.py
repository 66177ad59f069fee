"""One-time cost of dv_undistort_setup (new camera matrices on the host + both map pairs built and installed on the device) on a stereo ctx at 752x480 (EuRoC) and
1280x720 (ZED): wall clock of the call, median and minimum of 20 calls after one warm-up call (which also pays the allocations).  A set-up cost: no bar.
    python tests/tools/undistort_setup_cost.py [out.json]      (default: profiles/undistort_setup_cost.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dynamic_vins_amd import sim                                       # noqa: E402
from dynamic_vins_amd.frontend import Context, make_cam                # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "undistort_setup_cost.json")
res = {"what": "dv_undistort_setup, stereo ctx, wall clock per call in ms (host newK + 2 x (column walk + map kernel) + stream sync)", "calls": 20, "sizes": {}}
for name, w, h, cam in (("752x480", 752, 480, sim.EUROC), ("1280x720", 1280, 720, sim.ZED)):
    c = make_cam(*sim.cam_tuple(cam))
    ctx = Context(width=w, height=h, cam0=c, cam1=c)
    t0 = time.perf_counter(); ctx.undistort_setup(); first = (time.perf_counter() - t0) * 1e3
    ts = []
    for _ in range(20):
        t0 = time.perf_counter(); ctx.undistort_setup(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    res["sizes"][name] = dict(first_call_ms=round(first, 4), median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4))
    ctx.close()
print(json.dumps(res))
os.makedirs(os.path.dirname(out), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
