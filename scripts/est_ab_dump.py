"""Bit-identity of the estimator across two builds of the library: runs the configurations of tests/test_estimator_parity.py, test_dynamic_parity.py,
test_line_estimator_parity.py and test_free_ex_td.py (same simulators, seeds and frame counts, no oracle beside them) with dv_debug_set("hash_log", 1) on and
writes one SHA-256 per configuration over the raw bytes of every frame's dv_est_state, dv_est_get_landmarks, dv_est_get_instances (dynamic runs) and, at the
end, the hash-log rows.  The library is the one DVINS_HIP_LIB names (default: the tree's own); run it once per library, each in a fresh process, and compare:

    DVINS_HIP_LIB=<parent>/libdvins_hip.so python scripts/est_ab_dump.py parent.json
    python scripts/est_ab_dump.py head.json
    python scripts/est_ab_dump.py --compare parent.json head.json merged.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NOISE = dict(acc_n=0.02, gyr_n=0.002, acc_w=2e-4, gyr_w=2e-5)
LM_BYTES = 56          # sizeof(dv_landmark)


class Dump:
    def __init__(self, dev, dynamic):
        self.dev, self.dynamic, self.h, self.nbytes = dev, dynamic, hashlib.sha256(), 0

    def add(self, b):
        self.h.update(b)
        self.nbytes += len(b)

    def frame(self):
        dev, lib, h = self.dev, self.dev.ctx.lib, self.dev.ctx.h
        self.add(bytes(dev.state))
        buf, n = np.zeros(4096 * LM_BYTES, np.uint8), C.c_int(0)
        assert lib.dv_est_get_landmarks(h, buf.ctypes.data, 4096, C.byref(n)) == 0
        self.add(buf[: n.value * LM_BYTES].tobytes())
        if self.dynamic:
            inst, summ = dev.instances()
            self.add(inst.tobytes() + summ.tobytes())

    def finish(self):
        lib, h = self.dev.ctx.lib, self.dev.ctx.h
        rows, n = np.zeros((4096, 6), np.uint64), C.c_int(0)
        assert lib.dv_est_debug_hash_log(h, rows.ctypes.data, 4096, C.byref(n)) == 0 and 0 < n.value < 4096
        self.add(rows[: n.value].tobytes())
        return dict(sha256=self.h.hexdigest(), bytes=self.nbytes, solves=n.value)


def make(kw, dynamic=False):
    from dynamic_vins_amd.backend import Estimator
    from dynamic_vins_amd.frontend import Context
    ctx = Context(width=64, height=64, max_cnt=10, min_dist=5)
    assert ctx.lib.dv_debug_set(ctx.h, b"hash_log", 1) == 0
    dev = Estimator(ctx, **kw)
    return ctx, dev, Dump(dev, dynamic)


def feed(dev, ts, acc, gyr, k, until):
    while k < len(ts) and ts[k] <= until:
        dev.InputIMU(ts[k], acc[k], gyr[k])
        k += 1
    return k


def ego(use_imu, frames, two_phase=False, use_line=0, estimate=0):
    from dynamic_vins_amd import sim
    from tests import ba_gen
    T0, dtf = 1.0, 0.1
    if estimate:          # tests/test_free_ex_td.py: an excited trajectory, extrinsics 8 mm / 0.3 degrees off, samples reaching past t + td
        class Excited(sim.Trajectory):
            def ypr(self, t):
                y = sim.Trajectory.ypr(self, t)
                return np.array([y[0], 0.25 * np.sin(2.3 * t), 0.2 * np.sin(3.1 * t + 1.0)])
        traj, seed, lead = Excited(), 5, 0.06
        rng = np.random.default_rng(7)
        ric = [sim.R_IC @ ba_gen.small_rot(rng.normal(0, 0.005, 3)) for _ in range(2)]
        tic = [np.asarray(sim.T_IC0) + rng.normal(0, 0.008, 3), np.asarray(sim.T_IC1) + rng.normal(0, 0.008, 3)]
    else:
        traj, seed, lead, ric, tic = sim.Trajectory(), 3, 0.011, [sim.R_IC, sim.R_IC], [sim.T_IC0, sim.T_IC1]
    fs = sim.FeatureSim(traj, sim.EUROC, 752, 480, sim.room_points(3000), max_cnt=150, pix_sigma=0.3, seed=seed)
    ls = sim.LineSim(traj, 752, 480, n=80) if use_line else None
    kw = dict(use_imu=use_imu, stereo=1, max_iters=8, ric=ric, tic=tic, estimate=estimate, **NOISE)
    if use_line:
        kw.update(use_line=1, line_min_obs=5)
    ctx, dev, d = make(kw)
    ts, acc, gyr = sim.imu_stream(traj, T0 - 0.05, T0 + frames * dtf + 0.1, 200.0, **NOISE)
    k = 0
    for f in range(frames):
        t = T0 + f * dtf
        k = feed(dev, ts, acc, gyr, k, t + lead)
        rows = fs.frame(t)
        if ls is not None:
            dev.SetLines(ls.frame(t))
        if two_phase:
            assert dev.ProcessMeasurementsBegin(rows, t) == 0
            k = feed(dev, ts, acc, gyr, k, t + dtf + 0.011)
            dev.ProcessMeasurementsEnd()
        else:
            assert dev.ProcessMeasurements(rows, t)[0] == 0
        d.frame()
        if ls is not None:
            d.add(dev.lines().tobytes())
    out = d.finish()
    ctx.close()
    return out


def dynamic(frames, use_imu, use_det3d):
    from dynamic_vins_amd import dynsim, sim
    traj, cam = sim.Trajectory(), sim.EUROC
    fs = sim.FeatureSim(traj, cam, 752, 480, sim.room_points(3000), max_cnt=150, pix_sigma=0.3, seed=3)
    isim = dynsim.InstSim(traj, cam, 752, 480, with_det3d=bool(use_det3d))
    kw = dict(use_imu=use_imu, stereo=1, max_iters=8, plane_constraint=0, ric=[sim.R_IC, sim.R_IC], tic=[sim.T_IC0, sim.T_IC1], dynamic=1, use_det3d=use_det3d,
              instance_init_min_num=4, static_inst_threshold=1.0, use_line=0, **NOISE)
    ctx, dev, d = make(kw, dynamic=True)
    T0, dtf = 1.0, 0.1
    ts, acc, gyr = sim.imu_stream(traj, T0 - 0.05, T0 + frames * dtf + 0.2, 200.0, **NOISE)
    k = 0
    for f in range(frames):
        t = T0 + f * dtf
        k = feed(dev, ts, acc, gyr, k, t + 0.011)
        insts, ifeats, pts = isim.frame(t, visible=None)
        assert dev.ProcessMeasurementsDynamic(fs.frame(t), t, insts, ifeats, pts)[0] == 0
        d.frame()
    out = d.finish()
    ctx.close()
    return out


CONFIGS = {
    "imu_45": lambda: ego(1, 45),
    "vision_only_35": lambda: ego(0, 35),
    "two_phase_30": lambda: ego(1, 30, two_phase=True),
    "dynamic_det3d_60": lambda: dynamic(60, 1, 1),
    "dynamic_no_det3d_vision_only_40": lambda: dynamic(40, 0, 0),
    "line_imu_42": lambda: ego(1, 42, use_line=1),
    "line_vision_only_34": lambda: ego(0, 34, use_line=1),
    "estimate_1_40": lambda: ego(1, 40, estimate=1),
    "estimate_2_40": lambda: ego(1, 40, estimate=2),
    "estimate_3_40": lambda: ego(1, 40, estimate=3),
}


def main():
    if sys.argv[1] == "--compare":
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        merged = {name: dict(parent=a["digests"][name], head=b["digests"][name], equal=a["digests"][name] == b["digests"][name]) for name in CONFIGS}
        out = dict(what=__doc__.split("\n\n")[0].replace("\n", " "), parent_library=a["library"], head_library=b["library"], configurations=merged,
                   all_equal=all(m["equal"] for m in merged.values()))
        json.dump(out, open(sys.argv[4], "w"), indent=1)
        print("all digests equal" if out["all_equal"] else "DIGESTS DIFFER: " + ", ".join(n for n, m in merged.items() if not m["equal"]))
        return 0 if out["all_equal"] else 1
    from dynamic_vins_amd import _abi
    stamp = os.path.join(os.path.dirname(_abi.LIB_PATH), "BUILD_HEAD")
    res = dict(library=open(stamp).read().strip() if os.path.exists(stamp) else "unknown", digests={})
    for name, run in CONFIGS.items():
        res["digests"][name] = run()
        print(name, res["digests"][name], flush=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
