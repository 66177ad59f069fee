"""Phase table of be_solve_kernel<1, true> from its in-kernel stamps.  Needs a library built with -DBE_SOLVE_TS (make HIPFLAGS="... -DBE_SOLVE_TS"; DVINS_HIP_LIB
points at it) and a GPU.  Solves one 11-frame IMU window (n = 165, 250 landmarks: the benchmark's shape) repeatedly and reads the stamps the last full slot of every
solve left behind (wall_clock64, 10 ns ticks); a stamp set that is not monotonic (the last launch returned early) is dropped.

    DVINS_HIP_LIB=.../libdvins_hip.so python -m tests.tools.solve_phase_stamps [--solves 40] [--debug-set ldl_barriers]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ROWS = [("prologue (tables, accept decision)", 15, 0), ("scale + gradient", 0, 3), ("ldlt load (tile finish, barrier)", 3, 4), ("ldlt loop", 4, 5),
        ("back-sub", 6, 24), ("gn landmarks", 24, 8), ("dogleg", 8, 9), ("H*delta, candidate, final sums", 9, 10), ("total", 15, 10)]
SUMS = [("mf16: load + diag tile 0", 16), ("mf16: panels (sum over steps, wave 0)", 17), ("mf16: updates (sum over steps, wave 0)", 18),
        ("mf16: diag tiles 1.. (owner wave, sum)", 19), ("mf16: owner's panel + update before its diag (sum)", 20),
        ("chain: wait for W_k (sum)", 32), ("chain: own panel (sum)", 33), ("chain: own update (sum)", 34), ("chain: barrier B / count (sum)", 35)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=40)
    ap.add_argument("--debug-set", default="")
    args = ap.parse_args()
    from dynamic_vins_amd.backend import ba_solve
    from dynamic_vins_amd.frontend import Context
    from tests import ba_gen, oracle_py
    ctx = Context(width=64, height=48)
    for key in filter(None, args.debug_set.split(",")):
        assert ctx.lib.dv_debug_set(ctx.h, key.encode(), 1) == 0, key
    fn = ctx.lib.dv_debug_solve_ts
    fn.argtypes, fn.restype = [C.c_void_p], C.c_int
    base = ba_gen.make_window(oracle_py.load(), seed=505, nframes=11, nlm=250, max_iters=4)
    got = []
    for _ in range(args.solves + 3):
        ba_solve(ctx, base.clone())
        ts = np.zeros(48, np.int64)
        assert fn(ts.ctypes.data) == 0
        got.append(ts)
    got = got[3:]                                    # warm-up
    order = [15, 0, 3, 4, 5, 6, 24, 8, 9, 10]
    ok = [t for t in got if all(t[a] <= t[b] for a, b in zip(order, order[1:])) and t[10] - t[15] < 50000]
    print("solves %d, stamp sets kept %d (us)" % (len(got), len(ok)))
    if not ok:
        return 1
    for name, a, b in ROWS:
        v = np.array([(t[b] - t[a]) * 0.01 for t in ok])
        print("%-42s mean %7.2f  min %7.2f  max %7.2f" % (name, v.mean(), v.min(), v.max()))
    for name, k in SUMS:
        print("%-52s mean %7.2f" % (name, np.mean([t[k] * 0.01 for t in ok])))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
