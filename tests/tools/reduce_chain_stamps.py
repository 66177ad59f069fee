"""debug: phase stamps of be_reduce_kernel (pair block 0, one dense block) on a full window; library built with -DBE_RED_TS (DVINS_HIP_LIB selects it).
tests/tools/dbg_eval_reduce_ts.py prints the rows both forms of the pair block share; this one adds the stamp at a pair block's entry (index 4), which the form
without the list barrier and stamped builds of the shared form take.  A row whose stamps the loaded build does not take is left out.

    DVINS_HIP_LIB=.../libdvins_hip.so python tests/tools/reduce_chain_stamps.py
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ba_gen                                               # noqa: E402
import oracle_py                                            # noqa: E402
from dynamic_vins_amd import _abi, backend                  # noqa: E402
from dynamic_vins_amd.frontend import Context               # noqa: E402

ROWS = [(4, 0, "pair: entry -> list ready"), (0, 1, "pair: landmark loop"), (1, 2, "pair: wave sums + wait for wave 6"), (2, 3, "pair: store"),
        (4, 3, "pair: entry -> stored"), (4, 16, "pair: entry -> wave 6 starts"), (0, 16, "pair: list ready -> wave 6 starts"), (16, 17, "pair: wave 6 index chains"),
        (8, 9, "dense block")]

o = oracle_py.load()
ctx = Context(width=64, height=48)
P = ba_gen.make_window(o, seed=3, nlm=263, max_iters=1, with_prior=True)
backend.ba_solve(ctx, P)
print("prior n", P.prior.n if P.prior is not None else 0, "landmarks", len(P.landmarks), "factors", len(P.factors))
lib = _abi.load()
ts = (C.c_longlong * 64)()
lib.dv_debug_red_ts.argtypes = [C.POINTER(C.c_longlong)]
assert lib.dv_debug_red_ts(ts) == 0
for a, b, n in ROWS:
    if ts[a] and ts[b]:
        print("%-36s %8.2f us" % (n, (ts[b] - ts[a]) / 100.0))
ctx.close()
