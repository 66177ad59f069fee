"""Records tests/golden/solve_dataflow/: dv_ba_solve on every case of tests/test_solve_dataflow.py with the library that is loaded (DVINS_HIP_LIB selects another
build: the records in the repository come from the commit before the dataflow form of the factorisation loop).  Needs a GPU.

    python -m tests.tools.solve_dataflow_golden [--out DIR]
"""
import argparse
import json
import os

import numpy as np


def main():
    from dynamic_vins_amd.frontend import Context
    from tests import oracle_py
    from tests import test_solve_dataflow as t
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=t.GOLDEN)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    oracle = oracle_py.load()
    made = []

    def factory(**kw):
        made.append(Context(**kw))
        return made[-1]
    for name in t.CASES:
        dig, x, s = t.solve_case(factory, oracle, name)
        np.save(os.path.join(args.out, name + ".npy"), x)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(dict(s, input_sha1=dig, n=t.CASES[name][2]), f, indent=1, sort_keys=True)
            f.write("\n")
        print(name, s, flush=True)
    for c in made:
        c.close()


if __name__ == "__main__":
    main()
