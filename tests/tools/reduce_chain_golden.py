"""Records tests/golden/reduce_chain/: every case of tests/test_reduce_chain.py with the library that is loaded (DVINS_HIP_LIB selects another build: the records in the
repository come from the commit before be_reduce's pair blocks lost their list barrier, with buffer 8 (scale_l) added to dv_ba_debug_buffer).  Needs a GPU.

    python -m tests.tools.reduce_chain_golden [--out DIR] [--batch-only] [--batch-name NAME]

--batch-only writes the two-estimator dv_batch record alone (NAME.npz / NAME.json, default "batch"): run once as it is and once under DVINS_REDUCE_OCC=1 with
--batch-name batch_occ; the test's occupancy case calls it in a child process the same way.
"""
import argparse
import json
import os

import numpy as np


def main():
    from dynamic_vins_amd.frontend import Context
    from tests import oracle_py
    from tests import test_reduce_chain as t
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=t.GOLDEN)
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--batch-name", default="batch")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    made = []

    def factory(**kw):
        made.append(Context(**kw))
        return made[-1]

    def dump(name, arrays, meta):
        np.savez_compressed(os.path.join(args.out, name + ".npz"), **arrays)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
            f.write("\n")
    if not args.batch_only:
        oracle = oracle_py.load()
        ctx = factory(width=64, height=48)
        for name in t.CASES:
            dig, arrays, summ = t.run_case(ctx, oracle, name)
            full, digests = t.split_record(arrays)
            counts = {"%d,%d" % k: v for k, v in t.pair_counts(arrays["eval.lm_obs"]).items() if v}
            dump(name, full, dict(input_sha1=dig, summary=summ, sha1=digests, pair_counts=counts))
            print(name, summ, "pairs with landmarks:", len(counts), "largest:", max(counts.values(), default=0), flush=True)
    windows, digests, info = t.run_batch(factory)
    dump(args.batch_name, windows, dict(sha1=digests, info=info))
    print(args.batch_name, info, flush=True)
    for c in made:
        c.close()


if __name__ == "__main__":
    main()
