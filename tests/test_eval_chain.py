"""be_eval's workgroup kinds after their chains were shortened (`-m gpu`; be_eval.hip: packet entries with their reads issued together, the factor records requested ahead
of the geometry, the IMU Jacobian blocks on different waves, whitening with its reads issued together; the prior workgroup is pinned too, its code is the earlier one): the
restructuring changes WHEN an operand is loaded and WHICH lane forms an entry, never the operands or the order of the additions, so every number the evaluation writes
must keep the bits it had.  No tolerance anywhere in this file.

tests/golden/eval_chain/<case>.npz / .json are records made with the library of the commit BEFORE the change (that commit's be_eval.hip; only the read-back entry
dv_ba_debug_buffer was added to it) by tests/tools/eval_chain_golden.py.  Every case is run twice on a context whose linearisation buffers were filled with 0xFF bytes
first, so that an entry the kernel does NOT write is part of the comparison too:
  eval    dv_ba_eval (be_begin_impl(..., eval_only = true)): one BE_EVAL_X launch + the reduce
  solve   dv_ba_solve with max_iters = 3: BE_EVAL_X, two BE_EVAL_CAND_FULL launches into the other set, then the cost-only BE_EVAL_CAND_COST launch
and what is compared is, for both linearisation sets: the packets (columns < nlm), imu_out, prior_out, cand_cost, lm_obs, Hd, Sc, gvec, and after the solve the states
and the summary.  An array is recorded in full up to 128 KiB in the cases lm1 and lm17 and up to 16 KiB in the others, a larger one as its SHA-1 (equal digests = every
double equal; the full arrays of lm1 / lm17 say WHERE a difference sits).  The problems are regenerated from their seeds and their input digest is compared first.

  case      frames nlm nimu prior  what it holds
  lm1       11     1   10   82     a single landmark with ONE factor, a stereo one (kind 2): s_two false, the anchor's sums empty; anchored in the LAST frame
  lm17      11     17  10   82     one packet line and one landmark; landmark 1 has BE_MAX_OBS_FACTORS = 24 factors and is anchored in frame 0, landmark 2 is seen by the
                                   left camera only in frames 3 and 5 and by the right camera only in frame 6 (an s_flist slot of -1 on either side)
  lm33      11     33  10   82     two packet lines and one landmark
  f3        3      17  2    none   the smallest window with landmarks
  imu1      2      17  1    none   one IMU factor
  vo11      11     33  0    67     vision only: no IMU block, pose 0 constant
  p1 p63 p64 p65 p144  11  17  10  n = 1, 63, 64, 65, 144: the n_pad / groups boundaries of the A'dx partition (n_pad 64 with 4 thread groups up to 64, 128 with 2
                                   from 65 on, 192 with one beyond 128).  A prior header holds at most 16 blocks of at most 9 entries, so n = 144 is the largest prior whose
                                   dx is fully defined; n = BE_MAX_PRIOR = 192 cannot be described by a header and is not a case (it would take the same path as 144).
                                   63 / 64 / 65 are nine poses and a speed-bias block plus none / one / two td blocks, 144 is sixteen speed-bias blocks: the kernel takes the
                                   blocks as they come, the solve maps what it has a column for.
Batched forms: two estimators in a dv_batch for 18 frames (LPB 8, be_eval_batch_kernel) and the same in a child process under DVINS_EVAL_SPLIT=1 (the landmark and the
IMU / prior launches; the switch is read once per process), both against the recorded windows and buffer digests of the members after the last round.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dynamic_vins_amd import sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_chain")
FULL_BYTES, FULL_BYTES_REST, FULL_CASES = 128 * 1024, 16 * 1024, ("lm1", "lm17")
NSTATE_MAX, PK_SIZE, PK_STRIDE, IMU_OUT, MAX_PRIOR, MAX_LM, WIN = 178, 928, 1024, 936, 192, 1000, 10
# dv_ba_debug_buffer: which -> (name, number of 8-byte words (4-byte for lm_obs), one buffer per set)
BUFFERS = [("packets", PK_SIZE * PK_STRIDE, True), ("imu_out", WIN * IMU_OUT, True), ("prior_out", MAX_PRIOR + 1, True), ("cand_cost", MAX_LM + WIN + 1, False),
           ("lm_obs", MAX_LM, False), ("Hd", NSTATE_MAX * NSTATE_MAX, True), ("Sc", NSTATE_MAX * NSTATE_MAX, True), ("gvec", 2 * NSTATE_MAX, True)]
BLOCK_SIZE = {0: 6, 1: 9, 2: 6, 3: 1}
P63 = [(0, k) for k in range(9)] + [(1, 0)]
PRIORS = {"p1": [(3, 0)], "p63": P63, "p64": P63 + [(3, 0)], "p65": P63 + [(3, 0), (3, 0)], "p144": [(1, k % 11) for k in range(16)]}
CASES = ["lm1", "lm17", "lm33", "f3", "imu1", "vo11"] + list(PRIORS)


# ---------------------------------------------------------------- problems ----------------------------------------------------------------
def crafted_landmarks(base, nframes, seed):
    """33 landmarks with chosen factor patterns, geometrically consistent with the window `base` (tests/ba_gen.py's trajectory and rig): (factors, landmarks, inv_depth)"""
    from dynamic_vins_amd.backend import FACTOR_DTYPE, LM_DTYPE
    rng = np.random.default_rng(seed)
    traj = sim.Trajectory()
    times = 2.0 + 0.37 * base.seed + 0.1 * np.arange(nframes)
    R_wb, p_wb = [traj.R(t) for t in times], [traj.p(t) for t in times]
    ric, tic = [sim.R_IC, sim.R_IC], [sim.T_IC0, sim.T_IC1]

    def proj(k, cam, P):
        Pc = ric[cam].T @ (R_wb[k].T @ (P - p_wb[k]) - tic[cam])
        return Pc[:2] / Pc[2], Pc[2]
    pts = [P for P in sim.room_points(4000, seed=base.seed + 100)
           if all(z > 0.5 and np.abs(x).max() < 0.8 for k in range(nframes) for cam in (0, 1) for x, z in [proj(k, cam, P)])]
    assert len(pts) >= 33, len(pts)
    last = nframes - 1
    # (anchor, [(kind, frame)]): kind 0 left camera of frame, 1 right camera of frame, 2 right camera of the anchor frame
    both = lambda a, fs: [(2, a)] + [(kd, f) for f in fs for kd in (0, 1)]
    spec = [(last, [(2, last)]),
            (0, both(0, range(1, nframes)) + [(2, 0)] * (24 - 1 - 2 * (nframes - 1)) if nframes == 11 else both(0, range(1, nframes))),
            (min(2, last - 1), [(0, f) for f in (3, 4, 5) if f < nframes] + [(1, f) for f in (4, 6) if f < nframes] if nframes > 3 else [(0, last)])]
    while len(spec) < 33:
        a = int(rng.integers(0, last))
        fs = [f for f in range(a + 1, nframes) if rng.uniform() < 0.8] or [last]
        spec.append((a, ([(2, a)] if rng.uniform() < 0.7 else []) + [(kd, f) for f in fs for kd in (0, 1) if kd == 0 or rng.uniform() < 0.7]))
    factors, lms, inv_depth = [], [], []
    for li, (a, obs) in enumerate(spec):
        P = pts[li]
        pi = proj(a, 0, P)[0] + rng.normal(0, 0.4 / 460.0, 2)
        first, mask = len(factors), 1 << a
        for kd, f in obs:
            pj = proj(f, 0 if kd == 0 else 1, P)[0] + rng.normal(0, 0.4 / 460.0, 2)
            mask |= 1 << f
            factors.append((pi[0], pi[1], pj[0], pj[1], 0, 0, 0, 0, 0, 0, kd, li, a, f, (0, 0)))
        lms.append((first, len(factors) - first, a, mask))
        inv_depth.append(1.0 / (proj(a, 0, P)[1] * (1 + rng.normal(0, 0.08))))
    return np.array(factors, FACTOR_DTYPE), np.array(lms, LM_DTYPE), np.array(inv_depth)


def make_prior(oracle, prob, blocks, seed):
    """a prior over `blocks` [(type, idx)] in ba_gen.make_window's manner: (header, A, b)"""
    import ctypes as C
    from dynamic_vins_amd.backend import dv_ba_prior
    rng = np.random.default_rng(seed)
    prior, off = dv_ba_prior(), 0
    for i, (ty, idx) in enumerate(blocks):
        pb = prior.blocks[i]
        pb.type, pb.idx, pb.off, pb.size_local = ty, idx, off, BLOCK_SIZE[ty]
        x0 = np.array(prob.pose[idx] if ty == 0 else prob.speed_bias[idx] if ty == 1 else prob.ex_pose[idx] if ty == 2 else [0.0], float)
        x0[: 3 if ty in (0, 2) else len(x0)] += rng.normal(0, 0.01, 3 if ty in (0, 2) else len(x0))
        if ty in (0, 2):
            q = x0[3:] + rng.normal(0, 0.005, 4)
            x0[3:] = q / np.linalg.norm(q)
        for j in range(len(x0)):
            prior.x0[i][j] = x0[j]
        off += BLOCK_SIZE[ty]
    n = off
    M = rng.normal(0, 1, (n + 10, n)) * 30.0
    A = np.ascontiguousarray(M.T @ M)
    b = np.ascontiguousarray(A @ rng.normal(0, 0.01, n))
    prior.valid, prior.n, prior.nblocks = 1, n, len(blocks)
    oracle.lib.dvo_prior_c0.restype = C.c_double
    oracle.lib.dvo_prior_c0.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    prior.c0 = oracle.lib.dvo_prior_c0(A.ctypes.data, b.ctypes.data, n)
    return prior, A, b


_CRAFTED = {}


def make_problem(oracle, name):
    from dynamic_vins_amd.backend import WindowProblem
    from tests import ba_gen
    if name == "vo11":
        return ba_gen.make_window(oracle, seed=613, nframes=11, use_imu=0, nlm=33, with_prior=True, max_iters=3)
    nframes, seed = {"f3": (3, 614), "imu1": (2, 615)}.get(name, (11, 611))
    base = ba_gen.make_window(oracle, seed=seed, nframes=nframes, nlm=0, with_prior=nframes == 11, max_iters=3)
    base.seed = seed
    if seed not in _CRAFTED:
        _CRAFTED[seed] = crafted_landmarks(base, nframes, seed + 1000)
    fac, lms, lam = _CRAFTED[seed]
    nlm = {"lm1": 1, "lm33": 33}.get(name, 17)
    lms = lms[:nlm]
    fac, lam = fac[: lms[-1]["first"] + lms[-1]["count"]], lam[:nlm]
    prior, A, b = (base.prior, base.prior_A, base.prior_b)
    if name in PRIORS:
        prior, A, b = make_prior(oracle, base, PRIORS[name], seed + 2000)
    return WindowProblem(base.pose, base.speed_bias, base.ex_pose, 0.0, lam, fac, lms, base.imu, use_imu=1, max_iters=3, prior=prior, prior_A=A, prior_b=b)


def input_digest(prob):
    h = hashlib.sha1()
    arrs = [prob.pose, prob.speed_bias, prob.ex_pose, prob.td, prob.inv_depth, prob.factors, prob.landmarks, prob.imu]
    if prob.prior is not None:
        arrs += [np.frombuffer(bytes(prob.prior), np.uint8), prob.prior_A, prob.prior_b]
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------- the device's buffers ----------------------------------------------------------------
def debug_buffer(ctx, which, set_, host, nbytes):
    from dynamic_vins_amd._abi import DvinsError
    if ctx.lib.dv_ba_debug_buffer(ctx.h, which, set_, host, nbytes) != 0:
        raise DvinsError(ctx.lib.dv_last_error(ctx.h).decode())


def fill_buffers(ctx):
    for which in range(len(BUFFERS)):
        for set_ in (0, 1):
            debug_buffer(ctx, which, set_, None, 0)


def read_buffers(ctx):
    """{name or name + set: the whole buffer as uint64 (lm_obs: uint32)}"""
    out = {}
    for which, (name, words, per_set) in enumerate(BUFFERS):
        for set_ in ((0, 1) if per_set else (0,)):
            a = np.zeros(words, np.uint32 if name == "lm_obs" else np.uint64)
            debug_buffer(ctx, which, set_, a.ctypes.data, a.nbytes)
            out[name + (str(set_) if per_set else "")] = a
    return out


def snapshot(ctx, prob):
    """the buffers cut down to what the problem's sizes can reach: packets to its landmarks' columns, the others to their first entries (Hd, Sc: n^2)"""
    nlm, nimu, n = len(prob.landmarks), len(prob.imu), NSTATE_MAX
    npr = prob.prior.n if prob.prior is not None else 0
    cut = {"packets": lambda a: np.ascontiguousarray(a.reshape(PK_SIZE, PK_STRIDE)[:, :nlm]), "imu_out": lambda a: a[: nimu * IMU_OUT], "prior_out": lambda a: a[: npr + 1],
           "cand_cost": lambda a: a[: nlm + nimu + 1], "lm_obs": lambda a: a[:nlm], "Hd": lambda a: a[: n * n], "Sc": lambda a: a[: n * n], "gvec": lambda a: a[: 2 * n]}
    return {k: cut[k.rstrip("01")](v) for k, v in read_buffers(ctx).items()}


def state_vector(prob):
    return np.concatenate([prob.pose.ravel(), prob.speed_bias.ravel(), prob.ex_pose.ravel(), prob.td.ravel(), prob.inv_depth.ravel()])


def run_case(ctx, oracle, name):
    """(input digest, {"eval.<buffer>" / "solve.<buffer>" / "solve.x": array}, summary of the solve)"""
    from dynamic_vins_amd.backend import ba_eval, ba_solve
    prob = make_problem(oracle, name)
    dig, out = input_digest(prob), {}
    fill_buffers(ctx)
    cost, _, _ = ba_eval(ctx, prob)
    out.update({"eval." + k: v for k, v in snapshot(ctx, prob).items()})
    out["eval.cost"] = np.array([cost]).view(np.uint64)
    fill_buffers(ctx)
    s = ba_solve(ctx, prob)
    out.update({"solve." + k: v for k, v in snapshot(ctx, prob).items()})
    out["solve.x"] = state_vector(prob).view(np.uint64)
    summ = dict(iterations=int(s.iterations), successful=int(s.successful), termination=int(s.termination), slots=int(s.slots),
                initial_cost=float(s.initial_cost).hex(), final_cost=float(s.final_cost).hex())
    return dig, out, summ


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def split_record(arrays, name):
    """(arrays recorded in full, {name: sha1} of the others)"""
    lim = FULL_BYTES if name in FULL_CASES else FULL_BYTES_REST
    return {k: v for k, v in arrays.items() if v.nbytes <= lim}, {k: sha1(v) for k, v in arrays.items() if v.nbytes > lim}


def run_batch(ctx_factory, frames=18):
    """two estimators (IMU, stereo) in a dv_batch: ({"window<i>": array}, {"member<i>.<buffer>": sha1 of the whole buffer}, the batch's counters)"""
    from dynamic_vins_amd.backend import Batch, Estimator
    from tests import test_batch as tb
    kw = dict(use_imu=1, stereo=1, max_iters=8, ric=[sim.R_IC, sim.R_IC], tic=[sim.T_IC0, sim.T_IC1], **tb.NOISE)
    S, dtf = 2, 0.1
    ests = [Estimator(ctx_factory(width=64, height=64, max_cnt=10, min_dist=5), **kw) for _ in range(S)]
    for e in ests:
        fill_buffers(e.ctx)
    inputs = [tb.make_inputs(i, 0.37 * i, 1) for i in range(S)]
    batch = Batch([e.ctx for e in ests])
    imu = [sim.imu_stream(tr, T0 - 0.05, T0 + frames * dtf + 0.1, 200.0, **tb.NOISE) for tr, _, T0 in inputs]
    k = [0] * S
    for f in range(frames):
        for i, (tr, fs, T0) in enumerate(inputs):
            t = T0 + f * dtf
            ts, acc, gyr = imu[i]
            while k[i] < len(ts) and ts[k[i]] <= t + 0.011:
                ests[i].InputIMU(ts[k[i]], acc[k[i]], gyr[k[i]])
                k[i] += 1
            assert ests[i].ProcessMeasurementsBegin(fs.frame(t), t) == 0
        batch.enqueue()
        for e in ests:
            e.ProcessMeasurementsEnd()
    windows = {"window%d" % i: np.ascontiguousarray(e.window(), np.float64).view(np.uint64) for i, e in enumerate(ests)}
    digests = {"member%d.%s" % (i, name): sha1(a) for i, e in enumerate(ests) for name, a in read_buffers(e.ctx).items()}
    info = batch.info()
    batch.close()
    return windows, digests, info


# ---------------------------------------------------------------- tests ----------------------------------------------------------------
@pytest.fixture(scope="module")
def results(gpu_ctx_factory, oracle):
    ctx = gpu_ctx_factory(width=64, height=48)
    return {name: run_case(ctx, oracle, name) for name in CASES}


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz")), json.load(open(os.path.join(GOLDEN, name + ".json")))


@pytest.mark.parametrize("name", CASES)
def test_evaluation_gives_the_recorded_bits(results, name):
    dig, arrays, summ = results[name]
    garr, gj = golden(name)
    assert dig == gj["input_sha1"], "the generated problem differs from the one the record was made on"
    assert summ == gj["summary"]
    full, digests = split_record(arrays, name)
    assert sorted(full) == sorted(garr.files) and sorted(digests) == sorted(gj["sha1"])
    bad = [k for k in full if not np.array_equal(full[k], garr[k])] + [k for k in digests if digests[k] != gj["sha1"][k]]
    for k in bad:
        if k in full:
            d = np.flatnonzero(full[k] != garr[k])
            print(name, k, "differs in", d.size, "of", full[k].size, "words; first at", d[:8], "shape", full[k].shape)
    assert not bad, bad


def test_cases_hold_what_they_claim(oracle):
    """the crafted window itself: the shapes the packet phase branches on are there"""
    p = make_problem(oracle, "lm17")
    L, F = p.landmarks, p.factors
    fac = lambda l: F[L[l]["first"]: L[l]["first"] + L[l]["count"]]
    assert L[0]["count"] == 1 and fac(0)["kind"][0] == 2 and L[0]["anchor"] == 10
    assert L[1]["count"] == 24 and L[1]["anchor"] == 0
    f2 = fac(2)
    left, right = set(f2["fj"][f2["kind"] == 0]), set(f2["fj"][f2["kind"] == 1])
    assert left - right and right - left and left & right
    assert [make_problem(oracle, n).prior.n for n in PRIORS] == [1, 63, 64, 65, 144]
    q = make_problem(oracle, "vo11")
    assert len(q.imu) == 0 and q.prior.n == 67 and len(make_problem(oracle, "imu1").imu) == 1 and len(make_problem(oracle, "f3").pose) == 3


def check_batch(windows, digests, info, rec_name):
    garr, gj = golden(rec_name)
    assert info["batched_rounds"] >= 4, info
    bad = [k for k in windows if not np.array_equal(windows[k], garr[k])] + [k for k in gj["sha1"] if digests[k] != gj["sha1"][k]]
    assert sorted(windows) == sorted(garr.files) and sorted(digests) == sorted(gj["sha1"]) and not bad, bad


def test_batched_form_gives_the_recorded_bits(gpu_ctx_factory):
    check_batch(*run_batch(gpu_ctx_factory), "batch")


def test_split_batched_form_gives_the_recorded_bits(tmp_path):
    """DVINS_EVAL_SPLIT is read once per process: the group runs in a child"""
    out = str(tmp_path / "split")
    env = dict(os.environ, DVINS_EVAL_SPLIT="1")
    r = subprocess.run([sys.executable, "-m", "tests.tools.eval_chain_golden", "--batch-only", "--out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    garr, gj = np.load(os.path.join(out, "batch.npz")), json.load(open(os.path.join(out, "batch.json")))
    check_batch({k: garr[k] for k in garr.files}, gj["sha1"], gj["info"], "batch_split")
