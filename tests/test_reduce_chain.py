"""be_reduce's pair blocks without the list barrier (be_solve.hip: be_reduce_pair_own — every row wave compacts the pair's landmarks into a list of its own, wave 6
fetches its tables itself, the operands of a lane's first trips are requested together): the change moves WHEN an operand is loaded, never which landmark a lane and a
trip take nor the order of the additions, so every word the reduce writes must keep the bits it had.  No tolerance anywhere in this file.

tests/golden/reduce_chain/<case>.npz / .json are records made with the library of the commit BEFORE the change (that commit's be_solve.hip; only buffer 8, scale_l, was
added to the read-back entry dv_ba_debug_buffer) by tests/tools/reduce_chain_golden.py.  Every case is run twice; each run fills Hd / Sc / gvec of both sets and scale_l
with 0xFF bytes, so that a word the reduce does NOT write is part of the comparison too, then
  eval    dv_ba_eval: one evaluation + one reduce with first = 1 (the scale comes from h, scale_l is written)
  solve   dv_ba_solve with max_iters = 4: the first reduce, then reduces with first = 0 (scale_l is read), speculative ones (spec = 1 with pending = 1: the other set
          and the other mu) and, once the solve has ended, idle slots
  again   (case idle only) a second dv_ba_solve from the solved states with the buffers filled in between: it ends at once and its remaining slots are idle
and what is compared is Hd, Sc, gvec of both sets (whole buffers: gvec in full, Hd / Sc as SHA-1, equal digests = every word equal), scale_l, lm_obs and the summary.

  case      frames nlm   what it holds (pair = (fi, fj), fi >= fj)
  lm0       11     0     no landmark: every list is empty, every pair block reaches its stores with cnt == 0
  lm1       11     1     one landmark seen in exactly two frames (anchored in 3, seen in 7)
  c63 c64 c65 c128 c129   N landmarks common to pair (6, 2) and to no other pair: the trip edge (64 lanes) and the bound of the unrolled trips (128 entries)
  c1000     11     1000  BE_MAX_LM landmarks, all common to pair (6, 2): all 16 chunks of lm_obs, sixteen trips (the general loop behind the unrolled form)
  sparse    11     1000  pair (8, 5) is hit only in chunk 0 and in chunk 15 of lm_obs (landmarks 3, 40, 61 and 960, 977, 999), the chunks between are empty for it
  anchors   11     48    pair (7, 3): every landmark anchored in fi; pair (8, 4): every landmark anchored in fj; pair (9, 5): both kinds; pair (2, 1): anchored in
                         neither (frame 0); the diagonal blocks of all of them
  nf2 nf5   2, 5   6, 20 small windows: the pair blocks of frames outside the window return early
  vo        11     33    vision only: pose 0 is constant (pose_col[0] = -1), no IMU columns, prior over 67
  noprior   11     33    IMU on, prior absent (lm1 ... anchors have the prior over 82)
  idle      11     33    the second solve (above)
Batched forms: two estimators in a dv_batch for 18 frames (windows of different nlm in one launch of be_reduce_batch_kernel), and the same in a child process under
DVINS_REDUCE_OCC=1 (be_reduce_batch_occ_kernel; the switch is read once per process); both against the recorded windows and buffer digests of the members.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dynamic_vins_amd import sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reduce_chain")
NSTATE_MAX, MAX_LM = 178, 1000
# dv_ba_debug_buffer: name -> (which, number of words, bytes per word, one buffer per set)
BUFFERS = {"Hd": (5, NSTATE_MAX * NSTATE_MAX, 8, True), "Sc": (6, NSTATE_MAX * NSTATE_MAX, 8, True), "gvec": (7, 2 * NSTATE_MAX, 8, True),
           "scale_l": (8, MAX_LM, 8, False), "lm_obs": (4, MAX_LM, 4, False)}
FILLED = ("Hd", "Sc", "gvec", "scale_l")          # lm_obs belongs to the evaluation: read, never filled
FULL_BYTES = 16 * 1024
COMMON = {"c63": 63, "c64": 64, "c65": 65, "c128": 128, "c129": 129, "c1000": 1000}
CASES = ["lm0", "lm1"] + list(COMMON) + ["sparse", "anchors", "nf2", "nf5", "vo", "noprior", "idle"]
SPARSE_HITS = (3, 40, 61, 960, 977, 999)


# ---------------------------------------------------------------- problems ----------------------------------------------------------------
def landmark_spec(name):
    """[(anchor, [observing frames])] of the case's landmarks"""
    if name == "lm0":
        return []
    if name == "lm1":
        return [(3, [7])]
    if name in COMMON:
        return [(2, [6])] * COMMON[name]
    if name == "sparse":
        others = [(0, [1]), (1, [2, 3]), (5, [6]), (8, [9]), (4, [5, 7]), (2, [8, 10])]          # none of them holds frames 5 AND 8
        return [(5, [8]) if l in SPARSE_HITS else others[l % len(others)] for l in range(MAX_LM)]
    if name == "anchors":
        return ([(7, [3])] * 7 + [(4, [8])] * 9 + [(9, [5]), (5, [9])] * 5 + [(0, [1, 2])] * 6 + [(0, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])] * 4
                + [(3, [4, 6, 10]), (6, [2, 5]), (10, [0, 9]), (1, [10])] * 3)
    if name == "nf2":
        return [(0, [1])] * 4 + [(1, [0])] * 2
    if name == "nf5":
        return [(0, [1, 2, 3, 4]), (1, [2, 4]), (2, [3]), (4, [0, 2]), (3, [4])] * 4
    rng = np.random.default_rng(7700 + len(name))
    out = []
    for _ in range(33):
        a = int(rng.integers(0, 9))
        out.append((a, [f for f in range(a + 1, 11) if rng.uniform() < 0.7] or [10]))
    return out


def crafted_landmarks(base, nframes, spec, seed):
    """the landmarks of `spec`, geometrically consistent with the window `base` (tests/ba_gen.py's trajectory and rig): one left-camera factor per observing frame,
    every third landmark with the anchor's stereo factor as well -> (factors, landmarks, inv_depth)"""
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
    assert len(pts) >= 16, len(pts)
    factors, lms, inv_depth = [], [], []
    for li, (a, frames) in enumerate(spec):
        P = pts[li % len(pts)]
        pi = proj(a, 0, P)[0] + rng.normal(0, 0.4 / 460.0, 2)
        first, mask = len(factors), 1 << a
        obs = [(0, f) for f in frames] + ([(2, a)] if li % 3 == 0 else [])
        for kd, f in obs:
            pj = proj(f, 0 if kd == 0 else 1, P)[0] + rng.normal(0, 0.4 / 460.0, 2)
            mask |= 1 << f
            factors.append((pi[0], pi[1], pj[0], pj[1], 0, 0, 0, 0, 0, 0, kd, li, a, f, (0, 0)))
        lms.append((first, len(factors) - first, a, mask))
        inv_depth.append(1.0 / (proj(a, 0, P)[1] * (1 + rng.normal(0, 0.08))))
    return np.array(factors, FACTOR_DTYPE), np.array(lms, LM_DTYPE), np.array(inv_depth)


def make_problem(oracle, name):
    from dynamic_vins_amd.backend import FACTOR_DTYPE, LM_DTYPE, WindowProblem
    from tests import ba_gen
    nframes = {"nf2": 2, "nf5": 5}.get(name, 11)
    use_imu = 0 if name == "vo" else 1
    seed = 700 + CASES.index(name)
    base = ba_gen.make_window(oracle, seed=seed, nframes=nframes, nlm=0, use_imu=use_imu, with_prior=name != "noprior", max_iters=4)
    base.seed = seed
    spec = landmark_spec(name)
    if spec:
        fac, lms, lam = crafted_landmarks(base, nframes, spec, seed + 1000)
    else:
        fac, lms, lam = np.zeros(0, FACTOR_DTYPE), np.zeros(0, LM_DTYPE), np.zeros(0)
    return WindowProblem(base.pose, base.speed_bias, base.ex_pose, 0.0, lam, fac, lms, base.imu, use_imu=use_imu, max_iters=4,
                         prior=base.prior, prior_A=base.prior_A, prior_b=base.prior_b)


def pair_counts(lm_obs, nframes=11):
    """{(fi, fj), fi >= fj: number of landmarks whose lm_obs carries both bits}"""
    ob = np.asarray(lm_obs, np.int64)
    return {(fi, fj): int((((ob >> fi) & 1) & ((ob >> fj) & 1)).sum()) for fi in range(nframes) for fj in range(fi + 1)}


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
    for name in FILLED:
        for set_ in ((0, 1) if BUFFERS[name][3] else (0,)):
            debug_buffer(ctx, BUFFERS[name][0], set_, None, 0)


def read_buffers(ctx, nlm=MAX_LM):
    """{name or name + set: the whole buffer as uint64; lm_obs: its first nlm words as uint32}"""
    out = {}
    for name, (which, words, size, per_set) in BUFFERS.items():
        for set_ in ((0, 1) if per_set else (0,)):
            a = np.zeros(nlm if name == "lm_obs" else words, np.uint32 if size == 4 else np.uint64)
            if a.size:
                debug_buffer(ctx, which, set_, a.ctypes.data, a.nbytes)
            out[name + (str(set_) if per_set else "")] = a
    return out


def summary(s):
    return dict(iterations=int(s.iterations), successful=int(s.successful), termination=int(s.termination), slots=int(s.slots),
                initial_cost=float(s.initial_cost).hex(), final_cost=float(s.final_cost).hex())


def run_case(ctx, oracle, name):
    """(input digest, {"eval.<buffer>" / "solve.<buffer>" [/ "again.<buffer>"]: array}, summaries)"""
    from dynamic_vins_amd.backend import ba_eval, ba_solve
    prob = make_problem(oracle, name)
    nlm = len(prob.landmarks)
    dig, out, summ = input_digest(prob), {}, {}
    fill_buffers(ctx)
    cost, _, _ = ba_eval(ctx, prob)
    out.update({"eval." + k: v for k, v in read_buffers(ctx, nlm).items()})
    out["eval.cost"] = np.array([cost]).view(np.uint64)
    fill_buffers(ctx)
    summ["solve"] = summary(ba_solve(ctx, prob))
    out.update({"solve." + k: v for k, v in read_buffers(ctx, nlm).items()})
    if name == "idle":
        fill_buffers(ctx)
        summ["again"] = summary(ba_solve(ctx, prob))
        out.update({"again." + k: v for k, v in read_buffers(ctx, nlm).items()})
    return dig, out, summ


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def split_record(arrays):
    """(arrays recorded in full, {name: sha1} of the others)"""
    return {k: v for k, v in arrays.items() if v.nbytes <= FULL_BYTES}, {k: sha1(v) for k, v in arrays.items() if v.nbytes > FULL_BYTES}


def run_batch(ctx_factory, frames=18):
    """two estimators (IMU, stereo) in a dv_batch: ({"window<i>": array}, {"member<i>.<buffer>": sha1 of the whole buffer}, the batch's counters)"""
    from dynamic_vins_amd.backend import Batch, Estimator
    from tests import test_batch as tb
    kw = dict(use_imu=1, stereo=1, max_iters=8, ric=[sim.R_IC, sim.R_IC], tic=[sim.T_IC0, sim.T_IC1], **tb.NOISE)
    S, dtf = 2, 0.1
    ests = [Estimator(ctx_factory(width=64, height=64, max_cnt=10, min_dist=5), **kw) for _ in range(S)]          # (tests/test_batch.py: the members' feature counts differ, and so do their windows' nlm)
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
    info["n_landmarks"] = [int(e.state.n_landmarks) for e in ests]
    batch.close()
    return windows, digests, info


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz")), json.load(open(os.path.join(GOLDEN, name + ".json")))


# ---------------------------------------------------------------- tests ----------------------------------------------------------------
@pytest.fixture(scope="module")
def case_ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=64, height=48)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_reduce_gives_the_recorded_bits(case_ctx, oracle, name):
    garr, gj = golden(name)
    for run in (0, 1):
        dig, arrays, summ = run_case(case_ctx, oracle, name)
        assert dig == gj["input_sha1"], "the generated problem differs from the one the record was made on"
        assert summ == gj["summary"]
        full, digests = split_record(arrays)
        assert sorted(full) == sorted(garr.files) and sorted(digests) == sorted(gj["sha1"])
        bad = [k for k in full if not np.array_equal(full[k], garr[k])] + [k for k in digests if digests[k] != gj["sha1"][k]]
        for k in bad:
            if k in full:
                d = np.flatnonzero(full[k] != garr[k])
                print(name, "run", run, k, "differs in", d.size, "of", full[k].size, "words; first at", d[:8])
        assert not bad, (run, bad)


def test_cases_hold_what_they_claim(oracle):
    """the records themselves (no GPU): the counts per pair, from the recorded lm_obs, are what the case names say, and the generated problems agree with them"""
    for name in CASES:
        garr, gj = golden(name)
        prob = make_problem(oracle, name)
        assert input_digest(prob) == gj["input_sha1"], name
        L, F = prob.landmarks, prob.factors
        want = np.array([(1 << int(l["anchor"])) | int(np.bitwise_or.reduce(1 << F["fj"][l["first"]: l["first"] + l["count"]].astype(np.int64))) for l in L], np.uint32)
        for part in ("eval", "solve"):
            assert np.array_equal(garr[part + ".lm_obs"], want), (name, part)
        assert gj["pair_counts"] == {"%d,%d" % k: v for k, v in pair_counts(want).items() if v}, name
    pc = lambda name: pair_counts(golden(name)[0]["eval.lm_obs"])
    assert golden("lm0")[0]["eval.lm_obs"].size == 0
    assert {k: v for k, v in pc("lm1").items() if v} == {(3, 3): 1, (7, 3): 1, (7, 7): 1}
    for name, cnt in COMMON.items():
        assert {k: v for k, v in pc(name).items() if v} == {(2, 2): cnt, (6, 2): cnt, (6, 6): cnt}, name
    ob = golden("sparse")[0]["eval.lm_obs"].astype(np.int64)
    assert ob.size == MAX_LM and tuple(np.flatnonzero(((ob >> 8) & 1) & ((ob >> 5) & 1))) == SPARSE_HITS          # chunks 0 and 15 only
    P = make_problem(oracle, "anchors")
    anc, ob = P.landmarks["anchor"], golden("anchors")[0]["eval.lm_obs"].astype(np.int64)
    both = lambda fi, fj: ((ob >> fi) & 1) & ((ob >> fj) & 1) == 1
    assert set(anc[both(7, 3)]) == {7, 0} and set(anc[both(8, 4)]) == {4, 0} and set(anc[both(9, 5)]) == {9, 5, 0} and set(anc[both(2, 1)]) == {0}          # (0: anchored in neither)
    assert len(make_problem(oracle, "nf2").pose) == 2 and len(make_problem(oracle, "nf5").pose) == 5
    q = make_problem(oracle, "vo")
    assert len(q.imu) == 0 and q.prior.n == 67 and make_problem(oracle, "noprior").prior is None and len(make_problem(oracle, "noprior").imu) == 10
    gi = golden("idle")[1]["summary"]
    assert gi["again"]["iterations"] < gi["again"]["slots"] or gi["again"]["iterations"] <= 2, gi          # the second solve leaves idle slots behind


def check_batch(windows, digests, info, rec_name):
    garr, gj = golden(rec_name)
    assert info["batched_rounds"] >= 4, info
    assert info["n_landmarks"] == gj["info"]["n_landmarks"] and len(set(info["n_landmarks"])) == 2, info
    bad = [k for k in windows if not np.array_equal(windows[k], garr[k])] + [k for k in gj["sha1"] if digests[k] != gj["sha1"][k]]
    assert sorted(windows) == sorted(garr.files) and sorted(digests) == sorted(gj["sha1"]) and not bad, bad


@pytest.mark.gpu
def test_batched_form_gives_the_recorded_bits(gpu_ctx_factory):
    check_batch(*run_batch(gpu_ctx_factory), "batch")


@pytest.mark.gpu
def test_occupancy_batched_form_gives_the_recorded_bits(tmp_path):
    """DVINS_REDUCE_OCC is read once per process: the group runs in a child"""
    out = str(tmp_path / "occ")
    env = dict(os.environ, DVINS_REDUCE_OCC="1")
    r = subprocess.run([sys.executable, "-m", "tests.tools.reduce_chain_golden", "--batch-only", "--out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    garr, gj = np.load(os.path.join(out, "batch.npz")), json.load(open(os.path.join(out, "batch.json")))
    check_batch({k: garr[k] for k in garr.files}, gj["sha1"], gj["info"], "batch_occ")
