"""Crafted marginalization inputs (test input, no GPU): full 11-frame windows WITHOUT factors, landmarks or IMU whose prior is built to order, so that
dv_marginalize runs on the prior alone: be_marg_finish (Schur complement of the dropped block) and be_marg_eig (Jacobi + the 1e-8 clamp) at every kept size the
block types can form, at every drop shape, and on spectra no window prior has.  tests/test_marg_cases.py checks the generator and tests/ba_ref.py::marginalize
against a direct restatement; tests/test_marg_cases_gpu.py runs the device against both.

Blocks are (type, idx) with type 0 pose (6), 1 speed-bias (9), 2 extrinsic (6), 3 td (1), as in dv_ba_prior_block.  Mode 1 (kMarginSecondNew) drops pose 9,
mode 0 (kMarginOld) drops pose 0 and / or speed-bias 0.  The kernel scatters the prior through prior_map into [dropped | kept in canonical order]: canonical is
poses, speed-biases, ex0, ex1, td, each by index — the order of the new prior's header.

coupled=False: the prior is block diagonal between the dropped and the kept part and the kept part is K = Q diag(lambda) Q^T in canonical order with lambda
PRESCRIBED, so A' = K exactly (the elimination subtracts products with exact zeros), the spectrum and the rank are known, and x0 equals the states (dx = 0:
b' is the kept part of b).  b_kept = K x + sum beta_k q_k with beta on the clamped directions (lambda_k <= 1e-8), which the eigen form must project off.
`straddle` is the exception: its clamped 5e-9 and its kept 2e-8 eigenvector are 1.5e-8 apart, so the STORED matrix (entries rounded at eps |K|) defines
the two only to an angle theta ~ n eps |K| / 1.5e-8 ~ 1e-7 — any component of b in their plane comes back wrong by theta times its size in any implementation.
There beta is 0 on the 5e-9 vector and 1e-4 |b| on the 2e-8 one: the error theta 1e-4 stays under the 1e-9 bar while the 2e-8 eigenvalue still carries a
visible share beta^2 / 2e-8 of c0.
coupled=True: a random SPD prior M^T M over all blocks (M has D + 8 rows: condition ~1e4), x0 beside the states (dx != 0: b' = Schur(b + A dx)), `scale`
multiplies M (3000: norm ~1e9, the prior_scale of the window sweep).

Every case keeps its eigenvalues at least 1e3 n eps |A'| away from the 1e-8 threshold (margin()): closer than that the clamp decision is rounding.  `wide`
therefore spans max(1e-3, 2e3 n eps 1e9) .. 1e9: a lower end of 1e-3 at norm 1e9 satisfies that condition only for n <= 4."""
import ctypes as C

import numpy as np

from dynamic_vins_amd.backend import FACTOR_DTYPE, IMU_DTYPE, LM_DTYPE, WindowProblem, dv_ba_prior
from tests import ba_ref, oracle_py

EPS = np.finfo(np.float64).eps
CLAMP = 1e-8                                  # marginalization_factor.cpp:297-308
LOCAL = {0: 6, 1: 9, 2: 6, 3: 1}
GLOBAL = {0: 7, 1: 9, 2: 7, 3: 1}
SPECTRA = ("diag", "zero", "two_clusters", "indefinite", "straddle", "wide", "tiny_offdiag")
DROPS = {1: [[(0, 9)]], 0: [[(0, 0), (1, 0)], [(0, 0)], [(1, 0)]]}
MAX_BLOCKS = 16                               # dv_ba_prior::blocks


def reachable_sizes(nmax=96):
    """kept sizes the block types (6, 9, 6, 1; one td) can form: 1, and every n >= 6 with n mod 3 in {0, 1}"""
    return [1] + [n for n in range(6, nmax + 1) if n % 3 != 2]


def available(mode):
    """(6-dim blocks, 9-dim blocks) a kept list may hold: mode 1 keeps poses 0-8 and 10 (at most 10) and the speed-biases but that of frame 9 (frame 10's
    takes its index in the new header, as the pose does: the reference asserts that a kMarginSecondNew prior holds neither block of frame 9 but the pose it
    drops, estimator.cpp:591-612); mode 0 drops frame 0's blocks"""
    lo = 0 if mode == 1 else 1
    return [(0, k) for k in range(lo, 11) if not (mode == 1 and k == 9)] + [(2, 0), (2, 1)], [(1, k) for k in range(lo, 11) if not (mode == 1 and k == 9)]


def kept_blocks(n, mode, seed=0, ndropped=1):
    """one kept block list with n dims in canonical order; the mix of poses / extrinsics / speed-biases varies with the seed"""
    rng = np.random.default_rng([seed, n, mode])
    six, nine = available(mode)
    t = 1 if n % 3 == 1 else 0
    cand = [(a, b) for b in range(len(nine) + 1) for a in range(len(six) + 1) if 6 * a + 9 * b == n - t and a + b + t + ndropped <= MAX_BLOCKS]
    assert cand, f"no block list with {n} kept dims in mode {mode}"
    a, b = cand[rng.integers(len(cand))]
    out = [six[i] for i in rng.choice(len(six), a, replace=False)] + [nine[i] for i in rng.choice(len(nine), b, replace=False)] + [(3, 0)] * t
    return sorted(out)


def shifted(key, mode):
    """the block's key in the new prior's header (estimator.cpp:537-548 / 591-612)"""
    ty, idx = key
    if ty > 1:
        return key
    return (ty, idx - 1) if mode == 0 else (ty, 9 if idx == 10 else idx)


def margin(lam, n):
    """(distance of the spectrum from the clamp threshold, the distance a case must keep: 1e3 n eps |A'|)"""
    lam = np.asarray(lam, float)
    return float(np.abs(lam - CLAMP).min()), 1e3 * n * EPS * float(np.abs(lam).max())


def spectrum(name, n, rng):
    """the prescribed eigenvalues of the kept part (in the order of Q's columns)"""
    if name in ("diag", "tiny_offdiag"):      # repeated entries on purpose: the ascending sort must break exact ties by index
        return rng.choice([-1.0, 0.0, 0.25, 2.0, 64.0], n)
    if name == "zero":
        return np.zeros(n)
    if name == "two_clusters":                # one clamped, one kept, each n / 2 times
        return np.array([0.0] * (n // 2) + [3.0] * (n - n // 2))
    if name == "indefinite":
        k = (n + 3) // 4
        return np.concatenate([-10.0 ** rng.uniform(-3, 0, k), 10.0 ** rng.uniform(-2, 2, n - k)])
    if name == "straddle":
        return np.array([2e-8]) if n == 1 else np.concatenate([[5e-9, 2e-8], rng.uniform(0.5, 2.0, n - 2)])
    if name == "wide":
        lo = max(1e-3, 2e3 * n * EPS * 1e9)
        return np.array([1e9]) if n == 1 else np.concatenate([[lo, 1e9], 10.0 ** rng.uniform(np.log10(lo), 9, n - 2)])
    raise ValueError(name)


def _states(rng):
    pose, ex = np.zeros((11, 7)), np.zeros((2, 7))
    for x in (pose, ex):
        x[:, :3] = rng.normal(0, 1, (len(x), 3))
        q = rng.normal(0, 1, (len(x), 4))
        x[:, 3:] = q / np.linalg.norm(q, axis=1)[:, None]
    return pose, rng.normal(0, 0.5, (11, 9)), ex, float(rng.normal(0, 0.01))


def _beside(x, ty, rng):
    """a linearisation point a little off the state x (dx ~ 1e-2)"""
    x0 = np.array(x, float).copy()
    if ty in (0, 2):
        x0[:3] += rng.normal(0, 0.01, 3)
        q = ba_ref.qmul(x0[3:], np.concatenate([rng.normal(0, 0.005, 3), [1.0]]))
        x0[3:] = q / np.linalg.norm(q)
    else:
        x0 += rng.normal(0, 0.01 if ty == 1 else 0.001, len(x0))
    return x0


def make_prior_case(kept, dropped, spectrum_name, coupled, seed, permute, scale=1.0, null_on_dropped=False):
    """a WindowProblem for dv_marginalize / ba_ref.marginalize (mode 1 if pose 9 is dropped, else mode 0) with the prior described in the module docstring.
    kept: canonical list of (type, idx); dropped: the blocks the mode removes ([] for the empty case: the mode then finds nothing to drop).
    null_on_dropped: the whole prior is Q diag(lambda) Q^T with ONE eigenvalue 1e-10 whose vector lives on the dropped coordinates (a pivot of A_mm under
    1e-8), every other eigenvalue in 1e-2 .. 1e2, b = A x exactly consistent (the LDL^T that skips the pivot and the eigen pseudo-inverse then coincide).
    The result carries .truth: mode, n, m, blocks {shifted key: (off, size)} of the canonical kept order and, for coupled=False, K, Q, lam, beta, b_kept."""
    rng = np.random.default_rng(seed)
    kept, dropped = sorted(kept), sorted(dropped)
    assert len(set(kept + dropped)) == len(kept) + len(dropped) <= MAX_BLOCKS
    mode = 1 if (0, 9) in dropped or not dropped else 0
    pose, sb, ex, td = _states(rng)
    state = {0: pose, 1: sb, 2: ex, 3: np.array([[td]])}
    order = dropped + kept
    if permute:
        order = [order[i] for i in rng.permutation(len(order))]
    off, offs = 0, {}
    for k in order:
        offs[k] = off
        off += LOCAL[k[0]]
    D = off
    n, m = sum(LOCAL[k[0]] for k in kept), sum(LOCAL[k[0]] for k in dropped)
    pos_k = np.array([offs[k] + c for k in kept for c in range(LOCAL[k[0]])], int)
    pos_d = np.array([offs[k] + c for k in dropped for c in range(LOCAL[k[0]])], int)
    A, b = np.zeros((D, D)), np.zeros(D)
    truth = dict(mode=mode, n=n, m=m, spectrum=spectrum_name, coupled=coupled)
    o, truth["blocks"] = 0, {}
    for k in kept:
        truth["blocks"][shifted(k, mode)] = (o, LOCAL[k[0]], None)
        o += LOCAL[k[0]]
    if null_on_dropped:
        assert m > 0 and not coupled
        pos = np.concatenate([pos_d, pos_k])
        q0 = np.zeros(D)
        q0[:m] = rng.uniform(0.5, 1.0, m) * rng.choice([-1.0, 1.0], m)
        q0 /= np.linalg.norm(q0)
        M = rng.normal(0, 1, (D, D))
        M[:, 0] = q0
        Q, _ = np.linalg.qr(M)
        Q[:, 0] = q0
        lam = np.concatenate([[1e-10], 10.0 ** rng.uniform(-2, 2, D - 1)])
        F = (Q * lam) @ Q.T
        F = 0.5 * (F + F.T)
        A[np.ix_(pos, pos)] = F
        b[pos] = F @ rng.normal(0, 0.1, D)
        truth.update(lam_full=lam, q0=q0)
    elif coupled:
        M = rng.normal(0, 1, (D + 8, D)) * scale
        A = M.T @ M
        A = 0.5 * (A + A.T)
        b = A @ rng.normal(0, 0.1, D)
    else:
        lam = spectrum(spectrum_name, n, rng)
        if spectrum_name in ("diag", "tiny_offdiag"):
            Q = np.eye(n)
        else:
            Q, _ = np.linalg.qr(rng.normal(0, 1, (n, n)))
        K = (Q * lam) @ Q.T
        K = 0.5 * (K + K.T)
        if spectrum_name == "tiny_offdiag":
            K = K + 1e-305 * (1.0 - np.eye(n))
        Kx = K @ rng.normal(0, 0.1, n)
        bs = max(float(np.abs(Kx).max()), 1.0) if lam.any() else 1.0
        beta = np.where(lam <= CLAMP, bs * rng.uniform(0.5, 1.5, n), 0.0)
        if spectrum_name == "straddle":
            beta = np.where(lam == 2e-8, 1e-4 * bs, 0.0)
        bk = Kx + Q @ beta
        A[np.ix_(pos_k, pos_k)] = K
        b[pos_k] = bk
        if m:
            Md = rng.normal(0, 1, (m + 8, m))
            Dm = Md.T @ Md + np.eye(m)
            A[np.ix_(pos_d, pos_d)] = 0.5 * (Dm + Dm.T)
            b[pos_d] = rng.normal(0, 1, m)
        d, need = margin(lam, n)
        assert d >= need, (spectrum_name, n, d, need)
        truth.update(K=K, Q=Q, lam=lam, beta=beta, b_kept=bk)
    pr = dv_ba_prior()
    for i, k in enumerate(order):
        pb = pr.blocks[i]
        pb.type, pb.idx, pb.off, pb.size_local = k[0], k[1], offs[k], LOCAL[k[0]]
        x = state[k[0]][k[1]]
        x0 = _beside(x, k[0], rng) if coupled else x
        for j in range(GLOBAL[k[0]]):
            pr.x0[i][j] = float(x0[j])
    A, b = np.ascontiguousarray(A), np.ascontiguousarray(b)
    lib = oracle_py.load().lib
    lib.dvo_prior_c0.restype = C.c_double
    lib.dvo_prior_c0.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    pr.valid, pr.n, pr.nblocks, pr.c0 = 1, D, len(order), lib.dvo_prior_c0(A.ctypes.data, b.ctypes.data, D)
    prob = WindowProblem(pose, sb, ex, td, np.zeros(0), np.zeros(0, FACTOR_DTYPE), np.zeros(0, LM_DTYPE), np.zeros(0, IMU_DTYPE), use_imu=1,
                         prior=pr, prior_A=A, prior_b=b)
    prob.truth = truth
    return prob


def reference(prob):
    """ba_ref.marginalize of a case, computed once per case object; for coupled cases the threshold condition is asserted here from eigvalsh of its A'"""
    if getattr(prob, "ref", None) is None:
        t = prob.truth
        prob.ref = ba_ref.marginalize(oracle_py.load(), prob, t["mode"])
        if t["coupled"] or "lam_full" in t:
            d, need = margin(np.linalg.eigvalsh(prob.ref["A"]), t["n"])
            assert d >= need, (t["n"], d, need)
    return prob.ref


# ---------------------------------------------------------------- the case lists of tests/test_marg_cases*.py
SPECTRUM_SIZES = (1, 6, 7, 9, 16, 31, 33, 48, 49, 64, 81, 88)
DROP_SIZES = (7, 30, 61, 85)


def sweep_case(n, scale=1.0):
    """mode 1, coupled, permuted: part (a) (scale 1) and (b) (scale 3000) of the GPU test"""
    return make_prior_case(kept_blocks(n, 1, seed=n), [(0, 9)], None, True, 1000 + n, True, scale=scale)


def spectrum_case(n, name):
    """mode 1, block diagonal, permuted: part (c); `tiny_offdiag` shares its seed (hence lambda, b) with `diag`"""
    return make_prior_case(kept_blocks(n, 1, seed=n + 7), [(0, 9)], name, False, 2000 + 10 * n + (0 if name == "tiny_offdiag" else SPECTRA.index(name)), True)


def drop_case(n, dropped):
    """mode 0, coupled, permuted: part (d)"""
    return make_prior_case(kept_blocks(n, 0, seed=n + 3, ndropped=len(dropped)), dropped, None, True, 3000 + 10 * n + len(dropped) + dropped[0][0], True)


def null_pivot_case(n=30):
    """mode 0, pose 0 and speed-bias 0 dropped, the prior's 1e-10 eigenvector on their coordinates"""
    return make_prior_case(kept_blocks(n, 0, seed=5, ndropped=2), [(0, 0), (1, 0)], None, False, 4000, True, null_on_dropped=True)


def all_cases():
    """(id, maker) of every generated case"""
    out = [(f"sweep-n{n}", lambda n=n: sweep_case(n)) for n in reachable_sizes()]
    out += [(f"big-n{n}", lambda n=n: sweep_case(n, 3000.0)) for n in reachable_sizes(89)[::4]]
    out += [(f"{s}-n{n}", lambda n=n, s=s: spectrum_case(n, s)) for s in SPECTRA for n in SPECTRUM_SIZES]
    out += [(f"drop{'+'.join(str(t) for t, _ in d)}-n{n}", lambda n=n, d=d: drop_case(n, d)) for d in DROPS[0] for n in DROP_SIZES]
    out += [("null-pivot", null_pivot_case)]
    return out
