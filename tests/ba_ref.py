"""Plain float64 reference of the window solve's linear algebra (test infrastructure, numpy only).

From a `WindowProblem` (tests/ba_gen.py) it assembles the full normal equations over poses, speed-biases, free extrinsic / td blocks and inverse depths from
per-residual evaluations, then reduces, solves and Schur-complements them DENSELY with numpy.  The factors come from the CPU oracle's per-factor entry points
(dvo_proj_eval, dvo_imu_eval: the ones tests/test_back_parity.py checks the HIP factors against), the Huber corrector is ceres' in full (both branches,
oracle/back_solver.h:correct), the prior is the information form of include/dvins.h (cost c0/2 + b.dx + dx.A dx/2).  Nothing here follows the kernels' own
arithmetic (per-landmark packets, tiles, LDL^T): the dense formulation is what they must agree with.

Column layout (dv_ba_eval's documented order): per frame 6 pose columns (unless the pose is constant: frame 0 without IMU), then 9 speed-bias columns (use_imu);
then the free extrinsic (6 + 6) and td (1) columns; the landmark columns follow all of these in the full system."""
import ctypes as C

import numpy as np

EPS = np.finfo(np.float64).eps
LOCAL = {"pose": 6, "sb": 9, "ex": 6, "td": 1, "lm": 1}
KWIN = 10                     # kWinSize: the block shifts of dv_marginalize / dvo_marginalize


# ---------------------------------------------------------------- quaternions (x y z w) and the local parameterisation
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def qinv(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def pose_plus(x7, d6, plane_kind=0):
    """PoseLocalParameterization::Plus: p + dp (dz dropped under plane kind 1, dy under 2), q * [1, dtheta / 2] normalised"""
    out = np.array(x7, float).copy()
    dp = np.array(d6[:3], float).copy()
    if plane_kind == 1:
        dp[2] = 0.0
    elif plane_kind == 2:
        dp[1] = 0.0
    out[:3] += dp
    dq = np.array([d6[3] / 2, d6[4] / 2, d6[5] / 2, 1.0])
    q = qmul(x7[3:], dq / np.linalg.norm(dq))
    out[3:] = q / np.linalg.norm(q)
    return out


def pose_minus(x7_new, x7_old):
    """the exact inverse of pose_plus (no plane constraint): q_old^-1 q_new = [v, w] = [dtheta / 2, 1] / |.|, so dtheta = 2 v / w = 2 v / sqrt(1 - |v|^2)"""
    p = qmul(qinv(x7_old[3:]), x7_new[3:])
    if p[3] < 0:
        p = -p
    return np.concatenate([np.asarray(x7_new[:3]) - np.asarray(x7_old[:3]), 2.0 * p[:3] / p[3]])


def pose_dx(x7, x0_7):
    """MarginalizationFactor's dx of a 7-block: [p - p0, 2 positify(q0^-1 q).vec]"""
    p = qmul(qinv(x0_7[3:]), x7[3:])
    v = 2.0 * p[:3]
    if not p[3] >= 0:
        v = -v
    return np.concatenate([np.asarray(x7[:3]) - np.asarray(x0_7[:3]), v])


# ---------------------------------------------------------------- ceres::HuberLoss(1) + Corrector
def huber_correct(r, Js):
    """(corrected r, corrected Jacobians, cost) of one residual block under HuberLoss(1.0) with ceres' Corrector, both branches"""
    sq = float(r @ r)
    tiny = np.finfo(float).tiny
    if sq > 1.0:
        sr = np.sqrt(sq)
        rho = (2 * sr - 1, max(tiny, 1.0 / sr), -max(tiny, 1.0 / sr) / (2 * sq))
    else:
        rho = (sq, 1.0, 0.0)
    sqrt_rho1 = np.sqrt(rho[1])
    if sq == 0.0 or rho[2] <= 0.0:
        scaling, alpha_sq_norm = sqrt_rho1, 0.0
    else:
        D = 1.0 + 2.0 * sq * rho[2] / rho[1]
        alpha = 1.0 - np.sqrt(D)
        scaling, alpha_sq_norm = sqrt_rho1 / (1 - alpha), alpha / sq
    Jc = [sqrt_rho1 * (J - alpha_sq_norm * np.outer(r, r @ J)) for J in Js]
    return r * scaling, Jc, 0.5 * rho[0]


# ---------------------------------------------------------------- residual blocks
class Residual:
    """one residual block after its loss: r, [(block key, Jacobian on the block's local parameters)], cost; mag: None (rounding scales with |r|, |J| themselves) or,
    for the IMU factor, (|r| bound, [|J| bounds], M_W, |r_raw|, [|J_raw|]): entrywise bounds of the whitening product and of its weight matrix (imu_residual)"""
    __slots__ = ("r", "blocks", "cost", "mag")

    def __init__(self, r, blocks, cost, mag=None):
        self.r, self.blocks, self.cost, self.mag = r, blocks, cost, mag


def _bind(oracle):
    lib = oracle.lib
    lib.dvo_proj_eval.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dvo_preint_create.restype = C.c_void_p
    lib.dvo_preint_create.argtypes = [C.c_void_p] * 5
    lib.dvo_preint_set.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dvo_preint_destroy.argtypes = [C.c_void_p]
    lib.dvo_imu_eval.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _eval(fn, head, blocks, nres):
    blocks = [np.ascontiguousarray(b, np.float64) for b in blocks]
    J = [np.zeros(nres * len(b)) for b in blocks]
    par = (C.c_void_p * len(blocks))(*[b.ctypes.data for b in blocks])
    Jp = (C.c_void_p * len(blocks))(*[j.ctypes.data for j in J])
    r = np.zeros(nres)
    fn(*head, par, r.ctypes.data, Jp)
    return r, [j.reshape(nres, -1) for j in J]


def proj_residual(lib, f, pose, ex, lam, td, lm_key):
    """one reprojection block (kinds 0, 1, 2) after the Huber corrector; pose / extrinsic Jacobians keep their first 6 columns (ComputeJacobian = [I6; 0])"""
    kind, fi, fj = int(f["kind"]), int(f["fi"]), int(f["fj"])
    obs = np.array([f["pix"], f["piy"], 1.0, f["pjx"], f["pjy"], 1.0, f["vix"], f["viy"], f["vjx"], f["vjy"], f["td_i"], f["td_j"]])
    lk, tk = np.array([lam]), np.array([td])
    if kind == 0:
        blocks, keys = [pose[fi], pose[fj], ex[0], lk, tk], [("pose", fi), ("pose", fj), ("ex", 0), lm_key, ("td", 0)]
    elif kind == 1:
        blocks, keys = [pose[fi], pose[fj], ex[0], ex[1], lk, tk], [("pose", fi), ("pose", fj), ("ex", 0), ("ex", 1), lm_key, ("td", 0)]
    else:
        blocks, keys = [ex[0], ex[1], lk, tk], [("ex", 0), ("ex", 1), lm_key, ("td", 0)]
    r, J = _eval(lib.dvo_proj_eval, (kind, obs.ctypes.data), blocks, 2)
    J = [j[:, :6] if j.shape[1] == 7 else j for j in J]
    rc, Jc, cost = huber_correct(r, J)
    return Residual(rc, list(zip(keys, Jc)), cost)


def imu_residual(lib, rec, g_norm, pose, sb):
    fi, fj = int(rec["fi"]), int(rec["fj"])
    z, noise = np.zeros(3), np.zeros(4)
    lin_ba, lin_bg = np.ascontiguousarray(rec["lin_ba"], np.float64), np.ascontiguousarray(rec["lin_bg"], np.float64)
    h = lib.dvo_preint_create(z.ctypes.data, z.ctypes.data, lin_ba.ctypes.data, lin_bg.ctypes.data, noise.ctypes.data)
    try:
        dq = rec["dq"]
        dq_xyzw = np.array([dq[1], dq[2], dq[3], dq[0]])
        dp, dv = np.ascontiguousarray(rec["dp"], np.float64), np.ascontiguousarray(rec["dv"], np.float64)
        jac, cov = np.ascontiguousarray(rec["jacobian"], np.float64), np.ascontiguousarray(rec["covariance"], np.float64)
        lib.dvo_preint_set(h, float(rec["sum_dt"]), dp.ctypes.data, dq_xyzw.ctypes.data, dv.ctypes.data, jac.ctypes.data, cov.ctypes.data)
        r, J = _eval(lib.dvo_imu_eval, (h, float(g_norm)), [pose[fi], sb[fi], pose[fj], sb[fj]], 15)
    finally:
        lib.dvo_preint_destroy(h)
    keys = [("pose", fi), ("sb", fi), ("pose", fj), ("sb", fj)]
    J = [J[0][:, :6], J[1], J[2][:, :6], J[3]]
    # r = U r_raw, J = U J_raw with U = sqrt_info (LLT of the information matrix W = cov^-1, entries ~1e4 of both signs).  Two places lose digits:
    #  - the whitening product cancels, so r and J carry rounding of the size of |U| |r_raw|, |U| |J_raw| rather than of their own;
    #  - W itself: any float64 inverse of cov (cond ~5e5) is off entrywise by ~eps (|W| |cov| |W|), the first-order bound of a computed inverse, and two
    #    correct implementations (the oracle's, be_api.hip's Gauss-Jordan + Cholesky) differ by that much: J_raw,i^T dW J_raw,j is bounded by
    #    eps |J_raw,i|^T (|W| |cov| |W|) |J_raw,j|.
    cov = np.asarray(rec["covariance"], np.float64).reshape(15, 15)
    W = np.linalg.inv(cov)
    U = np.linalg.cholesky(0.5 * (W + W.T)).T
    aU, MW = np.abs(U), np.abs(W) @ np.abs(cov) @ np.abs(W)
    r_raw, J_raw = np.abs(np.linalg.solve(U, r)), [np.abs(np.linalg.solve(U, j)) for j in J]
    #  - the rotation Jacobians of the position and velocity residuals are skew(R_i^T (p_j - p_i - v_i dt + g dt^2 / 2)), skew(R_i^T (v_j - v_i + g dt)): formed
    #    from absolute states, they carry rounding of the size of the states, not of the difference
    dt = float(rec["sum_dt"])
    pi_, pj_, vi_, vj_ = pose[fi][:3], pose[fj][:3], sb[fi][:3], sb[fj][:3]
    sp = np.linalg.norm(pi_) + np.linalg.norm(pj_) + np.linalg.norm(vi_) * dt + 0.5 * g_norm * dt * dt
    sv = np.linalg.norm(vi_) + np.linalg.norm(vj_) + g_norm * dt
    J_raw[0] = J_raw[0].copy()
    J_raw[0][0:3, 3:6] += sp
    J_raw[0][6:9, 3:6] += sv
    mag = (aU @ r_raw, [aU @ j for j in J_raw], MW, r_raw, J_raw)
    return Residual(r, list(zip(keys, J)), 0.5 * float(r @ r), mag)


def residuals(oracle, prob, lm_from_factor=False, with_imu=None, only=None):
    """every reprojection and IMU residual block of prob at its current states.  Landmark l of the solve is keyed ("lm", l) and reads inv_depth[l] (dvo_ba_solve);
    with lm_from_factor the factor's own `lm` field names it (dvo_marginalize on a marg_subproblem).  with_imu: how many IMU factors (default all);
    only: a block key — just the residual blocks that touch it."""
    lib = _bind(oracle)
    out = []
    nimu = len(prob.imu) if with_imu is None else with_imu
    for k in range(nimu):
        rec = prob.imu[k]
        fi, fj = int(rec["fi"]), int(rec["fj"])
        if only is not None and only not in (("pose", fi), ("sb", fi), ("pose", fj), ("sb", fj)):
            continue
        out.append(imu_residual(lib, rec, prob.c.g_norm, prob.pose, prob.speed_bias))
    for l in range(len(prob.landmarks)):
        L = prob.landmarks[l]
        for f in prob.factors[L["first"]:L["first"] + L["count"]]:
            li = int(f["lm"]) if lm_from_factor else l
            if only is not None:
                kind = int(f["kind"])
                touch = {("lm", li), ("td", 0), ("ex", 0)}
                if kind != 0:
                    touch.add(("ex", 1))
                if kind != 2:
                    touch |= {("pose", int(f["fi"])), ("pose", int(f["fj"]))}
                if only not in touch:
                    continue
            out.append(proj_residual(lib, f, prob.pose, prob.ex_pose, prob.inv_depth[li], prob.td[0], ("lm", li)))
    return out


# ---------------------------------------------------------------- the prior in information form
_PRIOR_KIND = {0: "pose", 1: "sb", 2: "ex", 3: "td"}


def prior_blocks(prob):
    """[(key, off, size_local, x0 (global size))] of prob's prior (empty without one)"""
    if prob.prior is None or not prob.prior.valid:
        return []
    out = []
    for i in range(prob.prior.nblocks):
        pb = prob.prior.blocks[i]
        gs = {0: 7, 1: 9, 2: 7, 3: 1}[pb.type]
        out.append(((_PRIOR_KIND[pb.type], pb.idx), pb.off, pb.size_local, np.array(prob.prior.x0[i][:gs])))
    return out


def state_of(prob, key):
    kind, idx = key
    if kind == "pose":
        return prob.pose[idx]
    if kind == "sb":
        return prob.speed_bias[idx]
    if kind == "ex":
        return prob.ex_pose[idx]
    if kind == "td":
        return prob.td[:1]
    return prob.inv_depth[idx:idx + 1]


def prior_dx(prob):
    dx = np.zeros(prob.prior.n)
    for key, off, sz, x0 in prior_blocks(prob):
        x = state_of(prob, key)
        dx[off:off + sz] = pose_dx(x, x0) if len(x0) == 7 else np.asarray(x, float) - x0
    return dx


def _prior_terms(prob):
    if prob.prior is None or not prob.prior.valid:
        return None
    return (prob.prior_A, prob.prior_b, prob.prior.c0, prior_dx(prob), [(k, o, s) for k, o, s, _ in prior_blocks(prob)])


def prior_cost(prob, with_c0=True):
    pt = _prior_terms(prob)
    if pt is None:
        return 0.0
    A, b, c0, dx, _ = pt
    return (0.5 * c0 if with_c0 else 0.0) + b @ dx + 0.5 * dx @ A @ dx


# ---------------------------------------------------------------- column layout and the dense normal equations
def pose_columns(prob):
    """({key: first column} of the reduced system in dv_ba_eval's order, its size)"""
    cols, c = {}, 0
    for f in range(len(prob.pose)):
        if prob.c.use_imu or f > 0:
            cols[("pose", f)] = c
            c += 6
        if prob.c.use_imu:
            cols[("sb", f)] = c
            c += 9
    if prob.c.free_blocks & 1:
        cols[("ex", 0)], cols[("ex", 1)] = c, c + 6
        c += 12
    if prob.c.free_blocks & 2:
        cols[("td", 0)] = c
        c += 1
    return cols, c


def assemble(res, cols, N, prior=None):
    """dense H = J^T J, g = J^T r over the columns `cols` (a block without a column is constant), the magnitude accumulations |J|^T |J|, |J|^T |r| and that of
    the cost, and the cost.  prior: (A, b, c0, dx, [(key, off, size)]) added in information form: cost c0/2 + b.dx + dx.A dx/2, gradient b + A dx, Hessian A.
    Returns (cost, H, g, |H|, |g|, |cost|)."""
    H, g, Hm, gm = np.zeros((N, N)), np.zeros(N), np.zeros((N, N)), np.zeros(N)
    cost = cm = 0.0
    for rb in res:
        cost += rb.cost
        cm += abs(rb.cost)
        idx, Js, Ms = [], [], []
        for b, (key, J) in enumerate(rb.blocks):
            c = cols.get(key)
            if c is not None:
                idx.extend(range(c, c + J.shape[1]))
                Js.append(J)
                Ms.append(np.abs(J) if rb.mag is None else rb.mag[1][b])
        if not idx:
            continue
        J, aJ = np.hstack(Js), np.hstack(Ms)
        ix = np.ix_(idx, idx)
        H[ix] += J.T @ J
        g[idx] += J.T @ rb.r
        Hm[ix] += aJ.T @ aJ
        gm[idx] += aJ.T @ (np.abs(rb.r) if rb.mag is None else rb.mag[0])
        if rb.mag is not None:
            MW, ar = rb.mag[2], rb.mag[3]
            aR = np.hstack([rb.mag[4][b] for b, (key, _) in enumerate(rb.blocks) if cols.get(key) is not None])
            Hm[ix] += aR.T @ MW @ aR
            gm[idx] += aR.T @ (MW @ ar)
            cm += 0.5 * ar @ MW @ ar
    if prior is not None:
        A, b, c0, dx, pblocks = prior
        Adx = A @ dx
        cost += 0.5 * c0 + b @ dx + 0.5 * dx @ Adx
        adx = np.abs(dx)
        cm += 0.5 * abs(c0) + np.abs(b) @ adx + 0.5 * adx @ np.abs(A) @ adx
        gp, gpm = b + Adx, np.abs(b) + np.abs(A) @ adx
        for ka, oa, sa in pblocks:
            ca = cols.get(ka)
            if ca is None:
                continue
            g[ca:ca + sa] += gp[oa:oa + sa]
            gm[ca:ca + sa] += gpm[oa:oa + sa]
            for kb, ob, sb in pblocks:
                cb = cols.get(kb)
                if cb is not None:
                    H[ca:ca + sa, cb:cb + sb] += A[oa:oa + sa, ob:ob + sb]
                    Hm[ca:ca + sa, cb:cb + sb] += np.abs(A[oa:oa + sa, ob:ob + sb])
    return cost, H, g, Hm, gm, cm


class System:
    """the full (poses + landmarks) normal equations of one window at its current states"""

    def __init__(self, oracle, prob):
        self.prob = prob
        self.cols, self.np = pose_columns(prob)
        self.nlm = len(prob.landmarks)
        self.all_cols = dict(self.cols)
        for l in range(self.nlm):
            self.all_cols[("lm", l)] = self.np + l
        self.N = self.np + self.nlm
        self.cost, self.H, self.g, self.Hmag, self.gmag, self.cost_mag = assemble(residuals(oracle, prob), self.all_cols, self.N, _prior_terms(prob))

    def reduced(self):
        """(S, g, |S|, |g|): the dense Schur complement of the landmark block, S = H_pp - H_pl H_ll^-1 H_lp, g = g_p - H_pl H_ll^-1 g_l, and the magnitudes that
        bound what rounding can do to each entry: |J|^T|J| of H_pp plus |H_pl| |H_ll|^-1 |H_lp| of the elimination (|J|^T|r| likewise for g)."""
        p = self.np
        H, g, Hm, gm = self.H, self.g, self.Hmag, self.gmag
        if self.nlm == 0:
            return H.copy(), g.copy(), Hm.copy(), gm.copy()
        Hll = H[p:, p:]
        S = H[:p, :p] - H[:p, p:] @ np.linalg.solve(Hll, H[p:, :p])
        gr = g[:p] - H[:p, p:] @ np.linalg.solve(Hll, g[p:])
        hinv = 1.0 / np.diag(Hll)
        Sm = Hm[:p, :p] + (Hm[:p, p:] * hinv) @ Hm[p:, :p]
        grm = gm[:p] + (Hm[:p, p:] * hinv) @ gm[p:]
        return S, gr, Sm, grm

    def step(self, mu=1e-8):
        """the first Gauss-Newton step of the trust-region solve (back_solver.h:180-207, be_solve.hip:224): Jacobi scaling s = 1 / (1 + sqrt(H_ii)), diagonal
        d^2 = clamp(H_ii s^2, 1e-6, 1e32), A = s H s + mu d^2 and b = s g over poses AND landmarks, solved densely: A y = -b.
        Returns dict(A, b, y (scaled), delta = s y (the tangent step), scale, cond (2-norm condition number of A), dnorm = |d y| (what the dogleg holds
        against its radius))."""
        h = np.diag(self.H)
        s = 1.0 / (1.0 + np.sqrt(h))
        d2 = np.clip(h * s * s, 1e-6, 1e32)
        A = self.H * np.outer(s, s) + np.diag(mu * d2)
        b = s * self.g
        y = np.linalg.solve(A, -b)
        ev = np.linalg.eigvalsh(0.5 * (A + A.T))
        return dict(A=A, b=b, y=y, delta=s * y, scale=s, cond=ev[-1] / ev[0] if ev[0] > 0 else np.inf, dnorm=float(np.linalg.norm(np.sqrt(d2) * y)))

    def apply(self, delta):
        """a copy of the problem with the tangent step applied (pose_plus on poses and free extrinsics, plain addition elsewhere)"""
        q = self.prob.clone()
        pk = q.c.plane_kind
        for (kind, idx), c in self.cols.items():
            d = delta[c:c + LOCAL[kind]]
            if kind == "pose":
                q.pose[idx] = pose_plus(q.pose[idx], d, pk)
            elif kind == "sb":
                q.speed_bias[idx] += d
            elif kind == "ex":
                q.ex_pose[idx] = pose_plus(q.ex_pose[idx], d)
            else:
                q.td[0] += d[0]
        q.inv_depth += delta[self.np:]
        q._bind()
        return q

    def recover(self, before, after):
        """the tangent step that took `before` to `after`: the exact inverse of apply (a translation component a plane constraint drops reads 0)"""
        y = np.zeros(self.N)
        for (kind, idx), c in self.cols.items():
            if kind == "pose":
                y[c:c + 6] = pose_minus(after.pose[idx], before.pose[idx])
            elif kind == "sb":
                y[c:c + 9] = after.speed_bias[idx] - before.speed_bias[idx]
            elif kind == "ex":
                y[c:c + 6] = pose_minus(after.ex_pose[idx], before.ex_pose[idx])
            else:
                y[c] = after.td[0] - before.td[0]
        y[self.np:] = after.inv_depth - before.inv_depth
        return y

    def plane_columns(self):
        """the columns whose step pose_plus drops (plane kind 1: dz of every pose, 2: dy)"""
        pk = self.prob.c.plane_kind
        if pk == 0:
            return []
        comp = 2 if pk == 1 else 1
        return sorted(c + comp for (kind, _), c in self.cols.items() if kind == "pose")


def backward_error(A, b, y):
    """normwise backward error of y as a solution of A y = -b: |A y + b| / (|A| |y| + |b|), 2-norms"""
    return np.linalg.norm(A @ y + b) / (np.linalg.norm(A, 2) * np.linalg.norm(y) + np.linalg.norm(b))


# ---------------------------------------------------------------- marginalization
def marginalize(oracle, sub, mode, eps=1e-8):
    """MarginalizationInfo on a ba_gen.marg_subproblem, densely: H, g over [dropped | kept] blocks (every block a residual touches, constant in the solve or not),
    then A' = H_rr - H_rm H_mm^+ H_mr, b' = g_r - H_rm H_mm^+ g_m with H_mm^+ the eigen-clamped pseudo-inverse (eigenvalues <= eps zeroed).
    mode 0 (kMarginOld) drops pose 0, speed-bias 0 and the landmarks (prior, IMU factor (0,1), the landmarks' reprojection blocks); mode 1 (kMarginSecondNew)
    uses the prior alone and drops pose kWinSize-1.  c0 = sum over the eigenvalues > eps of A' of (v.b')^2 / lambda.
    Returns dict(blocks (ba_gen.prior_to_dict layout, keyed by the shifted block), A, b, c0, and the DV_MARG_EIGEN form: A_eig, b_eig (A', b' projected onto the
    eigenvectors with eigenvalues > eps), rank (their count))."""
    res = residuals(oracle, sub, lm_from_factor=True, with_imu=min(1, len(sub.imu))) if mode == 0 else []
    pblocks = prior_blocks(sub)
    touched = {}                      # key -> local size, in order of first use
    for k, _, sz, _ in pblocks:
        touched.setdefault(k, sz)
    for rb in res:
        for k, J in rb.blocks:
            touched.setdefault(k, J.shape[1])
    if mode == 0:
        dropped = [k for k in touched if k in (("pose", 0), ("sb", 0)) or k[0] == "lm"]
    else:
        dropped = [k for k in touched if k == ("pose", KWIN - 1)]
    kept = [k for k in touched if k not in dropped]
    cols, c = {}, 0
    for k in dropped + kept:
        cols[k] = c
        c += touched[k]
    m, N = sum(touched[k] for k in dropped), c
    prior = None
    if pblocks:
        prior = (sub.prior_A, sub.prior_b, sub.prior.c0, prior_dx(sub), [(k, o, s) for k, o, s, _ in pblocks])
    H, g = assemble(res, cols, N, prior)[1:3]
    Hmm = 0.5 * (H[:m, :m] + H[:m, :m].T)
    ev, V = np.linalg.eigh(Hmm)
    keep = ev > eps
    T = H[m:, :m] @ ((V[:, keep] / ev[keep]) @ V[:, keep].T)
    A = H[m:, m:] - T @ H[:m, m:]
    A = 0.5 * (A + A.T)
    b = g[m:] - T @ g[:m]
    ev2, V2 = np.linalg.eigh(A)
    k2 = ev2 > eps
    Vk = V2[:, k2]
    vb = Vk.T @ b
    c0 = float(np.sum(vb * vb / ev2[k2]))
    blocks = {}
    for k in kept:
        kind, idx = k
        if kind in ("pose", "sb"):
            t = idx - 1 if (mode == 0 or idx == KWIN) else idx
        else:
            t = idx
        code = {"pose": 0, "sb": 1, "ex": 2, "td": 3}[kind]
        blocks[(code, t)] = (cols[k] - m, touched[k], np.array(state_of(sub, k), float))
    return dict(blocks=blocks, A=A, b=b, c0=c0, A_eig=(Vk * ev2[k2]) @ Vk.T, b_eig=Vk @ vb, rank=int(k2.sum()), n=N - m, m=m,
                min_ev_mm=float(ev.min()) if m else np.inf)
