"""Plain float64 reference of the block-diagonal trust-region solve (test infrastructure, numpy only): what bd_solve.h (dv_obj_solve, dv_batch_obj_solve,
dv_line_solve) and the oracle's solver loop (dvo_obj_solve, dvo_line_solve) are held to by tests/test_bd_reference.py and tests/test_bd_reference_gpu.py.

A problem is a list of residual blocks, each on ONE variable block.  Residuals and Jacobians come from the oracle's per-factor entries (G.o_box_enclose,
G.o_box_dims, G.o_box_orientation, G.o_line: the ones tests/test_objfactor_reference*.py pin against a float64 restatement, documented non-derivative Jacobians included); everything after that is
written here from the Ceres 1.14 rule set (trust_region_minimizer.cc, dogleg_strategy.cc, corrector.cc), not from the kernel's or the oracle's
loop, and with other arithmetic: no normal equations.  With J the stacked Jacobian on the local parameters (6 per object pose, 3 per object dims, 4 per line; a block
without a residual is dropped, as Ceres drops it), S = 1 / (1 + |J column|) fixed at iteration 0 and D = sqrt(clip(diag((J S)^T (J S)), 1e-6, 1e32)):
    Gauss-Newton   y = least-squares solution of [J S; sqrt(mu) D] y = [-r; 0]  (numpy.linalg.lstsq), in the dogleg's coordinates gn = D y
    Cauchy         g = (J S)^T r / D, alpha = |g|^2 / |J S D^-1 g|^2
Every residual block touches one variable block, so the stacked matrix is block diagonal up to a row permutation and its least-squares solution is the blocks' own:
the solve goes block by block (`Linear.dense` builds the stacked system; tests/test_bd_reference.py checks that its dense solution is the same).
Losses (rho'' <= 0 for both, so the Ceres corrector scales residual and Jacobian by sqrt(rho')): Huber(1) on the point and dims factors, none on the orientation
factor, Cauchy(1) on the line factor.  cost = 0.5 sum rho by math.fsum; its magnitude accumulation 0.5 sum |rho| is the same number."""
import math

import numpy as np

from tests import ba_ref
from tests import obj_gen as G

EPS = np.finfo(np.float64).eps
STOPS = ("iterations", "gradient", "function", "parameter", "radius", "invalid")      # which rule ended the solve; termination 0 | 1 | 1 | 1 | 1 | 2
BAR = 1e-9                                                                            # the project's bar on a relative cost error: the unit of `margin`


# ---------------------------------------------------------------- retractions and their inverses
def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _orth_R(t):
    """the rotation U of an orthonormal line representation: the matrix of tests/line_geometry_np.py:orth_to_plk, R = Rz(t3) Ry(t2) Rx(t1)"""
    return _rot(2, t[2]) @ _rot(1, t[1]) @ _rot(0, t[0])


def line_plus(orth, d):
    """LineOrthParameterization::Plus (factor/line_parameterization.cpp:9-72): U <- U Rx(d0) Ry(d1) Rz(d2), W <- W R2(d3), read back as angles"""
    U = _orth_R(orth) @ _rot(0, d[0]) @ _rot(1, d[1]) @ _rot(2, d[2])
    return np.array([math.atan2(U[2, 1], U[2, 2]), math.asin(-U[2, 0]), math.atan2(U[1, 0], U[0, 0]), math.asin(math.sin(orth[3] + d[3]))])


def line_minus(new, old, near=None):
    """inverse of line_plus: U_old^T U_new = Rx(a) Ry(b) Rz(c) = [[cb cc, -cb sc, sb], [., ., -sa cb], [., ., ca cb]]; the phase while it stays inside (-pi/2, pi/2).
    Plus is many to one (whole turns, two Euler solutions, the folded phase): the principal values come back, or, with `near`, the preimage closest to near"""
    M = _orth_R(old).T @ _orth_R(new)
    d = np.array([math.atan2(-M[1, 2], M[2, 2]), math.asin(M[0, 2]), math.atan2(-M[0, 1], M[0, 0]), new[3] - old[3]])
    if near is not None:          # the discrete choices only: the other Euler solution (a + pi, pi - b, c + pi), the phase asin folded at +-pi / 2, whole turns
        near, tau = np.asarray(near, float), 2.0 * math.pi
        wrap = lambda v, n: v + tau * np.round((n - v) / tau)
        rots = [wrap(r, near[:3]) for r in (d[:3], np.array([d[0] + math.pi, math.pi - d[1], d[2] + math.pi]))]
        phis = [wrap(p, near[3]) for p in (d[3], math.pi - new[3] - old[3])]
        d = np.concatenate([min(rots, key=lambda r: np.abs(r - near[:3]).max()), [min(phis, key=lambda p: abs(p - near[3]))]])
    return d


def plus(key, x, d, plane_kind=0):
    if key[0] == "pose":
        return ba_ref.pose_plus(x, d, plane_kind)
    if key[0] == "dims":
        return np.asarray(x, float) + d
    return line_plus(x, d)


def minus(key, new, old, near=None):
    """the local step that took `old` to `new` (a translation component that a plane constraint drops reads 0; near: see line_minus)"""
    if key[0] == "pose":
        return ba_ref.pose_minus(new, old)
    if key[0] == "dims":
        return np.asarray(new, float) - old
    return line_minus(new, old, near)


# ---------------------------------------------------------------- losses: (rho, rho') of s = |r|^2
def huber1(s):
    return (s, 1.0) if s <= 1.0 else (2.0 * math.sqrt(s) - 1.0, 1.0 / math.sqrt(s))


def cauchy1(s):
    return math.log1p(s), 1.0 / (1.0 + s)


def no_loss(s):
    return s, 1.0


# ---------------------------------------------------------------- problems
class Evaluation:
    """cost, per variable block the corrected (J, r) stacked over its residual blocks, max |J^T r|, its magnitude max |J|^T |r|, and which loss branches ran"""

    def __init__(self):
        self.rho, self.rows, self.branches = [], {}, {}

    def add(self, key, r, J, loss, name):
        s = float(r @ r)
        rho, rho1 = loss(s)
        self.rho.append(rho)
        w = math.sqrt(rho1)
        self.rows.setdefault(key, []).append((w * J, w * r))
        if loss is huber1:
            tag = name + ("_outlier" if s > 1.0 else ("_inlier" if s > 0.0 else "_zero"))
            self.branches[tag] = self.branches.get(tag, 0) + 1

    def finish(self, keys):
        self.cost = 0.5 * math.fsum(self.rho)
        self.cost_mag = 0.5 * math.fsum(abs(v) for v in self.rho)
        self.J = {k: np.vstack([j for j, _ in self.rows[k]]) for k in keys}
        self.r = {k: np.concatenate([r for _, r in self.rows[k]]) for k in keys}
        self.gmax = max([float(np.abs(self.J[k].T @ self.r[k]).max()) for k in keys], default=0.0)
        self.gmag = max([float((np.abs(self.J[k]).T @ np.abs(self.r[k])).max()) for k in keys], default=0.0)
        del self.rows
        return self


class ObjRef:
    """InstanceManager::Optimization on a backend.ObjProblem: variable blocks ("pose", o, f) with a box or a point and ("dims", o) with a box; the point factor
    reads the dims at entry; |x| also holds the body poses of the frames that carry a detection (they are parameter blocks of the program that never move)."""

    def __init__(self, oracle, prob):
        self.lib, self.prob, self.plane_kind = oracle.lib, prob, prob.plane_kind
        self.dims0 = prob.dims.copy()
        pose_keys = {("pose", int(b["obj"]), int(b["frame"])) for b in prob.boxes} | {("pose", int(p["obj"]), int(p["frame"])) for p in prob.points}
        self.keys = sorted(pose_keys) + sorted({("dims", int(b["obj"])) for b in prob.boxes})
        frames = sorted({int(b["frame"]) for b in prob.boxes})
        self.xnorm2_const = float(sum(prob.body_pose[f] @ prob.body_pose[f] for f in frames))
        self.factors = {k: 0 for k in self.keys}          # residual blocks per variable block
        for b in prob.boxes:
            self.factors[("pose", int(b["obj"]), int(b["frame"]))] += 1
            self.factors[("dims", int(b["obj"]))] += 1
        for p in prob.points:
            self.factors[("pose", int(p["obj"]), int(p["frame"]))] += 1

    def x0(self):
        return {k: (self.prob.state[k[1], k[2]].copy() if k[0] == "pose" else self.prob.dims[k[1]].copy()) for k in self.keys}

    def store(self, x, prob):
        for k, v in x.items():
            if k[0] == "pose":
                prob.state[k[1], k[2]] = v
            else:
                prob.dims[k[1]] = v

    def load(self, prob):
        return {k: (prob.state[k[1], k[2]].copy() if k[0] == "pose" else prob.dims[k[1]].copy()) for k in self.keys}

    def evaluate(self, x):
        ev, P = Evaluation(), self.prob
        for b in P.boxes:
            o, f = int(b["obj"]), int(b["frame"])
            r, J = G.o_box_dims(self.lib, b["dims"], x[("dims", o)])
            ev.add(("dims", o), r, J[0], huber1, "dims")
            r, J = G.o_box_orientation(self.lib, b["R_cioi"], P.R_bc, P.body_pose[f], x[("pose", o, f)])
            ev.add(("pose", o, f), r, J[1][:, :6], no_loss, "orientation")
        for p in P.points:
            o, f = int(p["obj"]), int(p["frame"])
            r, J = G.o_box_enclose(self.lib, p["p_w"], self.dims0[o], x[("pose", o, f)])
            ev.add(("pose", o, f), r, J[0][:, :6], huber1, "point")
        return ev.finish(self.keys)


class LineRef:
    """Estimator::OptimizationWithOnlyLine on a backend.LineProblem: one 4-parameter block per observed line; poses and extrinsics are constant blocks, which
    Ceres removes from the program: nothing constant counts in |x|."""
    plane_kind, xnorm2_const = 0, 0.0

    def __init__(self, oracle, prob):
        self.lib, self.prob = oracle.lib, prob
        self.keys = sorted({("line", int(o["line"])) for o in prob.obs})
        self.factors = {k: 0 for k in self.keys}
        for o in prob.obs:
            self.factors[("line", int(o["line"]))] += 1

    def x0(self):
        return {k: self.prob.orth[k[1]].copy() for k in self.keys}

    def store(self, x, prob):
        for k, v in x.items():
            prob.orth[k[1]] = v

    def load(self, prob):
        return {k: prob.orth[k[1]].copy() for k in self.keys}

    def evaluate(self, x):
        ev, P = Evaluation(), self.prob
        for o in P.obs:
            k = ("line", int(o["line"]))
            r, J = G.o_line(self.lib, o["obs"], P.sqrt_info, P.pose[int(o["frame"])], P.ex_pose, x[k])
            ev.add(k, r, J[2], cauchy1, "line")
        return ev.finish(self.keys)


# ---------------------------------------------------------------- the linear algebra of one iteration
class Linear:
    """the scaled, regularised least-squares system of one evaluation: per block A_k = [J_k S_k; sqrt(mu) diag(D_k)], b_k = [r_k; 0]; A y = -b"""

    def __init__(self, keys, ev, S, mu):
        self.keys, self.S, self.mu = keys, S, mu
        self.JS = {k: ev.J[k] * S[k] for k in keys}
        self.r = ev.r
        self.D = {k: np.sqrt(np.clip((self.JS[k] ** 2).sum(axis=0), 1e-6, 1e32)) for k in keys}
        self.A = {k: np.vstack([self.JS[k], math.sqrt(mu) * np.diag(self.D[k])]) for k in keys}
        self.b = {k: np.concatenate([self.r[k], np.zeros(len(self.D[k]))]) for k in keys}
        self.y = {k: np.linalg.lstsq(self.A[k], -self.b[k], rcond=None)[0] for k in keys}
        self.gn = {k: self.D[k] * self.y[k] for k in keys}
        self.g = {k: self.JS[k].T @ self.r[k] / self.D[k] for k in keys}
        gg = math.fsum(float(v @ v) for v in self.g.values())
        JgJg = math.fsum(float(np.sum((self.JS[k] @ (self.g[k] / self.D[k])) ** 2)) for k in keys)
        self.gnorm, self.alpha = math.sqrt(gg), (gg / JgJg if JgJg > 0 else math.inf)
        self.gn_norm = math.sqrt(math.fsum(float(v @ v) for v in self.gn.values()))
        self.finite = all(np.isfinite(v).all() for v in self.y.values())

    def model_decrease(self, t):
        """-(J S t) . (r + J S t / 2) of a step t in the scaled coordinates"""
        s = []
        for k in self.keys:
            m = self.JS[k] @ t[k]
            s.append(-float(m @ (self.r[k] + 0.5 * m)))
        return math.fsum(s)

    def zero_columns(self):
        """{key: local columns whose Jacobian is identically zero}: the regularisation alone holds them at y = 0"""
        return {k: np.nonzero(~self.JS[k].any(axis=0))[0] for k in self.keys}

    def cond(self):
        """2-norm condition number of the stacked system with its identically zero Jacobian columns dropped: the worst over the blocks of sigma_max (of any block) /
        sigma_min"""
        smax, smin = 0.0, math.inf
        for k in self.keys:
            keep = self.JS[k].any(axis=0)
            if keep.any():
                sv = np.linalg.svd(self.A[k][:, keep], compute_uv=False)
                smax, smin = max(smax, sv[0]), min(smin, sv[-1])
        return smax / smin if smin > 0 else math.inf

    def backward_error(self, y):
        """normwise backward error of y = {key: scaled step} as a solution of the stacked least-squares problem min |A y + b|, measured on the square system it is
        equivalent to, A^T A y = -A^T b, the way tests/ba_ref.py:backward_error measures one: |A^T (A y + b)| / (|A|^2 |y| + |A^T b|), 2-norms of the stacked
        quantities (|A| of a block diagonal matrix: the largest of the blocks')"""
        num = math.sqrt(math.fsum(float(np.sum((self.A[k].T @ (self.A[k] @ y[k] + self.b[k])) ** 2)) for k in self.keys))
        nA = max(np.linalg.norm(self.A[k], 2) for k in self.keys)
        ny = math.sqrt(math.fsum(float(y[k] @ y[k]) for k in self.keys))
        nAb = math.sqrt(math.fsum(float(np.sum((self.A[k].T @ self.b[k]) ** 2)) for k in self.keys))
        return num / (nA * nA * ny + nAb)

    def dense(self):
        """(A, b, {key: first column}) of the stacked system"""
        rows, cols = sum(len(self.b[k]) for k in self.keys), sum(len(self.D[k]) for k in self.keys)
        A, b, at, r0, c0 = np.zeros((rows, cols)), np.zeros(rows), {}, 0, 0
        for k in self.keys:
            m, n = self.A[k].shape
            A[r0:r0 + m, c0:c0 + n], b[r0:r0 + m], at[k] = self.A[k], self.b[k], c0
            r0, c0 = r0 + m, c0 + n
        return A, b, at


def _dist(value, threshold, unit):
    d = abs(value - threshold)
    return math.inf if unit == 0.0 and d > 0.0 else (d / unit if unit > 0.0 else 0.0)


def solve(P, max_iters, count_const=True):
    """One trust-region solve of P (ObjRef / LineRef) from P.x0().  Returns dict(summary fields, records, x, branches, margin):
    records[i] (iteration i + 1): dict(x, cost (after the iteration), kind (0 Gauss-Newton | 1 Cauchy-limited | 2 interpolated | None: no step), beta_branch
    ("c<=0" | "c>0" with kind 2), rel, model_decrease, radius, mu (after the iteration), accepted, radius_move ("grow" | "shrink_accept" | "shrink_reject" | None),
    stop (None or one of STOPS), successful, margin);  `margin`: the smallest distance of a decision quantity from its threshold in units of what a relative
    cost error BAR = 1e-9 does to that quantity: rel (unit BAR cost / model decrease) against 1e-3 and, when accepted, 0.25 and 0.75; |gn| against the radius and,
    when it is outside, alpha |g| against the radius (quantities linear in the residual: unit BAR times themselves); the function-tolerance ratio |dcost| / cost
    against 1e-6 (unit BAR); the parameter-tolerance ratio against 1e-8 (unit BAR times itself); max |g| against 1e-10 (unit BAR times its magnitude
    accumulation max |J|^T |r|)."""
    keys, pk = P.keys, P.plane_kind
    xc2 = P.xnorm2_const if count_const else 0.0
    x = P.x0()
    xnorm = lambda z: math.sqrt(math.fsum(float(v @ v) for v in z.values()) + xc2)
    ev = P.evaluate(x)
    branches = dict(ev.branches)
    out = dict(initial_cost=ev.cost, cost_mag=ev.cost_mag, records=[], iterations=0, successful=0, termination=0, stop=None, first=None)
    S = {k: 1.0 / (1.0 + np.sqrt((ev.J[k] ** 2).sum(axis=0))) for k in keys}
    x_cost, x_norm = ev.cost, xnorm(x)
    margin = _dist(ev.gmax, 1e-10, BAR * ev.gmag)
    radius, mu, reuse, invalid, lin, dogleg_norm = 1e4, 1e-8, False, 0, None, 0.0
    stop = "gradient" if ev.gmax <= 1e-10 else None
    it = 0
    while stop is None:
        it += 1
        if it > max_iters:
            stop = "iterations"
            break
        out["iterations"] = it
        rec = dict(kind=None, beta_branch=None, rel=None, model_decrease=None, accepted=False, radius_move=None, stop=None, margin=math.inf)
        out["records"].append(rec)
        valid = True
        if not reuse:
            reuse = True
            while True:
                lin = Linear(keys, ev, S, mu)
                if lin.finite:
                    break
                mu *= 10.0
                if mu > 1.0:
                    break
            valid = lin.finite
            if it == 1:
                out["first"] = lin
        md = 0.0
        if valid:
            rec["margin"] = min(rec["margin"], _dist(lin.gn_norm, radius, BAR * lin.gn_norm))
            if lin.gn_norm <= radius:
                rec["kind"], step, dogleg_norm = 0, lin.gn, lin.gn_norm
            else:
                rec["margin"] = min(rec["margin"], _dist(lin.alpha * lin.gnorm, radius, BAR * lin.alpha * lin.gnorm))
                if lin.alpha * lin.gnorm >= radius:
                    rec["kind"], step, dogleg_norm = 1, {k: -(radius / lin.gnorm) * lin.g[k] for k in keys}, radius
                else:
                    # the point where the segment from the Cauchy point a = -alpha g to the Gauss-Newton point b leaves the ball: |a + beta (b - a)| = radius
                    b_dot_a = -lin.alpha * math.fsum(float(lin.g[k] @ lin.gn[k]) for k in keys)
                    a2 = (lin.alpha * lin.gnorm) ** 2
                    bma2 = a2 - 2.0 * b_dot_a + lin.gn_norm ** 2
                    c = b_dot_a - a2
                    d = math.sqrt(c * c + bma2 * (radius ** 2 - a2))
                    beta = (d - c) / bma2 if c <= 0 else (radius ** 2 - a2) / (d + c)
                    rec["kind"], rec["beta_branch"] = 2, ("c<=0" if c <= 0 else "c>0")
                    step = {k: (-lin.alpha * (1.0 - beta)) * lin.g[k] + beta * lin.gn[k] for k in keys}
                    dogleg_norm = math.sqrt(math.fsum(float(v @ v) for v in step.values()))
            t = {k: step[k] / lin.D[k] for k in keys}
            md = lin.model_decrease(t)
            rec["model_decrease"] = md
            valid = md > 0.0
            if valid:
                invalid = 0
        if not valid:
            invalid += 1
            if invalid >= 5:
                stop = "invalid"
            else:
                mu, reuse = mu * 10.0, False
        else:
            cand = {k: plus(k, x[k], S[k] * t[k], pk) for k in keys}
            cev = P.evaluate(cand)
            for name, n in cev.branches.items():
                branches[name] = branches.get(name, 0) + n
            sn = math.sqrt(math.fsum(float((x[k] - cand[k]) @ (x[k] - cand[k])) for k in keys))
            pr, fr = sn / (x_norm + 1e-8), (abs(x_cost - cev.cost) / x_cost if x_cost > 0 else 0.0)
            rec["margin"] = min(rec["margin"], _dist(pr, 1e-8, BAR * pr))
            if pr <= 1e-8:
                stop = "parameter"
            else:
                rec["margin"] = min(rec["margin"], _dist(fr, 1e-6, BAR))
                if fr <= 1e-6:
                    stop = "function"
            if stop is None:
                rel = (x_cost - cev.cost) / md
                unit = BAR * x_cost / md
                rec["rel"] = rel
                rec["margin"] = min(rec["margin"], _dist(rel, 1e-3, unit))
                if rel > 1e-3:
                    rec["accepted"] = True
                    rec["margin"] = min(rec["margin"], _dist(rel, 0.25, unit), _dist(rel, 0.75, unit))
                    x, ev, x_cost = cand, cev, cev.cost
                    x_norm = xnorm(x)
                    out["successful"] += 1
                    if rel < 0.25:
                        radius, rec["radius_move"] = 0.5 * radius, "shrink_accept"
                    if rel > 0.75:
                        if 3.0 * dogleg_norm > radius:
                            rec["radius_move"] = "grow"
                        radius = max(radius, 3.0 * dogleg_norm)
                    mu, reuse = max(1e-8, 2.0 * mu / 10.0), False
                    rec["margin"] = min(rec["margin"], _dist(ev.gmax, 1e-10, BAR * ev.gmag))
                    if ev.gmax <= 1e-10:
                        stop = "gradient"
                else:
                    radius, reuse, rec["radius_move"] = 0.5 * radius, True, "shrink_reject"
                    if radius < 1e-32:
                        stop = "radius"
        rec.update(x={k: v.copy() for k, v in x.items()}, cost=x_cost, radius=radius, mu=mu, stop=stop, successful=out["successful"])
        margin = min(margin, rec["margin"])
    out.update(stop=stop, termination={"iterations": 0, "invalid": 2}.get(stop, 1), final_cost=x_cost, x=x, branches=branches, margin=margin)
    return out


def after(sol, k):
    """(iterations, successful, termination, cost, x) of the same solve cut at max_iters = k: the solver is deterministic, so that run is this one's first k iterations"""
    recs = sol["records"]
    if k >= len(recs):
        return sol["iterations"], sol["successful"], sol["termination"], sol["final_cost"], sol["x"]
    if k == 0:
        return 0, 0, 0, sol["initial_cost"], None
    r = recs[k - 1]
    return k, r["successful"], 0, r["cost"], r["x"]
