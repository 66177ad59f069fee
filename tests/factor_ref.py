"""Plain float64 restatement of the factor formulas, the gauge fix and the outlier test (test infrastructure, numpy only).

Written from the mathematics of the reference, not from oracle/ and not from be_factor_dev.h:
  IMU factor        IntegrationBase::evaluate (imu/integration_base.h:175-201), IMUFactor::Evaluate (imu/imu_factor.h:31-172)
  projection        ProjectionTwoFrameOneCam / TwoFrameTwoCam / OneFrameTwoCamFactor::Evaluate (factor/projection_*_factor.cpp), quirk Q7 included
  gauge_fix         Estimator::Double2vector -> BodyState::GetOptimizationParameters (estimator.cpp:1110-1154, body.cpp:61-129), Utility::R2ypr / ypr2R
  reject_flags      OutliersRejection / ReprojectionError (vio_util.cpp:381-444)
Quaternions are stored x y z w as in the parameter blocks (para_pose: p, qx qy qz qw); the pre-integration's delta_q arrives w x y z (dv_ba_imu).

Every closed form is evaluated on `A` values: a float64 array that carries, beside its value, the SAME expression evaluated on absolute values (sums of
magnitudes for sums and differences, products of magnitudes for products): the size of the rounding a float64 evaluation of that expression can carry, entry
by entry, and exactly 0 where the expression is structurally zero.  The tests hold |device - reference| <= K eps magnitude.  The elementary functions (sin, cos,
asin, atan, atan2, sqrt: tests/objfactor_ref.py) carry |f(x)| + |f'(x)| m_x.

Three closed forms of the IMU factor are not the derivative of the residual once the gyroscope bias has moved from its linearisation point
(theta = dq_dbg (Bg_i - lin_bg) != 0), all in the rotation rows:
  d r_q / d b_g      is written with delta_q, not the corrected quaternion (imu_factor.h:132-133): exact at theta = 0, first-order gap beyond;
  d r_q / d theta_i  -(Qleft(Qj^-1 Qi) Qright(cq))_br (imu_factor.h:106-108) is the derivative for a UNIT cq; Utility::deltaQ does not normalise
                     (cq = dq [1, theta / 2], |cq|^2 = 1 + |theta|^2 / 4) and Eigen's inverse() divides by the squared norm, so the closed form is
                     |cq|^2 times the derivative: exact at theta = 0, second-order gap beyond, and EXACTLY that factor (asserted);
and one of the projection factors: Q7, kind 2 writes d r / d lambda with pts_i instead of pts_i_td (projection_one_frame_two_cam_factor.cpp:125).
The closed forms are what the device must match; tests/test_factor_reference.py pins down where and by how much they leave the derivative."""
import contextlib

import numpy as np

EPS = np.finfo(np.float64).eps
SQRT_INFO = 460.0 / 1.5          # kFocalLength / 1.5 * I2 (estimator.cpp:685-687)


# ---------------------------------------------------------------- values that carry the magnitude of their own expression
class A:
    __slots__ = ("v", "m")
    first_order = False          # see first_order() below; off, the products are products of magnitudes

    def __init__(self, v, m=None):
        self.v = np.asarray(v, np.float64)
        self.m = np.abs(self.v) if m is None else np.asarray(m, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, A) else A(x)

    def __add__(self, o):
        o = A.of(o)
        return A(self.v + o.v, self.m + o.m)

    __radd__ = __add__

    def __sub__(self, o):
        o = A.of(o)
        return A(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return A.of(o) - self

    def __neg__(self):
        return A(-self.v, self.m)

    def __mul__(self, o):
        o = A.of(o)
        if A.first_order:
            return A(self.v * o.v, np.abs(self.v) * o.m + self.m * np.abs(o.v))
        return A(self.v * o.v, self.m * o.m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = A.of(o)
        return A(self.v / o.v, self.m / np.abs(o.v) + np.abs(self.v) * o.m / (o.v * o.v))

    def __rtruediv__(self, o):
        return A.of(o) / self

    __array_ufunc__ = None          # numpy scalars and arrays on the left defer to the reflected operators

    def __matmul__(self, o):
        o = A.of(o)
        if A.first_order:
            return A(self.v @ o.v, np.abs(self.v) @ o.m + self.m @ np.abs(o.v))
        return A(self.v @ o.v, self.m @ o.m)

    def __rmatmul__(self, o):
        return A.of(o) @ self

    def __getitem__(self, k):
        return A(self.v[k], self.m[k])

    @property
    def T(self):
        return A(self.v.T, self.m.T)


@contextlib.contextmanager
def first_order():
    """Inside, a product carries |a| m_b + m_a |b| instead of m_a m_b (each m holds its own |value|, so the product's own rounding is in it).  The product of
    magnitudes is the expression on absolute values only while the operands are polynomials of the inputs; past a quotient or a function call the magnitudes are
    error bounds, and multiplying two of them squares their slack at every step (1e12 eps on a benign line Jacobian, 1e130 at the end of the orientation chain)."""
    old, A.first_order = A.first_order, True
    try:
        yield
    finally:
        A.first_order = old


def stack(rows):
    """A from a (nested) list of A scalars / floats"""
    if isinstance(rows, (list, tuple)):
        parts = [stack(r) for r in rows]
        return A(np.array([p.v for p in parts]), np.array([p.m for p in parts]))
    return A.of(rows)


def hcat(blocks):
    return A(np.hstack([A.of(b).v for b in blocks]), np.hstack([A.of(b).m for b in blocks]))


def zeros(*shape):
    return A(np.zeros(shape))


def eye3():
    return A(np.eye(3))


# elementary functions on A: the magnitude of f(x) is |f(x)| + |f'(x)| m_x (the function's own rounding plus what the rounding of its argument becomes)
def _elem(x, f, df):
    x = A.of(x)
    v = f(x.v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return A(v, np.abs(v) + np.where(x.m > 0, np.abs(df(x.v)) * x.m, 0.0))


def sin(x):
    return _elem(x, np.sin, np.cos)


def cos(x):
    return _elem(x, np.cos, np.sin)


def asin(x):
    return _elem(x, np.arcsin, lambda v: 1.0 / np.sqrt(1.0 - v * v))


def atan(x):
    return _elem(x, np.arctan, lambda v: 1.0 / (1.0 + v * v))


def sqrt(x):
    return _elem(x, np.sqrt, lambda v: 0.5 / np.sqrt(v))


def atan2(y, x):
    y, x = A.of(y), A.of(x)
    v = np.arctan2(y.v, x.v)
    n2 = x.v * x.v + y.v * y.v
    with np.errstate(invalid="ignore", divide="ignore"):
        return A(v, np.abs(v) + np.where((x.m > 0) | (y.m > 0), (np.abs(x.v) * y.m + np.abs(y.v) * x.m) / n2, 0.0))


def skew(v):
    z = A(0.0)
    return stack([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]])


# ---------------------------------------------------------------- quaternions x y z w
def qmul(a, b):
    ax, ay, az, aw = a[0], a[1], a[2], a[3]
    bx, by, bz, bw = b[0], b[1], b[2], b[3]
    return stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz])


def qinv(q):
    """Eigen::Quaternion::inverse(): conjugate over the squared norm"""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return stack([-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2])


def qR(q):
    """Eigen::Quaternion::toRotationMatrix() (no normalisation)"""
    x, y, z, w = q[0], q[1], q[2], q[3]
    return stack([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                  [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                  [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])


def qleft_br(q):
    """bottom-right 3x3 of Utility::Qleft(q) (utility.h: [w, -v^T; v, w I + skew(v)])"""
    return q[3] * eye3() + skew(q[:3])


def qright_br(q):
    """bottom-right 3x3 of Utility::Qright(q): w I - skew(v)"""
    return q[3] * eye3() - skew(q[:3])


def qleft4(q):
    """Utility::Qleft in the order w x y z"""
    w, v = q[3], q[:3]
    top = hcat([stack([w]), -v])
    return A(np.vstack([top.v[None, :], np.hstack([v.v[:, None], qleft_br(q).v])]), np.vstack([top.m[None, :], np.hstack([v.m[:, None], qleft_br(q).m])]))


def qright4(q):
    w, v = q[3], q[:3]
    top = hcat([stack([w]), -v])
    return A(np.vstack([top.v[None, :], np.hstack([v.v[:, None], qright_br(q).v])]), np.vstack([top.m[None, :], np.hstack([v.m[:, None], qright_br(q).m])]))


def plus_pose(x7, d6):
    """PoseLocalParameterization::Plus on plain arrays: p + dp, q * [dtheta / 2, 1] normalised"""
    x7 = np.asarray(x7, float)
    out = x7.copy()
    out[:3] += d6[:3]
    dq = A(np.array([d6[3] / 2, d6[4] / 2, d6[5] / 2, 1.0]))
    q = qmul(A(x7[3:]), dq).v
    out[3:] = q / np.linalg.norm(q)
    return out


# ---------------------------------------------------------------- IMU factor
def sqrt_info(cov):
    """U upper-triangular with U^T U = cov^-1 (LLT(cov^-1).matrixL().transpose(), imu_factor.h:74-75) as an A.  Its magnitude holds, beside |U|, the first-order
    reach of the inverse's own rounding: any float64 inverse W of cov is off by ~eps |W| |cov| |W| entrywise, which moves the factor by
    dU = triu'(U^-T dW U^-1) U, bounded entrywise by triu(|U^-T| (|W| |cov| |W|) |U^-1|) |U| (upper-triangular like U: the zeros below the diagonal stay exact)."""
    cov = np.asarray(cov, np.float64).reshape(15, 15)
    W = np.linalg.inv(cov)
    U = np.linalg.cholesky(0.5 * (W + W.T)).T
    Ui = np.linalg.inv(U)
    MW = np.abs(W) @ np.abs(cov) @ np.abs(W)
    return A(U, np.abs(U) + np.triu(np.abs(Ui.T) @ MW @ np.abs(Ui)) @ np.abs(U))


def imu_raw(pre, g_norm, pose_i, sb_i, pose_j, sb_j):
    """(r[15], J[15, 30]) before whitening, as A; columns: pose_i 6 | speed-bias_i 9 | pose_j 6 | speed-bias_j 9 (tangent space).
    pre: dict(sum_dt, dp[3], dq[4] w x y z, dv[3], lin_ba[3], lin_bg[3], jacobian[15, 15] in the order P R V BA BG)"""
    G = A(np.array([0.0, 0.0, float(g_norm)]))
    pose_i, sb_i, pose_j, sb_j = A(pose_i), A(sb_i), A(pose_j), A(sb_j)
    Pi, Qi, Pj, Qj = pose_i[:3], pose_i[3:], pose_j[:3], pose_j[3:]
    Vi, Bai, Bgi, Vj, Baj, Bgj = sb_i[:3], sb_i[3:6], sb_i[6:9], sb_j[:3], sb_j[3:6], sb_j[6:9]
    jac = A(np.asarray(pre["jacobian"], float).reshape(15, 15))
    dp_dba, dp_dbg, dq_dbg, dv_dba, dv_dbg = jac[0:3, 9:12], jac[0:3, 12:15], jac[3:6, 12:15], jac[6:9, 9:12], jac[6:9, 12:15]
    dq_wxyz = np.asarray(pre["dq"], float)
    dq = A(np.array([dq_wxyz[1], dq_wxyz[2], dq_wxyz[3], dq_wxyz[0]]))
    dt = A(float(pre["sum_dt"]))
    dba, dbg = Bai - A(pre["lin_ba"]), Bgi - A(pre["lin_bg"])
    theta = dq_dbg @ dbg
    cq = qmul(dq, hcat([theta / 2.0, stack([1.0])]))              # Utility::deltaQ: [1, theta / 2], not normalised
    cv = A(pre["dv"]) + dv_dba @ dba + dv_dbg @ dbg
    cp = A(pre["dp"]) + dp_dba @ dba + dp_dbg @ dbg
    RiT = qR(qinv(Qi))
    a = RiT @ (0.5 * G * dt * dt + Pj - Pi - Vi * dt)
    b = RiT @ (G * dt + Vj - Vi)
    qij = qmul(qinv(Qi), Qj)
    e = qmul(qinv(cq), qij)
    r = hcat([a - cp, 2.0 * e[:3], b - cv, Baj - Bai, Bgj - Bgi])
    J = zeros(15, 30)

    def put(r0, c0, blk):
        J.v[r0:r0 + 3, c0:c0 + 3] = blk.v
        J.m[r0:r0 + 3, c0:c0 + 3] = blk.m
    I3 = eye3()
    qji = qmul(qinv(Qj), Qi)
    put(0, 0, -RiT); put(0, 3, skew(a))
    put(3, 3, -(qleft4(qji) @ qright4(cq))[1:, 1:])
    put(6, 3, skew(b))
    put(0, 6, -(RiT * dt)); put(0, 9, -dp_dba); put(0, 12, -dp_dbg)
    put(3, 12, -(qleft_br(qmul(qji, dq)) @ dq_dbg))
    put(6, 6, -RiT); put(6, 9, -dv_dba); put(6, 12, -dv_dbg)
    put(9, 9, -I3); put(12, 12, -I3)
    put(0, 15, RiT)
    put(3, 18, qleft_br(e))
    put(6, 21, RiT); put(9, 24, I3); put(12, 27, I3)
    return r, J


def imu_factor(pre, g_norm, pose_i, sb_i, pose_j, sb_j, U=None):
    """whitened (r[15], J[15, 30]) as A; U: sqrt_info(pre["covariance"]) unless given"""
    r, J = imu_raw(pre, g_norm, pose_i, sb_i, pose_j, sb_j)
    if U is None:
        U = sqrt_info(pre["covariance"])
    return U @ r, U @ J


def imu_cq_norm2(pre, sb_i):
    """|corrected delta_q|^2 / |delta_q|^2 = 1 + |dq_dbg (Bg_i - lin_bg)|^2 / 4"""
    jac = np.asarray(pre["jacobian"], float).reshape(15, 15)
    th = jac[3:6, 12:15] @ (np.asarray(sb_i, float)[6:9] - np.asarray(pre["lin_bg"], float))
    return 1.0 + float(th @ th) / 4.0


def pre_from_record(rec):
    """dict for imu_raw from one IMU_DTYPE record"""
    return dict(sum_dt=float(rec["sum_dt"]), dp=np.array(rec["dp"], float), dq=np.array(rec["dq"], float), dv=np.array(rec["dv"], float),
                lin_ba=np.array(rec["lin_ba"], float), lin_bg=np.array(rec["lin_bg"], float), jacobian=np.array(rec["jacobian"], float).reshape(15, 15),
                covariance=np.array(rec["covariance"], float).reshape(15, 15))


# ---------------------------------------------------------------- projection factors
PROJ_KEYS = ("Ji", "Jj", "Jex0", "Jex1", "Jl", "Jtd")


def proj_factor(f, pose_i, pose_j, ex0, ex1, lam, td):
    """(r[2], dict Ji, Jj, Jex0, Jex1 [2, 6], Jl, Jtd [2]) of one residual block as A.  f: mapping with pix piy pjx pjy vix viy vjx vjy td_i td_j kind.
    Blocks a kind does not have (kind 0: ex1; kind 2: the poses) are exact zeros."""
    kind = int(f["kind"])
    pts_i, pts_j = A(np.array([f["pix"], f["piy"], 1.0])), A(np.array([f["pjx"], f["pjy"], 1.0]))
    vi, vj = A(np.array([f["vix"], f["viy"], 0.0])), A(np.array([f["vjx"], f["vjy"], 0.0]))
    pose_i, pose_j, ex0, ex1 = A(pose_i), A(pose_j), A(ex0), A(ex1)
    lam, td = A(float(lam)), A(float(td))
    pts_i_td = pts_i - (td - A(float(f["td_i"]))) * vi
    pts_j_td = pts_j - (td - A(float(f["td_j"]))) * vj
    Pi, Pj, tic = pose_i[:3], pose_j[:3], ex0[:3]
    Ri, Rj, ric = qR(pose_i[3:]), qR(pose_j[3:]), qR(ex0[3:])
    tcj, rcj = (tic, ric) if kind == 0 else (ex1[:3], qR(ex1[3:]))
    pc_i = pts_i_td / lam
    p_imu_i = ric @ pc_i + tic
    p_imu_j = Rj.T @ (Ri @ p_imu_i + Pi - Pj) if kind != 2 else p_imu_i
    pcj = rcj.T @ (p_imu_j - tcj)
    dep = pcj[2]
    s = A(SQRT_INFO)
    r = s * (hcat([stack([pcj[0] / dep]), stack([pcj[1] / dep])]) - pts_j_td[:2])
    z = A(0.0)
    red = s * stack([[1.0 / dep, z, -pcj[0] / (dep * dep)], [z, 1.0 / dep, -pcj[1] / (dep * dep)]])
    out = {k: zeros(2, 6) for k in ("Ji", "Jj", "Jex0", "Jex1")}
    lam2 = lam * lam
    if kind != 2:
        Am = rcj.T @ Rj.T
        ARi = Am @ Ri
        T = ARi @ ric
        out["Ji"] = hcat([red @ Am, red @ (ARi @ -skew(p_imu_i))])
        out["Jj"] = hcat([red @ -Am, red @ (rcj.T @ skew(p_imu_j))])
        if kind == 0:
            left = ric.T @ (Rj.T @ Ri - eye3())
            right = -(T @ skew(pc_i)) + skew(T @ pc_i) + skew(ric.T @ (Rj.T @ (Ri @ tic + Pi - Pj) - tic))
            out["Jex0"] = hcat([red @ left, red @ right])
        else:
            out["Jex0"] = hcat([red @ ARi, red @ (T @ -skew(pc_i))])
            out["Jex1"] = hcat([red @ -rcj.T, red @ skew(pcj)])
        out["Jl"] = red @ (T @ pts_i_td) * -1.0 / lam2
    else:
        T = rcj.T @ ric
        out["Jex0"] = hcat([red @ rcj.T, red @ (T @ -skew(pc_i))])
        out["Jex1"] = hcat([red @ -rcj.T, red @ skew(pcj)])
        out["Jl"] = red @ (T @ pts_i) * -1.0 / lam2               # Q7: pts_i, not pts_i_td
    out["Jtd"] = red @ (T @ vi) / lam * -1.0 + s * vj[:2]
    out["dep"] = dep                                              # depth of the point in camera j (not part of the record)
    return r, out


def proj_flat(r, J):
    """the 54 doubles of dv_proj_eval's record: r | Ji | Jj | Jex0 | Jex1 | Jl | Jtd, as A"""
    return hcat([r] + [A(J[k].v.reshape(-1), J[k].m.reshape(-1)) for k in PROJ_KEYS])


# ---------------------------------------------------------------- numeric Jacobians on the manifold
def _central(fun, blocks, kinds, h):
    """central differences of fun(blocks) -> residual vector; kinds[k]: "pose" (7 -> 6, Plus on the manifold) or "vec" (additive)"""
    cols = []
    for k, (b, kd) in enumerate(zip(blocks, kinds)):
        n = 6 if kd == "pose" else len(b)
        for c in range(n):
            d = np.zeros(n)
            vals = []
            for sg in (+1.0, -1.0):
                d[c] = sg * h
                pert = plus_pose(b, d) if kd == "pose" else np.asarray(b, float) + d
                vals.append(fun([pert if i == k else blocks[i] for i in range(len(blocks))]))
            cols.append((vals[0] - vals[1]) / (2.0 * h))
    return np.array(cols).T


def numeric_jacobian(fun, blocks, kinds, h=1e-3):
    """Richardson extrapolation of central differences at steps h and h / 2: (4 D(h / 2) - D(h)) / 3, error O(h^4)"""
    return (4.0 * _central(fun, blocks, kinds, h / 2.0) - _central(fun, blocks, kinds, h)) / 3.0


def imu_numeric(pre, g_norm, pose_i, sb_i, pose_j, sb_j, h=1e-3):
    """numeric 15 x 30 Jacobian of the raw residual"""
    return numeric_jacobian(lambda b: imu_raw(pre, g_norm, b[0], b[1], b[2], b[3])[0].v, [pose_i, sb_i, pose_j, sb_j], ["pose", "vec", "pose", "vec"], h)


def proj_numeric(f, pose_i, pose_j, ex0, ex1, lam, td, h=1e-4):
    """numeric Jacobians of one block in the layout of proj_factor's dict"""
    J = numeric_jacobian(lambda b: proj_factor(f, b[0], b[1], b[2], b[3], b[4][0], b[5][0])[0].v,
                         [pose_i, pose_j, ex0, ex1, np.array([lam]), np.array([td])], ["pose", "pose", "pose", "pose", "vec", "vec"], h)
    return dict(Ji=J[:, 0:6], Jj=J[:, 6:12], Jex0=J[:, 12:18], Jex1=J[:, 18:24], Jl=J[:, 24], Jtd=J[:, 25])


# ---------------------------------------------------------------- gauge fix (rotations as matrices)
def rot_of(q_xyzw):
    return qR(A(np.asarray(q_xyzw, float))).v


def r2ypr(R):
    """Utility::R2ypr (utility.h:86-101), degrees"""
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    y = np.arctan2(n[1], n[0])
    p = np.arctan2(-n[2], n[0] * np.cos(y) + n[1] * np.sin(y))
    r = np.arctan2(a[0] * np.sin(y) - a[1] * np.cos(y), -o[0] * np.sin(y) + o[1] * np.cos(y))
    return np.array([y, p, r]) / np.pi * 180.0


def ypr2r(ypr):
    """Utility::ypr2R (utility.h:104-131), degrees"""
    y, p, r = np.asarray(ypr, float) / 180.0 * np.pi
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1.0]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1.0, 0], [-np.sin(p), 0, np.cos(p)]])
    Rx = np.array([[1.0, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    return Rz @ Ry @ Rx


def quat_of(R):
    """x y z w of a rotation matrix without a case distinction: the eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix
    whose quadratic form is trace(R(q)^T R) (Bar-Itzhack)"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, V = np.linalg.eigh(K)
    return V[:, -1]


def qfromR_case(R):
    """which of the four cases of Eigen's matrix -> quaternion conversion R falls in: 0 trace > 0, else 1 + index of the largest diagonal entry
    (ties to the lower index, as `if (m(1,1) > m(0,0)) i = 1; if (m(2,2) > m(i,i)) i = 2`)"""
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return 1 + i


def quat_eigen(R):
    """x y z w as Eigen's Quaternion(Matrix3) conversion writes it (Shoemake's four cases, no normalisation).  Only for an expected matrix that is NOT a
    rotation (the singular branch on an un-normalised frame-0 quaternion: rot = R0 R00^T inherits the norm error), where quat_of's nearest rotation is not
    what the reference hands on; everywhere else the tests compare with quat_of."""
    c = qfromR_case(R)
    q = np.zeros(4)
    if c == 0:
        t = np.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
        return q
    i = c - 1
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3], q[j], q[k] = (R[k, j] - R[j, k]) * t, (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    return q


def gauge_singular(pose0, ypr0):
    """the Euler-singularity test of body.cpp:71 on the solved frame 0 (quaternion NOT normalised, as there) and the pre-solve ypr"""
    y00 = r2ypr(rot_of(np.asarray(pose0, float)[3:]))
    return bool(abs(abs(ypr0[1]) - 90) < 1.0 or abs(abs(y00[1]) - 90) < 1.0)


def gauge_fix(states, R0, ypr0, P0, use_imu, nframes):
    """Double2vector's yaw and position fix.  states: dict(pose[11, 7], sb[11, 9]).  -> dict
         R[11, 3, 3], P[11, 3], V[11, 3]   the fixed window (frames >= nframes: the input, R from the input quaternion as it is)
         R_mag, P_mag, V_mag               the same expressions on absolute values
         fixed[11]                         False for frames >= nframes (the caller compares those bit for bit with the input)
         singular                          whether the Euler-singularity branch was taken (rot = R0 R00^T instead of the yaw difference)
       With use_imu = 0 only the quaternion is normalised: P and V are the inputs themselves."""
    pose, sb = np.asarray(states["pose"], float), np.asarray(states["sb"], float)
    R0, ypr0, P0 = np.asarray(R0, float).reshape(3, 3), np.asarray(ypr0, float), np.asarray(P0, float)
    out = dict(R=np.zeros((11, 3, 3)), P=pose[:, :3].copy(), V=sb[:, :3].copy(), R_mag=np.zeros((11, 3, 3)), P_mag=np.abs(pose[:, :3]), V_mag=np.abs(sb[:, :3]),
               fixed=np.arange(11) < nframes, singular=False)
    rot, rot_mag = np.eye(3), np.eye(3)
    if use_imu:
        R00 = rot_of(pose[0, 3:])
        y00 = r2ypr(R00)
        out["singular"] = gauge_singular(pose[0], ypr0)
        if out["singular"]:
            rot, rot_mag = R0 @ R00.T, np.abs(R0) @ qR(A(pose[0, 3:])).m.T
        else:
            rot = ypr2r([ypr0[0] - y00[0], 0.0, 0.0])
            # yaw(R00) = atan2(R00[1, 0], R00[0, 0]): both entries shrink with cos(pitch) while their rounding (that of 1 - 2 (yy + zz), 2 (xy + zw)) does not, so
            # the yaw, and with it the four entries of the yaw rotation, carry rounding of the size 1 / |cos(pitch)|
            amp = 1.0 / max(abs(np.cos(y00[1] / 180.0 * np.pi)), 1e-300)
            rot_mag = np.abs(rot)
            rot_mag[:2, :2] += amp
    for i in range(11):
        q = A(pose[i, 3:])
        if i >= nframes:
            out["R"][i], out["R_mag"][i] = qR(q).v, qR(q).m
            continue
        n = np.linalg.norm(pose[i, 3:])
        Rn = qR(A(pose[i, 3:] / n))
        out["R"][i], out["R_mag"][i] = rot @ Rn.v, rot_mag @ Rn.m
        if use_imu:
            out["P"][i] = rot @ (pose[i, :3] - pose[0, :3]) + P0
            out["P_mag"][i] = rot_mag @ (np.abs(pose[i, :3]) + np.abs(pose[0, :3])) + np.abs(P0)
            out["V"][i], out["V_mag"][i] = rot @ sb[i, :3], rot_mag @ np.abs(sb[i, :3])
    return out


# ---------------------------------------------------------------- outlier test
def reject_errors(pose, ric, tic, inv_depth, factors, landmarks, focal):
    """per landmark: mean over its residual blocks of |pts_cj.xy / pts_cj.z - uv_j| (ReprojectionError), times focal — the quantity OutliersRejection compares with 3.
    pose[11, 7] (quaternions normalised first, as Double2vector leaves Rs); ric[2, 3, 3], tic[2, 3]: camera 0 lifts the anchor observation, kind 0 re-projects
    into camera 0 and kinds 1, 2 into camera 1; kind 2 observes in the anchor frame itself."""
    pose = np.asarray(pose, float)
    Rs = [rot_of(p[3:] / np.linalg.norm(p[3:])) for p in pose]
    ric, tic = np.asarray(ric, float).reshape(2, 3, 3), np.asarray(tic, float).reshape(2, 3)
    out = np.zeros(len(landmarks))
    for l, L in enumerate(landmarks):
        err, a = 0.0, int(L["anchor"])
        depth = 1.0 / inv_depth[l]
        for f in factors[int(L["first"]):int(L["first"]) + int(L["count"])]:
            j, cam = int(f["fj"]), 0 if int(f["kind"]) == 0 else 1
            pw = Rs[a] @ (ric[0] @ (depth * np.array([f["pix"], f["piy"], 1.0])) + tic[0]) + pose[a, :3]
            pc = ric[cam].T @ (Rs[j].T @ (pw - pose[j, :3]) - tic[cam])
            err += np.hypot(pc[0] / pc[2] - f["pjx"], pc[1] / pc[2] - f["pjy"])
        out[l] = err / int(L["count"]) * focal
    return out


def reject_flags(pose, ex_pose, ric, tic, inv_depth, factors, landmarks, focal, ex_from_state):
    """flags of OutliersRejection (error > 3) and the errors themselves; ex_from_state: the extrinsics are the state's para_ex_pose (normalised quaternion), not ric / tic"""
    if ex_from_state:
        ex = np.asarray(ex_pose, float).reshape(2, 7)
        ric = np.array([rot_of(e[3:] / np.linalg.norm(e[3:])) for e in ex])
        tic = ex[:, :3]
    err = reject_errors(pose, ric, tic, inv_depth, factors, landmarks, focal)
    return (err > 3).astype(np.uint8), err
