"""Plain float64 restatement of the line, box and instance factors (test infrastructure, numpy only), on the `A` values of tests/factor_ref.py.

Written from the mathematics of the reference, not from oracle/ and not from be_obj_dev.h:
  line_factor      lineProjectionFactor::Evaluate (factor/line_projection_factor.cpp:24-159), orth_to_plk / plk_to_pose / plk_from_pose
                   (line_detector/line_geometry.cpp:97-135, 210-229)
  line_plus        LineOrthParameterization::Plus (factor/line_parameterization.cpp:9-72)
  box_enclose      BoxEncloseStereoPointFactor::Evaluate (factor/box_factor.cpp:523-565)                                   I1
  box_dims         BoxDimsFactor::Evaluate (factor/box_factor.cpp:728-743)                                                  I2
  box_orientation  BoxOrientationFactor::Evaluate (factor/box_factor.cpp:752-806), Sophus SO3d(R).log(): Eigen's matrix -> quaternion conversion,
                   normalised, then the logarithm with its Taylor branch (|vec|^2 < 1e-20) and its |w| < 1e-10 branch           I3
  inst_proj        ProjectionInstanceFactor::Evaluate (factor/project_instance_factor.cpp:27-172)
Quaternions are stored x y z w after the position (p, qx qy qz qw).  Quaternion * vector is Eigen's v + w (2 u x v) + u x (2 u x v), inverse() divides the
conjugate by the squared norm, toRotationMatrix() does not normalise.

Forms that are NOT the derivative of the residual and are kept as the reference writes them (tests/test_objfactor_reference.py pins each gap):
  I1  d r / d P = N_p R_ojw with N_p = diag(e / |e|), e = R_ojw (p_obj - P) (sic: the object-frame point minus the WORLD position), without the factor -10 and
      without the clamp (a point inside the box has r = 0 and a Jacobian); the rotation columns are zero;
  I2  d r / d box = 2 (box - dims)^T for r = |box - dims|^4 / 100;
  I3  the body Jacobian is zero; the object Jacobian is -J_r^-1 R^T with J_r = sin t / t I + (1 - sin t / t) a a^T + (1 - cos t / t) hat(a), t = -|phi| (sic:
      (1 - cos t) / t is the right Jacobian);
  inst_proj  d r / d lambda = + reduce T pts_j / lambda^2: the sign, and pts_j without the td compensation;
  line   u1 = n / |n|, u2 = v / |v| are recomputed from norms: they are sign(cos phi) U1 and sign(sin phi) U2, so the orth Jacobian's columns carry the signs
         (s1, s2, s1 s2, s1 s2) against the derivative once cos phi or sin phi is negative.
Where the reference's own formula is 0 / 0 the restatement returns NaN in exactly those entries (numpy follows IEEE as Eigen does): N_p with a zero component
of e (that row of the Jacobian), the orientation J_r at theta = 0 (the 3 x 3 rotation block), u2 at phi = 0 (the whole orth Jacobian)."""
import numpy as np

from tests import factor_ref as fr
from tests.factor_ref import A, eye3, hcat, qR, qinv, skew, stack, zeros

SQRT_INFO = fr.SQRT_INFO


def cross(a, b):
    return stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def norm3(v):
    return fr.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def qrot(q, v):
    """Eigen::Quaternion::operator*(Vector3): uv = 2 u x v; v + w uv + u x uv"""
    u = q[:3]
    uv = cross(u, v)
    uv = uv + uv
    return v + q[3] * uv + cross(u, uv)


def flat(x):
    return A(x.v.reshape(-1), x.m.reshape(-1))


def _b66(TL, TR, BR):
    """[[TL TR] [0 BR]]: every 6 x 6 of the line factor has an exactly zero lower-left block"""
    z = np.zeros((3, 3))
    return A(np.block([[TL.v, TR.v], [z, BR.v]]), np.block([[TL.m, TR.m], [z, BR.m]]))


# ---------------------------------------------------------------- line factor
def orth_U(orth):
    s1, c1, s2, c2, s3, c3 = fr.sin(orth[0]), fr.cos(orth[0]), fr.sin(orth[1]), fr.cos(orth[1]), fr.sin(orth[2]), fr.cos(orth[2])
    return stack([[c2 * c3, s1 * s2 * c3 - c1 * s3, c1 * s2 * c3 + s1 * s3],
                  [c2 * s3, s1 * s2 * s3 + c1 * c3, c1 * s2 * s3 - s1 * c3],
                  [-s2, s1 * c2, c1 * c2]])


def _plk_to_pose(n, v, Rcw, tcw):
    vc = Rcw @ v
    return Rcw @ n + skew(tcw) @ vc, vc


def _plk_from_pose(n, v, Rcw, tcw):
    Rwc = Rcw.T
    return _plk_to_pose(n, v, Rwc, -(Rwc @ tcw))


def line_factor(obs, sqrt_info, pose, ex, orth, parts=False):
    """-> r (2), J_pose 2 x 6, J_ex 2 x 6, J_orth 2 x 4 as A; sqrt_info: the 2 x 2 row-major.  parts: also a dict with n_c, l_sqrt, cos / sin phi"""
    with np.errstate(all="ignore"), fr.first_order():
        obs, S, pose, ex, orth = A(obs), A(np.asarray(sqrt_info, float).reshape(2, 2)), A(pose), A(ex), A(orth)
        U = orth_U(orth)
        w1, w2 = fr.cos(orth[3]), fr.sin(orth[3])
        nw, vw = w1 * U[:, 0], w2 * U[:, 1]
        Rwb, twb, Rbc, tbc = qR(pose[3:]), pose[:3], qR(ex[3:]), ex[:3]
        nb, vb = _plk_from_pose(nw, vw, Rwb, twb)
        nc, vc = _plk_from_pose(nb, vb, Rbc, tbc)
        l2 = nc[0] * nc[0] + nc[1] * nc[1]
        l1 = fr.sqrt(l2)
        l3 = l2 * l1
        e1 = obs[0] * nc[0] + obs[1] * nc[1] + nc[2]
        e2 = obs[2] * nc[0] + obs[3] * nc[1] + nc[2]
        r = S @ stack([e1 / l1, e2 / l1])
        je = S @ stack([[obs[0] / l1 - nc[0] * e1 / l3, obs[1] / l1 - nc[1] * e1 / l3, 1.0 / l1],
                        [obs[2] / l1 - nc[0] * e2 / l3, obs[3] / l1 - nc[1] * e2 / l3, 1.0 / l1]])
        jeLc = hcat([je, zeros(2, 3)])
        invTbc = _b66(Rbc.T, -(Rbc.T @ skew(tbc)), Rbc.T)
        jp = _b66(Rwb.T @ skew(vw), skew(Rwb.T @ (nw + skew(vw) @ twb)), skew(Rwb.T @ vw))
        J_pose = jeLc @ (invTbc @ jp)
        J_ex = jeLc @ _b66(Rbc.T @ skew(vb), skew(Rbc.T @ (nb + skew(vb) @ tbc)), skew(Rbc.T @ vb))
        Rwc, twc = Rwb @ Rbc, Rwb @ tbc + twb
        invTwc = _b66(Rwc.T, -(Rwc.T @ skew(twc)), Rwc.T)
        nn, vn = norm3(nw), norm3(vw)
        u1, u2 = nw / nn, vw / vn
        u3 = cross(u1, u2)
        wn = fr.sqrt(nn * nn + vn * vn)
        w0, w1n = nn / wn, vn / wn
        jlo = zeros(6, 4)

        def put(r0, c, col):
            jlo.v[r0:r0 + 3, c], jlo.m[r0:r0 + 3, c] = col.v, col.m
        put(3, 0, w1n * u3); put(0, 1, -(w0 * u3)); put(0, 2, w0 * u2); put(3, 2, -(w1n * u1)); put(0, 3, -(w1n * u1)); put(3, 3, w0 * u2)
        J_orth = (jeLc @ invTwc) @ jlo
    if parts:
        return r, J_pose, J_ex, J_orth, dict(nc=nc.v, l_sqrt=float(l1.v), n_norm=float(np.linalg.norm(nc.v)), cphi=float(w1.v), sphi=float(w2.v), U=U.v)
    return r, J_pose, J_ex, J_orth


def line_flat(out):
    """the 34 doubles of dv_line_eval's record: r | J_pose | J_ex | J_orth"""
    return hcat([out[0], flat(out[1]), flat(out[2]), flat(out[3])])


def line_plus(orth, delta, fold=True):
    """orth (+) delta -> 4 as A.  fold=False: the phase is returned as phi + delta_3 instead of asin(sin(phi + delta_3)): the same U and W as a point of the
    parameter space, for derivatives at a phase outside (-pi/2, pi/2) (not a form of the reference)"""
    with np.errstate(all="ignore"), fr.first_order():
        orth, d = A(orth), A(delta)
        U = orth_U(orth)
        w1, w2 = fr.cos(orth[3]), fr.sin(orth[3])
        z, one = A(0.0), A(1.0)
        c, s = [fr.cos(d[k]) for k in range(4)], [fr.sin(d[k]) for k in range(4)]
        Rz = stack([[c[2], -s[2], z], [s[2], c[2], z], [z, z, one]])
        Ry = stack([[c[1], z, s[1]], [z, one, z], [-s[1], z, c[1]]])
        Rx = stack([[one, z, z], [z, c[0], -s[0]], [z, s[0], c[0]]])
        R = ((U @ Rx) @ Ry) @ Rz
        W10 = w2 * c[3] + w1 * s[3]
        phase = fr.asin(W10) if fold else orth[3] + d[3]
        return stack([fr.atan2(R[2, 1], R[2, 2]), fr.asin(-R[2, 0]), fr.atan2(R[1, 0], R[0, 0]), phase])


# ---------------------------------------------------------------- box factors
def box_enclose(p_w, dims, pose_obj, parts=False):
    """-> r (3), J 3 x 6 as A (rotation columns exactly zero; a clamped residual is exactly zero)"""
    with np.errstate(all="ignore"), fr.first_order():
        p, d, x = A(p_w), A(dims), A(pose_obj)
        P, q = x[:3], x[3:]
        qi = qinv(q)
        po = qrot(qi, p - P)
        ve = (A(np.abs(po.v), po.m) - d / 2.0) * 10.0
        out = ve.v > 0
        r = A(np.where(out, ve.v, 0.0), np.where(out, ve.m, 0.0))
        Rojw = qR(qi)
        e = Rojw @ (po - P)
        sg = e.v / np.abs(e.v)                                    # exactly +-1, NaN at 0
        Np = A(sg, np.where(np.isfinite(sg), 1.0, np.nan))
        J = hcat([stack([Np[i] * Rojw[i] for i in range(3)]), zeros(3, 3)])
    if parts:
        return r, J, dict(po=po.v, e=e.v, face=np.abs(po.v) - d.v / 2.0)
    return r, J


def box_flat(out):
    return hcat([out[0], flat(out[1])])


def box_dims(dims, box):
    """-> r (scalar), J 1 x 3 as A"""
    with fr.first_order():
        d = A(box) - A(dims)
        err = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        return err * err / 100.0, stack([2.0 * d])


def dims_flat(out):
    return hcat([stack([out[0]]), flat(out[1])])


def mulE(a, b):
    """the first-order product |a| m_b + |b| m_a whatever the mode (factor_ref.first_order)"""
    a, b = A.of(a), A.of(b)
    return A(a.v * b.v, np.abs(a.v) * b.m + np.abs(b.v) * a.m)


def matE(a, b):
    return A(a.v @ b.v, np.abs(a.v) @ b.m + a.m @ np.abs(b.v))


def qfromR(R):
    """Eigen's Quaternion(Matrix3) on A values, x y z w"""
    case = fr.qfromR_case(R.v)
    if case == 0:
        t = fr.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return stack([mulE(R[2, 1] - R[1, 2], t), mulE(R[0, 2] - R[2, 0], t), mulE(R[1, 0] - R[0, 1], t), w])
    i = case - 1
    j, k = (i + 1) % 3, (i + 2) % 3
    t = fr.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q = [None] * 4
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3], q[j], q[k] = mulE(R[k, j] - R[j, k], t), mulE(R[j, i] + R[i, j], t), mulE(R[k, i] + R[i, k], t)
    return stack(q)


def so3_log(R, wsign=None):
    """Sophus SO3d(R).log() -> (phi as A, dict branch, w, case).  wsign = +-1 replaces the sign of the quaternion's w (where a rounding decides it)"""
    q = qfromR(R)
    q = q / fr.sqrt(mulE(q[0], q[0]) + mulE(q[1], q[1]) + mulE(q[2], q[2]) + mulE(q[3], q[3]))
    w = q[3]
    if wsign is not None:
        w = A(wsign * np.abs(w.v), w.m)
    positive = (w.v > 0) if wsign is None else (wsign > 0)
    sq = mulE(q[0], q[0]) + mulE(q[1], q[1]) + mulE(q[2], q[2])
    if sq.v < 1e-20:
        branch, two_atan = "taylor", 2.0 / w - 2.0 / 3.0 * sq / mulE(mulE(w, w), w)
    else:
        n = fr.sqrt(sq)
        if abs(w.v) < 1e-10:
            branch, two_atan = "pi", A(np.pi if positive else -np.pi) / n
        else:
            branch, two_atan = "atan", 2.0 * fr.atan(n / w) / n
    return mulE(q[:3], two_atan), dict(branch=branch, w=float(w.v), case=fr.qfromR_case(R.v))


def ori_Jr(phi, derivative=False):
    """the reference's J_r (derivative=True: the right Jacobian it stands for, (1 - cos t) / t) and a, theta = -|phi|"""
    pn = fr.sqrt(mulE(phi[0], phi[0]) + mulE(phi[1], phi[1]) + mulE(phi[2], phi[2]))
    a = phi / pn if pn.v > 0 else phi                              # Eigen's normalized() leaves a zero vector alone
    th = A(-pn.v, pn.m)
    st = fr.sin(th) / th
    ct = (1.0 - fr.cos(th)) / th if derivative else 1.0 - fr.cos(th) / th
    aat = stack([[mulE(a[i], a[j]) for j in range(3)] for i in range(3)])
    return st * eye3() + mulE(1.0 - st, aat) + mulE(ct, skew(a)), a, th


def ori_Jr_inverse(phi):
    """the inverse of the reference's J_r = al I + (1 - al) a a^T + ga hat(a) in closed form: x I + (1 - x) a a^T + z hat(a) with x = al / (al^2 + ga^2),
    z = -ga / (al^2 + ga^2) (on a it is 1, across a it is the complex number al + i ga).  It carries what the rounding of phi does to the inverse: about
    1 / |phi|, through a = phi / |phi| and ga ~ 1 / |phi|.  The cofactor form cannot: its 1e36 terms cancel to a determinant of 1e24 at |phi| = 1e-12, and a
    bound that does not know that they move together reports twelve digits more than are lost."""
    pn = fr.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
    a = phi / pn if pn.v > 0 else phi
    th = A(-pn.v, pn.m)
    al, ga = fr.sin(th) / th, 1.0 - fr.cos(th) / th
    den = al * al + ga * ga
    x, z = al / den, -(ga / den)
    aat = stack([[a[i] * a[j] for j in range(3)] for i in range(3)])
    return x * eye3() + (1.0 - x) * aat + z * skew(a)


def inv3(J):
    """Eigen's 3 x 3 inverse(): cofactors over the determinant"""
    c = [[mulE(J[(i + 1) % 3, (j + 1) % 3], J[(i + 2) % 3, (j + 2) % 3]) - mulE(J[(i + 1) % 3, (j + 2) % 3], J[(i + 2) % 3, (j + 1) % 3]) for j in range(3)] for i in range(3)]
    det = mulE(J[0, 0], c[0][0]) + mulE(J[0, 1], c[0][1]) + mulE(J[0, 2], c[0][2])
    return stack([[c[j][i] / det for j in range(3)] for i in range(3)])


def box_orientation(R_cioi, R_bc, pose_body, pose_obj, wsign=None, derivative=False, parts=False):
    """-> r (3), J_body 3 x 6 (exactly zero), J_obj 3 x 6 (position columns exactly zero) as A"""
    with np.errstate(all="ignore"), fr.first_order():
        Rc, Rb = A(np.asarray(R_cioi, float).reshape(3, 3)), A(np.asarray(R_bc, float).reshape(3, 3))
        Rwbi, Rwoi = qR(A(pose_body)[3:]), qR(A(pose_obj)[3:])
        R = ((Rwoi.T @ Rwbi) @ Rb) @ Rc
        phi, info = so3_log(R, wsign)
        Jr, a, th = ori_Jr(phi, derivative)
        inv = inv3(A(Jr.v))                                       # the reference's arithmetic on J_r as it stands: the value, and the cofactors' own rounding
        if not derivative:
            inv = A(inv.v, inv.m + ori_Jr_inverse(phi).m)
        jac = -matE(inv, R.T)
    out = phi, zeros(3, 6), hcat([zeros(3, 3), jac])
    if parts:
        with np.errstate(all="ignore"), fr.first_order():
            info.update(R=R.v, theta=float(-th.v), Jr=Jr, a=a.v, inv=inv, inv_closed=None if derivative else ori_Jr_inverse(phi))
        return out + (info,)
    return out


def ori_flat(out):
    return hcat([out[0], flat(out[1]), flat(out[2])])


# ---------------------------------------------------------------- instance projection factor
def inst_proj(f, pbj, pbi, pex, poj, poi, lam, parts=False):
    """the 64 outputs of inst_proj_dev as A: r[2] | J wrt body pose j, body pose i, extrinsic, object pose j, object pose i (2 x 6 each) | J wrt inv_dep_j (2).
    f: mapping with pts_j[3] pts_i[3] vel_j[2] vel_i[2] td_j td_i cur_td"""
    with np.errstate(all="ignore"), fr.first_order():
        pts_j, pts_i = A(np.asarray(f["pts_j"], float)), A(np.asarray(f["pts_i"], float))
        vj, vi = A(np.append(np.asarray(f["vel_j"], float), 0.0)), A(np.append(np.asarray(f["vel_i"], float), 0.0))
        cur = A(float(f["cur_td"]))
        pts_i_td = pts_i - (cur - A(float(f["td_i"]))) * vi
        pts_j_td = pts_j - (cur - A(float(f["td_j"]))) * vj
        pbj, pbi, pex, poj, poi, lam = A(pbj), A(pbi), A(pex), A(poj), A(poi), A(float(lam))
        Pbj, Qbj, Pbi, Qbi, Pbc, Qbc, Poj, Qoj, Poi, Qoi = pbj[:3], pbj[3:], pbi[:3], pbi[3:], pex[:3], pex[3:], poj[:3], poj[3:], poi[:3], poi[3:]
        cam_j = pts_j_td / lam
        imu_j = qrot(Qbc, cam_j) + Pbc
        w_j = qrot(Qbj, imu_j) + Pbj
        obj_j = qrot(qinv(Qoj), w_j - Poj)
        w_i = qrot(Qoi, obj_j) + Poi
        imu_i = qrot(qinv(Qbi), w_i - Pbi)
        cam_i = qrot(qinv(Qbc), imu_i - Pbc)
        dep = cam_i[2]
        s, z = A(SQRT_INFO), A(0.0)
        r = s * (hcat([stack([cam_i[0] / dep]), stack([cam_i[1] / dep])]) - pts_i_td[:2])
        red = s * stack([[1.0 / dep, z, -cam_i[0] / (dep * dep)], [z, 1.0 / dep, -cam_i[1] / (dep * dep)]])
        Rbj, Rbiw, Rbc, Roj, Roi = qR(Qbj), qR(Qbi).T, qR(Qbc), qR(Qoj), qR(Qoi)
        Rcb, Rojw = Rbc.T, Roj.T
        t_oi = (Rcb @ Rbiw) @ Roi
        t_oj = t_oi @ Rojw
        t_bj = t_oj @ Rbj
        Jbj = red @ hcat([t_oj, -((t_oj @ Rbj) @ skew(imu_j))])
        Jbi = red @ hcat([-(Rcb @ Rbiw), Rcb @ skew(Rbiw @ (w_i - Pbi))])
        Jex = red @ hcat([t_bj - Rcb, -((t_bj @ Rbc) @ skew(cam_j)) + skew(Rcb @ (imu_i - Pbc))])
        Joj = red @ hcat([-(t_oi @ Rojw), t_oi @ skew(Rojw @ (w_j - Poj))])
        Joi = red @ hcat([Rcb @ Rbiw, -(t_oi @ skew(obj_j))])
        T = t_bj @ Rbc
        Jl = (red @ (T @ pts_j)) / (lam * lam)                    # sic: +, and pts_j instead of pts_j_td
        out = hcat([r, flat(Jbj), flat(Jbi), flat(Jex), flat(Joj), flat(Joi), Jl])
    if parts:
        return out, dict(dep=float(dep.v), red=red.v, T=T.v, pts_j_td=pts_j_td.v)
    return out


# ---------------------------------------------------------------- numeric derivatives
def richardson(fun, x, plus, n, h):
    """Richardson extrapolation of central differences of fun(plus(x, d)) at steps h and h / 2: error O(h^4)"""
    def D(step):
        cols = []
        for c in range(n):
            d = np.zeros(n)
            d[c] = step
            fp = fun(plus(x, d))
            d[c] = -step
            cols.append((fp - fun(plus(x, d))) / (2.0 * step))
        return np.array(cols).T
    return (4.0 * D(h / 2.0) - D(h)) / 3.0
