"""Seeded edge cases for tests/test_objfactor_reference.py (CPU: they reach what they are named for) and tests/test_objfactor_reference_gpu.py (the device
against tests/objfactor_ref.py on the same cases).  Every case is a plain dict of numpy inputs; nothing here evaluates the code under test."""
import functools
import itertools

import numpy as np

from tests import factor_ref as fr, line_geometry_np as LG
from tests.factor_cases import QCASE_ROT, _qexp, _qmul, _rand_q, _rot_axis, _unit

SI = fr.SQRT_INFO
HALF_PI = np.pi / 2
EX_Q = np.array([0.5, -0.5, 0.5, -0.5])


def _pose(rng, scale=2.0):
    return np.concatenate([rng.normal(0, scale, 3), _rand_q(rng)])


def _ex(rng):
    return np.concatenate([rng.normal(0, 0.05, 3), _unit(EX_Q + rng.normal(0, 0.02, 4))])


# ---------------------------------------------------------------- line factor
def _orth_from_camera(n_c, v_c, pose, ex):
    """orthonormal parameters (world frame) of the line whose Pluecker coordinates in the camera frame are (n_c, v_c)"""
    lb = LG.plk_to_pose(np.concatenate([n_c, v_c]), fr.rot_of(ex[3:]), ex[:3])
    return LG.plk_to_orth(LG.plk_to_pose(lb, fr.rot_of(pose[3:]), pose[:3]))


def _line_case(name, seed, si=(SI, 0, 0, SI), phi=None, theta2=None, lratio=None, shift=0.0, ex_identity=False, qnorm=(1.0, 1.0), near_camera=False):
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-0.6, 0.6, 4)
    pose, ex = _pose(rng), _ex(rng)
    if ex_identity:
        ex = np.array([0, 0, 0, 0, 0, 0, 1.0])
    if shift:
        pose[:3] += shift * _unit(rng.normal(0, 1, 3))
    orth = np.array([rng.uniform(-3, 3), rng.uniform(-1.4, 1.4), rng.uniform(-3, 3), rng.uniform(0.1, 1.4)])
    if lratio is not None or near_camera:
        # in the camera frame: a line 5 m away whose plane through the optical centre has the normal (eps cos a, eps sin a, 1): the camera's z = 0 plane, perturbed
        eps, al = (lratio if lratio is not None else 2.0), rng.uniform(0, 2 * np.pi)
        nrm = _unit([eps * np.cos(al), eps * np.sin(al), 1.0])
        v_c = _unit(np.cross(nrm, rng.normal(0, 1, 3)))
        orth = _orth_from_camera(5.0 * nrm, v_c, pose, ex)
    if phi is not None:
        orth[3] = phi
    if theta2 is not None:
        orth[1] = theta2
    pose[3:] *= qnorm[0]
    ex[3:] *= qnorm[1]
    return dict(name=name, obs=obs, si=np.array(si, float), pose=pose, ex=ex, orth=orth, lratio=lratio, shift=shift, phi=phi, theta2=theta2, qnorm=qnorm,
                ex_identity=ex_identity)


@functools.lru_cache(maxsize=None)
def line_cases():
    out = [_line_case("benign0", 600), _line_case("benign_asym", 601, si=(310.0, -42.0, 17.5, 295.0)), _line_case("benign_zero_info", 602, si=(0, 0, 0, 0))]
    out += [_line_case(f"quadrant{k + 1}", 610 + k, phi=p) for k, p in enumerate((0.7, 2.4, -2.4, -0.7))]
    out += [_line_case("phi1e-3", 620, phi=1e-3), _line_case("phi1e-6", 621, phi=1e-6), _line_case("phi_half_pi-1e-3", 622, phi=HALF_PI - 1e-3),
            _line_case("phi_half_pi-1e-6", 623, phi=HALF_PI - 1e-6), _line_case("phi0", 624, phi=0.0)]
    out += [_line_case("theta2+", 630, theta2=HALF_PI - 1e-6), _line_case("theta2-", 631, theta2=-(HALF_PI - 1e-6))]
    out += [_line_case("l1e-3", 640, lratio=1e-3), _line_case("l1e-6", 641, lratio=1e-6)]
    out += [_line_case("far1e3", 650, shift=1e3, near_camera=True), _line_case("ex_identity", 651, ex_identity=True)]
    out += [_line_case("qnorm+-", 660, qnorm=(1 + 1e-3, 1 - 1e-3)), _line_case("qnorm-+", 661, qnorm=(1 - 1e-3, 1 + 1e-3))]
    return out


# ---------------------------------------------------------------- line_plus
def _plus_case(name, orth, delta, **kw):
    return dict(name=name, orth=np.array(orth, float), delta=np.array(delta, float), **kw)


@functools.lru_cache(maxsize=None)
def plus_cases():
    rng = np.random.default_rng(700)
    out = []
    for k in range(3):
        out.append(_plus_case(f"zero{k}", [rng.uniform(-3, 3), rng.uniform(-1.4, 1.4), rng.uniform(-3, 3), rng.uniform(-1.4, 1.4)], np.zeros(4), zero=True))
    for c in range(4):
        d = rng.normal(0, 0.05, 4)
        d[c] = 3.0 * (-1) ** c
        out.append(_plus_case(f"big{c}", [rng.uniform(-3, 3), rng.uniform(-1.4, 1.4), rng.uniform(-3, 3), rng.uniform(0.1, 1.4)], d, big=c))
    # theta_1 = 0 and delta_0 = 0: U Ry(b) = Rz(theta_3) Ry(theta_2 + b), so theta_2 + delta_1 is the new pitch before asin
    out += [_plus_case("euler_over+", [0.0, 1.2, 0.8, 0.5], [0, 0.6, 0, 0.02], pitch=1.8), _plus_case("euler_over-", [0.0, -1.2, -2.1, 0.9], [0, -0.6, 0, 0.02], pitch=-1.8)]
    for sg, side in itertools.product((1, -1), (1, -1)):
        tgt = sg * (HALF_PI + side * 1e-6)
        out.append(_plus_case(f"fold{'+' if sg > 0 else '-'}{'out' if side > 0 else 'in'}", [0.4, -0.3, 1.1, sg * 1.0], [0.01, -0.02, 0.03, tgt - sg * 1.0], phase=tgt))
    out += [_plus_case("past_fold+", [0.4, 0.3, -1.1, 1.0], [0.01, 0.02, 0.03, 1.5], phase=2.5), _plus_case("past_fold-", [-0.4, 0.3, 2.0, -1.0], [0.01, 0.02, 0.03, -1.5], phase=-2.5)]
    out.append(_plus_case("u1z_1-1e-12", [0.0, 1.0, 0.3, 0.6], [0, HALF_PI - np.sqrt(2e-12) - 1.0, 0, 0.01], u1z=1 - 1e-12))
    # theta_1 = theta_2 = 0: U Rz(c) has the yaw theta_3 + c; theta_2 = theta_3 = 0: U Rx(a) has the roll theta_1 + a
    out += [_plus_case("cut2+", [0.0, 0.0, 2.0, 0.5], [0, 0, np.pi - 5e-10 - 2.0, 0.01], cut=(2, np.pi)), _plus_case("cut2-", [0.0, 0.0, -2.0, 0.5], [0, 0, -(np.pi - 5e-10) + 2.0, 0.01], cut=(2, -np.pi)),
            _plus_case("cut0+", [2.0, 0.0, 0.0, 0.5], [np.pi - 5e-10 - 2.0, 0, 0, 0.01], cut=(0, np.pi))]
    return out


# ---------------------------------------------------------------- box_enclose
def _box_case(name, seed, local=None, e=None, dims=None, P=None, q=None, qnorm=1.0, p_w=None, **kw):
    """local: the point in the object frame; e: the reference's R_ojw (p_obj - P) instead (p_obj = P + R e)"""
    rng = np.random.default_rng(seed)
    dims = rng.uniform(1.0, 4.5, 3) if dims is None else np.array(dims, float)
    P = rng.normal(0, 5.0, 3) if P is None else np.array(P, float)
    q = _rand_q(rng) if q is None else np.array(q, float)
    R = fr.rot_of(q)
    if p_w is None:
        if e is not None:
            local = P + R @ np.array(e, float)
        p_w = P + R @ (np.array(local(dims) if callable(local) else local, float))
    return dict(name=name, p_w=np.array(p_w, float), dims=dims, pose_obj=np.concatenate([P, q * qnorm]), qnorm=qnorm, **kw)


@functools.lru_cache(maxsize=None)
def box_cases():
    out = [_box_case("inside", 800, local=lambda d: d * [0.3, -0.2, 0.1], outside=(0, 0, 0))]
    for ax in range(3):
        f = np.array([0.3, -0.2, 0.1])
        f[ax] = 0.8 * (-1) ** ax
        out.append(_box_case("out_" + "xyz"[ax], 801 + ax, local=lambda d, f=f: d * f, outside=tuple(int(a == ax) for a in range(3))))
    out.append(_box_case("out_xyz", 804, local=lambda d: d * [0.7, -0.9, 0.6], outside=(1, 1, 1)))
    for ax, side in itertools.product(range(3), (1, -1)):
        def loc(d, ax=ax, side=side):
            v = d * [0.3, -0.2, 0.1]
            v[ax] = (d[ax] / 2 + side * 1e-9) * (-1) ** ax
            return v
        out.append(_box_case(f"face_{'xyz'[ax]}{'+' if side > 0 else '-'}1e-9", 810 + 2 * ax + (side < 0), local=loc, face=(ax, side * 1e-9)))
    for k, sg in enumerate(itertools.product((1, -1), repeat=3)):
        out.append(_box_case("e" + "".join("+" if s > 0 else "-" for s in sg), 820 + k, e=np.array(sg) * [0.9, 1.3, 0.6], esign=sg))
    for ax in range(3):
        # nearly the identity rotation: p_obj = P + R e ~ P + e, with P_ax = -3 e_ax the signs of e and p_obj differ on that axis alone
        e = np.array([0.9, -1.3, 0.6])
        P = e * 2.0
        P[ax] = -3.0 * e[ax]
        out.append(_box_case("e_vs_p_" + "xyz"[ax], 830 + ax, e=e, P=P, q=_qexp(np.array([0.05, -0.04, 0.06])), differ=ax))
    for ax in range(3):
        p = np.array([1.0, -2.0, 0.7])
        p[ax] = 0.0
        out.append(_box_case("e0_" + "xyz"[ax], 840 + ax, p_w=p, P=np.zeros(3), q=[0, 0, 0, 1.0], dims=[1.5, 3.0, 2.0], nan_row=ax))
    out.append(_box_case("far1e3", 850, P=1e3 * _unit([0.6, -0.5, 0.62]), local=lambda d: [d[0] / 2 + 1e-3, -0.2 * d[1], 0.1 * d[2]], outside=(1, 0, 0)))
    out.append(_box_case("dims1e-3", 851, dims=[1e-3] * 3, local=lambda d: [0.3e-3, -1e-3, 0.0], outside=(0, 1, 0)))
    out.append(_box_case("dims1e3", 852, dims=[1e3] * 3, local=lambda d: [499.0, -501.0, 10.0], outside=(0, 1, 0)))
    out += [_box_case("qnorm+", 860, local=lambda d: d * [0.7, -0.2, 0.1], qnorm=1 + 1e-3), _box_case("qnorm-", 861, local=lambda d: d * [0.3, -0.2, 0.8], qnorm=1 - 1e-3)]
    return out


# ---------------------------------------------------------------- box_dims
@functools.lru_cache(maxsize=None)
def dims_cases():
    rng = np.random.default_rng(900)
    out = []
    d = rng.uniform(1.0, 4.5, 3)
    out.append(dict(name="equal", dims=d, box=d.copy(), diff=0.0))
    for mag in (1e-8, 0.3, 3.0, 1e3):
        d = rng.uniform(1.0, 4.5, 3)
        out.append(dict(name=f"diff{mag:g}", dims=d, box=d + mag * _unit(rng.normal(0, 1, 3)), diff=mag))
    d = 1e3 + rng.uniform(0, 1, 3)
    out.append(dict(name="cancel1e-6_at_1e3", dims=d, box=d + 1e-6, diff=1e-6 * np.sqrt(3)))
    return out


# ---------------------------------------------------------------- box_orientation
def _ori_case(name, seed, angle=None, Rdes=None, exact_identity=False, qnorm=(1.0, 1.0), both_signs=False, **kw):
    """the product R_oiw R_wbi R_bc R_cioi is Rdes (a turn by `angle` about a seeded axis unless given): R_cioi = (R_oiw R_wbi R_bc)^T Rdes"""
    rng = np.random.default_rng(seed)
    if exact_identity:
        I, q = np.eye(3).ravel(), np.array([0, 0, 0, 0, 0, 0, 1.0])
        return dict(name=name, R_cioi=I, R_bc=I.copy(), pose_body=q, pose_obj=q.copy(), angle=0.0, both_signs=False, qnorm=qnorm, **kw)
    body, obj = _pose(rng), _pose(rng, 5.0)
    R_bc = np.array([[0, 0, 1.0], [-1, 0, 0], [0, -1, 0]]) @ fr.rot_of(_qexp(rng.normal(0, 0.02, 3)))
    if Rdes is None:
        Rdes = fr.rot_of(_qexp(angle * _unit(rng.normal(0, 1, 3))))
    M = fr.rot_of(obj[3:]).T @ fr.rot_of(body[3:]) @ R_bc
    body[3:] *= qnorm[0]
    obj[3:] *= qnorm[1]
    return dict(name=name, R_cioi=(M.T @ Rdes).ravel(), R_bc=R_bc.ravel(), pose_body=body, pose_obj=obj, angle=angle, both_signs=both_signs, qnorm=qnorm, **kw)


@functools.lru_cache(maxsize=None)
def ori_cases():
    out = [_ori_case("angle0", 1000, exact_identity=True, branch="taylor")]
    out += [_ori_case("angle1e-12", 1001, angle=1e-12, branch="taylor"), _ori_case("angle1e-9", 1002, angle=1e-9, branch="atan")]
    out += [_ori_case(f"angle{a:g}", 1003 + k, angle=a, branch="atan") for k, a in enumerate((1e-6, 1e-3, 1.0, 3.0))]
    out += [_ori_case("pi-1e-3", 1010, angle=np.pi - 1e-3, branch="atan"), _ori_case("pi-1e-6", 1011, angle=np.pi - 1e-6, branch="atan", both_signs=True),
            _ori_case("pi_w_branch", 1012, angle=np.pi, branch="pi", both_signs=True)]
    for k, (nm, axis, qc) in enumerate(QCASE_ROT):
        Rdes = _rot_axis(axis, 179.0) if axis is not None else fr.rot_of(_qexp(np.array([0.02, -0.01, 0.015])))
        out.append(_ori_case("qfromR_" + nm, 1020 + k, Rdes=Rdes, qcase=qc))
    out.append(_ori_case("w_negative", 1030, Rdes=_rot_axis(0, -179.0), qcase=1, wneg=True))
    out += [_ori_case("qnorm+-", 1040, angle=0.8, qnorm=(1 + 1e-3, 1 - 1e-3)), _ori_case("qnorm-+", 1041, angle=2.2, qnorm=(1 - 1e-3, 1 + 1e-3))]
    return out


# ---------------------------------------------------------------- instance projection factor
def _inst_case(name, seed, lam=None, td_gap=0.003, front=None, same_obj=False, same_body=False, ex_identity=False, qnorm=None, shift=0.0):
    """the point is lifted from camera j, the object is placed around it, moved to its pose at i, and the observation in i is the reprojection plus noise;
    front: body i is moved so that the point lands `front` metres in front of camera i"""
    rng = np.random.default_rng(seed)
    ex = np.array([0, 0, 0, 0, 0, 0, 1.0]) if ex_identity else np.concatenate([rng.normal(0, 0.05, 3), _unit(EX_Q + rng.normal(0, 0.01, 4))])
    bj = np.concatenate([rng.normal(0, 0.5, 3), _qexp(rng.normal(0, 0.1, 3))])
    bi = bj.copy() if same_body else np.concatenate([bj[:3] + rng.normal(0, 0.3, 3), _qmul(bj[3:], _qexp(rng.normal(0, 0.1, 3)))])
    lam = 1.0 / rng.uniform(5.0, 10.0) if lam is None else lam
    f = dict(pts_j=np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), 1.0]), vel_j=rng.normal(0, 0.1, 2), vel_i=rng.normal(0, 0.1, 2))
    cur_td = 0.004
    f["cur_td"], f["td_j"], f["td_i"] = cur_td, cur_td - td_gap, cur_td - (td_gap * 0.5 if td_gap else 0.0)
    R = fr.rot_of
    pj_td = f["pts_j"] - (cur_td - f["td_j"]) * np.append(f["vel_j"], 0.0)
    w_j = R(bj[3:]) @ (R(ex[3:]) @ (pj_td / lam) + ex[:3]) + bj[:3]
    qoj = _qexp(rng.normal(0, 0.3, 3))
    local = rng.normal(0, 0.7, 3)
    oj = np.concatenate([w_j - R(qoj) @ local, qoj])
    oi = oj.copy() if same_obj else np.concatenate([oj[:3] + rng.normal(0, 0.4, 3), _qmul(qoj, _qexp(rng.normal(0, 0.2, 3)))])
    w_i = R(oi[3:]) @ local + oi[:3]
    if front is not None:
        imu_i = R(ex[3:]) @ np.array([0.2 * front, -0.1 * front, front]) + ex[:3]
        bi[:3] = w_i - R(bi[3:]) @ imu_i
    cam_i = R(ex[3:]).T @ (R(bi[3:]).T @ (w_i - bi[:3]) - ex[:3])
    f["pts_i"] = np.array([cam_i[0] / cam_i[2], cam_i[1] / cam_i[2], 1.0]) + np.append(rng.normal(0, 2e-3, 2) + (cur_td - f["td_i"]) * f["vel_i"], 0.0)
    blocks = [bj, bi, ex, oj, oi]
    if shift:
        t = shift * _unit(rng.normal(0, 1, 3))
        for b in (bj, bi, oj, oi):
            b[:3] += t
    if qnorm is not None:
        for b, s in zip(blocks, qnorm):
            b[3:] *= s
    return dict(name=name, f=f, pbj=bj, pbi=bi, pex=ex, poj=oj, poi=oi, lam=float(lam), td_gap=td_gap, front=front, same_obj=same_obj, same_body=same_body,
                shift=shift, qnorm=qnorm)


@functools.lru_cache(maxsize=None)
def inst_cases():
    out = [_inst_case(f"benign{k}", 1100 + k) for k in range(3)]
    out.append(_inst_case("front1e-3", 1110, front=1e-3))
    out += [_inst_case(f"depth{d:g}", 1120 + k, lam=1.0 / d) for k, d in enumerate((0.2, 1.0, 10.0, 200.0))]
    out += [_inst_case("td0", 1130, td_gap=0.0), _inst_case("td0.05", 1131, td_gap=0.05)]
    out += [_inst_case("same_obj", 1140, same_obj=True), _inst_case("same_body", 1141, same_body=True), _inst_case("ex_identity", 1142, ex_identity=True)]
    out += [_inst_case("qnorm+-", 1150, qnorm=(1 + 1e-3, 1 - 1e-3, 1 + 1e-3, 1 - 1e-3, 1 + 1e-3)), _inst_case("qnorm-+", 1151, qnorm=(1 - 1e-3, 1 + 1e-3, 1 - 1e-3, 1 + 1e-3, 1 - 1e-3))]
    out.append(_inst_case("shift1e3", 1160, shift=1e3))
    return out


def inst_arrays(cases):
    """(factor records, five pose arrays and the inverse depths) for backend.inst_proj_eval"""
    from dynamic_vins_amd.backend import INSTPROJ_DTYPE
    fac = np.zeros(len(cases), INSTPROJ_DTYPE)
    for k, c in enumerate(cases):
        for key in ("pts_j", "pts_i", "vel_j", "vel_i", "td_j", "td_i", "cur_td"):
            fac[key][k] = c["f"][key]
    return fac, [np.array([c[b] for c in cases]) for b in ("pbj", "pbi", "pex", "poj", "poi")] + [np.array([c["lam"] for c in cases])]
