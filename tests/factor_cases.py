"""Seeded edge cases for tests/test_factor_reference.py (CPU: they reach what they are named for) and tests/test_factor_reference_gpu.py (the device
against tests/factor_ref.py on the same cases).  Every case is a plain dict of numpy inputs; nothing here evaluates the code under test."""
import functools
import itertools

import numpy as np

from dynamic_vins_amd.backend import FACTOR_DTYPE, IMU_DTYPE, LM_DTYPE
from tests import factor_ref as fr

G_NORM = 9.81
FOCAL = 460.0


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def _qexp(w):
    """x y z w of the rotation vector w"""
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(th / 2) * np.asarray(w) / th, [np.cos(th / 2)]])


def _qmul(a, b):
    return fr.qmul(fr.A(a), fr.A(b)).v


def _rand_q(rng):
    return _unit(rng.normal(0, 1, 4))


# ---------------------------------------------------------------- IMU factor
def _imu_case(name, seed, sum_dt=0.1, dba=1e-3, dbg=1e-3, signs=(1, 1, 1), near_pi=False, cond=None):
    rng = np.random.default_rng(seed)
    dt = sum_dt
    lin_ba, lin_bg = rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)
    dq = _qexp(rng.normal(0, 0.3, 3) * min(dt, 1.0))
    dp, dv = rng.normal(0, 0.5, 3) * dt * dt + rng.normal(0, 0.3, 3) * dt, rng.normal(0, 1.0, 3) * dt
    jac = np.eye(15)
    jac[0:3, 9:12] = -0.5 * dt * dt * np.eye(3) + rng.normal(0, 0.05, (3, 3)) * dt * dt
    jac[0:3, 12:15] = rng.normal(0, 0.2, (3, 3)) * dt ** 3
    jac[3:6, 12:15] = -dt * np.eye(3) + rng.normal(0, 0.05, (3, 3)) * dt
    jac[6:9, 9:12] = -dt * np.eye(3) + rng.normal(0, 0.05, (3, 3)) * dt
    jac[6:9, 12:15] = rng.normal(0, 0.3, (3, 3)) * dt * dt
    Q, _ = np.linalg.qr(rng.normal(0, 1, (15, 15)))
    ev = np.logspace(-8, -3, 15) if cond is None else np.logspace(-3 - np.log10(cond), -3, 15)
    cov = (Q * ev) @ Q.T
    cov = 0.5 * (cov + cov.T)
    Qi = _rand_q(rng)
    Pi, Vi = rng.normal(0, 3, 3), rng.normal(0, 1, 3)
    Ri = fr.rot_of(Qi)
    Gv = np.array([0, 0, G_NORM])
    Pj = Pi + Vi * dt - 0.5 * Gv * dt * dt + Ri @ dp + rng.normal(0, 0.01, 3)
    Vj = Vi - Gv * dt + Ri @ dv + rng.normal(0, 0.01, 3)
    rel = _qexp(_unit(rng.normal(0, 1, 3)) * (np.pi - 5e-4)) if near_pi else _qexp(rng.normal(0, 0.01, 3))
    Qj = _qmul(_qmul(Qi, dq), rel)
    # the signs of the three quaternions' w: the factor has no sign fix, the residual flips with them
    Qi, Qj, dq = [q * (s if q[3] >= 0 else -s) for q, s in zip((Qi, Qj, dq), signs)]
    sb_i = np.concatenate([Vi, lin_ba + (_unit(rng.normal(0, 1, 3)) * dba if dba else 0.0), lin_bg + (_unit(rng.normal(0, 1, 3)) * dbg if dbg else 0.0)])
    sb_j = np.concatenate([Vj, sb_i[3:] + rng.normal(0, 1e-3, 6)])
    rec = np.zeros(1, IMU_DTYPE)
    rec["sum_dt"], rec["dp"], rec["dv"], rec["lin_ba"], rec["lin_bg"] = dt, dp, dv, lin_ba, lin_bg
    rec["dq"] = [dq[3], dq[0], dq[1], dq[2]]
    rec["jacobian"], rec["covariance"] = jac.reshape(-1), cov.reshape(-1)
    rec["fi"], rec["fj"] = 0, 1
    return dict(name=name, rec=rec, pre=fr.pre_from_record(rec[0]), pose_i=np.concatenate([Pi, Qi]), sb_i=sb_i, pose_j=np.concatenate([Pj, Qj]), sb_j=sb_j,
                signs=signs, near_pi=near_pi, dba=dba, dbg=dbg, cond=cond)


@functools.lru_cache(maxsize=None)
def imu_cases():
    out = [_imu_case(f"benign{k}", 100 + k) for k in range(3)]
    for k, sg in enumerate(itertools.product((1, -1), repeat=3)):
        out.append(_imu_case("sign" + "".join("+" if s > 0 else "-" for s in sg), 110 + k, signs=sg))
    out += [_imu_case("near_pi", 120, near_pi=True), _imu_case("near_pi_neg", 121, near_pi=True, signs=(-1, 1, -1)),
            _imu_case("dt0.005", 122, sum_dt=0.005), _imu_case("dt10", 123, sum_dt=10.0)]
    for k, (a, g) in enumerate(itertools.product((0.0, 1e-3, 0.3), repeat=2)):
        out.append(_imu_case(f"dba{a:g}_dbg{g:g}", 130 + k, dba=a, dbg=g))
    out.append(_imu_case("cond1e9", 140, cond=1e9))
    return out


# ---------------------------------------------------------------- projection factors
def _proj_case(name, seed, kind, lam=None, td_gap=0.01, same_pose=False, front=None):
    rng = np.random.default_rng(seed)
    f = np.zeros(1, FACTOR_DTYPE)[0]
    f["kind"] = kind
    f["pix"], f["piy"] = rng.uniform(-0.5, 0.5, 2)
    f["vix"], f["viy"], f["vjx"], f["vjy"] = rng.normal(0, 0.2, 4)
    td = rng.normal(0, 0.01)
    f["td_i"], f["td_j"] = td - td_gap, td - td_gap * 0.5 + (rng.normal(0, 0.003) if td_gap else 0.0)
    lam = rng.uniform(0.05, 0.8) if lam is None else lam
    pose_i = np.concatenate([rng.normal(0, 2, 3), _rand_q(rng)])
    pose_j = pose_i.copy()
    if not same_pose:
        pose_j[:3] += rng.normal(0, 0.3, 3)
        pose_j[3:] = _qmul(pose_i[3:], _qexp(rng.normal(0, 0.05, 3)))
    ex0 = np.concatenate([rng.normal(0, 0.05, 3), _unit(np.array([0.5, -0.5, 0.5, -0.5]) + rng.normal(0, 0.01, 4))])
    ex1 = np.concatenate([ex0[:3] + [0, -0.12, 0] + rng.normal(0, 0.003, 3), _unit(ex0[3:] + rng.normal(0, 0.003, 4))])
    if kind == 2:
        pose_j = pose_i.copy()
    # where the point falls in camera j with a perfect observation
    pts_i_td = np.array([f["pix"], f["piy"], 1.0]) - td_gap * np.array([f["vix"], f["viy"], 0.0])
    Ri, Rj, ric = fr.rot_of(pose_i[3:]), fr.rot_of(pose_j[3:]), fr.rot_of(ex0[3:])
    exj = ex0 if kind == 0 else ex1
    rcj = fr.rot_of(exj[3:])
    p_imu_i = ric @ (pts_i_td / lam) + ex0[:3]
    if front is not None:          # the point lands `front` metres in front of camera j: move frame j (kinds 0, 1) or camera 1 (kind 2) there
        target = np.array([0.2 * front, -0.1 * front, front])
        if kind == 2:
            ex1[:3] = p_imu_i - rcj @ target
        else:
            pose_j[:3] = Ri @ p_imu_i + pose_i[:3] - Rj @ (rcj @ target + exj[:3])
    p_imu_j = p_imu_i if kind == 2 else Rj.T @ (Ri @ p_imu_i + pose_i[:3] - pose_j[:3])
    pcj = rcj.T @ (p_imu_j - (ex0 if kind == 0 else ex1)[:3])
    vj = np.array([f["vjx"], f["vjy"]])
    obs = pcj[:2] / pcj[2] + (td - f["td_j"]) * vj + rng.normal(0, 2e-3, 2)
    f["pjx"], f["pjy"] = obs
    return dict(name=name, f=f, pose_i=pose_i, pose_j=pose_j, ex0=ex0, ex1=ex1, lam=float(lam), td=float(td), kind=kind, td_gap=td_gap, front=front, pcj_z=float(pcj[2]))


@functools.lru_cache(maxsize=None)
def proj_cases():
    out = []
    for kind in range(3):
        out += [_proj_case(f"k{kind}_benign{s}", 200 + 10 * kind + s, kind) for s in range(3)]
        out += [_proj_case(f"k{kind}_depth{1 / lam:g}", 240 + 10 * kind + n, kind, lam=lam) for n, lam in enumerate((5.0, 1.0, 0.1, 0.005))]
        out.append(_proj_case(f"k{kind}_front1e-3", 280 + kind, kind, front=1e-3))
        out += [_proj_case(f"k{kind}_td0", 290 + kind, kind, td_gap=0.0), _proj_case(f"k{kind}_td0.05", 300 + kind, kind, td_gap=0.05)]
    out += [_proj_case(f"k{kind}_same_pose", 310 + kind, kind, same_pose=True) for kind in (0, 1)]
    return out


# ---------------------------------------------------------------- gauge fix
def _rot_axis(axis, deg):
    w = np.zeros(3)
    w[axis] = np.deg2rad(deg)
    return fr.rot_of(_qexp(w))


QCASE_ROT = [("small", None, 0), ("x179", 0, 1), ("y179", 1, 2), ("z179", 2, 3)]      # name, axis of a 179 degree turn, the case of qfromR it must reach


def _gauge_case(name, seed, pitch00=3.0, pitch0=2.0, nframes=11, use_imu=1, nlm=1, norm_dev=0.0, branches=True):
    """a solved window whose frame 0 has pitch `pitch00` (degrees), a pre-solve frame 0 with pitch `pitch0`; with `branches`, frames 1..4 (those below nframes) are
    turned so that the EXPECTED rotation after the fix is 179 degrees about x, y, z and a small angle: one frame per case of the matrix -> quaternion conversion"""
    rng = np.random.default_rng(seed)
    pose, sb = np.zeros((11, 7)), rng.normal(0, 1, (11, 9))
    pose[:, :3] = np.cumsum(rng.normal(0, 0.5, (11, 3)), axis=0) + rng.normal(0, 5, 3)
    R00 = fr.ypr2r([rng.uniform(-170, 170), pitch00, rng.uniform(-20, 20)])
    R0 = fr.ypr2r([rng.uniform(-170, 170), pitch0, rng.uniform(-20, 20)])
    ypr0 = fr.r2ypr(R0)
    P0 = rng.normal(0, 5, 3)
    pose[0, 3:] = fr.quat_of(R00)
    for i in range(1, 11):
        pose[i, 3:] = _qmul(pose[i - 1, 3:], _qexp(rng.normal(0, 0.05, 3)))
    want = {}
    if branches:
        probe = fr.gauge_fix(dict(pose=pose, sb=sb), R0, ypr0, P0, use_imu, 1)
        rot = probe["R"][0] @ fr.rot_of(pose[0, 3:]).T          # the fix's rotation (frame 0 is normalised here)
        for k, (_, axis, qc) in enumerate(QCASE_ROT):
            i = 1 + (k + 1) % 4          # frames 2, 3, 4, 1
            if i >= nframes:
                continue
            Rdes = _rot_axis(axis, 179.0) if axis is not None else fr.rot_of(_qexp(rng.normal(0, 0.02, 3)))
            pose[i, 3:] = fr.quat_of(rot.T @ Rdes)
            want[i] = qc
    if norm_dev:
        pose[:, 3:] *= (1.0 + norm_dev * np.where(np.arange(11) % 2 == 0, 1.0, -1.0))[:, None]
    pose[:, 3:] *= np.where(rng.random(11) < 0.5, -1.0, 1.0)[:, None]          # either sign of the input quaternion
    lam = rng.uniform(0.01, 2.0, nlm)
    return dict(name=name, pose=pose, sb=sb, lam=lam, nframes=nframes, use_imu=use_imu, R0=R0, ypr0=ypr0, P0=P0, want_qcase=want,
                want_singular=bool(use_imu and (abs(abs(pitch00) - 90) < 1 or abs(abs(pitch0) - 90) < 1)))


@functools.lru_cache(maxsize=None)
def gauge_cases():
    out = [_gauge_case("small", 400)]
    k = 0
    for p in (89.5, -89.5, 88.9, -88.9):
        for where in ("solved", "before", "both"):
            k += 1
            out.append(_gauge_case(f"{where}{p:+g}", 400 + k, pitch00=p if where != "before" else 5.0, pitch0=p if where != "solved" else -4.0))
    out += [_gauge_case(f"nf{nf}_imu{ui}", 420 + 2 * nf + ui, nframes=nf, use_imu=ui) for nf in (1, 2, 11) for ui in (0, 1)]
    out += [_gauge_case("nf2_singular", 450, nframes=2, pitch00=89.5), _gauge_case("noimu_pitch89.5", 451, use_imu=0, pitch00=89.5)]
    out += [_gauge_case("norm+-1e-3", 460, norm_dev=1e-3), _gauge_case("norm+-1e-3_singular", 461, norm_dev=1e-3, pitch0=-89.5),
            _gauge_case("norm+-1e-3_noimu", 462, norm_dev=1e-3, use_imu=0)]
    out += [_gauge_case(f"nlm{n}", 470 + k, nlm=n) for k, n in enumerate((0, 1, 1000))]
    return out


# ---------------------------------------------------------------- outlier test
def _reject_case(name, seed, nlm, counts, ex_from_state, nframes=11):
    """landmarks whose mean reprojection error is SET: the observations are the exact projections at the given states plus offsets whose lengths average to the
    target.  Targets: 1e-6 px on either side of the 3 px bar for most, a few far from it."""
    rng = np.random.default_rng(seed)
    pose = np.zeros((11, 7))
    pose[:, :3] = np.cumsum(rng.normal(0, 0.15, (11, 3)), axis=0)
    q = _rand_q(rng)
    for i in range(11):
        q = _qmul(q, _qexp(rng.normal(0, 0.03, 3)))
        pose[i, 3:] = q * (1.0 + (1e-3 if i % 3 == 0 else -1e-3 if i % 3 == 1 else 0.0)) * (-1.0 if i % 4 == 0 else 1.0)
    base = np.array([0.5, -0.5, 0.5, -0.5])

    def extr():
        t0 = rng.normal(0, 0.05, 3)
        q0 = _unit(base + rng.normal(0, 0.02, 4))
        return np.array([np.concatenate([t0, q0]), np.concatenate([t0 + [0, -0.12, 0] + rng.normal(0, 0.005, 3), _unit(q0 + rng.normal(0, 0.005, 4))])])
    ex_arg, ex_state = extr(), extr()
    ex_state[:, 3:] *= 1.0 + 1e-3          # para_ex_pose is normalised by the reader, not by the solver
    ric = np.array([fr.rot_of(e[3:]) for e in ex_arg])
    tic = ex_arg[:, :3].copy()
    act = ex_state if ex_from_state else ex_arg
    ric_a = np.array([fr.rot_of(e[3:] / np.linalg.norm(e[3:])) for e in act])
    tic_a = act[:, :3]
    Rs = [fr.rot_of(p[3:] / np.linalg.norm(p[3:])) for p in pose]
    lms, facs = np.zeros(nlm, LM_DTYPE), []
    lam = rng.uniform(0.05, 0.5, nlm)
    targets = np.zeros(nlm)
    for l in range(nlm):
        cnt = counts[l % len(counts)]
        a = int(rng.integers(0, nframes))
        pt = rng.uniform(-0.4, 0.4, 2)
        sel = l % 5
        targets[l] = (3.0 + 1e-6, 3.0 - 1e-6, 3.0 + 1e-6, 3.0 - 1e-6, (0.4, 11.0)[(l // 5) % 2])[sel]
        w = rng.uniform(0.5, 1.5, cnt)
        w *= cnt / w.sum()
        lms[l] = (len(facs), cnt, a, 0)
        for k in range(cnt):
            j = (a + (k + 1) // 2) % nframes if cnt > 1 else (a + 1 + int(rng.integers(0, max(nframes - 1, 1)))) % nframes
            kind = (k % 2) if j != a else 2 * (k % 2)          # left block kind 0, right block kind 1 (kind 2 in the anchor frame itself)
            if cnt == 1:
                kind = l % 3
                j = a if kind == 2 else j
            f = np.zeros(1, FACTOR_DTYPE)[0]
            f["kind"], f["lm"], f["fi"], f["fj"] = kind, l, a, j
            f["pix"], f["piy"] = pt
            cam = 0 if kind == 0 else 1
            pw = Rs[a] @ (ric_a[0] @ (np.array([pt[0], pt[1], 1.0]) / lam[l]) + tic_a[0]) + pose[a, :3]
            pc = ric_a[cam].T @ (Rs[j].T @ (pw - pose[j, :3]) - tic_a[cam])
            ang = rng.uniform(0, 2 * np.pi)
            e = targets[l] * w[k] / FOCAL
            f["pjx"], f["pjy"] = pc[0] / pc[2] + e * np.cos(ang), pc[1] / pc[2] + e * np.sin(ang)
            facs.append(f)
    return dict(name=name, pose=pose, ex_state=ex_state, ric=ric, tic=tic, lam=lam, factors=np.array(facs, FACTOR_DTYPE), landmarks=lms, nframes=nframes,
                ex_from_state=ex_from_state, targets=targets)


@functools.lru_cache(maxsize=None)
def reject_cases():
    out = []
    for k, nlm in enumerate((1, 7, 8, 9)):
        for xs in (0, 1):
            out.append(_reject_case(f"nlm{nlm}_ex{xs}", 500 + 2 * k + xs, nlm, (1, 22, 22, 1, 5, 22, 1, 22, 3), xs))
    out += [_reject_case("nlm1_count22", 520, 1, (22,), 0), _reject_case("nlm9_count1", 521, 9, (1,), 1), _reject_case("nlm9_count22", 522, 9, (22,), 0),
            _reject_case("nlm1000", 523, 1000, (1, 22, 4, 9, 22, 1, 13), 1)]
    return out
