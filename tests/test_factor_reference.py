"""CPU validation of tests/factor_ref.py, the float64 restatement tests/test_factor_reference_gpu.py holds the HIP factors, the gauge fix and the outlier
test against.  No GPU, and (apart from (b)) no code of the project: the reference against its own derivatives and invariants.
  (a) the closed-form Jacobians equal Richardson-extrapolated central differences on the manifold over the whole case list of tests/factor_cases.py, wherever
      the closed form is the derivative; where it knowingly is not (d r_q / d b_g and d r_q / d theta_i of the IMU factor once b_g has left its linearisation
      point, quirk Q7 of the one-frame projection factor) the gap is zero at the point of agreement and has the slope the algebra predicts.
      NUM_TOL below is the measured Richardson error of the reference against its own closed form (a property of the reference, never applied to the device).
  (b) the restatement equals the CPU oracle's entries (dvo_imu_eval, dvo_proj_eval) within K eps of the magnitude accumulation: two independent float64
      evaluations, whose largest ratio over the case list sets K_IMU / K_PROJ of the GPU module (10 times that ratio).
  (c) gauge_fix invariants and reject_flags sanity.
  (d) every edge case reaches what it is named for (signs, angles, condition numbers, the singular branch, the four cases of the matrix -> quaternion
      conversion, the landmark-count tails and the 3 px bar).
Measured here: closed form vs Richardson, max |dJ| / (1 + max |J|): IMU 8.9e-13 (dba0.001_dbg0), projection 1.4e-9 (k0_front1e-3: a point 1 mm in front of
the camera, J ~ 1e8, step scaled with the depth); restatement vs oracle, in eps of the magnitude: IMU r 2.5e-5 (near_pi_neg), J 0.027 (benign1), projection
0.23 (k2_depth10).  The ratios are far below 1 because the magnitude adds up every operand of every operation, and for the IMU factor because it includes
what the inverse of the covariance (cond 1e5, 1e9 in cond1e9) can lose: with |U| alone the same ratios are 1e3 / 1e5 (4e5 / 5e7 in cond1e9)."""
import numpy as np
import pytest

from tests import ba_ref, factor_cases as fc, factor_ref as fr

NUM_TOL = 2e-8                # (a) |numeric - closed| <= NUM_TOL (1 + max |J|): ten times the largest Richardson error measured over the case list (1.4e-9), rounded up
K_IMU, K_PROJ = 0.3, 2.5      # (b) -> the GPU module's bars: ten times the largest reference-vs-oracle ratio measured over the case list (0.027, 0.23), rounded up
ORACLE_SHARE = 0.5            # what (b) itself asserts: the oracle stays within half of the bar the device is held to (measured: a tenth)

IMU = fc.imu_cases()
PROJ = fc.proj_cases()
GAUGE = fc.gauge_cases()
REJECT = fc.reject_cases()


def _ids(cases):
    return [c["name"] for c in cases]


def _ratio(dev, ref):
    """max |dev - ref.v| / (eps ref.m); an entry without magnitude is structurally zero and must be exactly 0"""
    err = np.abs(np.asarray(dev) - ref.v)
    if np.any(err[ref.m == 0] != 0):
        return np.inf
    nz = ref.m > 0
    return float((err[nz] / (fr.EPS * ref.m[nz])).max()) if nz.any() else 0.0


# ---------------------------------------------------------------- (a) closed forms vs numeric derivatives
@pytest.mark.parametrize("c", IMU, ids=_ids(IMU))
def test_imu_closed_form_is_the_derivative(c):
    Jc = fr.imu_raw(c["pre"], fc.G_NORM, c["pose_i"], c["sb_i"], c["pose_j"], c["sb_j"])[1].v.copy()
    Jn = fr.imu_numeric(c["pre"], fc.G_NORM, c["pose_i"], c["sb_i"], c["pose_j"], c["sb_j"])
    Jc[3:6, 3:6] /= fr.imu_cq_norm2(c["pre"], c["sb_i"])          # the closed form is |cq|^2 times the derivative (factor_ref docstring); 1 at dbg = 0
    mask = np.ones((15, 30), bool)
    if c["dbg"] != 0:
        mask[3:6, 12:15] = False                                   # d r_q / d b_g is written with delta_q: test_imu_gyro_bias_gap_is_first_order
    err = np.abs(Jn - Jc)[mask].max() / (1.0 + np.abs(Jc).max())
    print(f"\n[num] imu {c['name']} {err:.3g}")
    assert err <= NUM_TOL


def test_imu_gyro_bias_gap_is_first_order():
    """d r_q / d b_g: exact at dbg = 0, and the gap to the derivative grows linearly with |dbg| (slope 1 in log-log, two decades)"""
    c = fc._imu_case("slope", 150, dbg=0.0)
    d = np.array([0.6, -0.48, 0.64])
    gaps = []
    for s in (0.0, 1e-4, 1e-3, 1e-2):
        sb_i = c["sb_i"].copy()
        sb_i[6:9] = c["pre"]["lin_bg"] + s * d
        Jc = fr.imu_raw(c["pre"], fc.G_NORM, c["pose_i"], sb_i, c["pose_j"], c["sb_j"])[1].v
        Jn = fr.imu_numeric(c["pre"], fc.G_NORM, c["pose_i"], sb_i, c["pose_j"], c["sb_j"])
        gaps.append(np.abs(Jn - Jc)[3:6, 12:15].max())
    print(f"\n[slope] imu dbg gaps {gaps}")
    assert gaps[0] <= NUM_TOL
    for a, b in ((1, 2), (2, 3)):
        assert 0.95 <= np.log10(gaps[b] / gaps[a]) <= 1.05, gaps


@pytest.mark.parametrize("c", PROJ, ids=_ids(PROJ))
def test_projection_closed_form_is_the_derivative(c):
    _, Jc = fr.proj_factor(c["f"], c["pose_i"], c["pose_j"], c["ex0"], c["ex1"], c["lam"], c["td"])
    Jn = fr.proj_numeric(c["f"], c["pose_i"], c["pose_j"], c["ex0"], c["ex1"], c["lam"], c["td"], h=1e-4 * min(1.0, abs(Jc["dep"].v) * 3))
    worst = 0.0
    for k in fr.PROJ_KEYS:
        if k == "Jl" and c["kind"] == 2 and c["td_gap"] != 0:
            continue                                               # Q7: test_q7_gap_is_linear_in_the_td_shift
        scale = 1.0 + max(np.abs(Jc[q].v).max() for q in fr.PROJ_KEYS)
        worst = max(worst, np.abs(Jn[k] - Jc[k].v).max() / scale)
    print(f"\n[num] proj {c['name']} {worst:.3g}")
    assert worst <= NUM_TOL


def test_q7_gap_is_linear_in_the_td_shift():
    """kind 2 writes d r / d lambda with pts_i: exact at td = td_i, and the gap is linear in td - td_i (it is reduce T velocity_i (td - td_i) / lambda^2)"""
    gaps = []
    for g in (0.0, 1e-3, 1e-2, 5e-2):
        c = fc._proj_case("q7", 330, 2, td_gap=g)
        _, Jc = fr.proj_factor(c["f"], c["pose_i"], c["pose_j"], c["ex0"], c["ex1"], c["lam"], c["td"])
        Jn = fr.proj_numeric(c["f"], c["pose_i"], c["pose_j"], c["ex0"], c["ex1"], c["lam"], c["td"])
        gaps.append(np.abs(Jn["Jl"] - Jc["Jl"].v).max())
        scale = 1.0 + np.abs(Jc["Jl"].v).max()
    print(f"\n[slope] Q7 gaps {gaps}")
    assert gaps[0] <= NUM_TOL * scale
    assert 0.95 <= np.log10(gaps[2] / gaps[1]) <= 1.05 and 0.95 <= np.log(gaps[3] / gaps[2]) / np.log(5.0) <= 1.05, gaps


# ---------------------------------------------------------------- (b) the restatement vs the oracle's entries
def _oracle_imu(lib, c):
    rec = c["rec"][0]
    z, noise = np.zeros(3), np.zeros(4)
    lin_ba, lin_bg = np.ascontiguousarray(rec["lin_ba"], np.float64), np.ascontiguousarray(rec["lin_bg"], np.float64)
    h = lib.dvo_preint_create(z.ctypes.data, z.ctypes.data, lin_ba.ctypes.data, lin_bg.ctypes.data, noise.ctypes.data)
    try:
        dq = rec["dq"]
        dq_xyzw = np.array([dq[1], dq[2], dq[3], dq[0]])
        dp, dv = np.ascontiguousarray(rec["dp"], np.float64), np.ascontiguousarray(rec["dv"], np.float64)
        jac, cov = np.ascontiguousarray(rec["jacobian"], np.float64), np.ascontiguousarray(rec["covariance"], np.float64)
        lib.dvo_preint_set(h, float(rec["sum_dt"]), dp.ctypes.data, dq_xyzw.ctypes.data, dv.ctypes.data, jac.ctypes.data, cov.ctypes.data)
        r, J = ba_ref._eval(lib.dvo_imu_eval, (h, float(fc.G_NORM)), [c["pose_i"], c["sb_i"], c["pose_j"], c["sb_j"]], 15)
    finally:
        lib.dvo_preint_destroy(h)
    return r, np.hstack([J[0][:, :6], J[1], J[2][:, :6], J[3]])


def _oracle_proj(lib, c):
    f, kind = c["f"], c["kind"]
    obs = np.array([f["pix"], f["piy"], 1.0, f["pjx"], f["pjy"], 1.0, f["vix"], f["viy"], f["vjx"], f["vjy"], f["td_i"], f["td_j"]])
    lk, tk = np.array([c["lam"]]), np.array([c["td"]])
    blocks = {0: [c["pose_i"], c["pose_j"], c["ex0"], lk, tk], 1: [c["pose_i"], c["pose_j"], c["ex0"], c["ex1"], lk, tk], 2: [c["ex0"], c["ex1"], lk, tk]}[kind]
    r, J = ba_ref._eval(lib.dvo_proj_eval, (kind, obs.ctypes.data), blocks, 2)
    J = [j[:, :6] if j.shape[1] == 7 else j[:, 0] for j in J]
    z = np.zeros((2, 6))
    parts = [J[0], J[1], J[2], z, J[3], J[4]] if kind == 0 else J if kind == 1 else [z, z, J[0], J[1], J[2], J[3]]
    return np.concatenate([r] + [np.asarray(p).reshape(-1) for p in parts])


@pytest.mark.parametrize("c", IMU, ids=_ids(IMU))
def test_imu_restatement_equals_the_oracle(oracle, c):
    lib = ba_ref._bind(oracle)
    ro, Jo = _oracle_imu(lib, c)
    r, J = fr.imu_factor(c["pre"], fc.G_NORM, c["pose_i"], c["sb_i"], c["pose_j"], c["sb_j"])
    rr, rj = _ratio(ro, r), _ratio(Jo, J)
    print(f"\n[oracle] imu {c['name']} r {rr:.3g} J {rj:.3g}")
    assert rr <= ORACLE_SHARE * K_IMU and rj <= ORACLE_SHARE * K_IMU


@pytest.mark.parametrize("c", PROJ, ids=_ids(PROJ))
def test_projection_restatement_equals_the_oracle(oracle, c):
    lib = ba_ref._bind(oracle)
    got = _oracle_proj(lib, c)
    ref = fr.proj_flat(*fr.proj_factor(c["f"], c["pose_i"], c["pose_j"], c["ex0"], c["ex1"], c["lam"], c["td"]))
    ra = _ratio(got, ref)
    print(f"\n[oracle] proj {c['name']} {ra:.3g}")
    assert ra <= ORACLE_SHARE * K_PROJ


# ---------------------------------------------------------------- (c) gauge_fix invariants
@pytest.mark.parametrize("c", GAUGE, ids=_ids(GAUGE))
def test_gauge_fix_invariants(c):
    pose, sb, nf = c["pose"], c["sb"], c["nframes"]
    g = fr.gauge_fix(dict(pose=pose, sb=sb), c["R0"], c["ypr0"], c["P0"], c["use_imu"], nf)
    Rin = np.array([fr.rot_of(p[3:] / np.linalg.norm(p[3:])) for p in pose])
    tol = 64 * fr.EPS
    assert g["singular"] == c["want_singular"] == (bool(c["use_imu"]) and fr.gauge_singular(pose[0], c["ypr0"]))
    if c["use_imu"]:
        assert np.array_equal(g["P"][0], c["P0"])
        if g["singular"]:
            assert np.abs(g["R"][0] - c["R0"]).max() <= tol * g["R_mag"][0].max() + 4e-3 * (abs(np.linalg.norm(pose[0, 3:]) - 1) > 1e-6)      # R0 R00^T R00n: R00 is not normalised there
        else:
            dy = (fr.r2ypr(g["R"][0])[0] - c["ypr0"][0] + 180.0) % 360.0 - 180.0
            assert abs(dy) <= 1e-9 + 0.2 * (abs(np.linalg.norm(pose[0, 3:]) - 1) > 1e-6), dy
    else:
        assert np.array_equal(g["P"], pose[:, :3]) and np.array_equal(g["V"], sb[:, :3])          # bit-identical
    for i in range(nf):
        assert np.abs(g["R"][i] @ g["R"][i].T - np.eye(3)).max() <= (1e-2 if g["singular"] else tol * g["R_mag"][i].max() ** 2)
        for j in range(nf):
            if g["singular"] and abs(np.linalg.norm(pose[0, 3:]) - 1) > 1e-6:
                continue          # rot = R0 R00^T with an un-normalised R00 is not a rotation: the reference's own behaviour, relative poses scale with it
            scale = g["R_mag"][i].max() * g["R_mag"][j].max()
            assert np.abs(g["R"][i].T @ g["R"][j] - Rin[i].T @ Rin[j]).max() <= tol * scale
            pm = scale * (np.abs(pose[i, :3]).max() + np.abs(pose[j, :3]).max() + np.abs(pose[0, :3]).max() + np.abs(c["P0"]).max())
            assert np.abs(g["R"][i].T @ (g["P"][j] - g["P"][i]) - Rin[i].T @ (pose[j, :3] - pose[i, :3])).max() <= tol * pm
        assert np.abs(g["R"][i].T @ g["V"][i] - Rin[i].T @ sb[i, :3]).max() <= 1e-2 * g["singular"] + tol * g["R_mag"][i].max() ** 2 * np.abs(sb[i, :3]).max()      # body-frame velocity
    for i in range(nf, 11):
        assert not g["fixed"][i] and np.array_equal(g["P"][i], pose[i, :3]) and np.array_equal(g["V"][i], sb[i, :3])


def test_euler_and_quaternion_helpers():
    rng = np.random.default_rng(7)
    for _ in range(50):
        ypr = np.array([rng.uniform(-179, 179), rng.uniform(-89, 89), rng.uniform(-179, 179)])
        R = fr.ypr2r(ypr)
        assert np.abs(fr.r2ypr(R) - ypr).max() <= 1e-9
        q = fr.quat_of(R)
        assert np.abs(fr.rot_of(q) - R).max() <= 16 * fr.EPS
    for axis, want in ((0, 1), (1, 2), (2, 3)):
        assert fr.qfromR_case(fc._rot_axis(axis, 179.0)) == want
    assert fr.qfromR_case(np.eye(3)) == 0


# ---------------------------------------------------------------- (d) every case reaches what it is named for
def test_imu_cases_reach_their_edges():
    seen_signs, angles = set(), []
    for c in IMU:
        pre = c["pre"]
        signs = tuple(int(np.sign(w)) for w in (c["pose_i"][6], c["pose_j"][6], pre["dq"][0]))
        assert signs == tuple(c["signs"]), (c["name"], signs)
        seen_signs.add(signs)
        r = fr.imu_raw(pre, fc.G_NORM, c["pose_i"], c["sb_i"], c["pose_j"], c["sb_j"])[0].v
        ang = 2 * np.arcsin(min(1.0, np.linalg.norm(r[3:6]) / 2 * np.sqrt(fr.imu_cq_norm2(pre, c["sb_i"]))))          # rotation between cq and Qi^-1 Qj, folded into [0, pi]
        if c["near_pi"]:
            assert abs(ang - np.pi) < 1e-3 + 2e-3, (c["name"], ang)          # 5e-4 from pi by construction; the bias correction (dbg 1e-3, dt 0.1) moves it by ~1e-4
            angles.append(ang)
        assert np.linalg.norm(c["sb_i"][3:6] - pre["lin_ba"]) == pytest.approx(c["dba"], rel=1e-9, abs=1e-15)
        assert np.linalg.norm(c["sb_i"][6:9] - pre["lin_bg"]) == pytest.approx(c["dbg"], rel=1e-9, abs=1e-15)
        if c["cond"]:
            assert np.linalg.cond(pre["covariance"]) >= 1e8
    assert len(seen_signs) == 8 and len(angles) == 2
    assert {c["pre"]["sum_dt"] for c in IMU} >= {0.005, 10.0}
    assert {(c["dba"], c["dbg"]) for c in IMU} >= {(a, g) for a in (0.0, 1e-3, 0.3) for g in (0.0, 1e-3, 0.3)}
    # the sign of the residual follows the signs of the quaternions: flipping any one of them flips r_q and nothing else
    c = IMU[0]
    r0 = fr.imu_raw(c["pre"], fc.G_NORM, c["pose_i"], c["sb_i"], c["pose_j"], c["sb_j"])[0].v
    pj = c["pose_j"].copy(); pj[3:] *= -1
    r1 = fr.imu_raw(c["pre"], fc.G_NORM, c["pose_i"], c["sb_i"], pj, c["sb_j"])[0].v
    assert np.array_equal(r1[3:6], -r0[3:6]) and np.array_equal(np.delete(r1, [3, 4, 5]), np.delete(r0, [3, 4, 5]))


def test_projection_cases_reach_their_edges():
    depths, fronts = {k: [] for k in range(3)}, 0
    for c in PROJ:
        r, J = fr.proj_factor(c["f"], c["pose_i"], c["pose_j"], c["ex0"], c["ex1"], c["lam"], c["td"])
        depths[c["kind"]].append(1.0 / c["lam"])
        assert np.abs(r.v).max() < 50, (c["name"], r.v)          # the observation sits on the projection: the residual stays a few pixels wherever the point is
        if c["front"] is not None:
            assert abs(J["dep"].v - 1e-3) <= 1e-9 and c["pcj_z"] == pytest.approx(J["dep"].v, rel=1e-6)
            fronts += 1
        if "td0.05" in c["name"]:
            assert c["td"] - c["f"]["td_i"] == pytest.approx(0.05, rel=1e-12)
        if c["name"].endswith("td0"):
            assert c["td"] == c["f"]["td_i"]
        if "same_pose" in c["name"]:
            assert np.array_equal(c["pose_i"], c["pose_j"])
        # structural zeros of the kind
        if c["kind"] == 0:
            assert not J["Jex1"].m.any()
        if c["kind"] == 2:
            assert not J["Ji"].m.any() and not J["Jj"].m.any()
    assert fronts == 3
    for k in range(3):
        assert min(depths[k]) <= 0.2 and max(depths[k]) >= 200.0


@pytest.mark.parametrize("c", GAUGE, ids=_ids(GAUGE))
def test_gauge_cases_reach_their_branches(c):
    g = fr.gauge_fix(dict(pose=c["pose"], sb=c["sb"]), c["R0"], c["ypr0"], c["P0"], c["use_imu"], c["nframes"])
    assert g["singular"] == c["want_singular"]
    for i, qc in c["want_qcase"].items():
        assert i < c["nframes"] and fr.qfromR_case(g["R"][i]) == qc, (i, qc, fr.qfromR_case(g["R"][i]))
    nn = np.linalg.norm(c["pose"][:, 3:], axis=1)
    if "norm" in c["name"]:
        assert np.all(np.abs(np.abs(nn - 1) - 1e-3) < 1e-9)


def test_gauge_case_list_covers_the_issue():
    names = {c["name"] for c in GAUGE}
    reached = set()
    for c in GAUGE:
        reached |= set(c["want_qcase"].values())
        y00 = fr.r2ypr(fr.rot_of(c["pose"][0, 3:]))[1]
        for p in (abs(y00), abs(c["ypr0"][1])):
            if abs(p - 89.5) < 1e-6:
                assert c["want_singular"] or not c["use_imu"]
            if abs(p - 88.9) < 1e-6 and abs(abs(y00) - 90) >= 1 and abs(abs(c["ypr0"][1]) - 90) >= 1:
                assert not c["want_singular"]
    assert reached == {0, 1, 2, 3}
    assert {(c["nframes"], c["use_imu"]) for c in GAUGE} >= {(n, u) for n in (1, 2, 11) for u in (0, 1)}
    assert {len(c["lam"]) for c in GAUGE} >= {0, 1, 1000}
    assert {f"{w}{p:+g}" for w in ("solved", "before", "both") for p in (89.5, -89.5, 88.9, -88.9)} <= names
    assert any(c["want_singular"] for c in GAUGE) and any(not c["want_singular"] and c["use_imu"] for c in GAUGE)


@pytest.mark.parametrize("c", REJECT, ids=_ids(REJECT))
def test_reject_cases_sit_on_both_sides_of_the_bar(c):
    flags, err = fr.reject_flags(c["pose"], c["ex_state"], c["ric"], c["tic"], c["lam"], c["factors"], c["landmarks"], fc.FOCAL, c["ex_from_state"])
    assert np.abs(err - 3.0).min() >= 1e-9
    assert np.abs(err - c["targets"]).max() <= 1e-9          # the constructed errors are what the reference measures
    near = np.abs(c["targets"] - 3.0) < 1e-5
    assert np.all(np.abs(np.abs(err[near] - 3.0) - 1e-6) < 1e-9)
    assert np.array_equal(flags, (c["targets"] > 3).astype(np.uint8))
    if len(err) >= 2:
        assert flags.min() == 0 and flags.max() == 1
    # the other set of extrinsics decides differently: a kernel that reads the wrong one cannot pass
    other, _ = fr.reject_flags(c["pose"], c["ex_state"], c["ric"], c["tic"], c["lam"], c["factors"], c["landmarks"], fc.FOCAL, 1 - c["ex_from_state"])
    if len(err) >= 7:
        assert not np.array_equal(other, flags)


def test_reject_case_list_covers_the_issue():
    assert {len(c["landmarks"]) for c in REJECT} >= {1, 7, 8, 9, 1000}
    cnt = np.concatenate([c["landmarks"]["count"] for c in REJECT])
    assert cnt.min() == 1 and cnt.max() == 22
    kinds = np.concatenate([c["factors"]["kind"] for c in REJECT])
    assert set(kinds.tolist()) == {0, 1, 2}
    assert {c["ex_from_state"] for c in REJECT} == {0, 1}
    for c in REJECT:
        assert np.abs(c["ex_state"][:, :3] - c["tic"]).max() > 1e-3          # the state's extrinsics are not the arguments
