"""CPU validation of tests/objfactor_ref.py, the float64 restatement tests/test_objfactor_reference_gpu.py holds the HIP line, box and instance factors
against.  No GPU, and (apart from (b)) no code of the project.
  (a) closed forms against Richardson-extrapolated central differences through PoseLocalParameterization::Plus and LineOrthParameterization::Plus wherever the
      closed form is the derivative (line factor, the pose blocks of the instance factor); where it knowingly is not, the gap is pinned: I1 is the derivative
      times -sign(e) sign(p_obj) / 10 on rows outside the box, and non-zero where the derivative is zero (inside; and zero where it is not: the rotation
      columns); I2 is 50 / |box - dims|^2 times the derivative; I3 with (1 - cos t) / t in place of 1 - cos t / t IS the derivative and the two J_r differ by
      exactly (1 + 1 / |phi|) hat(a); the inverse-depth form plus the derivative is reduce T velocity_j (cur_td - td_j) / lambda^2 (zero at a td gap of zero:
      there the form is minus the derivative); the line factor's orth Jacobian is the derivative with the column signs (s1, s2, s1 s2, s1 s2), s1 = sign cos
      phi, s2 = sign sin phi.  NUM_TOL is a property of the reference and never applied to the device.
  (b) the restatement against the CPU oracle (dvo_line_eval, dvo_line_plus, dvo_box_*_eval, dvo_inst_proj_eval) in eps of the magnitude over the whole case
      list, non-finite patterns equal; ten times the largest ratio, rounded up, is that factor's K for the GPU module.
  (c) independent cross-checks: inst_proj with pose_oj == pose_oi against factor_ref.proj_factor kind 0; line_plus composed with bd_ref.line_minus; exp(r) == R.
  (d) every case reaches what it is named for.
Measured here: closed form vs Richardson, max |dJ| / (1 + max |J|): line 1.5e-5 (far1e3: the body 1e3 m out, step 1e-6; 5e-7 in l1e-6, below 3e-10 elsewhere), orientation
2.3e-10 (angle1e-9), instance 1.7e-5 (shift1e3; 1.9e-6 in front1e-3, below 5e-8 elsewhere): NUM_TOL = 2e-4;
restatement vs oracle, in eps of the magnitude: line 0.020 (ex_identity), line_plus 0.42 (big3), box_enclose 0.34 (inside), box_dims 0 (every case
bit-identical), box_orientation 0.026 (angle0.001), inst_proj 0.043 (depth200).
Every restatement is evaluated with first-order products (factor_ref.first_order): with products of magnitudes the bar of a benign line Jacobian was 1e12 eps of
the entry and 1e33 in l1e-6.  The orientation Jacobian's magnitude goes through the closed-form inverse of J_r (objfactor_ref.ori_Jr_inverse), which this module
holds equal to the cofactor inverse.  Median magnitude over |value| now: line 1e2 to 2e3 (l1e-3 1e5, far1e3 7e4, l1e-6 1e8: the cancellations themselves),
orientation 4e2 to 1e3 at angles from 1 up, and 3e5, 2e8, 3e11, 6e13 at 1e-3, 1e-6, 1e-9, 1e-12: the 1 / theta of the formula.
  (e) what the bars reject: a record with its Jacobian negated or zeroed misses K in every case; the record scaled by 1 + 1e-6 and by 1 + 1e-9 misses K in every
      case but those of LOOSE, where the reference's own conditioning is above the perturbation."""
import numpy as np
import pytest

from tests import bd_ref, factor_cases as fc, factor_ref as fr, obj_gen as G, objfactor_cases as oc, objfactor_ref as R
from tests.test_factor_reference import ORACLE_SHARE, _ids, _ratio

NUM_TOL = 2e-4                # (a) |numeric - closed| <= NUM_TOL (1 + max |J|): ten times the largest Richardson error measured over the case lists (1.7e-5), rounded up
# (b) -> the GPU module's bars: ten times the largest reference-vs-oracle ratio measured over the case list (0.020, 0.42, 0.34, 0, 0.026, 0.043), rounded up
K_LINE, K_PLUS, K_BOX, K_DIMS, K_ORI, K_INST = 0.3, 5.0, 4.0, 0.0, 0.3, 0.5
# K_DIMS = 0 is bit equality.  It is what the rule gives: oracle and restatement agree bit for bit on every box_dims case (box - dims is exact or one rounding,
# then three squares, two sums, a square and a division in the same order), and the device met it on the MI355X.  A compiler that contracts d.d into fused
# multiply-adds would move the last bit and fail this bar without a defect in the kernel: then the bar, not the kernel, is what to look at.
K = dict(line=K_LINE, plus=K_PLUS, box=K_BOX, dims=K_DIMS, ori=K_ORI, inst=K_INST)

FAMILIES = ("line", "plus", "box", "dims", "ori", "inst")
CASES = dict(line=oc.line_cases(), plus=oc.plus_cases(), box=oc.box_cases(), dims=oc.dims_cases(), ori=oc.ori_cases(), inst=oc.inst_cases())
ALL = [(fam, c) for fam in FAMILIES for c in CASES[fam]]
ALL_IDS = [f"{fam}-{c['name']}" for fam, c in ALL]
INST_KEYS = ("pbj", "pbi", "pex", "poj", "poi")


# ---------------------------------------------------------------- shared with the GPU module
def references(fam, c):
    """the restatement's flat record of a case as a list of A: one entry, or both signs of the logarithm where a rounding decides it (ori, both_signs)"""
    if fam == "line":
        return [R.line_flat(R.line_factor(c["obs"], c["si"], c["pose"], c["ex"], c["orth"]))]
    if fam == "plus":
        return [R.line_plus(c["orth"], c["delta"])]
    if fam == "box":
        return [R.box_flat(R.box_enclose(c["p_w"], c["dims"], c["pose_obj"]))]
    if fam == "dims":
        return [R.dims_flat(R.box_dims(c["dims"], c["box"]))]
    if fam == "ori":
        return [R.ori_flat(R.box_orientation(c["R_cioi"], c["R_bc"], c["pose_body"], c["pose_obj"], wsign=s)) for s in ((1, -1) if c["both_signs"] else (None,))]
    return [R.inst_proj(c["f"], c["pbj"], c["pbi"], c["pex"], c["poj"], c["poi"], c["lam"])]


def ratio_nf(dev, ref):
    """_ratio over the finite entries of the reference; inf unless the device is non-finite in exactly the reference's non-finite entries"""
    dev, fin = np.asarray(dev, float), np.isfinite(ref.v)
    if not np.array_equal(np.isfinite(dev), fin):
        return np.inf
    return _ratio(dev[fin], fr.A(ref.v[fin], ref.m[fin]))


def case_ratio(fam, dev, refs):
    """the ratio of a flat device record against the case's reference (the better of the two signs in r and J together, where there are two);
    line_plus: the two atan2 outputs are compared modulo 2 pi"""
    dev = np.array(dev, float)
    best = np.inf
    for ref in refs:
        d = dev.copy()
        if fam == "plus":
            for k in (0, 2):
                d[k] = ref.v[k] + (d[k] - ref.v[k] + np.pi) % (2 * np.pi) - np.pi
        best = min(best, ratio_nf(d, ref))
    return best


def oracle_flat(lib, fam, c):
    from tests.test_inst_proj_factor import o_eval
    if fam == "line":
        r, J = G.o_line(lib, c["obs"], c["si"], c["pose"], c["ex"], c["orth"])
        assert not J[0][:, 6].any() and not J[1][:, 6].any()
        return np.concatenate([r, J[0][:, :6].ravel(), J[1][:, :6].ravel(), J[2].ravel()])
    if fam == "plus":
        return G.o_line_plus(lib, c["orth"], c["delta"])
    if fam == "box":
        r, J = G.o_box_enclose(lib, c["p_w"], c["dims"], c["pose_obj"])
        assert not J[0][:, 6].any()
        return np.concatenate([r, J[0][:, :6].ravel()])
    if fam == "dims":
        r, J = G.o_box_dims(lib, c["dims"], c["box"])
        return np.concatenate([r, J[0].ravel()])
    if fam == "ori":
        r, J = G.o_box_orientation(lib, c["R_cioi"], c["R_bc"], c["pose_body"], c["pose_obj"])
        assert not J[0][:, 6].any() and not J[1][:, 6].any()
        return np.concatenate([r, J[0][:, :6].ravel(), J[1][:, :6].ravel()])
    f = c["f"]
    obs = np.concatenate([f["pts_j"], f["pts_i"], f["vel_j"], f["vel_i"], [f["td_j"], f["td_i"]]])
    r, J = o_eval(lib, obs, f["cur_td"], [c[k] for k in INST_KEYS] + [np.array([c["lam"]])])
    assert not any(J[b][:, 6].any() for b in range(5))
    return np.concatenate([r] + [J[b][:, :6].ravel() for b in range(5)] + [J[5][:, 0]])


def oracle_ratio(lib, fam, c):
    with np.errstate(all="ignore"):
        return case_ratio(fam, oracle_flat(lib, fam, c), references(fam, c))


def _rel(num, closed):
    return float(np.abs(num - closed).max() / (1.0 + np.abs(closed).max()))


# ---------------------------------------------------------------- (a) closed forms vs numeric derivatives
LINE_A = [c for c in CASES["line"] if c["qnorm"] == (1.0, 1.0)]          # Plus normalises: at a non-unit quaternion the derivative through Plus is taken elsewhere


@pytest.mark.parametrize("c", LINE_A, ids=_ids(LINE_A))
def test_line_closed_form_is_the_derivative_up_to_the_column_signs(c):
    r, Jp, Je, Jo, p = R.line_factor(c["obs"], c["si"], c["pose"], c["ex"], c["orth"], parts=True)
    h = 1e-3 * min(1.0, p["l_sqrt"] / p["n_norm"]) / (1.0 + c["shift"])
    Jn = fr.numeric_jacobian(lambda b: R.line_factor(c["obs"], c["si"], b[0], b[1], c["orth"])[0].v, [c["pose"], c["ex"]], ["pose", "pose"], h)
    worst = max(_rel(Jn[:, :6], Jp.v), _rel(Jn[:, 6:], Je.v))
    if c["name"] != "phi0":
        fold = abs(c["orth"][3]) + 2 * h < np.pi / 2              # the reference's own Plus while the differences stay inside the principal range of the phase, the unfolded phase otherwise
        Jn = R.richardson(lambda x: R.line_factor(c["obs"], c["si"], c["pose"], c["ex"], x)[0].v, c["orth"], lambda x, d: R.line_plus(x, d, fold=fold).v, 4, h)
        s1, s2 = np.sign(p["cphi"]), np.sign(p["sphi"])
        worst = max(worst, _rel(Jn, Jo.v * np.array([s1, s2, s1 * s2, s1 * s2])))
    print(f"\n[num] line {c['name']} {worst:.3g}")
    assert worst <= NUM_TOL, worst


def test_line_orth_jacobian_flips_with_the_quadrant():
    """the sign cases differ from the derivative by O(1): in quadrant 2 columns 0, 2, 3 flip, in quadrant 4 columns 1, 2, 3, in quadrant 3 columns 0, 1"""
    for name, flips in (("quadrant1", ()), ("quadrant2", (0, 2, 3)), ("quadrant3", (0, 1)), ("quadrant4", (1, 2, 3))):
        c = next(x for x in CASES["line"] if x["name"] == name)
        Jo = R.line_factor(c["obs"], c["si"], c["pose"], c["ex"], c["orth"])[3].v
        Jn = R.richardson(lambda x: R.line_factor(c["obs"], c["si"], c["pose"], c["ex"], x)[0].v, c["orth"], lambda x, d: R.line_plus(x, d, fold=False).v, 4, 1e-3)
        for col in range(4):
            want = -Jn[:, col] if col in flips else Jn[:, col]
            assert np.abs(Jo[:, col]).max() > 1e-3 and _rel(want, Jo[:, col]) <= NUM_TOL, (name, col)


BOX_H = 1e-5
def _box_smooth(c):
    """unit quaternion, N_p finite, and far enough from every face that the differences do not straddle it"""
    if c["qnorm"] != 1.0 or "nan_row" in c:
        return False
    p = R.box_enclose(c["p_w"], c["dims"], c["pose_obj"], parts=True)[2]
    return np.abs(p["face"]).min() > 20 * BOX_H * max(1.0, np.abs(p["po"]).max())


BOX_A = [c for c in CASES["box"] if _box_smooth(c)]


@pytest.mark.parametrize("c", BOX_A, ids=_ids(BOX_A))
def test_box_enclose_gap_to_the_derivative(c):
    """I1"""
    r, J, p = R.box_enclose(c["p_w"], c["dims"], c["pose_obj"], parts=True)
    Jn = fr.numeric_jacobian(lambda b: R.box_enclose(c["p_w"], c["dims"], b[0])[0].v, [c["pose_obj"]], ["pose"], BOX_H)
    assert not J.v[:, 3:].any()
    for i in range(3):
        assert np.abs(J.v[i, :3]).max() > 0.1
        if r.v[i] > 0:
            assert _rel(Jn[i, :3], -10.0 * np.sign(p["po"][i]) * np.sign(p["e"][i]) * J.v[i, :3]) <= NUM_TOL
            assert np.abs(Jn[i, 3:]).max() > 1e-3 * np.abs(p["po"]).max()          # the derivative has rotation columns, the closed form does not
        else:
            assert r.v[i] == 0.0 and r.m[i] == 0.0 and not Jn[i].any()


def test_box_enclose_gap_is_covered():
    names = {c["name"] for c in BOX_A}
    assert len(BOX_A) >= 12 and {"inside", "out_x", "out_y", "out_z", "out_xyz", "far1e3"} <= names


@pytest.mark.parametrize("c", CASES["dims"], ids=_ids(CASES["dims"]))
def test_box_dims_gap_to_the_derivative(c):
    """I2: r = |d|^4 / 100 has the derivative |d|^2 d / 25 = (|d|^2 / 50) 2 d"""
    r, J = R.box_dims(c["dims"], c["box"])
    d = c["box"] - c["dims"]
    h = 1e-2 * max(np.linalg.norm(d), 1e-6)
    Jn = R.richardson(lambda x: np.array([R.box_dims(c["dims"], x)[0].v]), c["box"], lambda x, dd: x + dd, 3, h)
    want = (d @ d) / 50.0 * J.v
    if c["name"] == "equal":
        assert r.v == 0.0 and not J.v.any() and np.abs(Jn).max() <= h ** 3
    else:
        assert np.abs(Jn - want).max() <= 1e-6 * np.abs(want).max() + 1e-9 * fr.EPS ** 0.5 * (np.abs(c["box"]).max() / h) * np.abs(r.m)


ORI_A = [c for c in CASES["ori"] if c["qnorm"] == (1.0, 1.0) and not c["both_signs"] and c["name"] != "angle0"]


@pytest.mark.parametrize("c", ORI_A, ids=_ids(ORI_A))
def test_box_orientation_gap_to_the_derivative(c):
    """I3"""
    args = (c["R_cioi"], c["R_bc"])
    r, Jb, Jo, p = R.box_orientation(*args, c["pose_body"], c["pose_obj"], parts=True)
    rd, _, Jd, pd = R.box_orientation(*args, c["pose_body"], c["pose_obj"], derivative=True, parts=True)
    Jn = fr.numeric_jacobian(lambda b: R.box_orientation(*args, b[0], b[1])[0].v, [c["pose_body"], c["pose_obj"]], ["pose", "pose"], 1e-4)
    worst = _rel(Jn[:, 6:], Jd.v)
    print(f"\n[num] ori {c['name']} {worst:.3g}")
    assert worst <= NUM_TOL
    assert not Jb.v.any() and not Jb.m.any() and not Jo.v[:, :3].any() and not Jo.m[:, :3].any()
    assert not Jn[:, :3].any() and not Jn[:, 6:9].any() and np.abs(Jn[:, 3:6]).max() > 0.3          # the body rotation moves the residual, its Jacobian is zero
    th, a = p["theta"], p["a"]
    gap = p["Jr"].v - pd["Jr"].v
    want = (1.0 + 1.0 / th) * np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    assert np.abs(gap - want).max() <= 8 * fr.EPS * (1.0 + 1.0 / th)
    assert np.abs(Jo.v[:, 3:] - Jd.v[:, 3:]).max() > 1e-2                      # and it shows in the Jacobian at every angle


INST_A = [c for c in CASES["inst"] if c["qnorm"] is None]


@pytest.mark.parametrize("c", INST_A, ids=_ids(INST_A))
def test_inst_proj_closed_form_is_the_derivative(c):
    out, p = R.inst_proj(c["f"], *[c[k] for k in INST_KEYS], c["lam"], parts=True)
    h = 1e-4 * min(1.0, abs(p["dep"]) * 3) / (1.0 + c["shift"])
    Jn = fr.numeric_jacobian(lambda b: R.inst_proj(c["f"], b[0], b[1], b[2], b[3], b[4], b[5][0]).v[:2], [c[k] for k in INST_KEYS] + [np.array([c["lam"]])],
                             ["pose"] * 5 + ["vec"], h * min(1.0, c["lam"]))
    closed = out.v[2:62].reshape(5, 2, 6)
    worst = max(_rel(Jn[:, 6 * b:6 * b + 6], closed[b]) for b in range(5))
    # inverse depth: closed + derivative = reduce T (pts_j - pts_j_td) / lambda^2
    want = p["red"] @ p["T"] @ (c["f"]["pts_j"] - p["pts_j_td"]) / c["lam"] ** 2
    worst = max(worst, _rel(out.v[62:] + Jn[:, 30], want))
    print(f"\n[num] inst {c['name']} {worst:.3g}")
    assert worst <= NUM_TOL
    if c["td_gap"] == 0:
        assert not want.any() and np.abs(out.v[62:]).max() > 1.0          # the form is minus the derivative


# ---------------------------------------------------------------- (b) restatement vs oracle
@pytest.mark.parametrize("fam,c", ALL, ids=ALL_IDS)
def test_restatement_equals_the_oracle(oracle, fam, c):
    ra = oracle_ratio(oracle.lib, fam, c)
    print(f"\n[oracle] {fam} {c['name']} {ra:.3g}")
    assert ra <= ORACLE_SHARE * K[fam], ra


def test_exact_zeros_of_the_oracle(oracle):
    c = CASES["dims"][0]
    assert c["name"] == "equal" and not oracle_flat(oracle.lib, "dims", c).any() and not references("dims", c)[0].v.any()
    c = CASES["box"][0]
    assert c["name"] == "inside" and not oracle_flat(oracle.lib, "box", c)[:3].any()
    c = CASES["ori"][0]
    assert c["name"] == "angle0" and not oracle_flat(oracle.lib, "ori", c)[:3].any()


# ---------------------------------------------------------------- (c) independent cross-checks
@pytest.mark.parametrize("c", INST_A, ids=_ids(INST_A))          # unit quaternions: q^-1 and q cancel as rotations only there
def test_inst_proj_with_a_static_object_is_the_two_frame_projection(c):
    f = c["f"]
    out = R.inst_proj(f, c["pbj"], c["pbi"], c["pex"], c["poj"], c["poj"], c["lam"])
    g = dict(kind=0, pix=f["pts_j"][0], piy=f["pts_j"][1], pjx=f["pts_i"][0], pjy=f["pts_i"][1], vix=f["vel_j"][0], viy=f["vel_j"][1], vjx=f["vel_i"][0], vjy=f["vel_i"][1],
             td_i=f["td_j"], td_j=f["td_i"])
    r, _ = fr.proj_factor(g, c["pbj"], c["pbi"], c["pex"], c["pex"], c["lam"], f["cur_td"])
    assert np.all(np.abs(out.v[:2] - r.v) <= fr.EPS * (out.m[:2] + r.m))


def test_line_plus_and_line_minus_are_inverse():
    rng = np.random.default_rng(77)
    for c in CASES["line"]:
        o = c["orth"]
        if abs(o[3]) >= 1.5 or abs(o[1]) >= 1.5:
            continue
        d = rng.normal(0, 0.05, 4)
        if abs(o[3] + d[3]) >= 1.5:
            d[3] = -d[3]
        assert np.allclose(bd_ref.line_minus(R.line_plus(o, d).v, o), d, rtol=0, atol=1e-12), c["name"]
    for c in CASES["plus"]:
        if c.get("zero"):
            out = R.line_plus(c["orth"], c["delta"])
            assert np.all(np.abs(out.v - c["orth"]) <= fr.EPS * out.m)          # delta = 0 on principal-range input: every component returns within its bar


def _exp(w):
    th = np.linalg.norm(w)
    if th < 1e-8:
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        return np.eye(3) + Kx + 0.5 * Kx @ Kx
    a = w / th
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


@pytest.mark.parametrize("c", [c for c in CASES["ori"] if c["qnorm"] == (1.0, 1.0)], ids=lambda c: c["name"])
def test_box_orientation_residual_is_the_logarithm(c):
    """exp(r) == R entrywise: the rounding of R (3 products of rotations: 16 eps) and what the rounding of r (eps m_r) moves exp by (at most |dr| an entry)"""
    ref = R.box_orientation(c["R_cioi"], c["R_bc"], c["pose_body"], c["pose_obj"], parts=True)
    assert np.abs(_exp(ref[0].v) - ref[3]["R"]).max() <= fr.EPS * (16 + 4 * ref[0].m.max())
    if c["name"] != "angle0":
        inv, closed = ref[3]["inv"], ref[3]["inv_closed"]          # the cofactor inverse of J_r equals its closed form within the magnitude it carries
        assert np.all(np.abs(inv.v - closed.v) <= fr.EPS * inv.m)


# ---------------------------------------------------------------- (d) branch proofs
def test_line_cases_reach_their_edges():
    seen = {}
    for c in CASES["line"]:
        out = R.line_factor(c["obs"], c["si"], c["pose"], c["ex"], c["orth"], parts=True)
        p, flat = out[4], R.line_flat(out[:4])
        seen[c["name"]] = (np.sign(p["cphi"]), np.sign(p["sphi"]))
        nf = ~np.isfinite(flat.v)
        assert nf[26:].all() and not nf[:26].any() if c["name"] == "phi0" else not nf.any(), c["name"]
        if not c["si"].any():
            assert not flat.v.any() and not flat.m.any()          # everything under a zero sqrt_info is structurally zero
        if c["lratio"]:
            assert 0.5 * c["lratio"] < p["l_sqrt"] / p["n_norm"] < 2 * c["lratio"]
        if c["shift"]:
            assert np.linalg.norm(c["pose"][:3]) > 990
    assert [seen[f"quadrant{k}"] for k in (1, 2, 3, 4)] == [(1, 1), (-1, 1), (-1, -1), (1, -1)]
    by = {c["name"]: c for c in CASES["line"]}
    assert np.any(by["benign_asym"]["si"][[1, 2]] != 0) and by["benign_asym"]["si"][1] != by["benign_asym"]["si"][2] and not by["benign_zero_info"]["si"].any()
    assert [by[n]["orth"][3] for n in ("phi1e-3", "phi1e-6", "phi0")] == [1e-3, 1e-6, 0.0]
    assert np.isclose(np.pi / 2 - by["phi_half_pi-1e-6"]["orth"][3], 1e-6, rtol=1e-6) and np.isclose(np.pi / 2 - by["phi_half_pi-1e-3"]["orth"][3], 1e-3, rtol=1e-9)
    assert np.isclose(np.pi / 2 - by["theta2+"]["orth"][1], 1e-6, rtol=1e-6) and np.isclose(np.pi / 2 + by["theta2-"]["orth"][1], 1e-6, rtol=1e-6)
    assert np.array_equal(by["ex_identity"]["ex"], [0, 0, 0, 0, 0, 0, 1])
    for n, (a, b) in (("qnorm+-", (1, -1)), ("qnorm-+", (-1, 1))):
        assert np.isclose(np.linalg.norm(by[n]["pose"][3:]) - 1, a * 1e-3) and np.isclose(np.linalg.norm(by[n]["ex"][3:]) - 1, b * 1e-3)


def test_plus_cases_reach_their_edges():
    for c in CASES["plus"]:
        o, d = c["orth"], c["delta"]
        out = R.line_plus(o, d)
        assert np.isfinite(out.v).all() and np.isfinite(out.m).all()
        ph = o[3] + d[3]
        for fold in (np.pi / 2, -np.pi / 2):
            assert abs(ph - fold) >= 1e-9                          # the fold decision cannot depend on libm
        if "phase" in c:
            assert abs(ph - c["phase"]) < 1e-15
            if c["name"].startswith("fold"):
                assert np.isclose(abs(abs(ph) - np.pi / 2), 1e-6, rtol=1e-6)
            if abs(ph) > np.pi / 2:
                assert abs(out.v[3] - (np.sign(ph) * np.pi - ph)) < 1e-9          # folded
            else:
                assert abs(out.v[3] - ph) < 1e-9
        if "pitch" in c:
            assert abs(o[1] + d[1] - c["pitch"]) < 1e-15 and abs(c["pitch"]) > np.pi / 2
            assert abs(out.v[1] - (np.sign(c["pitch"]) * np.pi - c["pitch"])) < 1e-12          # the other Euler solution comes back
        if "big" in c:
            assert abs(d[c["big"]]) == 3.0
        if "u1z" in c:
            assert abs(abs(np.sin(out.v[1])) - c["u1z"]) < 1e-13 and abs(np.pi / 2 - abs(out.v[1]) - np.sqrt(2e-12)) < 1e-9
        if "cut" in c:
            k, at = c["cut"]
            assert abs(out.v[k] - at) < 1e-9 and abs(out.v[k] - at) > 1e-10
        if c.get("zero"):
            assert not d.any() and abs(o[1]) < np.pi / 2 and abs(o[3]) < np.pi / 2 and abs(o[0]) < np.pi and abs(o[2]) < np.pi
    assert {c["big"] for c in CASES["plus"] if "big" in c} == {0, 1, 2, 3}


def test_box_cases_reach_their_edges():
    signs, differ, faces, nan_rows = set(), set(), set(), set()
    for c in CASES["box"]:
        r, J, p = R.box_enclose(c["p_w"], c["dims"], c["pose_obj"], parts=True)
        assert np.abs(p["face"]).min() >= 1e-12                    # no case so close to a face that the clamp could depend on a rounding
        assert not J.v[:, 3:].any() and not J.m[:, 3:].any()
        if "outside" in c:
            assert tuple(int(x > 0) for x in r.v) == c["outside"] and tuple(int(x > 0) for x in p["face"]) == c["outside"]
            assert all(r.v[i] == 0.0 and r.m[i] == 0.0 for i in range(3) if not c["outside"][i])
        if c["name"] == "inside":
            Rojw = fr.rot_of(c["pose_obj"][3:]).T
            assert np.allclose(np.abs(J.v[:, :3]), np.abs(Rojw), atol=1e-14)          # r = 0 and the Jacobian is still +-R rows
        if "face" in c:
            ax, dist = c["face"]
            assert abs(p["face"][ax] - dist) < 1e-12 + 1e-6 * abs(dist) and (r.v[ax] > 0) == (dist > 0)
            faces.add((ax, np.sign(dist)))
        if "esign" in c:
            assert tuple(np.sign(p["e"])) == c["esign"] and np.abs(p["e"]).min() > 0.1
            signs.add(c["esign"])
        if "differ" in c:
            ne = np.sign(p["e"]) != np.sign(p["po"])
            assert ne[c["differ"]] and ne.sum() == 1 and np.abs(p["e"]).min() > 0.1 and np.abs(p["po"]).min() > 0.1
            differ.add(c["differ"])
        nf = ~np.isfinite(J.v)
        if "nan_row" in c:
            assert p["e"][c["nan_row"]] == 0 and nf[c["nan_row"], :3].all() and nf.sum() == 3 and np.isfinite(r.v).all()
            nan_rows.add(c["nan_row"])
        else:
            assert not nf.any()
        if c["name"] == "far1e3":
            assert np.linalg.norm(c["pose_obj"][:3]) > 999 and abs(p["face"][0] - 1e-3) < 1e-9
    assert len(signs) == 8 and differ == {0, 1, 2} and nan_rows == {0, 1, 2} and len(faces) == 6
    by = {c["name"]: c for c in CASES["box"]}
    assert np.all(by["dims1e-3"]["dims"] == 1e-3) and np.all(by["dims1e3"]["dims"] == 1e3)
    for n, s in (("qnorm+", 1), ("qnorm-", -1)):
        c = by[n]
        assert np.isclose(np.linalg.norm(c["pose_obj"][3:]) - 1, s * 1e-3)
        # inverse() is not conjugate(): with the conjugate the residual differs far beyond rounding
        q = c["pose_obj"][3:]
        po_conj = fr.rot_of(q * [-1, -1, -1, 1]) @ (c["p_w"] - c["pose_obj"][:3])
        po = R.box_enclose(c["p_w"], c["dims"], c["pose_obj"], parts=True)[2]["po"]
        assert np.abs(po_conj - po).max() > 1e-4


def test_dims_cases_reach_their_edges():
    by = {c["name"]: c for c in CASES["dims"]}
    assert np.array_equal(by["equal"]["dims"], by["equal"]["box"])
    for mag in (1e-8, 0.3, 3.0, 1e3):
        c = by[f"diff{mag:g}"]
        assert np.isclose(np.linalg.norm(c["box"] - c["dims"]), mag, rtol=1e-6)
    c = by["cancel1e-6_at_1e3"]
    assert c["dims"].min() >= 1e3 and np.allclose(c["box"] - c["dims"], 1e-6, rtol=1e-6)


def test_ori_cases_reach_their_edges():
    qcases, angles = set(), []
    for c in CASES["ori"]:
        r, Jb, Jo, p = R.box_orientation(c["R_cioi"], c["R_bc"], c["pose_body"], c["pose_obj"], parts=True)
        assert not Jb.v.any() and not Jb.m.any() and not Jo.v[:, :3].any() and not Jo.m[:, :3].any()
        nf = ~np.isfinite(Jo.v)
        if c["name"] == "angle0":
            assert not r.v.any() and not r.m.any() and nf[:, 3:].all() and p["branch"] == "taylor"
        else:
            assert not nf.any() and np.isfinite(r.v).all()
        if c.get("angle") is not None and c["qnorm"] == (1.0, 1.0):
            assert abs(p["theta"] - c["angle"]) <= 1e-15 + 1e-9 * c["angle"] + (1e-7 if c["angle"] > 3.1 else 0), (c["name"], p["theta"])
            angles.append(c["angle"])
        if "branch" in c:
            assert p["branch"] == c["branch"], (c["name"], p["branch"])
        if c["name"] == "pi_w_branch":
            assert abs(p["w"]) < 1e-10 and abs(p["theta"] - np.pi) < 1e-10
        if "qcase" in c:
            assert p["case"] == c["qcase"]
            qcases.add(p["case"])
        if c.get("wneg"):
            assert p["w"] < 0 and p["branch"] == "atan"
    assert qcases == {0, 1, 2, 3}
    assert sorted(angles)[:7] == [0.0, 1e-12, 1e-9, 1e-6, 1e-3, 1.0, 3.0] and sum(c["both_signs"] for c in CASES["ori"]) == 2
    by = {c["name"]: c for c in CASES["ori"]}
    for n, (a, b) in (("qnorm+-", (1, -1)), ("qnorm-+", (-1, 1))):
        assert np.isclose(np.linalg.norm(by[n]["pose_body"][3:]) - 1, a * 1e-3) and np.isclose(np.linalg.norm(by[n]["pose_obj"][3:]) - 1, b * 1e-3)


def test_inst_cases_reach_their_edges():
    by = {c["name"]: c for c in CASES["inst"]}
    for c in CASES["inst"]:
        out, p = R.inst_proj(c["f"], *[c[k] for k in INST_KEYS], c["lam"], parts=True)
        assert np.isfinite(out.v).all() and p["dep"] > 0
        if c["front"] is not None:
            assert abs(p["dep"] - c["front"]) < 1e-9 and np.abs(out.v[2:]).max() > 1e6
    assert [np.isclose(1 / by[f"depth{d:g}"]["lam"], d) for d in (0.2, 1.0, 10.0, 200.0)] == [True] * 4
    f = by["td0"]["f"]
    assert f["cur_td"] == f["td_j"] == f["td_i"] and np.isclose(by["td0.05"]["f"]["cur_td"] - by["td0.05"]["f"]["td_j"], 0.05)
    assert np.array_equal(by["same_obj"]["poj"], by["same_obj"]["poi"]) and np.array_equal(by["same_body"]["pbj"], by["same_body"]["pbi"])
    assert np.array_equal(by["ex_identity"]["pex"], [0, 0, 0, 0, 0, 0, 1])
    for n in ("qnorm+-", "qnorm-+"):
        assert all(np.isclose(abs(np.linalg.norm(by[n][k][3:]) - 1), 1e-3, rtol=1e-3) for k in INST_KEYS)
    assert all(np.linalg.norm(by["shift1e3"][k][:3]) > 990 for k in ("pbj", "pbi", "poj", "poi"))


# ---------------------------------------------------------------- (e) what the bars reject
JAC = dict(line=slice(2, 34), plus=slice(0, 4), box=slice(3, 21), dims=slice(1, 4), ori=slice(3, 39), inst=slice(2, 64))          # line_plus has no Jacobian: its outputs
# where a relative perturbation may pass: 1 + 1e-6 under the 1 / theta of the orientation inverse (eps / theta = 2e-4, 2e-7 times the slack of a first-order bound);
# 1 + 1e-9 also at theta = 1e-6 and under the six digits l_sqrt lost in l1e-6
LOOSE = {1e-6: {("ori", "angle1e-12"), ("ori", "angle1e-9")}, 1e-9: {("ori", "angle1e-12"), ("ori", "angle1e-9"), ("ori", "angle1e-06"), ("line", "l1e-6")}}


@pytest.mark.parametrize("fam,c", ALL, ids=ALL_IDS)
def test_bars_reject_a_wrong_record(fam, c):
    with np.errstate(all="ignore"):
        refs = references(fam, c)
        v = refs[0].v
        sel = np.zeros(len(v), bool)
        sel[JAC[fam]] = True
        sel &= np.isfinite(v) & (v != 0)
        if not sel.any():
            assert not np.nan_to_num(v[JAC[fam]]).any()          # nothing to get wrong: zero sqrt_info, box == dims, angle 0
            return
        out = {}
        for name, dev in (("negated", np.where(sel, -v, v)), ("zeroed", np.where(sel, 0.0, v)), (1e-6, v * (1 + 1e-6)), (1e-9, v * (1 + 1e-9))):
            out[name] = case_ratio(fam, dev, refs)
            if (fam, c["name"]) not in LOOSE.get(name, ()):
                assert out[name] > K[fam], (name, out[name])
    print(f"\n[reject] {fam} {c['name']} " + " ".join(f"{k}:{r:.2g}" for k, r in out.items()))
