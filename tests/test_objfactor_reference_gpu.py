"""The HIP line, box and instance factors (dv_line_eval, dv_line_plus, dv_box_enclose_eval, dv_box_dims_eval, dv_box_orientation_eval, dv_inst_proj_eval:
be_obj.hip, be_obj_dev.h) against the float64 restatement of tests/objfactor_ref.py, which tests/test_objfactor_reference.py validates without a GPU, on the
edge cases of tests/objfactor_cases.py (each proven there to reach the branch it is named for).
  (a) every case: |device - reference| <= K eps magnitude entry by entry, structurally zero entries exactly 0.0, the non-finite pattern equal; K_LINE ... K_INST
      are ten times the largest restatement-vs-oracle ratio (tests/test_objfactor_reference.py).  No case is left out.
  (b) launch shape: n in {1, 63, 64, 65, 129}, the case list rotated so that every case sits at every index: the record of a case is bit-identical wherever it
      sits; one direct call per entry with 64 sentinel doubles on either side of the output, which come back untouched.
  (c) dv_line_solve with max_iters = 0 on the scene built from the line cases (all but phi0; solved in one part per distinct extrinsic and sqrt_info, the
      case's pose in its own frame slot): initial_cost within K_EVAL = 1e3 eps of 0.5 sum |rho| of the restatement's residuals.
Measured on the MI355X, ratios in eps of the magnitude: (bars: line 0.3, line_plus 5, box_enclose 4, box_dims 0, box_orientation 0.3, inst_proj 0.5)
    line   benign0 0.014; benign_asym 0.0088; benign_zero_info 0; quadrant1-4 0.0092 0.019 0.017 0.0090; phi1e-3 0.019; phi1e-6 0.012; phi_half_pi-1e-3 0.013
           phi_half_pi-1e-6 0.0098; phi0 0.0070; theta2+ 0.0062; theta2- 0.0056; l1e-3 0.0039; l1e-6 0.0033; far1e3 0.015; ex_identity 0.020; qnorm+- 0.013; qnorm-+ 0.0049
    plus   zero 0 0 0.060; big 0.19 0 0.22 0.42; euler_over+ 0; euler_over- 0.065; the four folds 0.30; past_fold+ 0.12; past_fold- 0.24; u1z_1-1e-12 0.087; the three cuts 0
    box    inside 0.34; out_y 0.086; e+-- 0.18; e-++ 0.17; dims1e-3 0.24; the other 25 cases 0 (bit-identical to the restatement)
    dims   all six cases 0
    ori    angle0 0; angle1e-12 0.012; angle1e-9 0.010; angle1e-6 0.0078; angle0.001 0.026; angle1 0.0096; angle3 0.0039; pi-1e-3 0.015; pi-1e-6 0.014; pi_w_branch 0.0031
           qfromR small 0.012, x179 0.012, y179 0.020, z179 0.0059; w_negative 0.0051; qnorm+- 0.0032; qnorm-+ 0.011
    inst   benign 0.016 0.020 0.0049; front1e-3 3.3e-6; depth0.2 0.014; depth1 0.020; depth10 0.011; depth200 0.043; td0 0.0076; td0.05 0.029; same_obj 0.016
           same_body 0.022; ex_identity 0.029; qnorm+- 0.013; qnorm-+ 0.016; shift1e3 0.0010
    What these bars reject (a negated or zeroed Jacobian in every case, a relative 1e-9 in all but four) is asserted in tests/test_objfactor_reference.py (e).
    (b)    bit-identical at every index for every n; the sentinels untouched.
    (c)    see the test's docstring."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import factor_ref as fr
from tests.test_objfactor_reference import ALL, ALL_IDS, CASES, FAMILIES, K, case_ratio, references

pytestmark = pytest.mark.gpu
K_EVAL = 1e3          # the bar tests/test_bd_reference_gpu.py holds the same quantity to

STRIDE = dict(line=34, plus=4, box=21, dims=4, ori=39, inst=64)
ENTRY = dict(line="dv_line_eval", plus="dv_line_plus", box="dv_box_enclose_eval", dims="dv_box_dims_eval", ori="dv_box_orientation_eval", inst="dv_inst_proj_eval")


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=64, height=48)


def inputs(fam, cases):
    """the host arrays of a batch, in the order of the entry's arguments (n goes where the ABI has it)"""
    from dynamic_vins_amd import backend as B
    from tests.objfactor_cases import inst_arrays
    col = lambda k: np.ascontiguousarray(np.array([c[k] for c in cases], np.float64))
    if fam == "line":
        f = np.zeros(len(cases), B.LINE_DTYPE)
        f["obs"], f["sqrt_info"] = col("obs"), col("si")
        return [f, col("pose"), col("ex"), col("orth")]
    if fam == "plus":
        return [col("orth"), col("delta")]
    if fam == "box":
        f = np.zeros(len(cases), B.BOXPT_DTYPE)
        f["pts_w"], f["dims"] = col("p_w"), col("dims")
        return [f, col("pose_obj")]
    if fam == "dims":
        return [col("dims"), col("box")]
    if fam == "ori":
        return [col("R_cioi"), col("R_bc"), col("pose_body"), col("pose_obj")]
    fac, blocks = inst_arrays(cases)
    return [fac] + [np.ascontiguousarray(b, np.float64) for b in blocks]


def device(ctx, fam, cases):
    """flat records [n, stride] through the backend's entry"""
    from dynamic_vins_amd import backend as B
    a, n = inputs(fam, cases), len(cases)
    if fam == "line":
        return np.hstack([x.reshape(n, -1) for x in B.line_eval(ctx, *a)])
    if fam == "plus":
        return B.line_plus(ctx, *a)
    if fam == "box":
        return np.hstack([x.reshape(n, -1) for x in B.box_enclose_eval(ctx, *a)])
    if fam == "dims":
        return np.hstack([x.reshape(n, -1) for x in B.box_dims_eval(ctx, *a)])
    if fam == "ori":
        return np.hstack([x.reshape(n, -1) for x in B.box_orientation_eval(ctx, *a)])
    return B.inst_proj_eval(ctx, *a)


def direct(ctx, fam, cases, out):
    """the entry itself on a caller's output pointer"""
    a, n = inputs(fam, cases), len(cases)
    p = [C.c_void_p(x.ctypes.data) for x in a]
    args = p + [n] if fam in ("plus", "dims", "ori") else [p[0], n] + p[1:]          # n follows the factor records, or the inputs where there are none
    return getattr(ctx.lib, ENTRY[fam])(ctx.h, *args, C.c_void_p(out))


@pytest.fixture(scope="module")
def base(ctx):
    return {fam: device(ctx, fam, CASES[fam]) for fam in FAMILIES}


@pytest.mark.parametrize("fam,c", ALL, ids=ALL_IDS)
def test_device_matches_reference(base, fam, c):
    """(a)"""
    k = next(i for i, x in enumerate(CASES[fam]) if x is c)
    with np.errstate(all="ignore"):
        ra = case_ratio(fam, base[fam][k], references(fam, c))
    print(f"\n[gpu] {fam} {c['name']} {ra:.3g}")
    if fam == "dims" and c["name"] == "equal":
        assert not base[fam][k].any()
    assert ra <= K[fam], ra


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("fam", FAMILIES)
def test_result_does_not_depend_on_the_launch_shape(ctx, base, fam):
    """(b): with every rotation of the list each case sits at every index below n, 0, 63, 64 and n - 1 among them"""
    cases, want = CASES[fam], _bits(base[fam])
    m = len(cases)
    for n in (1, 63, 64, 65, 129):
        for off in range(m):
            idx = (np.arange(n) + off) % m
            got = _bits(device(ctx, fam, [cases[i] for i in idx]))
            assert got.shape == (n, STRIDE[fam])
            bad = np.nonzero((got != want[idx]).any(axis=1))[0]
            assert len(bad) == 0, (n, off, bad[:5], [cases[i]["name"] for i in idx[bad[:5]]])


@pytest.mark.parametrize("fam", FAMILIES)
def test_output_is_written_inside_its_bounds(ctx, base, fam):
    """(b): 64 sentinel doubles on either side of the output buffer come back untouched"""
    cases = CASES[fam]
    n, s, sentinel = len(cases), STRIDE[fam], -1.2345678e300
    buf = np.full(n * s + 128, sentinel)
    assert direct(ctx, fam, cases, buf.ctypes.data + 64 * 8) == 0
    assert np.all(buf[:64] == sentinel) and np.all(buf[64 + n * s:] == sentinel)
    assert np.array_equal(_bits(buf[64:64 + n * s].reshape(n, s)), _bits(base[fam]))


def line_scenes():
    """the line cases but phi0, grouped by (extrinsic, sqrt_info) into LineProblems: line k of a scene is seen once, in frame k, which holds the case's pose"""
    groups = {}
    for c in CASES["line"]:
        if c["name"] != "phi0":
            groups.setdefault((c["ex"].tobytes(), c["si"].tobytes()), []).append(c)
    out = []
    for g in groups.values():
        out += [g[i:i + 11] for i in range(0, len(g), 11)]
    return out


def test_line_solve_evaluates_the_same_residuals(ctx, base, oracle):
    """(c).  A LineProblem has one extrinsic and one sqrt_info, the case list has several: the scene is solved in parts (line_scenes) and its cost is their sum.
      whole scene  |sum of initial_cost - 0.5 sum rho| <= K_EVAL eps 0.5 sum |rho| over all cases but phi0: the issue's check.
      every part   the same bar on the part's own cost, plus ten times what the CPU oracle's residuals (dvo_line_eval) give against the restatement's on that
                   part: the disagreement of two independent float64 evaluations, the rule every K of this module comes from.  rho = log(1 + |r|^2) has no
                   magnitude of its own for what r lost before it: with l_sqrt / |n_c| = 1e-6 the components of n_c under the root are what six digits of
                   cancellation leave, and r carries 8.4e4 eps relative in the oracle and the restatement alike (3e2 in l1e-3 and far1e3, 0 elsewhere).
    Measured on the MI355X, in eps of 0.5 sum |rho|: whole scene 668 (cost 125.389); parts: l1e-6 4.2e3 (oracle against restatement 4.2e3),
    far1e3 63 (63), l1e-3 7.4 (17), the other 16 parts 0 (0).
    The solve's cost equals the cost of dv_line_eval's own residuals bit for bit on 18 parts (0.78 eps on far1e3): line_orth_dev is line_eval_kernel's arithmetic."""
    from dynamic_vins_amd.backend import LINEOBS_DTYPE, LineProblem, line_solve
    from tests import obj_gen as G, objfactor_ref as R
    scenes = line_scenes()
    assert sum(len(g) for g in scenes) == len(CASES["line"]) - 1
    index = {c["name"]: k for k, c in enumerate(CASES["line"])}
    half_rho = lambda r: 0.5 * np.log1p(float(r @ r))
    bad, dev_total, ref_total, mag_total = {}, [], [], []
    for g in scenes:
        pose = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (11, 1))
        obs = np.zeros(len(g), LINEOBS_DTYPE)
        for k, c in enumerate(g):
            pose[k] = c["pose"]
            obs[k] = (k, k, c["obs"])
        ref = [half_rho(R.line_factor(c["obs"], c["si"], c["pose"], c["ex"], c["orth"])[0].v) for c in g]
        orc = [half_rho(G.o_line(oracle.lib, c["obs"], c["si"], c["pose"], c["ex"], c["orth"])[0]) for c in g]
        own = sum(half_rho(base["line"][index[c["name"]], :2]) for c in g)          # from dv_line_eval's residuals
        s = line_solve(ctx, LineProblem(np.array([c["orth"] for c in g]), pose, g[0]["ex"], g[0]["si"], obs, max_iters=0))
        cost, mag, between = float(np.sum(ref)), float(np.sum(np.abs(ref))), abs(float(np.sum(orc)) - float(np.sum(ref)))
        err = abs(s.initial_cost - cost)
        unit = fr.EPS * mag if mag > 0 else 1.0
        name = "+".join(c["name"] for c in g)
        print(f"\n[cost] {name} cost {cost:.6g} ratio {err / unit:.3g} (oracle against restatement {between / unit:.3g}; solve against dv_line_eval's own residuals {abs(s.initial_cost - own) / unit:.3g})")
        if err > K_EVAL * fr.EPS * mag + 10.0 * between:
            bad[name] = err / unit
        dev_total.append(s.initial_cost); ref_total.append(cost); mag_total.append(mag)
    total = abs(math.fsum(dev_total) - math.fsum(ref_total)) / (fr.EPS * math.fsum(mag_total))
    print(f"\n[cost] whole scene: cost {math.fsum(ref_total):.6g} ratio {total:.3g}")
    assert total <= K_EVAL, total
    assert not bad, bad
