"""The HIP window solve against the dense float64 reference of tests/ba_ref.py (validated without a GPU by tests/test_ba_reference.py), over one sweep of windows:
VO and VIO at every window size the estimator builds while the window fills (nframes 4..11: n = 18..60 without IMU, right-hand-side row in a tile of its own at
n = 48; n = 60..165 with IMU), each with and without a prior, plus no / one / 1000 landmarks, Huber outliers, both plane constraints and free extrinsic / td blocks
(n up to 178: the generic factorisation).
  (a) dv_ba_eval's reduced camera system S, g and cost against the dense Schur complement, entry by entry within K_EVAL = 1e3 eps of the entry's magnitude
      accumulation (tests/ba_ref.py: |J|^T|J|, |J|^T|r| through the elimination; for the IMU factor also its whitening and its information matrix cov^-1, whose
      computation from the covariance (cond ~5e5) alone moves H by thousands of eps |J|^T|J| — tests/test_ba_reference.py::test_magnitude_model_covers_another_imu_whitening).
  (b) one iteration of dv_ba_solve in both LDL^T forms (MF16 and "ldl_generic"): the step recovered from the states solves the reference's scaled, regularized
      full system with a normwise backward error <= 1e-11, and equals the reference step to 1e-8 on every window of QUALIFY (all but the VIO windows without a
      prior, whose 4 gauge directions only mu = 1e-8 pins): there the condition number of that system is asserted <= 1e6.
  (c) eight iterations: MF16, generic and oracle agree (as tests/test_back_parity.py::test_mfma16_factorisation_agrees_with_the_generic_form) at every size.
  (d) dv_marginalize (DV_MARG_INFO and DV_MARG_EIGEN) against the dense marginalization.
The VIO windows start closer to the truth than ba_gen's defaults (LOW) so that the first step is the Gauss-Newton one, inside the initial trust region 1e4 (what
remains, |d y| ~4e3 - 9e3, comes from the speed-bias directions the IMU data pull on and does not shrink with the state noise); their priors are firm enough
(prior_scale 3000) to pin the gauge directions: condition numbers ~1e5.
Measured on the MI355X (ratios in eps of the magnitude; backward error; |y - y_ref| / |y_ref|):
    vo4(n=18) S 149 g 99 c 25 | be 1e-14 dy 4e-14; vo4p(n=18) S 76 g 73 c 35 | be 8e-15 dy 3e-14; vio4(n=60) S 91 g 116 c 0 | be 3e-15 dy 3e-09
    vio4p(n=60) S 44 g 13 c 1 | be 6e-15 dy 5e-12; vo5(n=24) S 216 g 47 c 22 | be 3e-15 dy 1e-13; vo5p(n=24) S 201 g 15 c 10 | be 2e-15 dy 1e-14
    vio5(n=75) S 33 g 4 c 0 | be 4e-15 dy 5e-09; vio5p(n=75) S 133 g 58 c 0 | be 3e-15 dy 2e-12; vo6(n=30) S 60 g 14 c 5 | be 3e-15 dy 2e-13
    vo6p(n=30) S 49 g 37 c 5 | be 4e-15 dy 1e-14; vio6(n=90) S 110 g 1 c 0 | be 4e-15 dy 9e-09; vio6p(n=90) S 150 g 46 c 0 | be 3e-15 dy 2e-12
    vo7(n=36) S 240 g 16 c 8 | be 2e-15 dy 2e-13; vo7p(n=36) S 56 g 10 c 3 | be 1e-15 dy 1e-14; vio7(n=105) S 50 g 15 c 0 | be 3e-15 dy 1e-08
    vio7p(n=105) S 82 g 22 c 0 | be 5e-15 dy 2e-12; vo8(n=42) S 130 g 44 c 9 | be 3e-15 dy 1e-13; vo8p(n=42) S 61 g 16 c 0 | be 1e-15 dy 2e-14
    vio8(n=120) S 84 g 17 c 0 | be 2e-15 dy 5e-09; vio8p(n=120) S 179 g 5 c 0 | be 2e-15 dy 6e-12; vo9(n=48) S 232 g 111 c 4 | be 5e-15 dy 8e-14
    vo9p(n=48) S 131 g 20 c 7 | be 5e-15 dy 2e-14; vio9(n=135) S 181 g 3 c 0 | be 4e-15 dy 4e-09; vio9p(n=135) S 107 g 2 c 0 | be 5e-15 dy 2e-12
    vo10(n=54) S 253 g 36 c 21 | be 8e-15 dy 7e-14; vo10p(n=54) S 118 g 30 c 5 | be 3e-15 dy 1e-14; vio10(n=150) S 144 g 16 c 0 | be 3e-15 dy 7e-09
    vio10p(n=150) S 287 g 57 c 1 | be 3e-15 dy 3e-12; vo11(n=60) S 286 g 58 c 1 | be 8e-15 dy 1e-13; vo11p(n=60) S 71 g 16 c 2 | be 3e-15 dy 1e-14
    vio11(n=165) S 240 g 3 c 0 | be 3e-15 dy 6e-09; vio11p(n=165) S 122 g 12 c 0 | be 3e-15 dy 2e-12; nlm0p(n=165) S 12 g 137 c 0 | be 1e-15 dy 3e-12
    nlm1(n=165) S 705 g 2 c 0 | be 4e-15 dy 2e-08; nlm1000p(n=165) S 82 g 11 c 3 | be 2e-15 dy 1e-12; huber(n=165) S 141 g 3 c 0 | be 4e-15 dy 2e-12
    plane1(n=165) S 198 g 15 c 1 | be 3e-15 dy 4e-12; plane2(n=60) S 76 g 12 c 9 | be 2e-15 dy 2e-14; free1(n=177) S 875 g 204 c 1 | be 2e-15 dy 4e-12
    free2(n=166) S 317 g 47 c 0 | be 2e-15 dy 3e-12; free3(n=178) S 261 g 121 c 0 | be 5e-15 dy 2e-12
"""
import numpy as np
import pytest

from tests import ba_gen, ba_ref
from tests.conftest import iterations_agree

pytestmark = pytest.mark.gpu

LOW = dict(pose_noise=(0.002, 0.0007), sb_noise=0.0, prior_x0_noise=0.0003)
PRIOR = dict(with_prior=True, prior_scale=3000.0)
FREE = dict(with_prior=True, feat_vel=True, td_true=0.01, ex_noise=(0.01, 0.005), prior_ex_scale=1.0, prior_ex_offset=0.01)
FREE_LOW = dict(FREE, td_true=0.001, ex_noise=(0.001, 0.0005), prior_ex_offset=0.001, prior_scale=3000.0)
K_EVAL = 1e3

SWEEP = {}
for _nf in range(4, 12):
    SWEEP[f"vo{_nf}"] = dict(seed=200 + _nf, use_imu=0, nframes=_nf)
    SWEEP[f"vo{_nf}p"] = dict(seed=220 + _nf, use_imu=0, nframes=_nf, with_prior=True)
    SWEEP[f"vio{_nf}"] = dict(seed=240 + _nf, nframes=_nf, **LOW)
    SWEEP[f"vio{_nf}p"] = dict(seed=260 + _nf, nframes=_nf, **PRIOR, **LOW)
SWEEP.update({
    "nlm0p": dict(seed=281, nlm=0, **PRIOR, **LOW), "nlm1": dict(seed=282, nlm=1, **LOW), "nlm1000p": dict(seed=283, nlm=1000, **PRIOR, **LOW),
    "huber": dict(seed=284, outlier_ratio=0.1, **PRIOR, **LOW), "plane1": dict(seed=285, plane_kind=1, **PRIOR, **LOW),
    "plane2": dict(seed=286, use_imu=0, plane_kind=2, with_prior=True), "free1": dict(seed=287, free_blocks=1, **FREE_LOW, **LOW),
    "free2": dict(seed=288, free_blocks=2, **FREE_LOW, **LOW), "free3": dict(seed=289, free_blocks=3, **FREE_LOW, **LOW)})
QUALIFY = [n for n in SWEEP if not (n.startswith("vio") and not n.endswith("p")) and n != "nlm1"]      # the forward check of (b) must run on these


@pytest.fixture(scope="module")
def ctxs(gpu_ctx_factory):
    mf16, gen = gpu_ctx_factory(width=64, height=48), gpu_ctx_factory(width=64, height=48)
    assert gen.lib.dv_debug_set(gen.h, b"ldl_generic", 1) == 0
    return mf16, gen


def _window(oracle, name, **kw):
    """the sweep window `name`.  ba_gen's prior A = P (M^T M) P is symmetric only to its rounding (up to ~5e3 eps |A_ij| at prior_scale 3000), and the kernels read
    one triangle or the other: A is replaced by its symmetric part, which the oracle and the prior's c0 (dvo_prior_c0) use anyway."""
    prob = ba_gen.make_window(oracle, **dict(SWEEP[name], **kw))
    if prob.prior is not None:
        prob.prior_A = np.ascontiguousarray(0.5 * (prob.prior_A + prob.prior_A.T))
        prob._bind()
    return prob


def _ratio(dev, ref, mag):
    """max |dev - ref| / (eps mag); an entry without magnitude (no contribution) must match exactly"""
    err = np.abs(dev - ref)
    if np.any(err[mag == 0] != 0):
        return np.inf
    nz = mag > 0
    return float((err[nz] / (ba_ref.EPS * mag[nz])).max()) if nz.any() else 0.0


@pytest.mark.parametrize("name", list(SWEEP))
def test_reduced_system_matches_reference(ctxs, oracle, name):
    """(a) S, g, cost of dv_ba_eval vs the dense reference within K_EVAL eps of the magnitude accumulations."""
    from dynamic_vins_amd.backend import ba_eval
    prob = _window(oracle, name)
    cost, S, g = ba_eval(ctxs[0], prob)
    ref = ba_ref.System(oracle, prob)
    Sr, gr, Sm, gm = ref.reduced()
    assert S.shape == Sr.shape
    rs, rg, rc = _ratio(S, Sr, Sm), _ratio(g, gr, gm), abs(cost - ref.cost) / (ba_ref.EPS * ref.cost_mag)
    print(f"\n[eval] {name} n={ref.np} S {rs:.3g} g {rg:.3g} cost {rc:.3g}")
    assert rs <= K_EVAL and rg <= K_EVAL and rc <= K_EVAL, (rs, rg, rc)


@pytest.mark.parametrize("name", list(SWEEP))
def test_first_step_solves_the_reference_system(ctxs, oracle, name):
    """(b) one dv_ba_solve iteration, MF16 and generic: accepted, backward error <= 1e-11 in the reference's scaled regularized system, and the reference step
    to 1e-8 (landmarks included) on the QUALIFY windows, whose system must have a condition number <= 1e6.  A translation component a plane constraint drops is not in the states:
    it is taken as the value that minimises the residual."""
    from dynamic_vins_amd.backend import ba_solve
    prob = _window(oracle, name, max_iters=1)
    ref = ba_ref.System(oracle, prob)
    st = ref.step()
    assert st["dnorm"] <= 1e4, st["dnorm"]                # the solver's first step is the Gauss-Newton step
    if name in QUALIFY:
        assert st["cond"] <= 1e6, st["cond"]
    pc = ref.plane_columns()
    keep = np.setdiff1d(np.arange(ref.N), pc)
    for form, c in zip(("mf16", "generic"), ctxs):
        dev = prob.clone()
        s = ba_solve(c, dev)
        assert s.iterations == 1 and s.successful == 1, (form, s.iterations, s.successful)
        y = ref.recover(prob, dev) / st["scale"]
        if pc:
            r = st["A"][:, keep] @ y[keep] + st["b"]
            y[pc] = np.linalg.lstsq(st["A"][:, pc], -r, rcond=None)[0]
        be = ba_ref.backward_error(st["A"], st["b"], y)
        dy = np.linalg.norm(y[keep] - st["y"][keep]) / np.linalg.norm(st["y"][keep])
        print(f"\n[step] {name} {form} n={ref.np} N={ref.N} cond {st['cond']:.3g} backward {be:.3g} |y - y_ref| / |y_ref| {dy:.3g}")
        assert be <= 1e-11, (form, be)
        if name in QUALIFY:
            assert dy <= 1e-8, (form, dy)


@pytest.mark.parametrize("name", list(SWEEP))
def test_full_solve_forms_agree(ctxs, oracle, name):
    """(c) eight iterations: MF16 == generic to rounding (same decisions, states 1e-9), both == the oracle (states 1e-6)"""
    from dynamic_vins_amd.backend import ba_solve
    ref = _window(oracle, name, max_iters=8)
    a, b = ref.clone(), ref.clone()
    so = ba_gen.oracle_solve(oracle, ref)
    sa, sb = ba_solve(ctxs[0], a), ba_solve(ctxs[1], b)
    assert (sa.iterations, sa.successful, sa.termination) == (sb.iterations, sb.successful, sb.termination)
    assert iterations_agree(sa, so) and sa.termination == so.termination, (sa.iterations, so.iterations)
    assert abs(sa.final_cost - sb.final_cost) <= 1e-10 * abs(sb.final_cost) + 1e-12
    for x, y in ((a.pose, b.pose), (a.speed_bias, b.speed_bias), (a.inv_depth, b.inv_depth), (a.ex_pose, b.ex_pose), (a.td, b.td)):
        assert x.size == 0 or np.abs(x - y).max() < 1e-9, np.abs(x - y).max()
    assert np.abs(a.pose - ref.pose).max() < 1e-6 and (a.inv_depth.size == 0 or np.abs(a.inv_depth - ref.inv_depth).max() < 1e-6)
    assert np.abs(a.speed_bias - ref.speed_bias).max() < 1e-6
    assert np.abs(a.ex_pose - ref.ex_pose).max() < 1e-6 and abs(a.td[0] - ref.td[0]) < 1e-6


MARG = {"vio_m0": (dict(seed=301, with_prior=True), 0, "info"), "vio_m1": (dict(seed=302, with_prior=True), 1, "info"),
        "vo_m0": (dict(seed=303, use_imu=0, with_prior=True), 0, "info"), "vo_m1": (dict(seed=304, use_imu=0, with_prior=True), 1, "info"),
        "vio_noprior_m0": (dict(seed=22), 0, "info"), "plane1_m0": (dict(seed=305, with_prior=True, plane_kind=1), 0, "info"),
        "plane2_m0": (dict(seed=306, use_imu=0, with_prior=True, plane_kind=2), 0, "info"),
        "free_ex_td_m0": (dict(seed=307, free_blocks=3, **FREE), 0, "info"), "free_ex_td_m1": (dict(seed=308, free_blocks=3, **FREE), 1, "info"),
        "eig_vio_m0": (dict(seed=309, with_prior=True), 0, "eigen"), "eig_vo_m1": (dict(seed=310, use_imu=0, with_prior=True), 1, "eigen"),
        "eig_free_m0": (dict(seed=311, free_blocks=3, **FREE), 0, "eigen")}


@pytest.mark.parametrize("name", list(MARG))
def test_marginalization_matches_reference(ctxs, oracle, name):
    """(d) dv_marginalize vs the dense marginalization, block by block, with the tolerances of test_back_parity.py::test_marginalization_matches_oracle; under
    DV_MARG_EIGEN against the reference's projection onto the eigenvalues > 1e-8 of A' (and its rank, diag4[3])"""
    from dynamic_vins_amd.backend import marginalize, set_marg_form
    kw, mode, form = MARG[name]
    full = ba_gen.make_window(oracle, **kw)
    ba_gen.oracle_solve(oracle, full)                     # linearise at the optimum like the estimator does
    sub = ba_gen.marg_subproblem(full, mode)
    r = ba_ref.marginalize(oracle, sub, mode)
    ctx = ctxs[0]
    set_marg_form(ctx, form)
    try:
        pd, Ad, bd, diag = marginalize(ctx, sub, mode)
    finally:
        set_marg_form(ctx, "info")
    bd_blocks = ba_gen.prior_to_dict(pd, Ad, bd)
    assert pd.valid == 1 and pd.n == r["n"] and set(bd_blocks) == set(r["blocks"])
    for k in bd_blocks:
        assert bd_blocks[k][1] == r["blocks"][k][1] and np.array_equal(bd_blocks[k][2], r["blocks"][k][2])
    A, b = (r["A_eig"], r["b_eig"]) if form == "eigen" else (r["A"], r["b"])
    Ar, br = ba_gen.permute_prior(r["blocks"], A, b, bd_blocks)
    scale = np.abs(Ar).max()
    ea, eb = np.abs(Ad - Ar).max() / scale, np.abs(bd - br).max() / np.abs(br).max()
    print(f"\n[marg] {name} n={pd.n} A {ea:.3g} b {eb:.3g} c0 {pd.c0:.6g} / {r['c0']:.6g}")
    assert np.allclose(Ad, Ar, rtol=0, atol=1e-9 * scale + 1e-6), ea
    assert np.allclose(bd, br, rtol=0, atol=1e-9 * np.abs(br).max() + 1e-6), eb
    assert np.isclose(pd.c0, r["c0"], rtol=1e-6), (pd.c0, r["c0"])
    if form == "eigen":
        assert diag[3] == r["rank"], (diag[3], r["rank"])
