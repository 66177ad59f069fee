"""tests/ba_ref.py — the plain float64 restatement of the window solve that tests/test_ba_reference_gpu.py holds the HIP kernels to — checked without a GPU:
its cost against the oracle's, its gradient against central differences of its own cost, its first Gauss-Newton step against one oracle iteration and its
marginalization against the oracle's (to the tolerances of tests/test_back_parity.py::test_marginalization_matches_oracle)."""
import numpy as np
import pytest

from tests import ba_gen, ba_ref

FREE = dict(feat_vel=True, td_true=0.01, ex_noise=(0.01, 0.005), prior_ex_scale=1.0, prior_ex_offset=0.01)

COST_CASES = [dict(seed=61, use_imu=0, nframes=6, nlm=60), dict(seed=62, nframes=7, nlm=60, with_prior=True), dict(seed=63, nlm=80, with_prior=True, outlier_ratio=0.3),
              dict(seed=64, use_imu=0, nlm=60, with_prior=True, plane_kind=2), dict(seed=65, nlm=60, with_prior=True, free_blocks=3, **FREE)]


@pytest.mark.parametrize("kw", COST_CASES, ids=[str(i) for i in range(len(COST_CASES))])
def test_reference_cost_equals_the_oracle_initial_cost(oracle, kw):
    prob = ba_gen.make_window(oracle, max_iters=1, **kw)
    ref = ba_ref.System(oracle, prob)
    s = ba_gen.oracle_solve(oracle, prob.clone())
    assert abs(ref.cost - s.initial_cost) <= 1e-12 * s.initial_cost, (ref.cost, s.initial_cost)


def _perturb(prob, key, k, h):
    kind, idx = key
    e = np.zeros(ba_ref.LOCAL[kind])
    e[k] = h
    if kind == "pose":
        prob.pose[idx] = ba_ref.pose_plus(prob.pose[idx], e)
    elif kind == "ex":
        prob.ex_pose[idx] = ba_ref.pose_plus(prob.ex_pose[idx], e)
    elif kind == "sb":
        prob.speed_bias[idx, k] += h
    elif kind == "td":
        prob.td[0] += h
    else:
        prob.inv_depth[idx] += h


FD_CASES = [dict(seed=71, nframes=5, nlm=25, with_prior=True, outlier_ratio=0.3, free_blocks=3, **FREE),
            dict(seed=72, nframes=6, nlm=25, use_imu=0, with_prior=True, free_blocks=3, **FREE)]


@pytest.mark.parametrize("kw", FD_CASES, ids=["vio", "vo"])
def test_reference_gradient_matches_central_differences(oracle, kw):
    """g = J^T r of the reference against central differences of its own cost in every free column: poses (the prior's rotation blocks included), speed-biases,
    extrinsics, td, inverse depths.  The IMU factors are evaluated at their pre-integration's linearisation biases: the factor's bias Jacobian of the rotation
    residual is exact only there (IMUFactor::Evaluate uses delta_q, not the bias-corrected one).  Likewise the prior's Jacobian is J0 on the local coordinates
    (MarginalizationFactor), the derivative of its rotation dx only where q0^-1 q = 1: the prior's rotations are linearised at the states, its positions, speed-biases
    and td are not, so A dx still reaches the rotation columns."""
    prob = ba_gen.make_window(oracle, **kw)
    for rec in prob.imu:
        rec["lin_ba"], rec["lin_bg"] = prob.speed_bias[rec["fi"], 3:6], prob.speed_bias[rec["fi"], 6:9]
    for i, (key, _, _, x0) in enumerate(ba_ref.prior_blocks(prob)):
        if len(x0) == 7:
            for j in range(3, 7):
                prob.prior.x0[i][j] = ba_ref.state_of(prob, key)[j]
    ref = ba_ref.System(oracle, prob)
    in_prior = {k for k, _, _, _ in ba_ref.prior_blocks(prob)}
    assert ("ex", 1) in in_prior and ("td", 0) in in_prior and np.abs(ba_ref.prior_dx(prob)).max() > 0
    h = 1e-6
    worst = 0.0
    for key, c in ref.all_cols.items():
        for k in range(ba_ref.LOCAL[key[0]]):
            val = []
            for sgn in (1.0, -1.0):
                q = prob.clone()
                _perturb(q, key, k, sgn * h)
                v = sum(rb.cost for rb in ba_ref.residuals(oracle, q, only=key))
                if key in in_prior:
                    v += ba_ref.prior_cost(q, with_c0=False)
                val.append(v)
            fd = (val[0] - val[1]) / (2 * h)
            err = abs(fd - ref.g[c + k]) / (ref.gmag[c + k] + 1.0)
            worst = max(worst, err)
            assert err <= 1e-6, (key, k, fd, ref.g[c + k], ref.gmag[c + k])
    print(f"worst |fd - g| / (|J|^T|r| + 1) = {worst:.2e}")


LOW = dict(pose_noise=(0.003, 0.001), sb_noise=0.1)          # a VIO window whose first step is the Gauss-Newton one (|d y| inside the initial radius 1e4)
STEP_CASES = [dict(seed=81, use_imu=0, nframes=8, nlm=80), dict(seed=134, nframes=4, with_prior=True, prior_scale=1000.0, **LOW),
              dict(seed=83, use_imu=0, nlm=100, with_prior=True, outlier_ratio=0.2)]


@pytest.mark.parametrize("kw", STEP_CASES, ids=["vo", "vio_prior", "huber"])
def test_reference_step_matches_one_oracle_iteration(oracle, kw):
    """the dense step applied to the states == the oracle's states after one accepted iteration, to 1e-9.  Only on windows whose scaled, regularized system has
    a condition number <= 1e6 (asserted): a VIO window without a prior keeps 4 gauge directions that only mu = 1e-8 pins, along which two correct solvers differ
    by far more.  The step must also lie inside the initial trust region (1e4), or the oracle's step is not the Gauss-Newton one."""
    prob = ba_gen.make_window(oracle, max_iters=1, **kw)
    ref = ba_ref.System(oracle, prob)
    st = ref.step()
    assert st["cond"] <= 1e6 and st["dnorm"] <= 1e4, (st["cond"], st["dnorm"])
    if kw.get("outlier_ratio"):          # some blocks take Huber's outer branch (there the corrected 0.5 |r|^2 = 0.5 sqrt(s) differs from the cost sqrt(s) - 0.5)
        assert any(abs(rb.cost - 0.5 * float(rb.r @ rb.r)) > 1e-9 for rb in ba_ref.residuals(oracle, prob))
    mine = ref.apply(st["delta"])
    q = prob.clone()
    s = ba_gen.oracle_solve(oracle, q)
    assert s.iterations == 1 and s.successful == 1
    for a, b in ((mine.pose, q.pose), (mine.speed_bias, q.speed_bias), (mine.inv_depth, q.inv_depth)):
        assert np.abs(a - b).max() <= 1e-9, np.abs(a - b).max()
    print(f"cond {st['cond']:.3g}  |dy| {st['dnorm']:.3g}  max state diff {max(np.abs(mine.pose - q.pose).max(), np.abs(mine.inv_depth - q.inv_depth).max()):.2e}")


MARG_CASES = [(dict(seed=21, with_prior=True), 0), (dict(seed=23, with_prior=True), 1), (dict(seed=24, with_prior=True, use_imu=0), 0),
              (dict(seed=91, use_imu=0, with_prior=True), 1), (dict(seed=92, with_prior=True, plane_kind=1), 0),
              (dict(seed=93, with_prior=True, free_blocks=3, **FREE), 0), (dict(seed=22), 0)]


@pytest.mark.parametrize("kw,mode", MARG_CASES, ids=[str(i) for i in range(len(MARG_CASES))])
def test_reference_marginalization_matches_oracle(oracle, kw, mode):
    full = ba_gen.make_window(oracle, **kw)
    ba_gen.oracle_solve(oracle, full)
    sub = ba_gen.marg_subproblem(full, mode)
    po, Ao, bo = ba_gen.oracle_marginalize(oracle, sub, mode)
    r = ba_ref.marginalize(oracle, sub, mode)
    bo_blocks = ba_gen.prior_to_dict(po, Ao, bo)
    assert po.valid == 1 and po.n == r["n"] and set(bo_blocks) == set(r["blocks"])
    for k in bo_blocks:
        assert bo_blocks[k][1] == r["blocks"][k][1] and np.array_equal(bo_blocks[k][2], r["blocks"][k][2])
    Ar, br = ba_gen.permute_prior(r["blocks"], r["A"], r["b"], bo_blocks)
    scale = np.abs(Ao).max()
    assert np.allclose(Ar, Ao, rtol=0, atol=1e-9 * scale + 1e-6), np.abs(Ar - Ao).max() / scale
    assert np.allclose(br, bo, rtol=0, atol=1e-9 * np.abs(bo).max() + 1e-6), np.abs(br - bo).max()
    assert np.isclose(r["c0"], po.c0, rtol=1e-6), (r["c0"], po.c0)


def _sqrt_info_gauss_jordan(cov):
    """U with U^T U = cov^-1 formed as csrc/be_api.hip:imu_sqrt_info forms it (Gauss-Jordan with partial pivoting, symmetrised, Cholesky): another correct float64 whitening"""
    a = np.hstack([cov, np.eye(15)])
    for c in range(15):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        a[[c, p]] = a[[p, c]]
        a[c] /= a[c, c]
        for i in range(15):
            if i != c and a[i, c] != 0.0:
                a[i] -= a[i, c] * a[c]
    return np.linalg.cholesky(0.5 * (a[:, 15:] + a[:, 15:].T)).T


@pytest.mark.parametrize("kw", [dict(seed=281, nlm=0, with_prior=True, prior_scale=3000.0), dict(seed=287, free_blocks=1, with_prior=True, feat_vel=True, prior_ex_scale=1.0),
                                dict(seed=271, nframes=11)], ids=["imu_prior_only", "free_ex", "vio"])
def test_magnitude_model_covers_another_imu_whitening(oracle, kw):
    """Where the IMU entries of the reduced system lose their digits: the information matrix W = cov^-1 (cond(cov) ~5e5) that whitens the factor.  Whitened
    with the Gauss-Jordan sqrt_info of be_api.hip instead of the oracle's, H moves by thousands of eps |J|^T|J| — as far as dv_ba_eval's S sits from the reference
    on IMU-dominated windows — but by a few eps of the magnitude model of ba_ref.imu_residual, which adds eps |J_raw|^T |W||cov||W| |J_raw| to |J|^T|J|."""
    p = ba_gen.make_window(oracle, **kw)
    ref = ba_ref.System(oracle, p)
    res = ba_ref.residuals(oracle, p)
    for rb, rec in zip(res, p.imu):
        cov = np.asarray(rec["covariance"]).reshape(15, 15)
        T = _sqrt_info_gauss_jordan(cov) @ np.linalg.inv(np.linalg.cholesky(np.linalg.inv(cov)).T)
        rb.r, rb.blocks = T @ rb.r, [(k, T @ J) for k, J in rb.blocks]
    H2, g2 = ba_ref.assemble(res, ref.all_cols, ref.N, ba_ref._prior_terms(p))[1:3]
    plain = ba_ref.residuals(oracle, p)
    for rb in plain:
        rb.mag = None
    Hm0 = ba_ref.assemble(plain, ref.all_cols, ref.N, ba_ref._prior_terms(p))[3]
    m, mg = ref.Hmag > 0, ref.gmag > 0
    dH = np.abs(H2 - ref.H)[m]
    r_model, r_plain = (dH / (ba_ref.EPS * ref.Hmag[m])).max(), (dH / (ba_ref.EPS * Hm0[m])).max()
    r_g = (np.abs(g2 - ref.g)[mg] / (ba_ref.EPS * ref.gmag[mg])).max()
    print(f"dH / eps: {r_model:.3g} of the model, {r_plain:.3g} of |J|^T|J|; dg {r_g:.3g}")
    assert r_plain > 1e3 and r_model <= 10 and r_g <= 10
