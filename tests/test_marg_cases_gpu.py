"""dv_marginalize on the crafted priors of tests/marg_cases.py (validated without a GPU by tests/test_marg_cases.py) against the dense float64 reference
tests/ba_ref.py::marginalize and, where the prior is block diagonal, against the answer known by construction.  Only the prior takes part (no factors, no IMU), so
be_marg_finish and be_marg_eig run at sizes, drop shapes and spectra no window prior has:
  (a) mode 1 at every kept size the block types can form, n = 1, 6, 7, 9, ... 89 (57 sizes), coupled SPD prior at unit norm, block order shuffled, both forms:
      A', b' within 1e-9 of their largest entry (no absolute floor), c0 to 1e-6, the new header; DV_MARG_EIGEN also rank, spectrum to 1e-11 |A'|, bitwise symmetry.
  (b) every fourth of those sizes at norm ~1e9 with the bars of tests/test_back_parity.py (1e-9 scale + 1e-6).
  (c) DV_MARG_EIGEN (and DV_MARG_INFO for A', b') on seven spectra x twelve sizes of block-diagonal priors: the clamp on negative, repeated, zero and straddling
      eigenvalues, a diagonal and a zero A', off-diagonal entries of 1e-305.
  (d) mode 0 dropping pose 0 + speed-bias 0 (m = 15), pose 0 (6), speed-bias 0 (9) at n = 7, 30, 61, 85, and a dropped block with a pivot of 1e-10.
  (e) the empty return, the size limit (refused in marg_plan with the limit of the drop size in the message) and bitwise reproducibility.
be_marg_finish factors on the matrix cores (16 wide) only in DV_MARG_INFO form and only where its tiles fit beside the LDS image (marg_args); by that formula the
mode-1 sweep runs it at n = 60 .. 63, 70 .. 79 and 82 .. 89 (first: 60) and the 4-wide panel form everywhere else (test_sweep_runs_both_factorisations);
DV_MARG_EIGEN always takes the panel form.  Largest accepted n: 89 beside 6 dropped dims, 88 beside 9, 85 beside 15.
No generated case is left out.  A wrong result does fail here: with two prior_map entries swapped in marg_plan (on a scratch build) every size of (a) fails.
Measured on the MI355X beside the session's contention filler, 176 tests in 3.2 s (worst error / bar of A', b', c0, spectrum per part and form; Jacobi sweeps min-max;
the module's `stats` fixture prints this table):
    (a) info A 7.5e-7 b 2.6e-6 c0 1.8e-9 | eigen A 1.6e-5 b 1.6e-5 c0 1.6e-8 spectrum 3.5e-4 sweeps 0-9          (57 sizes)
    (b) info A 3.4e-7 b 1.3e-6 c0 1.2e-9 | eigen A 1.6e-5 b 1.9e-5 c0 1.7e-8 spectrum 3.7e-4 sweeps 0-9          (15 sizes)
    (c) eigen: diag A 0 b 3.7e-7 c0 4.2e-10 sweeps 0 | zero all 0, sweeps 0 | two_clusters A 3.1e-5 b 3.2e-5 c0 2.8e-8 spectrum 1.5e-4 sweeps 0-22
        indefinite A 2.1e-5 b 3.5e-4 c0 2.3e-7 spectrum 1.8e-4 sweeps 0-12 | straddle A 1.6e-5 b 5.8e-3 c0 1.2e-3 spectrum 2.0e-4 sweeps 0-9
        wide A 2.0e-5 b 2.4e-5 c0 3.6e-12 spectrum 1.9e-4 sweeps 0-18 | tiny_offdiag A 4.2e-6 b 5.4e-5 c0 5.7e-8 spectrum 1.8e-4 sweeps 0
        info (A', b' only): A 0 on every spectrum (the elimination is exact on a block-diagonal prior), b <= 2.8e-6
    (d) m=15 info A 1.2e-6 b 9.6e-7 c0 3.2e-10 | eigen A 1.5e-5 b 1.7e-5 c0 1.4e-8 spectrum 2.8e-4 sweeps 5-9;  m=6 and m=9 the same within a factor 2
        null pivot (bar 1e-7): A 6.1e-3 b 1.1e-3 c0 7.3e-6 in both forms, smallest pivot 2.3e-9, spectrum (against the device's own A') 1.7e-4, sweeps 9
    (e) n = 90, 91, 93, 94, 96, 99, 120 refused in both forms with "at most 89 kept dims beside 6 dropped ones"; 87 beside 15 and 90 beside 9 refused, 85 and 88 accepted"""
import numpy as np
import pytest

from tests import ba_gen, marg_cases as mc

pytestmark = pytest.mark.gpu
EPS = mc.EPS
FORMS = ("info", "eigen")


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=64, height=48)


@pytest.fixture(scope="module")
def stats():
    s = {}
    yield s
    print("\n[marg-cases] part: worst A / b / c0 / spectrum error over its bar, sweeps min-max, cases")
    for part in sorted(s):
        v = s[part]
        print(f"[marg-cases] {part}: A {v['A']:.3g} b {v['b']:.3g} c0 {v['c0']:.3g} spectrum {v['ev']:.3g} sweeps {v['smin']}-{v['smax']} cases {v['cases']}")


def _run(ctx, prob, form):
    from dynamic_vins_amd.backend import marg_spectrum, marginalize, set_marg_form
    set_marg_form(ctx, form)
    try:
        pd, A, b, diag = marginalize(ctx, prob, prob.truth["mode"])
        ev, sweeps = marg_spectrum(ctx) if form == "eigen" and pd.valid else (None, None)
    finally:
        set_marg_form(ctx, "info")
    return dict(pd=pd, A=A, b=b, diag=diag.copy(), ev=ev, sweeps=sweeps)


def _ratio(err, bar):
    return 0.0 if err == 0 else (np.inf if bar == 0 else err / bar)


def _check(prob, out, form, stats, part, tol=1e-9, floor=0.0, c0_rtol=1e-6, c0=True, spectrum_of=None):
    """the bars of part (a): header, A', b', c0 against the reference in the device's layout; eigen form: rank, spectrum (of the reference's A', or of spectrum_of), symmetry,
    sweeps.  Returns the reference (A, b) used."""
    r, t = mc.reference(prob), prob.truth
    pd, Ad, bd, diag = out["pd"], out["A"], out["b"], out["diag"]
    blocks = ba_gen.prior_to_dict(pd, Ad, bd)
    assert pd.valid == 1 and pd.n == r["n"] == t["n"] and pd.nblocks == len(r["blocks"]) and set(blocks) == set(r["blocks"])
    for k in blocks:          # sizes, linearisation points, shifted indices; and the canonical order of the kept blocks
        assert blocks[k][1] == r["blocks"][k][1] and np.array_equal(blocks[k][2], r["blocks"][k][2]) and blocks[k][0] == t["blocks"][k][0], k
    A, b = (r["A_eig"], r["b_eig"]) if form == "eigen" else (r["A"], r["b"])
    Ar, br = ba_gen.permute_prior(r["blocks"], A, b, blocks)
    sa, sb = np.abs(Ar).max(), np.abs(br).max()
    ra, rb = _ratio(np.abs(Ad - Ar).max(), tol * sa + floor), _ratio(np.abs(bd - br).max(), tol * sb + floor)
    rc = _ratio(abs(pd.c0 - r["c0"]), c0_rtol * abs(r["c0"])) if c0 else 0.0
    rev = 0.0
    if form == "eigen":
        ref_ev = np.linalg.eigvalsh(r["A"] if spectrum_of is None else spectrum_of)
        rev = _ratio(np.abs(out["ev"] - ref_ev).max(), 1e-11 * np.abs(ref_ev).max())
    print(f"\n[marg-cases] {part} {form} n={pd.n} m={t['m']} {t['spectrum'] or 'coupled'}: A {ra:.3g} b {rb:.3g} c0 {rc:.3g} ({pd.c0:.6g} / {r['c0']:.6g}) spectrum {rev:.3g} "
          f"sweeps {out['sweeps']} rank {diag[3]:.0f} / {r['rank']} min pivot {diag[1]:.3g}")
    v = stats.setdefault(f"{part} {form}", dict(A=0.0, b=0.0, c0=0.0, ev=0.0, smin=None, smax=None, cases=0))
    v.update(A=max(v["A"], ra), b=max(v["b"], rb), c0=max(v["c0"], rc), ev=max(v["ev"], rev), cases=v["cases"] + 1)
    if form == "eigen":
        v["smin"], v["smax"] = out["sweeps"] if v["smin"] is None else min(v["smin"], out["sweeps"]), out["sweeps"] if v["smax"] is None else max(v["smax"], out["sweeps"])
    assert ra <= 1 and rb <= 1, (ra, rb)
    assert rc <= 1, (pd.c0, r["c0"])
    assert diag[0] == pd.c0
    if form == "eigen":
        assert diag[3] == r["rank"], (diag[3], r["rank"])
        assert len(out["ev"]) == pd.n and np.all(np.diff(out["ev"]) >= 0) and rev <= 1, rev
        assert np.array_equal(Ad, Ad.T)                   # the kernel writes both triangles from one value
        assert 0 <= out["sweeps"] <= 30
    return Ar, br


def _mf16(D, m):
    """marg_args: the 16-wide form runs when the factor's tiles, twice (fragments and the staged A', b'), fit in the place of A | b | W2"""
    n = D - m
    nb = (16 * ((m + 15) // 16) + n + 16) >> 4
    return m > 0 and n > 0 and 2 * (nb * (nb + 1) // 2 * 256) <= D * D + D + max(n * n, 1024)


# ---------------------------------------------------------------- (a), (b): sizes
@pytest.mark.parametrize("n", mc.reachable_sizes(89))
def test_size_sweep_unit_norm(ctx, stats, n):
    prob = mc.sweep_case(n)
    for form in FORMS:
        _check(prob, _run(ctx, prob, form), form, stats, "(a)")


def test_sweep_runs_both_factorisations():
    mf = [n for n in mc.reachable_sizes(89) if _mf16(n + 6, 6)]
    print(f"\n[marg-cases] 16-wide form at n = {mf}")
    assert mf and mf[0] == 60 and len(mf) < len(mc.reachable_sizes(89)) - 20
    assert not any(_mf16(n + 6, 6) for n in mc.reachable_sizes(58)) and _mf16(61 + 15, 15) and _mf16(85 + 15, 15) and not _mf16(7 + 15, 15)


@pytest.mark.parametrize("n", mc.reachable_sizes(89)[::4])
def test_size_sweep_norm_1e9(ctx, stats, n):
    prob = mc.sweep_case(n, 3000.0)
    assert n < 6 or 1e8 < np.abs(prob.prior_A).max() < 1e10
    for form in FORMS:
        _check(prob, _run(ctx, prob, form), form, stats, "(b)", floor=1e-6)


# ---------------------------------------------------------------- (c): spectra
def _c0_rtol(lam):
    """Weyl's bound on the relative error of the smallest kept eigenvalue under a perturbation of K_EVAL eps |A'|; beyond 1e-6 only where that eigenvalue is tiny against the norm"""
    kept = lam[lam > 1e-8]
    return 1e-6 if not len(kept) else max(1e-6, 1e3 * EPS * np.abs(lam).max() / kept.min())


@pytest.mark.parametrize("n", mc.SPECTRUM_SIZES)
@pytest.mark.parametrize("name", mc.SPECTRA)
def test_spectra(ctx, stats, name, n):
    prob = mc.spectrum_case(n, name)
    t = prob.truth
    lam, Q = t["lam"], t["Q"]
    keep = lam > 1e-8
    norm = np.abs(lam).max()
    out = _run(ctx, prob, "eigen")
    _check(prob, out, "eigen", stats, f"(c) {name}", c0_rtol=_c0_rtol(lam))
    Ad, bd = out["A"], out["b"]                           # (the header check of _check: the device's layout is the canonical one of Q)
    assert out["diag"][3] == keep.sum()
    assert np.abs(out["ev"] - np.sort(lam)).max() <= 1e-11 * norm
    want = (Q * (lam * keep)) @ Q.T
    scale = np.abs(want).max()
    assert np.abs(Ad - want).max() <= 1e-9 * scale
    for k in np.flatnonzero(~keep):
        assert abs(Q[:, k] @ bd) <= 1e-9 * np.linalg.norm(bd), (k, lam[k], Q[:, k] @ bd)
        assert np.linalg.norm(Ad @ Q[:, k]) <= 1e-9 * scale, (k, lam[k])
    if name == "diag":
        assert out["sweeps"] == 0
        assert np.array_equal(np.diag(Ad)[keep], lam[keep]) and not np.diag(Ad)[~keep].any() and not (Ad - np.diag(np.diag(Ad))).any()
    if name == "zero":
        assert not Ad.any() and not bd.any() and out["pd"].c0 == 0.0 and out["diag"][3] == 0
    if name == "tiny_offdiag":
        twin = _run(ctx, mc.spectrum_case(n, "diag"), "eigen")
        assert np.array_equal(Ad, twin["A"]) and np.array_equal(bd, twin["b"]) and out["pd"].c0 == twin["pd"].c0 and np.array_equal(out["ev"], twin["ev"])
    _check(prob, _run(ctx, prob, "info"), "info", stats, f"(c) {name}", c0=False)      # A' is not clamped in this form: its LDL^T c0 is another quantity here


# ---------------------------------------------------------------- (d): drop shapes
@pytest.mark.parametrize("n", mc.DROP_SIZES)
@pytest.mark.parametrize("dropped", mc.DROPS[0], ids=lambda d: "+".join("pose0" if t == 0 else "sb0" for t, _ in d))
def test_drop_shapes_mode0(ctx, stats, dropped, n):
    prob = mc.drop_case(n, dropped)
    assert prob.truth["mode"] == 0 and prob.truth["m"] == sum(mc.LOCAL[t] for t, _ in dropped)
    for form in FORMS:
        out = _run(ctx, prob, form)
        _check(prob, out, form, stats, f"(d) m={prob.truth['m']}")
        assert out["diag"][2] == 0 and out["diag"][1] > 1e-8


def test_dropped_block_with_a_pivot_under_the_threshold(ctx, stats):
    """the prior's 1e-10 eigenvector lives on the dropped coordinates: the device skips the pivot, the reference clamps the eigenvalue of A_mm, and with b = A x in the
    range of A the two pseudo-inverses give the same prior — to the 1e-7 of tests/test_back_parity.py::test_marginalization_with_a_rank_deficient_A_mm"""
    prob = mc.null_pivot_case()
    a_info = None
    for form in FORMS:
        out = _run(ctx, prob, form)
        assert out["diag"][2] != 0.0 and out["diag"][1] <= 1e-8, out["diag"]
        assert np.isfinite(out["A"]).all() and np.isfinite(out["b"]).all()
        # (the Jacobi's 1e-11 is a bar against the A' it decomposes, the device's own, as in tests/test_marg_eigen.py::test_eigen_spectrum_matches_lapack: here that A' and the
        # reference's agree to 1e-7 only)
        _check(prob, out, form, stats, "(d) null pivot", tol=1e-7, spectrum_of=a_info)
        a_info = out["A"]


# ---------------------------------------------------------------- (e): empty, refused, reproducible
def test_mode1_prior_without_pose9_is_empty(ctx):
    prob = mc.make_prior_case(mc.kept_blocks(30, 1, seed=1), [], None, True, 5000, True)
    for form in FORMS:
        out = _run(ctx, prob, form)
        assert out["pd"].valid == 0 and out["pd"].n == 0 and not out["diag"].any()


def _accepted_or_refused(ctx, stats, prob, limit):
    from dynamic_vins_amd._abi import DvinsError
    refused = 0
    for form in FORMS:
        try:
            out = _run(ctx, prob, form)
        except DvinsError as e:
            refused += 1
            assert f"at most {limit} kept dims beside {prob.truth['m']} dropped ones" in str(e) and f"this prior has {prob.truth['n']}" in str(e), str(e)
            continue
        _check(prob, out, form, stats, "(e)")
    return refused


def test_size_limit_is_refused_with_its_figure_and_the_ctx_stays_usable(ctx, stats):
    from dynamic_vins_amd.backend import get_marg_form
    refused = 0
    for n in mc.reachable_sizes(96)[len(mc.reachable_sizes(89)):] + [99, 120]:
        refused += _accepted_or_refused(ctx, stats, mc.make_prior_case(mc.kept_blocks(n, 1, seed=n), [(0, 9)], None, True, 1000 + n, True), 89)
    assert refused == 2 * 7                               # be_marg_finish_smem(n + 6, n) > 156 KB from n = 90 on, in both forms
    assert get_marg_form(ctx) == "info"
    prob = mc.sweep_case(48)
    for form in FORMS:
        _check(prob, _run(ctx, prob, form), form, stats, "(e)")


@pytest.mark.parametrize("dropped,top,over", [([(0, 0), (1, 0)], 85, 87), ([(0, 0)], 88, 90), ([(1, 0)], 88, 90)], ids=["m15", "m6", "m9"])
def test_size_limit_per_drop_size(ctx, stats, dropped, top, over):
    """the largest kept size the block types can form under each limit is accepted, the next one refused (mode 0; 89 beside 6 dropped dims is part (a)'s last size)"""
    m = sum(mc.LOCAL[t] for t, _ in dropped)
    limit = {6: 89, 9: 88, 15: 85}[m]
    assert _accepted_or_refused(ctx, stats, mc.drop_case(top, dropped), limit) == 0
    assert _accepted_or_refused(ctx, stats, mc.drop_case(over, dropped), limit) == 2


def test_two_runs_agree_bitwise_at_an_odd_size(ctx):
    prob = mc.sweep_case(33)
    for form in FORMS:
        a, b = _run(ctx, prob, form), _run(ctx, prob, form)
        for k in ("A", "b", "diag"):
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (form, k)
        assert a["pd"].c0 == b["pd"].c0
        if form == "eigen":
            assert np.array_equal(a["ev"].view(np.uint64), b["ev"].view(np.uint64)) and a["sweeps"] == b["sweeps"]
