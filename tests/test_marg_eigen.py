"""DV_MARG_EIGEN (dv_set_marg_form): the reference's marginalization arithmetic on the device — A' eigen-decomposed by be_marg_eig (parallel Jacobi), eigenvalues
<= 1e-8 zeroed (MarginalizationInfo::marginalize, marginalization_factor.cpp:297-308) — against the CPU oracle, which does the same.  The default form DV_MARG_INFO
 is covered by tests/test_back_parity.py and stays untouched.  GPU tests are marked; the last three tests run without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ba_gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
FULL = os.environ.get("DVINS_LONGRUN", "0") == "1"
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=64, height=64, max_cnt=10, min_dist=5)


@pytest.fixture
def eig_ctx(ctx):
    from dynamic_vins_amd.backend import set_marg_form
    set_marg_form(ctx, "eigen")
    yield ctx
    set_marg_form(ctx, "info")


def _compare(po, Ao, bo, pd, Ad, bd, a_tol=1e-9, b_tol=1e-9):
    assert pd.valid == po.valid == 1 and pd.n == po.n and pd.nblocks == po.nblocks
    bo_blocks, bd_blocks = ba_gen.prior_to_dict(po, Ao, bo), ba_gen.prior_to_dict(pd, Ad, bd)
    assert set(bo_blocks) == set(bd_blocks)
    Ao_p, bo_p = ba_gen.permute_prior(bo_blocks, Ao, bo, bd_blocks)
    scale = np.abs(Ao_p).max()
    assert np.allclose(Ad, Ao_p, rtol=0, atol=a_tol * scale + 1e-6), np.abs(Ad - Ao_p).max() / scale
    assert np.allclose(bd, bo_p, rtol=0, atol=b_tol * np.abs(bo_p).max() + 1e-6), np.abs(bd - bo_p).max()
    assert np.isclose(pd.c0, po.c0, rtol=1e-6), (pd.c0, po.c0)


@gpu
@pytest.mark.parametrize("kw,mode", [(dict(seed=21, with_prior=True), 0), (dict(seed=22), 0), (dict(seed=23, with_prior=True), 1),
                                     (dict(seed=24, with_prior=True, use_imu=0), 0), (dict(seed=25, with_prior=True, nlm=300), 0)])
def test_eigen_form_matches_oracle(eig_ctx, oracle, kw, mode):
    """the windows of tests/test_back_parity.py::test_marginalization_matches_oracle, marginalized in DV_MARG_EIGEN form, with that test's tolerances"""
    from dynamic_vins_amd.backend import marg_spectrum, marginalize
    full = ba_gen.make_window(oracle, **kw)
    ba_gen.oracle_solve(oracle, full)
    sub = ba_gen.marg_subproblem(full, mode)
    po, Ao, bo = ba_gen.oracle_marginalize(oracle, sub, mode)
    pd, Ad, bd, diag = marginalize(eig_ctx, sub, mode)
    _compare(po, Ao, bo, pd, Ad, bd)
    assert diag[1] > 1e-8
    ev, sweeps = marg_spectrum(eig_ctx)
    assert len(ev) == pd.n and diag[3] == (ev > 1e-8).sum() and diag[0] == pd.c0
    print(f"n={pd.n} kept={int(diag[3])} sweeps={sweeps} lambda=[{ev[0]:.3g}, {ev[-1]:.3g}]")


def _crafted_mode1(oracle, beta=1.0, seed=23):
    """a mode-1 sub-problem whose prior has ONE eigenvalue 1e-10 (far below the 1e-8 clamp, far above rounding at |A| ~ 1e2) along q, q zero on the coordinates
    of the pose being dropped — so q survives the Schur complement as an eigenvector of A' with the same eigenvalue — every other eigenvalue >= 1e-6, b = A x + beta q"""
    full = ba_gen.make_window(oracle, seed=seed, with_prior=True)
    sub = ba_gen.marg_subproblem(full, 1)
    pr = sub.prior
    n = pr.n
    drop = [b for b in range(pr.nblocks) if pr.blocks[b].type == 0 and pr.blocks[b].idx == 9]
    assert drop, "the prior has no block of the pose kMarginSecondNew drops"
    d0 = pr.blocks[drop[0]].off
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 1, n)
    q[d0:d0 + 6] = 0.0
    q /= np.linalg.norm(q)
    M = rng.normal(0, 1, (n, n))
    M[:, 0] = q
    Q, _ = np.linalg.qr(M)
    Q[:, 0] = q                                            # (the QR keeps the first column up to its sign)
    lam = np.concatenate([[1e-10], 10.0 ** rng.uniform(-6, 2, n - 1)])
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    b = A @ rng.normal(0, 0.01, n) + beta * q
    sub.prior_A, sub.prior_b = np.ascontiguousarray(A), np.ascontiguousarray(b)
    oracle.lib.dvo_prior_c0.restype = C.c_double
    oracle.lib.dvo_prior_c0.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    pr.c0 = oracle.lib.dvo_prior_c0(sub.prior_A.ctypes.data, sub.prior_b.ctypes.data, n)
    sub._bind()
    return sub, q


def _q_in(q, prior_in, pd):
    """q (in the input prior's layout) in the layout of the device's output prior pd (blocks matched by key)"""
    bi = ba_gen.prior_to_dict(prior_in, None, None)
    out = np.zeros(pd.n)
    for key, (off, sz, _) in ba_gen.prior_to_dict(pd, None, None).items():
        out[off:off + sz] = q[bi[key][0]:bi[key][0] + sz]
    return out


@gpu
def test_eigen_form_clamps_what_the_reference_clamps(ctx, oracle):
    """the discriminating case: an A' eigenvalue of 1e-10.  The oracle (the reference's arithmetic) zeroes it and projects b' off q; DV_MARG_EIGEN must do the same,
    DV_MARG_INFO keeps q^T b' = beta (its c0 is not asserted: whether its LDL^T skips that pivot is a coin flip)"""
    from dynamic_vins_amd.backend import marginalize, set_marg_form
    beta = 1.0
    sub, q = _crafted_mode1(oracle, beta)
    po, Ao, bo = ba_gen.oracle_marginalize(oracle, sub, 1)
    set_marg_form(ctx, "eigen")
    try:
        pd, Ad, bd, diag = marginalize(ctx, sub, 1)
    finally:
        set_marg_form(ctx, "info")
    _compare(po, Ao, bo, pd, Ad, bd)
    qo = _q_in(q, sub.prior, pd)
    assert abs(qo @ bd) <= 1e-9 * np.linalg.norm(bd), qo @ bd
    assert diag[3] == pd.n - 1                              # one eigenvalue clamped
    p0, A0, b0, d0 = marginalize(ctx, sub, 1)               # the default form: the near-null direction keeps its component
    assert abs(qo @ b0 - beta) < 1e-6, qo @ b0


@gpu
def test_eigen_spectrum_matches_lapack(ctx, oracle):
    """dv_marg_last_spectrum: the eigenvalues of A' before the clamp, against numpy.linalg.eigvalsh of the DV_MARG_INFO A' (the same A' the eigen form decomposes)"""
    from dynamic_vins_amd.backend import marg_spectrum, marginalize, set_marg_form
    sub, _ = _crafted_mode1(oracle)
    p0, A0, b0, _ = marginalize(ctx, sub, 1)
    set_marg_form(ctx, "eigen")
    try:
        marginalize(ctx, sub, 1)
        ev, sweeps = marg_spectrum(ctx)
    finally:
        set_marg_form(ctx, "info")
    ref = np.linalg.eigvalsh(A0)
    norm = np.abs(ref).max()
    assert len(ev) == len(ref) == p0.n
    assert np.all(np.diff(ev) >= 0)
    assert np.abs(ev - ref).max() <= 1e-11 * norm, np.abs(ev - ref).max() / norm
    print(f"n={p0.n} sweeps={sweeps} lambda_min={ev[0]:.3g} lambda_max={ev[-1]:.3g}")
    assert 1 <= sweeps <= 20                                # measured on an MI355X: 15 (the windows of test_eigen_form_matches_oracle: 10 - 12); the cap is 30


@gpu
def test_eigen_form_is_bitwise_reproducible(eig_ctx, oracle):
    from dynamic_vins_amd.backend import marg_spectrum, marginalize
    full = ba_gen.make_window(oracle, seed=21, with_prior=True)
    ba_gen.oracle_solve(oracle, full)
    sub = ba_gen.marg_subproblem(full, 0)
    p1, A1, b1, d1 = marginalize(eig_ctx, sub, 0)
    e1 = marg_spectrum(eig_ctx)
    p2, A2, b2, d2 = marginalize(eig_ctx, sub, 0)
    e2 = marg_spectrum(eig_ctx)
    assert np.array_equal(A1.view(np.uint64), A2.view(np.uint64)) and np.array_equal(b1.view(np.uint64), b2.view(np.uint64))
    assert np.array_equal(d1.view(np.uint64), d2.view(np.uint64)) and p1.c0 == p2.c0
    assert np.array_equal(e1[0].view(np.uint64), e2[0].view(np.uint64)) and e1[1] == e2[1]


def _large_prior_mode1(oracle):
    """a mode-1 sub-problem whose kept prior has 123 dims: pose 9 (dropped), poses 0-3 and the speed-biases of all 11 frames (16 blocks)"""
    from dynamic_vins_amd.backend import dv_ba_prior
    full = ba_gen.make_window(oracle, seed=26, with_prior=True)
    sub = ba_gen.marg_subproblem(full, 1)
    pr = dv_ba_prior()
    blocks = [(0, 9, 6)] + [(0, k, 6) for k in range(4)] + [(1, k, 9) for k in range(11)]
    off = 0
    for i, (ty, idx, sz) in enumerate(blocks):
        pb = pr.blocks[i]
        pb.type, pb.idx, pb.off, pb.size_local = ty, idx, off, sz
        x0 = sub.pose[idx] if ty == 0 else sub.speed_bias[idx]
        for j in range(len(x0)):
            pr.x0[i][j] = float(x0[j])
        off += sz
    rng = np.random.default_rng(26)
    M = rng.normal(0, 1, (off + 5, off))
    pr.valid, pr.n, pr.nblocks, pr.c0 = 1, off, len(blocks), 0.0
    sub.prior, sub.prior_A, sub.prior_b = pr, np.ascontiguousarray(M.T @ M), np.ascontiguousarray(rng.normal(0, 1, off))
    sub._bind()
    return sub


@gpu
def test_refusals_leave_the_ctx_usable(gpu_ctx_factory, oracle):
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.backend import Batch, get_marg_form, marg_spectrum, marginalize, set_marg_form
    a = gpu_ctx_factory(width=64, height=64, max_cnt=10, min_dist=5)
    b = gpu_ctx_factory(width=64, height=64, max_cnt=10, min_dist=5)
    with pytest.raises(DvinsError, match="no DV_MARG_EIGEN marginalization"):
        marg_spectrum(a)
    with pytest.raises(DvinsError, match="DV_MARG_INFO"):             # form 2
        set_marg_form(a, 2)
    assert get_marg_form(a) == "info"
    with pytest.raises(ValueError):
        set_marg_form(a, "sqrt")
    # a dv_batch member cannot switch ...
    B = Batch([a, b])
    with pytest.raises(DvinsError, match="dv_batch member"):
        set_marg_form(a, "eigen")
    assert get_marg_form(a) == "info"
    B.close()                                               # (Batch owns the handle: close() destroys it once and clears it)
    # ... and a batch is not built over an eigen-form ctx
    set_marg_form(a, "eigen")
    assert get_marg_form(a) == "eigen"
    arr = (C.c_void_p * 2)(a.h, b.h)
    assert not a.lib.dv_batch_create(arr, 2)
    assert b"DV_MARG_EIGEN" in a.lib.dv_last_error(None)
    # a prior with more kept dims than fit (123)
    big = _large_prior_mode1(oracle)
    with pytest.raises(DvinsError, match="at most 89 kept dims"):
        marginalize(a, big, 1)
    # still usable: the form holds, an ordinary marginalization runs and matches the oracle
    full = ba_gen.make_window(oracle, seed=23, with_prior=True)
    ba_gen.oracle_solve(oracle, full)
    sub = ba_gen.marg_subproblem(full, 1)
    po, Ao, bo = ba_gen.oracle_marginalize(oracle, sub, 1)
    pd, Ad, bd, _ = marginalize(a, sub, 1)
    _compare(po, Ao, bo, pd, Ad, bd)
    assert get_marg_form(a) == "eigen" and get_marg_form(b) == "info"


@gpu
def test_estimator_eigen_form_against_the_oracle():
    """images -> tracker -> estimator in DV_MARG_EIGEN form for 300 raw frames at 640x360 (DVINS_LONGRUN=1: 1000), the oracle estimator fed the same rows; bars no looser
    than tests/test_longrun_parity.py's.  Prints the window-deviation course of both forms."""
    import marg_form_longrun
    frames = 1000 if FULL else 300
    st = marg_form_longrun.run("raw", "eigen", frames)
    info = marg_form_longrun.run("raw", "info", frames)
    for s in (st, info):
        print(s["form"], "solved", s["solved"], "mismatches", s["iter_plus_minus_one"] + s["iter_other"], "ate %.3g" % s["ate_hip_vs_oracle_m"], "max_dp %.3g" % s["max_dp_m"],
              "first above", s["first_frame_with_window_deviation_above"], "sweeps", s.get("jacobi_sweeps_min_max_mean"))
    solved = st["solved"]
    assert solved >= frames - 12
    assert st["flags_differ"] == 0, st
    mismatches = st["iter_plus_minus_one"] + st["iter_other"]
    assert mismatches <= max(2, solved // 150), st["iteration_mismatches"]
    assert all(abs(m["hip"] - m["oracle"]) <= 3 for m in st["iteration_mismatches"]), st["iteration_mismatches"]
    assert st["ate_hip_vs_oracle_m"] < 2e-4 and st["max_abs_traj_diff_m"] < 5e-4, st
    chk, last = st["marg_checked"], st["marg_last4"]
    kmin, kmax = st["kept_eigenvalues_min_max"]
    assert chk > 0 and last[3] == int(last[3]) and kmin <= last[3] <= kmax, (chk, last, kmin, kmax)      # the health report carries J0's kept-eigenvalue count


@gpu
@pytest.mark.parametrize("threads", [1, 2])
def test_runner_eigen_form_equals_python_pipeline(threads):
    """dv_runner over ctxs whose estimators were created with marg_form="eigen" inherits the form: states bit-identical to the Python pipeline's"""
    from dynamic_vins_amd import sim
    from dynamic_vins_amd.backend import Runner, get_marg_form
    from dynamic_vins_amd.pipeline import Pipeline, SyntheticSequence
    w, h, S, frames = 752, 480, 2, 30
    cam = sim.scaled_cam(sim.ZED, w, h, 1280, 720)
    seqs = [SyntheticSequence(w, h, cam, frames, rate=20.0, phase=1.3 * i) for i in range(S)]
    kw = dict(max_cnt=150, min_dist=30, max_iters=8, est_kw=dict(marg_form="eigen"))
    pipes = [Pipeline(q, **kw) for q in seqs]
    ref = [Pipeline(q, **kw) for q in seqs]
    assert all(get_marg_form(p.ctx) == "eigen" for p in pipes)
    runner = Runner(pipes, group_size=0, threads=threads)
    runner.run(frames - 1)
    for i in range(S):
        for _ in range(frames - 1):
            ref[i].step()
        st, poses, iters, fr = runner.get(i)
        assert fr == frames - 1 and st.frame == ref[i].last_state.frame and st.nonlinear == ref[i].last_state.nonlinear
        assert np.array_equal(np.ctypeslib.as_array(st.window), ref[i].est.window()), f"sequence {i}: window states differ"
        want = np.array(ref[i].poses)
        assert len(poses) == len(want) >= frames - 14
        assert np.array_equal(poses[:, 1:], want)
    runner.close()
    for p in pipes + ref:
        p.ctx.close()


# ---- without a GPU ----

def test_marg_form_symbols_are_exported_and_mirrored():
    from dynamic_vins_amd import _abi
    names = ("dv_set_marg_form", "dv_get_marg_form", "dv_marg_last_spectrum")
    hdr = open(os.path.join(ROOT, "include", "dvins.h")).read()
    assert "#define DV_MARG_INFO  0" in hdr and "#define DV_MARG_EIGEN 1" in hdr
    assert (_abi.DV_MARG_INFO, _abi.DV_MARG_EIGEN) == (0, 1)
    lib = _abi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in names:
        assert n in _abi.SIGNATURES and n in exported and getattr(lib, n) is not None


def test_node_refuses_a_bogus_marg_form_in_the_parse(tmp_path):
    node = os.path.join(ROOT, "dynamic_vins_amd", "bin", "dvins_node")
    r = subprocess.run([node, str(tmp_path / "none.yaml"), str(tmp_path), "--marg-form", "bogus"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--marg-form takes info or eigen" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([node, str(tmp_path / "none.yaml"), str(tmp_path), "--marg-form"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--marg-form" in r.stderr


def test_shim_set_marginalization_form_links_against_the_library(tmp_path):
    src = tmp_path / "use_form.cpp"
    src.write_text('#include "dvins_shim.hpp"\n'
                   'int main(int argc, char** argv) {\n'
                   '    if (argc > 99) { dynamic_vins::Estimator e(argv[1]); e.SetMarginalizationForm(DV_MARG_EIGEN); }\n'
                   '    return 0;\n'
                   '}\n')
    exe = tmp_path / "use_form"
    lib = os.path.join(ROOT, "dynamic_vins_amd", "lib")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"), str(src), "-o", str(exe),
                        "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert subprocess.run([str(exe)], capture_output=True, timeout=60).returncode == 0
