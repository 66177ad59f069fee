"""The crafted marginalization cases of tests/marg_cases.py and the dense reference tests/ba_ref.py::marginalize, checked WITHOUT a GPU (in the style of
tests/test_ba_reference.py): the reference against a Schur complement and numpy.linalg.eigh written here, and — where the prior is block diagonal, so that the
answer is known by construction — against the prescribed Q, lambda; the block lists; the distance of every spectrum from the clamp threshold."""
import numpy as np
import pytest

from tests import ba_gen, ba_ref, marg_cases as mc

CASES = dict(mc.all_cases())
EPS = mc.EPS


def _direct(prob, mode):
    """[dropped | kept] of the prior in the prior's own block order, Schur complement with the eigen-clamped pseudo-inverse, eigh of A': dict like ba_ref.marginalize's"""
    pr = prob.prior
    blocks = [(pr.blocks[i].type, pr.blocks[i].idx, pr.blocks[i].off, pr.blocks[i].size_local) for i in range(pr.nblocks)]
    is_drop = lambda ty, idx: (ty == 0 and idx == 9) if mode == 1 else (ty in (0, 1) and idx == 0)
    di = [o + c for ty, idx, o, s in blocks if is_drop(ty, idx) for c in range(s)]
    ki = [o + c for ty, idx, o, s in blocks if not is_drop(ty, idx) for c in range(s)]
    H = prob.prior_A
    g = prob.prior_b + H @ ba_ref.prior_dx(prob)
    w, V = np.linalg.eigh(H[np.ix_(di, di)])
    P = sum((np.outer(V[:, k], V[:, k]) / w[k] for k in range(len(w)) if w[k] > 1e-8), np.zeros((len(di), len(di))))
    A = H[np.ix_(ki, ki)] - H[np.ix_(ki, di)] @ P @ H[np.ix_(di, ki)]
    A = 0.5 * (A + A.T)
    b = g[ki] - H[np.ix_(ki, di)] @ (P @ g[di])
    w2, V2 = np.linalg.eigh(A)
    A_eig, b_eig, c0, rank = np.zeros_like(A), np.zeros_like(b), 0.0, 0
    for k in range(len(w2)):
        if w2[k] > 1e-8:
            y = V2[:, k] @ b
            A_eig += w2[k] * np.outer(V2[:, k], V2[:, k])
            b_eig += y * V2[:, k]
            c0 += y * y / w2[k]
            rank += 1
    return dict(A=A, b=b, A_eig=A_eig, b_eig=b_eig, c0=c0, rank=rank, ev=w2)


def _c0_rtol(ev, floor):
    """Weyl: an eigenvalue moves by at most the perturbation's norm, K_EVAL eps |A'| here, so the smallest kept one carries that relative to itself into c0"""
    kept = ev[ev > 1e-8]
    return floor if not len(kept) else max(floor, 1e3 * EPS * np.abs(ev).max() / kept.min())


def test_reachable_sizes_are_all_the_block_types_can_form():
    for mode, top in ((1, 96), (0, 96)):
        six, nine = mc.available(mode)
        can = {6 * a + 9 * b + t for a in range(len(six) + 1) for b in range(len(nine) + 1) for t in (0, 1) if a + b + t >= 1 and a + b + t + 1 <= mc.MAX_BLOCKS}
        assert sorted(x for x in can if x <= top) == mc.reachable_sizes(top)
    assert mc.reachable_sizes()[:6] == [1, 6, 7, 9, 10, 12] and len(mc.reachable_sizes()) == 62 and len(mc.reachable_sizes(89)) == 57


@pytest.mark.parametrize("mode", [0, 1])
def test_block_lists_are_valid(mode):
    mixes = set()
    for n in mc.reachable_sizes():
        for seed in (n, n + 3, n + 7):
            kept = mc.kept_blocks(n, mode, seed=seed, ndropped=2 if mode == 0 else 1)
            assert len(set(kept)) == len(kept) and sum(mc.LOCAL[t] for t, _ in kept) == n and kept == sorted(kept)
            assert sum(t == 0 for t, _ in kept) <= 10 and sum(t == 1 for t, _ in kept) <= 11 and (0, 9 if mode == 1 else 0) not in kept
            assert len({mc.shifted(k, mode) for k in kept}) == len(kept)          # no two blocks meet in the new header
            assert all(0 <= i <= 10 for t, i in kept if t < 2) and all(i in (0, 1) for t, i in kept if t == 2) and all(i == 0 for t, i in kept if t == 3)
            if mode == 0:
                assert (0, 0) not in kept and (1, 0) not in kept
            mixes.add((n, sum(t == 1 for t, _ in kept)))
    assert len({n for n, _ in mixes}) == 62 and len(mixes) > 62          # every size, and the mix does vary with the seed


@pytest.mark.parametrize("name", list(CASES))
def test_case_header_is_valid(name):
    prob = CASES[name]()
    pr, t = prob.prior, prob.truth
    rows = sorted((pr.blocks[i].off, pr.blocks[i].size_local, pr.blocks[i].type, pr.blocks[i].idx) for i in range(pr.nblocks))
    assert len({(ty, idx) for _, _, ty, idx in rows}) == pr.nblocks <= mc.MAX_BLOCKS
    off = 0
    for o, s, ty, idx in rows:
        assert o == off and s == mc.LOCAL[ty]
        off += s
    assert off == pr.n == t["n"] + t["m"] and pr.valid == 1
    keys = {(ty, idx) for _, _, ty, idx in rows}
    if t["mode"] == 1:                                                # pose 9 is in the prior exactly when the mode has it to drop
        assert ((0, 9) in keys) == (t["m"] == 6)
    else:
        assert t["m"] == 6 * ((0, 0) in keys) + 9 * ((1, 0) in keys) > 0
    assert np.array_equal(prob.prior_A, prob.prior_A.T)
    assert prob.c.nframes == 11 and prob.c.nfac == prob.c.nlm == prob.c.nimu == 0


@pytest.mark.parametrize("name", list(CASES))
def test_reference_matches_a_direct_restatement(name):
    prob = CASES[name]()
    t = prob.truth
    r = mc.reference(prob)
    d = _direct(prob, t["mode"])
    assert r["n"] == t["n"] and r["m"] == t["m"] and set(r["blocks"]) == set(t["blocks"])
    sa, sb = max(np.abs(d["A"]).max(), 1e-300), max(np.abs(d["b"]).max(), 1e-300)
    # the reference keeps the kept blocks in the prior's order, like _direct
    assert np.abs(r["A"] - d["A"]).max() <= 1e-10 * sa and np.abs(r["b"] - d["b"]).max() <= 1e-10 * sb
    assert np.abs(r["A_eig"] - d["A_eig"]).max() <= 1e-9 * sa and np.abs(r["b_eig"] - d["b_eig"]).max() <= 1e-9 * sb
    assert r["rank"] == d["rank"] and np.isclose(r["c0"], d["c0"], rtol=_c0_rtol(d["ev"], 1e-9), atol=0)
    # the threshold condition, from the spectrum the reference sees
    dist, need = mc.margin(d["ev"], t["n"])
    assert dist >= need, (dist, need)
    if "lam" not in t:
        return
    # block diagonal: the answer by construction, in the canonical kept order
    lam, Q = t["lam"], t["Q"]
    dist, need = mc.margin(lam, t["n"])
    assert dist >= need
    keep = lam > 1e-8
    norm = max(np.abs(lam).max(), 1e-300)
    A, b = ba_gen.permute_prior(r["blocks"], r["A"], r["b"], t["blocks"])
    Ae, be = ba_gen.permute_prior(r["blocks"], r["A_eig"], r["b_eig"], t["blocks"])
    # exact zeros in the coupling: nothing of A' is rounded; x0 is the state, but q0^-1 q comes out of its four products as 0 or +-eps/4, so dx <= 1e-16 and b' = b + A dx
    assert np.array_equal(A, t["K"]) and np.abs(b - t["b_kept"]).max() <= 1e-14 * max(norm, np.abs(b).max())
    assert np.abs(Ae - (Q * (lam * keep)) @ Q.T).max() <= 1e-12 * norm
    assert r["rank"] == keep.sum()
    assert np.abs(np.sort(lam) - d["ev"]).max() <= 1e-12 * norm
    want = Q[:, keep] @ (Q[:, keep].T @ t["b_kept"])
    assert np.abs(be - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-300)
    for k in np.flatnonzero(~keep):
        assert abs(Q[:, k] @ be) <= 1e-9 * np.linalg.norm(be), (k, lam[k], Q[:, k] @ be)
    kept = lam[keep]
    c0 = float(np.sum((Q[:, keep].T @ t["b_kept"]) ** 2 / kept))
    assert np.isclose(r["c0"], c0, rtol=_c0_rtol(lam, 1e-9), atol=0), (r["c0"], c0)


def test_spectra_hold_what_their_names_say():
    for n in mc.SPECTRUM_SIZES:
        lam = {s: mc.spectrum_case(n, s).truth["lam"] for s in mc.SPECTRA}
        assert not lam["zero"].any() and (lam["indefinite"] < 0).sum() == (n + 3) // 4 and lam["indefinite"].min() >= -1 and lam["indefinite"][lam["indefinite"] < 0].max() <= -1e-3
        assert np.array_equal(lam["diag"], lam["tiny_offdiag"]) and len(set(lam["two_clusters"])) == min(n, 2)
        assert np.abs(lam["wide"]).max() == 1e9 and (n == 1 or {5e-9, 2e-8} <= set(lam["straddle"]))
        for s in mc.SPECTRA:
            if s != "wide":
                assert np.abs(lam[s]).max() <= 1e2
        K = mc.spectrum_case(n, "tiny_offdiag").truth["K"]
        assert n == 1 or (K[~np.eye(n, dtype=bool)] == 1e-305).all()
    d, t = mc.spectrum_case(33, "diag"), mc.spectrum_case(33, "tiny_offdiag")
    assert np.array_equal(d.truth["b_kept"], t.truth["b_kept"]) and np.array_equal(np.diag(d.truth["K"]), np.diag(t.truth["K"]))
    assert len(set(d.truth["lam"])) < 33                              # exact ties


def test_null_pivot_case_has_its_null_vector_on_the_dropped_block():
    prob = mc.null_pivot_case()
    r = mc.reference(prob)
    assert r["m"] == 15 and r["min_ev_mm"] <= 1e-8 and abs(r["min_ev_mm"] - 1e-10) < 1e-12
    assert np.linalg.eigvalsh(r["A"]).min() > 1e-3                        # A' itself is well conditioned: the two forms of the new prior coincide
    assert r["rank"] == r["n"]
