"""Premises of the stereo matcher's hostile cases (tests/sgm_hostile.py), asserted on the restatement (tests/sgm_ref.py) alone, on the CPU: every case reaches what it
was built for, so that a later change of a generator or of a seed cannot hollow tests/test_stereo_sgm_hostile.py out silently.  Every premise prints its count."""
import numpy as np
import pytest

from tests import sgm_hostile as sh
from tests import sgm_ref as sr

FLOOR = 8          # valid winners a planted band must show at its shift


def band(i):
    return slice(sh.PLANTED_BAND * i, sh.PLANTED_BAND * (i + 1))


def test_every_case_of_the_issue_is_there():
    """the families, their shapes and their counts: a case dropped from tests/sgm_hostile.py fails here, not silently on the device"""
    shapes = lambda fam: sorted({(c.w, c.h, c.D) for c in sh.CASES.values() if c.family == fam})
    assert shapes("narrow") == sorted([(37, 6, 64), (37, 6, 128), (5, 3, 256), (63, 2, 64)])
    assert shapes("thin") == sorted([(70, 1, 64), (130, 1, 128), (1, 9, 128), (1, 1, 64), (1, 1, 256), (2, 2, 64)])
    assert shapes("seams") == sorted([(256, 4, 64), (257, 5, 64), (253, 4, 64), (254, 4, 64), (255, 4, 64), (71, 22, 64), (70, 24, 64), (70, 22, 64)])
    assert shapes("planted") == [(88, 24, 64), (152, 24, 128), (280, 24, 256)]
    assert all(c.w < c.D for c in sh.CASES.values() if c.family == "narrow")
    assert [(c.w + c.h - 1) % 4 for n, c in sh.CASES.items() if n.startswith(("seams_71x22", "seams_70x24", "seams_70x22")) and n.endswith("random")] == [0, 1, 3]
    for corner, par in sh.CORNERS.items():
        assert sh.CASES["corners_260x6_d256_%s_random" % corner].par == par
    wide = {(c.w, c.h, c.D) for c in sh.CASES.values() if c.par == sh.WIDE_OPEN and c.family == "corners_256"}
    assert wide == {(70, 23, 64), (130, 9, 128), (67, 5, 64), (260, 6, 256)}
    assert any(c.par == dict(lr_max_diff=300) for c in sh.CASES.values())
    assert len(sh.names("saturated")) == 5 and sh.CASES["saturated_anti_checker"].par == dict(p1=255, p2=255)
    for n in sh.names("layout"):
        c = sh.CASES[n]
        assert (c.extra, c.lead, c.mems) == (5, 3, ("host", "pinned", "device"))
    assert {sh.CASES[n].w for n in sh.names("layout")} == {37, 257}
    print("%d cases in %d families" % (len(sh.CASES), len({c.family for c in sh.CASES.values()})))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_planted_winners_reach_both_ends_of_the_range(D):
    """default parameters: every shift below n_disp comes back as valid winners at that shift, n_disp - 1 included (the subpixel rule's upper end, the uniqueness scan with
    nothing above d* + 1), and the right image's winner reaches n_disp - 1 too; shift 0's valid pixels read 0.0 like invalid ones, so it is counted on d*"""
    name = "planted_d%d_default" % D
    l, r, par, _ = sh.case(name)
    res = sh.reference(name)
    assert l.shape == (24, D + 24) and par == sr.params(n_disp=D)
    shifts = sh.planted_shifts(D)
    assert shifts == [0, 1, D // 64, D // 64 + 1, D // 2 - 1, D - 2, D - 1, D + 3]
    counts = {}
    for i, s in enumerate(shifts):
        ds, valid = res["dstar"][band(i)], res["out"][band(i)] > 0
        if s >= D:
            assert np.array_equal(r[band(i)][:, :D + 24 - s], l[band(i)][:, s:])          # the shift is really there, outside the range
            continue
        assert np.array_equal(r[band(i)][:, :D + 24 - s], l[band(i)][:, s:])
        n = int((ds == 0).sum()) if s == 0 else int((valid & (ds == s)).sum())
        counts[s] = n
        assert n >= FLOOR, (s, n)
        if s > 0:
            assert np.abs(res["out"][band(i)][valid & (ds == s)] - s).max() <= 0.5
    n_dr = int((res["dr"][band(6)] == D - 1).sum())
    top = res["out"][band(6)][(res["out"][band(6)] > 0) & (res["dstar"][band(6)] == D - 1)]
    print("planted D = %d, seed %d: winners per shift %s (shift 0: d* = 0, others: valid with d* = shift); dr = n_disp - 1 at %d pixels" % (D, sh.PLANTED_SEEDS[D], counts, n_dr))
    assert n_dr >= 1
    assert (top == np.float32(D - 1)).all()          # d16 = 16 d* at the upper end: no subpixel term


@pytest.mark.parametrize("D", [64, 128, 256])
def test_planted_shift_outside_the_range_still_reports(D):
    """band 7 is shifted by n_disp + 3: no winner can be the shift, yet the rules leave valid pixels there — wrong ones, which the device must report identically"""
    res = sh.reference("planted_d%d_default" % D)
    s = sh.planted_shifts(D)[7]
    assert s == D + 3 and not (res["dstar"][band(7)] == s).any() and int(res["dstar"].max()) <= D - 1
    n = int((res["out"][band(7)] > 0).sum())
    print("planted D = %d: %d valid pixels in the band shifted by %d" % (D, n, s))
    assert n >= 1


@pytest.mark.parametrize("D", [64, 128, 256])
def test_planted_wide_open_covers_every_lane_slot(D):
    """uniqueness = 0 without the left-right test: the valid winners take every residue mod 2 and mod 4, i.e. every slot j = d % K of a lane and neighbours d* +- 1 in the
    next lane, whichever K the kernel was built for"""
    name = "planted_d%d_wide_open" % D
    res, dflt = sh.reference(name), sh.reference("planted_d%d_default" % D)
    assert sh.case(name)[2] == sr.params(n_disp=D, uniqueness=0, lr_max_diff=-1)
    assert res["S"] is dflt["S"] or np.array_equal(res["S"], dflt["S"])
    valid = res["out"] > 0
    ds = res["dstar"][valid].astype(int)
    for K in (2, 4):
        seen = sorted(set((ds % K).tolist()))
        print("planted wide open D = %d: %d valid pixels (default: %d), %d distinct winners, residues mod %d: %s" % (D, int(valid.sum()), int((dflt["out"] > 0).sum()),
                                                                                                                  len(set(ds.tolist())), K, seen))
        assert seen == list(range(K))
    assert int(valid.sum()) > int((dflt["out"] > 0).sum()) and ds.max() == D - 1
    assert (valid == ((res["dstar"] > 0) & (res["dstar"] <= np.arange(D + 24)[None, :]))).all()          # only d* <= x is left of the validity tests (d* = 0 reads 0.0)


@pytest.mark.parametrize("name", sh.names("narrow") + sh.names("thin"))
def test_narrow_and_thin_complete_and_agree_with_the_naive_form(name):
    l, r, par, _ = sh.case(name)
    res = sh.reference(name)
    h, w = l.shape
    for item, dt in zip(sh.ITEMS, (np.uint64, np.uint64, np.uint16, np.int16, np.int16)):
        assert res[item].dtype == dt and res[item].shape[:2] == (h, w)
    assert res["S"].shape == (h, w, par["n_disp"]) and res["out"].dtype == np.float32
    beyond = res["dstar"] > np.arange(w)[None, :]
    print("%s: d* > x at %d of %d pixels, %d valid" % (name, int(beyond.sum()), h * w, int((res["out"] > 0).sum())))
    assert not res["out"][beyond].any()
    assert (res["dr"] < np.maximum(w - np.arange(w), 1)[None, :]).all()          # dR only ranges over x + d < w
    if (w, h) == (1, 1):
        assert res["dstar"][0, 0] == 0 and res["dr"][0, 0] == 0 and res["out"][0, 0] == 0 and res["codes_l"][0, 0] == 0 and res["codes_r"][0, 0] == 0
    naive = sr.sgm_naive(l, r, **par)
    for item in sh.ITEMS:
        assert naive[item].dtype == res[item].dtype and np.array_equal(naive[item], res[item]), item
    assert np.array_equal(naive["out"].view(np.uint32), res["out"].view(np.uint32))


def test_planted_d64_agrees_with_the_naive_form():
    """both parameter sets, in the scalar loops from the census on.  The planted cases at D = 128 and 256 are left to the vectorised form to keep the suite quick: the
    scalar loops took 4 s and 10 s for them when they were run once (default parameters), and agreed there too"""
    for name in ("planted_d64_default", "planted_d64_wide_open"):
        l, r, par, _ = sh.case(name)
        res, naive = sh.reference(name), sr.sgm_naive(l, r, **par)
        for item in sh.ITEMS:
            assert naive[item].dtype == res[item].dtype and np.array_equal(naive[item], res[item]), (name, item)
        assert np.array_equal(naive["out"].view(np.uint32), res["out"].view(np.uint32)), name


def test_saturated_reaches_the_largest_sums():
    top = {n: int(sh.reference(n)["S"].max()) for n in sh.names()}
    anti = top["saturated_anti_checker"]
    runner_up = max((v, n) for n, v in top.items() if n != "saturated_anti_checker")
    print("S.max(): anti-checker at p1 = p2 = 255: %d of the bound %d; next: %d (%s)" % (anti, 8 * (64 + 255), runner_up[0], runner_up[1]))
    assert anti == max(top.values()) and anti > runner_up[0] and anti < 65536 and anti <= 8 * (64 + 255)
    assert (anti << 8 | 255) < 2 ** 31          # the (S, d) key of the winner search stays a positive int
    for n in ("saturated_all_0", "saturated_all_255"):
        res = sh.reference(n)
        assert not res["codes_l"].any() and not res["dstar"].any() and not res["dr"].any() and not res["out"].any()
    l, r, _, _ = sh.case("saturated_ramp")
    res = sh.reference("saturated_ramp")
    assert (np.diff(l.astype(int), axis=0) == 0).all() and np.array_equal(r[:, :-3], l[:, 3:])
    n3 = int(((res["out"] > 0) & (res["dstar"] == 3)).sum())
    print("ramp: %d valid pixels, %d of them at d* = 3; %d distinct left codes" % (int((res["out"] > 0).sum()), n3, len(np.unique(res["codes_l"]))))
    assert n3 >= FLOOR
    l, r, _, _ = sh.case("saturated_zero_against_random")
    assert not l.any() and r.any() and not sh.reference("saturated_zero_against_random")["codes_l"].any()


def test_the_rule_d_star_within_x_decides_somewhere():
    """a cost of 64 for x - d < 0 is above every Hamming distance, so d* > x is rare: it needs a left border whose own matches are all bad.  The anti-checker has it"""
    res = sh.reference("saturated_anti_checker")
    beyond = res["dstar"] > np.arange(res["dstar"].shape[1])[None, :]
    print("anti-checker: d* > x at %d pixels" % int(beyond.sum()))
    assert beyond.sum() >= 1 and not res["out"][beyond].any()


@pytest.mark.parametrize("kind", sh.PROPERTY_KINDS)
@pytest.mark.parametrize("shape", sh.PROPERTY_SHAPES)
def test_the_self_comparisons_hold_on_the_restatement(shape, kind):
    """what tests/test_stereo_sgm_hostile.py asserts of the device alone is true of the specification: a vertical flip of both images flips S and the map (the eight
    directions map onto each other, every tie rule is in d alone); a constant added to both images changes no code"""
    w, h, D = shape
    l, r = sh.property_pair(kind, w, h, D)
    assert l.shape == (h, w) and int(max(l.max(), r.max())) <= sh.PROPERTY_TOP and sh.PROPERTY_TOP + sh.PROPERTY_ADD <= 255
    a, f, c = sr.sgm(l, r, n_disp=D), sr.sgm(l[::-1], r[::-1], n_disp=D), sr.sgm(l + sh.PROPERTY_ADD, r + sh.PROPERTY_ADD, n_disp=D)
    n_valid = int((a["out"] > 0).sum())
    print("%dx%d D = %d %s: %d valid pixels, %d distinct winners" % (w, h, D, kind, n_valid, len(np.unique(a["dstar"]))))
    assert n_valid >= 4 * FLOOR
    assert np.array_equal(f["S"], a["S"][::-1]) and np.array_equal(f["out"].view(np.uint32), a["out"][::-1].view(np.uint32))
    assert not np.array_equal(f["codes_l"], a["codes_l"][::-1])          # the codes themselves are not mirror images: the bit order is row-major
    for item in sh.ITEMS:
        assert np.array_equal(c[item], a[item]), item
    assert np.array_equal(c["out"].view(np.uint32), a["out"].view(np.uint32))


@pytest.mark.parametrize("name", sh.names())
def test_the_host_rules_accept_every_case(name):
    """dv_stereo_sgm_check has no minimum size: 1 x 1 is a frame like any other"""
    from dynamic_vins_amd.frontend import sgm_check
    c = sh.CASES[name]
    _, _, par, (extra, _) = sh.case(name)
    sgm_check(c.w, c.h, stride=c.w + extra, **par)
