"""Front-end parity on degenerate images (generators and conditions: tests/front_hostile.py).

CPU (`-m "not gpu"`): every case is shown, on the oracle alone, to reach the branch it is named for — the tie rule of the selection sort, the candidate census
against the device's limits, more than DISC_CAP discs on a tile, a conflict inside an acceptance step, pyramids smaller than the window, more than 5 px of drift,
partial rejection, level passes that use all 30 iterations, repeated points and equal keys in the position order — and the figures are printed.
GPU: the HIP entries against the oracle, bit for bit (float32 as uint32 views, status and counts exactly), the bar of tests/test_front_parity.py.
The partly flat frames overflow a candidate buffer of their own size if zero responses are emitted as candidates: the device must return the oracle's corners."""
import numpy as np
import pytest

from tests import front_hostile as fh

RULES = ("cpu", "cuda")
IMAGES = fh.detector_images()
LK_CASES = fh.lk_cases()
GFTT_MIN_DISTS = (0, 3, 15) + fh.MIN_DISTS
TIE_CASES = ("tiled", "tiled_mirror")
STEP_TIE_CASES = ("binary", "checker8", "noise2")            # 0 / 255 images (thresholded texture, checkerboard, noise) whose plateaus tie a whole acceptance step
CONFLICT_CASES = ("noise2", "checker8", "binary")
LIMIT_W, LIMIT_H = 320, 240


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tex(h, w, seed):
    return fh.tex_u8(h, w, seed)


# =============================================================== conditions (oracle only)
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_census_and_restatement(oracle, name, rule):
    """the candidate census of every detector image beside the device's limits, and the numpy restatement of the selection against the oracle at every min_dist"""
    img = IMAGES[name]
    c = fh.census(oracle, img, rule)
    print(f"\n[census] {name} {rule}: {c} (limits: {fh.SEL_CAP} per value bin, {fh.SEL_MAX_CELLS} cells)")
    h, w = img.shape
    assert c["max_bin"] <= fh.SEL_CAP and w * h <= fh.SEL_MAX_CELLS          # inside the stated limits at every min_dist >= 1
    assert c["without_zeros"] <= c["cap"]
    if name in fh.PARTLY_FLAT and (w, h) == (fh.W, fh.H):
        assert c["with_zeros"] > c["cap"] >= c["without_zeros"]              # overflows the candidate buffer iff zero responses are emitted
    if name in STEP_TIE_CASES:
        assert 64 <= c["max_same_value"] <= fh.SEL_CAP
    for md in GFTT_MIN_DISTS:
        for max_n in (0, 7, 40):
            ref = oracle.gftt(img, max_n if max_n else fh.SEL_MAX_ACC, 0.01, md, rule=rule)
            got = fh.np_gftt(oracle, img, max_n, 0.01, md, rule=rule)
            assert np.array_equal(got, ref), (md, max_n)
    if name in fh.PARTLY_FLAT:
        ref = oracle.gftt(img, 50, 0.01, 5, rule=rule)                        # the oracle returns corners from the textured part, none from a whole flat frame
        assert len(ref) == 0 if name == "flat_whole" else len(ref) >= 20


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("md", [0, 3, 15])
@pytest.mark.parametrize("name", TIE_CASES)
def test_tie_conditions(oracle, name, rule, md):
    img = IMAGES[name]
    st = {}
    got = fh.np_gftt(oracle, img, 40, 0.01, md, rule=rule, stats=st)
    assert np.array_equal(got, oracle.gftt(img, 40, 0.01, md, rule=rule))
    _, cnt = np.unique(st["values"], return_counts=True)
    shared = int(cnt[cnt > 1].sum())
    cuts = fh.tie_cut_max_ns(oracle, img, md, rule)
    print(f"\n[ties] {name} {rule} min_dist {md}: {len(got)} corners, {len(cnt)} distinct values, {shared} share a value, max_n with the cut inside a tie group: {cuts[:8]}...")
    assert shared >= 10 and len(cuts) >= 3
    n = cuts[0]
    wrong = fh.np_gftt(oracle, img, n, 0.01, md, rule=rule, reverse_ties=True)
    assert {tuple(p) for p in wrong} != {tuple(p) for p in oracle.gftt(img, n, 0.01, md, rule=rule)}


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", CONFLICT_CASES)
def test_in_step_conflict_condition(oracle, name, rule):
    tot = {}
    for md in (2, 2.5, 3.5):
        st = {}
        fh.np_gftt(oracle, IMAGES[name], 0, 0.01, md, rule=rule, stats=st)
        tot[md] = st["in_step_conflicts"]
    print(f"\n[conflicts inside a step of 64] {name} {rule}: {tot}")
    assert all(v >= 1 for v in tot.values())


def _limit_images():
    return fh.checker(LIMIT_H, LIMIT_W, 4), _tex(LIMIT_H, LIMIT_W, 5)


@pytest.mark.parametrize("rule", RULES)
def test_limit_conditions(oracle, rule):
    """the two refusals: one value bin over SEL_CAP (and the candidate buffer NOT overflowed, so that flag 4 stands alone), and a min-distance grid over SEL_MAX_CELLS"""
    chk, benign = _limit_images()
    c = fh.census(oracle, chk, rule)
    print(f"\n[limits] 4 px checkerboard {LIMIT_W} x {LIMIT_H} {rule}: {c}; min_dist 1 -> {LIMIT_W * LIMIT_H} cells")
    assert c["top_bin"] > fh.SEL_CAP and c["without_zeros"] > fh.SEL_CAP and c["with_zeros"] <= c["cap"]
    assert LIMIT_W * LIMIT_H > fh.SEL_MAX_CELLS
    b = fh.census(oracle, benign, rule)
    assert b["max_bin"] <= fh.SEL_CAP and b["with_zeros"] <= b["cap"]


def _oracle_tracker(oracle, max_cnt, min_dist):
    cam = fh.cam_for(fh.W, fh.H)
    return oracle.tracker(fh.W, fh.H, max_cnt, min_dist, 1, 1, cam, cam)


def test_crowded_disc_condition(oracle):
    """a contracting sequence through the oracle's tracker: on some frame on which the detector runs, more than DISC_CAP tracked points reach one tile (the cull test
    of gftt_tile_body) while another tile stays below; the tracker fills up to DV_MAX_FEATS, and the points handed to the next frame's tracking hold equal sort keys"""
    o = _oracle_tracker(oracle, fh.CROWD_MAX_CNT, fh.CROWD_MIN_DIST)
    seq = fh.crowded_sequence()
    over, full_with_ties = [], []
    for k, (l, r) in enumerate(seq):
        rows = o.track_image(l, r, 0.05 * k)
        old = rows[rows["track_cnt"] > 1]
        per_tile = fh.discs_per_tile(np.ascontiguousarray(old["left"][:, 3:5], np.float32), fh.W, fh.H, fh.CROWD_MIN_DIST) if k else np.zeros((5, 3), int)
        keys = fh.order_keys(np.ascontiguousarray(rows["left"][:, 3:5], np.float32))
        ties = len(keys) - len(np.unique(keys))
        print(f"\n[crowded] frame {k}: {len(rows)} rows, {len(old)} tracked, {int((rows['track_cnt'] == 1).sum())} new, {ties} points share a pixel with an earlier one, "
              f"most discs on a tile {per_tile.max()}, fewest {per_tile.min()} (DISC_CAP {fh.DISC_CAP})")
        if len(old) < fh.CROWD_MAX_CNT and (rows["track_cnt"] == 1).sum() >= 1 and per_tile.max() > fh.DISC_CAP and per_tile.min() <= fh.DISC_CAP:
            over.append(k)                                          # the detector ran with the fallback on one tile and the culled list on another
        if k + 1 < len(seq) and len(rows) == fh.CROWD_MAX_CNT and ties >= 1:
            full_with_ties.append(k)                                # frame k + 1 ranks DV_MAX_FEATS previous points, some with equal keys
    assert len(over) >= 1 and len(full_with_ties) >= 1, (over, full_with_ties)


@pytest.mark.parametrize("value", [0, 255])
def test_flat_sequence_condition(oracle, value):
    seq = fh.flat_sequence(value)
    for rule in RULES:
        c = fh.census(oracle, seq[0][0], rule)
        print(f"\n[flat sequence] value {value} {rule}: {c}")
        assert c["with_zeros"] > c["cap"] >= c["without_zeros"]
    o = _oracle_tracker(oracle, 50, 5)
    full = np.full((fh.H, fh.W), 255, np.uint8)
    for naive in (False, True):
        rows = (o.track_image(seq[0][0], seq[0][1], 0.0, full, naive=True) if naive else _oracle_tracker(oracle, 50, 5).track_image(seq[0][0], seq[0][1], 0.0))
        assert len(rows) >= 20 and (rows["left"][:, 3] >= 88).all()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(LK_CASES))
def test_lk_case_conditions(oracle, name, rule):
    c = LK_CASES[name]
    h, w = c.a.shape
    n = len(c.pts)
    pt, st = fh.oracle_track(oracle, rule, c.a, c.b, c.pts, True)
    pf, sf = fh.oracle_track(oracle, rule, c.a, c.b, c.pts, False)
    p0, s0 = fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=0)
    p3, s3 = fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=c.levels[0])
    fig = dict(n=n, size=(w, h), track=int(st.sum()), track_no_flow_back=int(sf.sum()), lk_level0=int(s0.sum()), lk_top=int(s3.sum()))
    if name.startswith("tiny"):
        sizes = fh.pyramid_sizes(w, h, 3)
        fig["levels"] = sizes
        assert len(oracle.lk(c.a, c.b, c.pts, max_level=3)[0]) == n          # the oracle accepts the size with max_level 3
        differs = [not np.array_equal(_bits(fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=ml)[0]), _bits(p0)) for ml in (1, 2, 3)]
        fig["levels_above_0_change_the_result"] = differs
        if rule == "cuda":      # this tracker builds every level: the ones smaller than the 21 x 21 window are really used (each changes the result)
            assert all(differs) and all(min(sw, sh) < fh.LK_WIN for sw, sh in sizes[1:]) and max(sizes[-1]) < fh.LK_WIN
        else:                   # buildOpticalFlowPyramid stops before a level of <= 21 px: level 0 alone
            assert not any(differs) and ((w + 1) // 2 <= fh.LK_WIN or (h + 1) // 2 <= fh.LK_WIN)
    if name == "edges":
        assert 0 < st.sum() < n and 0 < sf.sum() < n                          # both status values occur
    if name.startswith("drift"):
        for ml in c.levels:
            far = tot = 0
            for init in c.inits.values():
                p, _ = fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=ml, initial=init)
                far += int((np.hypot(*(p - init).T) > 5).sum()); tot += n
            fig[f"moved_over_5px_level{ml}"] = round(far / tot, 3)
            assert far >= 0.2 * tot
        if name == "drift_tiled":      # some points lock onto the neighbouring period: their result is a period (32 px) away from another start's result
            res = np.stack([fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=0, initial=i)[0] for i in c.inits.values()])
            spread = np.abs(res[:, :, 0] - (c.pts[:, 0] + 3.0)[None, :])
            fig["locked_on_another_period"] = int((spread > 16).sum())
            assert fig["locked_on_another_period"] >= 1
    if name in ("stripes", "half_flat", "binary"):
        rej = n - int(s0.sum())
        fig["rejected"] = rej
        _, same = fh.oracle_lk(oracle, rule, c.a, c.a, c.pts, max_level=0)
        assert np.array_equal(same, s0)                                       # rejected by the matrix tests (image a alone decides), not by leaving the image
        assert 0.1 * n <= rej <= 0.9 * n
    if name in ("rotated", "noise"):
        p30, _ = fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=0, iters=30)
        p31, _ = fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=0, iters=31)
        fig["level_passes_using_all_30_iterations"] = int((_bits(p30) != _bits(p31)).any(1).sum())
        assert fig["level_passes_using_all_30_iterations"] >= 5
        fig["rejected_by_flow_back"] = int(((sf > 0) & (st == 0)).sum())
        assert fig["rejected_by_flow_back"] >= 1 and st.sum() >= 1            # forward / backward disagreement rejects some points and keeps others
        if name == "noise":
            _, same = fh.oracle_lk(oracle, rule, c.a, c.a, c.pts, max_level=c.levels[0])
            fig["left_the_image"] = int(((same > 0) & (s3 == 0)).sum())
            assert same.all() and fig["left_the_image"] >= 1                  # every point passes the matrix tests: a cleared status is an iterate outside the image
    print(f"\n[lk case] {name} {rule}: {fig}")


def test_point_set_conditions(oracle):
    sets = fh.point_sets()
    assert [len(sets[k]) for k in ("n1", "n63", "n64", "n65", "n1024")] == [1, 63, 64, 65, 1024]
    t = sets["triple"]
    assert len(t) == 63 and np.array_equal(t[0::3], t[1::3]) and np.array_equal(t[0::3], t[2::3]) and len(np.unique(t, axis=0)) == 21
    assert (np.diff(sets["rows_desc"][:, 1]) <= 0).all()
    a, b = fh.point_set_pair()
    for rule in RULES:
        p, s = fh.oracle_lk(oracle, rule, a, b, t)
        assert np.array_equal(_bits(p[0::3]), _bits(p[1::3])) and np.array_equal(s[0::3], s[2::3]) and s.sum() > 0.8 * len(t)


# =============================================================== the device against the oracle
@pytest.fixture(scope="module")
def ctx_of(gpu_ctx_factory):
    """one context per image size, created at exactly that size: the candidate buffer a user of that size gets"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            cam = _cam(fh.cam_for(w, h))
            made[(w, h)] = gpu_ctx_factory(width=w, height=h, max_cnt=150, min_dist=15, cam0=cam, cam1=cam)
        return made[(w, h)]
    return get


def _cam(p):
    from dynamic_vins_amd.frontend import make_cam
    return make_cam(*p)


def _rows_equal(g, r):
    assert len(g) == len(r), f"feature count {len(g)} vs {len(r)}"
    for name in ("id", "track_cnt", "has_right"):
        assert np.array_equal(g[name], r[name]), name
    assert np.array_equal(g["left"].view(np.uint64), r["left"].view(np.uint64)), "left observation"
    assert np.array_equal(g["right"].view(np.uint64), r["right"].view(np.uint64)), "right observation"


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_detector_bit_exact(ctx_of, oracle, name, rule):
    """response map and corners of every degenerate image, every min_dist (0, the non-integer ones, below 1), max_n that cut inside tie groups; no error on flat frames"""
    img = IMAGES[name]
    h, w = img.shape
    ctx = ctx_of(w, h)
    assert np.array_equal(_bits(ctx.min_eigen(img, rule=rule)), _bits(oracle.min_eigen(img, rule=rule)))
    for md in GFTT_MIN_DISTS:
        max_ns = [0, 7, 40]
        if name in TIE_CASES and md in (0, 3, 15):
            max_ns += fh.tie_cut_max_ns(oracle, img, md, rule)[:3]
        for max_n in max_ns:
            got = ctx.gftt(img, max_n, 0.01, md, rule=rule)
            ref = oracle.gftt(img, max_n if max_n else fh.SEL_MAX_ACC, 0.01, md, rule=rule)
            assert got.shape == ref.shape and np.array_equal(got, ref), (md, max_n)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
def test_detector_refusals_leave_the_context_usable(gpu_ctx_factory, oracle, rule):
    """a value bin over 8192 candidates -> flag 4; a min-distance grid over 32768 cells -> flag 2; each a DvinsError, and the oracle's corners right after it"""
    from dynamic_vins_amd import DvinsError
    ctx = gpu_ctx_factory(width=LIMIT_W, height=LIMIT_H, max_cnt=150, min_dist=15)
    chk, benign = _limit_images()
    ref = oracle.gftt(benign, 150, 0.01, 15, rule=rule)
    with pytest.raises(DvinsError, match=r"flags=4$"):
        ctx.gftt(chk, 150, 0.01, 3, rule=rule)
    got = ctx.gftt(benign, 150, 0.01, 15, rule=rule)
    assert np.array_equal(got, ref) and len(ref) > 50
    with pytest.raises(DvinsError, match=r"flags=2$"):
        ctx.gftt(benign, 150, 0.01, 1, rule=rule)
    assert np.array_equal(ctx.gftt(benign, 150, 0.01, 15, rule=rule), ref)
    assert np.array_equal(ctx.gftt(benign, 150, 0.01, 0.99, rule=rule), oracle.gftt(benign, 150, 0.01, 0.99, rule=rule))       # below 1 there is no grid and no limit


@pytest.mark.gpu
@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("value", [0, 255])
def test_flat_sequence_bit_exact(gpu_ctx_factory, oracle, value, naive):
    """three stereo frames with a saturated region over 2/3 of the frame through the tracker, raw mode and naive mode (the GPU detector's rule): rows bit for bit"""
    from dynamic_vins_amd.frontend import DV_MODE_NAIVE
    cam = fh.cam_for(fh.W, fh.H)
    c = gpu_ctx_factory(width=fh.W, height=fh.H, max_cnt=50, min_dist=5, cam0=_cam(cam), cam1=_cam(cam))
    o = _oracle_tracker(oracle, 50, 5)
    full = np.full((fh.H, fh.W), 255, np.uint8)
    for k, (l, r) in enumerate(fh.flat_sequence(value)):
        if naive:
            g, ref = c.track_stereo(l, r, 0.05 * k, full, DV_MODE_NAIVE), o.track_image(l, r, 0.05 * k, full, naive=True)
        else:
            g, ref = c.track_stereo(l, r, 0.05 * k), o.track_image(l, r, 0.05 * k)
        _rows_equal(g, ref)
    assert len(g) >= 20


@pytest.mark.gpu
def test_crowded_discs_bit_exact(gpu_ctx_factory, ctx_of, oracle):
    """the contracting sequence at min_dist 2, max_cnt 1024 on 130 x 70: more than DISC_CAP discs reach a tile (the fallback that tests every disc), the tracker fills to its
    capacity and the position order ranks 1024 points with equal keys among them"""
    cam = fh.cam_for(fh.W, fh.H)
    c = gpu_ctx_factory(width=fh.W, height=fh.H, max_cnt=fh.CROWD_MAX_CNT, min_dist=fh.CROWD_MIN_DIST, cam0=_cam(cam), cam1=_cam(cam))
    o = _oracle_tracker(oracle, fh.CROWD_MAX_CNT, fh.CROWD_MIN_DIST)
    seq = fh.crowded_sequence()
    first = None
    for k, (l, r) in enumerate(seq):
        g, ref = c.track_stereo(l, r, 0.05 * k), o.track_image(l, r, 0.05 * k)
        _rows_equal(g, ref)
        first = ref if first is None else first
    # the operator form: the same discs stamped into a mask, the detector under it
    op = ctx_of(fh.W, fh.H)
    pts = np.ascontiguousarray(first["left"][:, 3:5], np.float32)
    full = np.full((fh.H, fh.W), 255, np.uint8)
    mo, mg = oracle.circle_mask(full, pts, fh.CROWD_MIN_DIST), op.circle_mask(full, pts, fh.CROWD_MIN_DIST)
    assert np.array_equal(mo, mg)
    for rule in RULES:
        got, ref = op.gftt(seq[1][0], 0, 0.01, fh.CROWD_MIN_DIST, mg, rule=rule), oracle.gftt(seq[1][0], fh.SEL_MAX_ACC, 0.01, fh.CROWD_MIN_DIST, mo, rule=rule)
        assert np.array_equal(got, ref)


def _dev_lk(ctx, rule, a, b, pts, **kw):
    return ctx.lk_cuda(a, b, pts, **kw) if rule == "cuda" else ctx.lk(a, b, pts, **kw)


def _dev_track(ctx, rule, a, b, pts, flow_back):
    return ctx.track_by_lk_gpu(a, b, pts, flow_back) if rule == "cuda" else ctx.track_by_lk(a, b, pts, flow_back, 0.5)


def _same(dev, ref, what):
    assert np.array_equal(dev[1], ref[1]), ("status", what)
    assert np.array_equal(_bits(dev[0]), _bits(ref[0])), ("positions", what)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(LK_CASES))
def test_tracker_bit_exact(ctx_of, oracle, name, rule):
    """every tracker case four ways: single direction at each max_level, the same with every initial flow of the case, fused with and without the backward check"""
    c = LK_CASES[name]
    h, w = c.a.shape
    ctx = ctx_of(w, h)
    for ml in c.levels:
        _same(_dev_lk(ctx, rule, c.a, c.b, c.pts, max_level=ml), fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=ml), (ml, "no initial flow"))
        for key, init in c.inits.items():
            _same(_dev_lk(ctx, rule, c.a, c.b, c.pts, max_level=ml, initial=init), fh.oracle_lk(oracle, rule, c.a, c.b, c.pts, max_level=ml, initial=init), (ml, key))
    for fb in (True, False):
        _same(_dev_track(ctx, rule, c.a, c.b, c.pts, fb), fh.oracle_track(oracle, rule, c.a, c.b, c.pts, fb), ("fused", fb))


@pytest.mark.gpu
@pytest.mark.parametrize("rule", RULES)
def test_point_sets_bit_exact(ctx_of, oracle, rule):
    """point counts around a wavefront and at the tracker's capacity, every point three times, rows descending: per point the oracle's result and the result of the
    same point submitted alone"""
    a, b = fh.point_set_pair()
    h, w = a.shape
    ctx = ctx_of(w, h)
    sets = fh.point_sets()
    for key, pts in sets.items():
        dev = _dev_lk(ctx, rule, a, b, pts)
        _same(dev, fh.oracle_lk(oracle, rule, a, b, pts), key)
        devt = _dev_track(ctx, rule, a, b, pts, True)
        _same(devt, fh.oracle_track(oracle, rule, a, b, pts, True), (key, "fused"))
        step = 3 if key == "triple" else max(1, len(pts) // 16)
        for i in range(0, len(pts), step):
            one = _dev_lk(ctx, rule, a, b, pts[i:i + 1])
            assert one[1][0] == dev[1][i] and np.array_equal(_bits(one[0][0]), _bits(dev[0][i])), (key, i)
            one = _dev_track(ctx, rule, a, b, pts[i:i + 1], True)
            assert one[1][0] == devt[1][i] and np.array_equal(_bits(one[0][0]), _bits(devt[0][i])), (key, i, "fused")
