"""Object-tracker parity on hostile detections (generators, restatements and conditions: tests/inst_hostile.py).

CPU (`-m "not gpu"`): every case is shown, on the oracle alone or on a numpy restatement, to reach the branch it is named for — the level count of the ROI pyramid, an
eroded-away mask, points lost to a size change, the lost_num life cycle, more objects than the tables start with, the caps, non-finite velocities, each side of the
association's tests, the detector's limits — and the figures are printed.
GPU: dv_track_stereo_enqueue / dv_inst_track_enqueue / the two collects against OracleTracker.track_image + OracleInsts.track on the same frames, bit for bit: the
background rows, the instance table field by field, the object rows (ids, track counts, has_right, uint64 patterns), the points.  No tolerance anywhere.
The limits (include/dvins.h beside dv_inst_config): a frame one of whose objects exceeds one is refused by dv_inst_track_collect with "device error flags=N", the
context stays usable, and after dv_inst_reset parity holds again.  Flag 8 (extra points) needs an image 8000 px wide and is driven through the operator form in
tests/test_extra_points_hostile.py; flag 16 is no longer raised (include/dvins.h)."""
import ctypes as C

import numpy as np
import pytest

from tests import front_hostile as fh
from tests import inst_hostile as ih

GEOMETRY = ih.geometry_cases()
RESIZE = ih.resize_cases()
CONTENT = ih.content_cases()
CONFIG = ih.config_cases()
ASSOC = ih.assoc_cases()
MISSES = (1, 2, 3, 4)
_REF = {}


def ref_of(oracle, case):
    """the oracle's output of a case, computed once and shared by the condition test and the device test"""
    if case.name not in _REF:
        _REF[case.name] = ih.run_oracle(oracle, case)[0]
    return _REF[case.name]


@pytest.fixture(scope="module")
def gpu(gpu_ctx_factory):
    return True


def counts(ref, track_id):
    return [len(ih.obj_feats(f, track_id)) for f in ref]


# =============================================================== conditions (oracle only)
@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_geometry_conditions(oracle, name):
    """A: the restated level rule gives the claimed count; a mask that erodes to nothing yields no corner; every other ROI that has interior pixels yields corners and
    keeps one on the second frame.  (cv::erode does not erode from outside the image: a mask of ones stays as it is however small the ROI, so the empty erosion needs an
    object smaller than its box — the rim_* cases; with a mask of ones only ROIs of 1 or 2 px, which have no interior pixel, are barren.)"""
    case, levels = GEOMETRY[name]
    d = case.dets[0][0]
    x, y, w, h = d["rect"]
    ref = ref_of(oracle, case)
    n0, n1 = counts(ref, 5)
    kept = int((ih.obj_feats(ref[1], 5)["track_cnt"] >= 2).sum())
    er = ih.erode_np(d["mask"])
    assert np.array_equal(er, oracle.erode(d["mask"], 5))
    print(f"\n[geometry] {name}: rect {d['rect']}, levels {ih.roi_levels(w, h)}, eroded mask pixels {int((er > 0).sum())} of {w * h}, corners {n0}, kept on frame 1: {kept} of {n1}")
    assert ih.roi_levels(w, h) == levels
    if name.startswith("rim_") or min(w, h) <= 2:
        assert (name.startswith("rim_") and not er.any()) or min(w, h) <= 2
        assert n0 == 0 and n1 == 0
    elif name.startswith("ones_") and min(w, h) <= 5:
        assert er.all()                                                # the border rule: nothing eroded, the 3 x 3 (2 x 2) interior is searched
        assert (n0, n1) == {"ones_4x4": (0, 1), "ones_5x5": (1, 1)}[name]      # what the oracle finds there on these frames (pinned; frame 1 of 4 x 4 finds one)
    else:
        assert n0 >= 1 and kept >= 1
    if name.startswith("levels"):
        assert levels == int(name[6])
    if name.startswith("flush"):
        assert x == 0 or y == 0 or x + w == case.w or y + h == case.h


def test_level_rule_boundaries():
    got = {s: ih.roi_levels(s, s) for s in (21, 22, 41, 42, 43, 83, 84, 85, 86, 167, 168, 169, 170)}
    print(f"\n[levels] square ROI side -> levels: {got}; mask pitches {[(w, (w + 15) // 16 * 16) for w in (1, 16, 17, 43)]}")
    assert [got[s] for s in (41, 42, 43)] == [1, 1, 2] and [got[s] for s in (83, 84, 85, 86)] == [2, 2, 3, 3] and [got[s] for s in (167, 168, 169, 170)] == [3, 3, 4, 4]
    assert ih.roi_levels(17, 200) == 1 and ih.roi_levels(200, 43) == 2


@pytest.mark.parametrize("name", sorted(RESIZE))
def test_resize_conditions(oracle, name):
    """B: between frame 0 and frame 1 at least one previous point is lost TO the padded border (kept when the zero fill is replaced by the frames' real pixels) or to the
    InBorder test (passes both LK passes and the 0.5 px test), shown by ih.resize_loss_causes' restatement, which must keep exactly the points the oracle's object manager
    keeps; and at least one survives with track_cnt >= 2"""
    case = RESIZE[name]
    ref = ref_of(oracle, case)
    (x0, y0, w0, h0), (x1, y1, w1, h1) = case.dets[0][0]["rect"], case.dets[1][0]["rect"]
    f0, f1 = ih.obj_feats(ref[0], 9), ih.obj_feats(ref[1], 9)
    kept = int((f1["track_cnt"] >= 2).sum())
    # the previous points stay ROI-local: a point of frame 0 at (u, v) shows the scene point that frame 1's ROI holds at (u + x0 - x1 - 1, v + y0 - y1)
    u, v = f0["left"][:, 3] + x0 - x1 - 1, f0["left"][:, 4] + y0 - y1
    outside = int(((u < 1) | (v < 1) | (u > w1 - 2) | (v > h1 - 2) | (u > max(w0, w1) - 2) | (v > max(h0, h1) - 2)).sum())
    why = ih.resize_loss_causes(oracle, case, f0)
    n_pad, n_inb = int(why["padding"].sum()), int(why["in_border"].sum())
    print(f"\n[resize] {name}: {case.dets[0][0]['rect']} -> {case.dets[1][0]['rect']}, levels {ih.roi_levels(max(w0, w1), max(h0, h1))} (was {ih.roi_levels(w0, h0)}), "
          f"{len(f0)} points, {kept} survive, {len(f0) - kept} lost: {n_pad} to the zero padding, {n_inb} to InBorder ({outside} scene points leave the new ROI)")
    assert np.array_equal(f0["id"][why["status"]], f1["id"][f1["track_cnt"] >= 2])          # the restated tracking is the object manager's
    assert n_pad + n_inb >= 1 and kept >= 1
    if name in ("grow_41_43", "shrink_43_41"):
        assert {ih.roi_levels(w0, h0), ih.roi_levels(w1, h1)} == {1, 2}


@pytest.mark.parametrize("order", ["desc", "shuffled"])
@pytest.mark.parametrize("miss", MISSES)
def test_life_cycle_conditions(oracle, miss, order):
    """C: new ids go to the background first, then to the objects by ascending id whatever the list order; the object that returns after one miss keeps an old id, the
    one that returns after erasure (two misses or more) keeps none"""
    case, back = ih.life_case(miss, order)
    ref = ref_of(oracle, case)
    assert [int(d["track_id"]) for d in case.dets[0]] != [3, 7, 11]
    blocks0, ok0 = ih.new_ids_in_order(ref[0])
    assert blocks0 == 4 and ok0                                        # background + three objects new in the same frame
    assert all(ih.new_ids_in_order(f)[1] for f in ref)
    before, after = ih.obj_feats(ref[1], 7), ih.obj_feats(ref[back], 7)
    old = int(np.isin(after["id"], before["id"]).sum())
    vis = [[int(i) for i in f[1]["id"]] for f in ref]
    print(f"\n[life] miss {miss} {order}: visible per frame {vis}; object 7 had {len(before)} points, returns in frame {back} with {len(after)}, {old} old ids, "
          f"max track_cnt {int(after['track_cnt'].max())}")
    for k, f in enumerate(ref):
        assert (7 in vis[k]) == (not 2 <= k < 2 + miss) and 3 in vis[k] and 11 in vis[k]
    assert len(after) >= 1
    assert old >= 1 if miss == 1 else (old == 0 and int(after["track_cnt"].max()) == 1)


@pytest.mark.parametrize("with_disparity", [False, True])
def test_count_conditions(oracle, with_disparity):
    """D: 1, 9, 17, 1 objects: rows for every object of the 17-object frame (and points for every one when the disparity map is set)"""
    case = ih.count_case(with_disparity)
    ref = ref_of(oracle, case)
    n = [len(f[1]) for f in ref]
    print(f"\n[counts] disparity {with_disparity}: objects per frame {n}, rows {[len(f[2]) for f in ref]}, points {[len(f[3]) for f in ref]}, fewest rows of an object in frame 2: {int(ref[2][1]['n_feats'].min())}")
    assert n == [1, 9, 17, 1] and (ref[2][1]["n_feats"] >= 1).all()
    assert sorted(ref[2][1]["id"]) == list(ref[2][1]["id"]) and len(set(ref[2][1]["id"])) == 17
    if with_disparity:
        assert (ref[2][1]["n_points"] >= 1).all() and (ref[1][1]["n_points"] >= 1).all()
    else:
        assert all(len(f[3]) == 0 for f in ref)


@pytest.mark.parametrize("name", sorted(CONTENT))
def test_content_conditions(oracle, name):
    """E: the per-object count is 0 in the empty cases and equals the cap in the cap cases"""
    case, want = CONTENT[name]
    ref = ref_of(oracle, case)
    n = counts(ref, 4)
    print(f"\n[content] {name}: rows per frame {n}, tracked {[int((ih.obj_feats(f, 4)['track_cnt'] >= 2).sum()) for f in ref]}")
    if want is not None:
        assert n[0] == want
    if want == 0:
        assert not any(n)
    if name == "cap4":
        assert n == [4, 4, 4] and (ih.obj_feats(ref[1], 4)["track_cnt"] == 2).all()          # at the cap, every point tracked: the next frame wants no corner
    if name in ("noise2", "checker"):
        assert n[0] >= 10


@pytest.mark.parametrize("name", sorted(CONFIG))
def test_config_conditions(oracle, name):
    """F: stereo 0 leaves no right observation; the backward check rejects points that flow_back 0 keeps; equal timestamps give non-finite velocities"""
    case = CONFIG[name]
    ref = ref_of(oracle, case)
    fo = ref[2][2]
    vel = np.concatenate([fo["left"][:, 5:7].ravel(), fo["right"][:, 5:7].ravel()])
    print(f"\n[config] {name}: {len(fo)} object rows in frame 2, {int(fo['has_right'].sum())} with a right observation, velocities: {int(np.isinf(vel).sum())} inf, {int(np.isnan(vel).sum())} nan")
    assert len(fo) >= 10
    if name == "mono":
        assert not fo["has_right"].any() and not ref[2][0]["has_right"].any()
    else:
        assert fo["has_right"].sum() >= 5
    if name == "equal_times":
        assert not np.isfinite(vel).all()
    if name == "flow_back0":
        a, b = ref_of(oracle, CONFIG["flow_back0"]), ref_of(oracle, CONFIG["flow_back1"])
        assert any(not np.array_equal(x[2]["id"], y[2]["id"]) or not np.array_equal(x[2]["has_right"], y[2]["has_right"]) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(ASSOC))
def test_association_conditions(oracle, name):
    """G: the crafted pair falls on the stated side (IoU in float32 as rect_iou computes it) and the oracle associates as the restated loop does"""
    case, want = ASSOC[name]
    dets, boxes = case.dets[0], case.boxes3d[0]
    ious = {(d["track_id"], i): float(ih.rect_iou_f32(d["rect"], ih.box_rect(b))) for d in dets for i, b in enumerate(boxes)}
    got = ih.np_associate(dets, boxes)
    print(f"\n[association] {name}: IoU {ious}, restated {got}")
    assert got == want
    io = ref_of(oracle, case)[0][1]
    for o in io:
        i = got.get(int(o["id"]))
        assert int(o["has_box3d"]) == int(i is not None)
        if i is not None:
            assert o["box3d"].tobytes() == boxes[i].tobytes()
    if name == "iou_above":
        assert 0.1 < ious[(2, 0)] < 0.102
    if name == "iou_below":
        assert 0.09 < ious[(2, 0)] < 0.1
    if name == "iou_exactly_0.1":
        assert np.float32(ious[(2, 0)]) == np.float32(0.1)
    if name == "half_to_even":
        assert ih.box_rect(boxes[0]) == (54, 5, 60, 50) and ih.rect_iou_f32(dets[0]["rect"], (55, 5, 60, 50)) < np.float32(0.1)
    if name == "equal_distance":
        assert np.hypot(3.0, 4.0) == 5.0
    if name == "nan_centre":
        assert ious[(2, 0)] > 0.5


@pytest.mark.parametrize("rule", ["cpu"])
def test_limit_conditions(oracle, rule):
    """H: the grid limit on both sides at min_dynamic_dist 1, and at the workload's parameters; the value-bin limit of the 4 px checkerboard object; the candidate buffer
    of an ROI that covers its frame is exceeded by the 2 and 3 px checkerboards and by no block-noise or binary image (flag 1: the 2 px one at 130 x 70 is the case)"""
    ok, bad = ih.grid_limit_case(172), ih.grid_limit_case(173)
    cells = [ih.grid_cells(*c.dets[0][0]["rect"][2:], c.inst_min) for c in (ok, bad)]
    work = ih.grid_cells(1240, 700, 5)
    print(f"\n[limits] grid cells {cells} around {fh.SEL_MAX_CELLS}; a 1240 x 700 detection at min_dynamic_dist 5: {work} cells")
    assert cells == [32680, 32870] and cells[0] <= fh.SEL_MAX_CELLS < cells[1]
    assert work == 248 * 140 == 34720 > fh.SEL_MAX_CELLS
    assert len(ref_of(oracle, ok)[0][2]) == 50                       # the accepted ROI fills the object on the oracle
    b = ih.bin_limit_case()
    c = fh.census(oracle, b.frames[0][0], rule)
    print(f"[limits] 4 px checkerboard object {ih.LIMIT}: {c}; grid cells at min_dynamic_dist 3: {ih.grid_cells(*ih.LIMIT, 3)}")
    assert c["top_bin"] > fh.SEL_CAP and c["with_zeros"] <= c["cap"] and ih.grid_cells(*ih.LIMIT, 3) <= fh.SEL_MAX_CELLS
    cen = ih.flag1_census(oracle)
    print(f"[limits] largest candidate census / buffer: {cen[:5]}")
    assert all(n <= cap for name, _, n, cap in cen if not name.startswith("checker"))
    c1 = fh.census(oracle, ih.cand_limit_case().frames[0][0], rule)
    print(f"[limits] 2 px checkerboard object {ih.SMALL}: {c1}")
    assert c1["without_zeros"] > c1["cap"] and c1["without_zeros"] <= fh.SEL_CAP + c1["cap"] and ih.grid_cells(*ih.SMALL, 5) <= fh.SEL_MAX_CELLS


# =============================================================== the device against the oracle
def _run(oracle, case):
    ih.sequences_equal(ih.run_device(case), ref_of(oracle, case), case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_geometry_bit_exact(gpu, oracle, name):
    _run(oracle, GEOMETRY[name][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RESIZE))
def test_resize_bit_exact(gpu, oracle, name):
    _run(oracle, RESIZE[name])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["desc", "shuffled"])
@pytest.mark.parametrize("miss", MISSES)
def test_life_cycle_bit_exact(gpu, oracle, miss, order):
    _run(oracle, ih.life_case(miss, order)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("with_disparity", [False, True])
def test_counts_bit_exact(gpu, oracle, with_disparity):
    _run(oracle, ih.count_case(with_disparity))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONTENT))
def test_content_bit_exact(gpu, oracle, name):
    _run(oracle, CONTENT[name][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONFIG))
def test_config_bit_exact(gpu, oracle, name):
    _run(oracle, CONFIG[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ASSOC))
def test_association_bit_exact(gpu, oracle, name):
    _run(oracle, ASSOC[name][0])


@pytest.mark.gpu
def test_grid_limit_accepted_bit_exact(gpu, oracle):
    _run(oracle, ih.grid_limit_case(172))


def _well_formed(out):
    rows, insts, feats, pts = out
    assert len(insts) >= 1 and int(insts["n_feats"].sum()) == len(feats) and int(insts["n_points"].sum()) == len(pts)
    assert np.array_equal(insts["first_feat"], np.concatenate([[0], np.cumsum(insts["n_feats"])[:-1]]))
    assert len(set(feats["id"])) == len(feats) and (feats["track_cnt"] >= 1).all()


@pytest.mark.gpu
def test_grid_limit_refused(gpu, oracle):
    """flag 2: the 190 x 173 ROI at min_dynamic_dist 1 is refused by the collect, which names the flag and returns nothing; the next pair works (the object, left without
    points, is detected afresh: what a new object manager of the oracle yields); after dv_inst_reset and a fresh oracle.insts parity holds on the benign pair"""
    from dynamic_vins_amd import DvinsError
    case = ih.grid_limit_case(173)
    cam = case.cam()
    trk = oracle.tracker(case.w, case.h, case.bg[0], case.bg[1], 1, 1, cam, cam)
    ctx = ih.make_ctx(case)
    try:
        l, r = case.frames[0]
        ctx.track_stereo_enqueue(l, r, case.times[0])
        ctx.inst_track_enqueue(case.times[0], case.dets[0])
        ih.rows_equal(ctx.track_stereo_collect(), trk.track_image(l, r, case.times[0]), "frame 0 background")
        with pytest.raises(DvinsError, match=r"device error flags=2\b"):
            ctx.inst_track_collect()
        out = ih.device_frame(ctx, case, 1)
        _well_formed(out)
        ih.frame_equal(out, ih.run_oracle(oracle, case, tracker=trk, frames=[1])[0][0], "frame behind the refusal")
        ctx.inst_reset()
        ref = ih.run_oracle(oracle, case, tracker=trk, frames=[2, 3])[0]
        for k in (2, 3):
            ih.frame_equal(ih.device_frame(ctx, case, k), ref[k - 2], f"frame {k} behind dv_inst_reset")
        assert len(ref[1][2]) == 50 and (ref[1][2]["track_cnt"] == 2).sum() >= 25
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [1, 4])
def test_frame_limit_refused(gpu, oracle, flag):
    """flag 4: the 4 px checkerboard as an object over the whole 320 x 240 frame; flag 1: the 2 px checkerboard over the whole 130 x 70 frame (the background tracker
    refuses the same image for the same reason); after a reset of both trackers parity holds on the benign pair"""
    from dynamic_vins_amd import DvinsError
    case = ih.bin_limit_case() if flag == 4 else ih.cand_limit_case()
    ctx = ih.make_ctx(case)
    try:
        l, r = case.frames[0]
        ctx.track_stereo_enqueue(l, r, case.times[0])
        ctx.inst_track_enqueue(case.times[0], case.dets[0])
        with pytest.raises(DvinsError, match=rf"device error flags={flag}\b"):
            ctx.track_stereo_collect()
        with pytest.raises(DvinsError, match=rf"object tracker device error flags={flag}\b"):
            ctx.inst_track_collect()
        ctx.reset()
        ref = ih.run_oracle(oracle, case, first=1)[0]
        for k in (1, 2):
            ih.frame_equal(ih.device_frame(ctx, case, k), ref[k - 1], f"frame {k} behind the reset")
        assert len(ref[1][2]) >= 20
    finally:
        ctx.close()


@pytest.mark.gpu
def test_host_refusals_leave_the_tracker_usable(gpu, oracle):
    """a rectangle outside the image, two detections with one id, a detection without a mask, a second enqueue before the collect: each is refused with its message and
    the frame then goes through with the good list, bit for bit; a collect into buffers that are too small loses its frame, and the next frame is the oracle's"""
    from dynamic_vins_amd import DvinsError
    from dynamic_vins_amd.frontend import dv_inst_det
    case = ih.life_case(1, "desc")[0]
    ref = ref_of(oracle, case)
    ctx = ih.make_ctx(case)

    def bad_lists(k):
        good = case.dets[k]
        m = np.full((10, 10), 255, np.uint8)
        yield "outside the image", good[:1] + [dict(track_id=99, class_id=0, rect=(case.w - 5, 3, 10, 10), mask=m, points=None)]
        yield "outside the image", [dict(track_id=98, class_id=0, rect=(-1, 3, 10, 10), mask=m, points=None)]
        yield "same track id", good + [dict(good[0])]

    try:
        for k in range(len(case.frames)):
            l, r = case.frames[k]
            ctx.track_stereo_enqueue(l, r, case.times[k])
            if k < 3:
                for msg, dets in bad_lists(k):
                    with pytest.raises(DvinsError, match=msg):
                        ctx.inst_track_enqueue(case.times[k], dets)
            if k == 3:
                arr = (dv_inst_det * 1)()
                arr[0].track_id, arr[0].x, arr[0].y, arr[0].w, arr[0].h, arr[0].mask = 3, 6, 8, 34, 30, None
                assert ctx.lib.dv_inst_track_enqueue(ctx.h, case.times[k], C.addressof(arr), 1, None, 0) != 0
                assert b"without a mask" in ctx.lib.dv_last_error(ctx.h)
            ctx.inst_track_enqueue(case.times[k], case.dets[k])
            if k == 1:
                with pytest.raises(DvinsError, match="not collected"):
                    ctx.inst_track_enqueue(case.times[k], case.dets[k])
            rows = ctx.track_stereo_collect()
            if k == 2:
                oi, of, op = ctx._inst_out
                ni, nf, npt = C.c_int(7), C.c_int(7), C.c_int(7)
                assert ctx.lib.dv_inst_track_collect(ctx.h, oi.ctypes.data, len(oi), C.byref(ni), of.ctypes.data, 3, C.byref(nf), op.ctypes.data, len(op), C.byref(npt)) != 0
                assert b"too small" in ctx.lib.dv_last_error(ctx.h)
                ih.rows_equal(rows, ref[k][0], "frame 2 background")
                continue
            ih.frame_equal((rows,) + tuple(ctx.inst_track_collect()), ref[k], f"{case.name} frame {k}")
    finally:
        ctx.close()
