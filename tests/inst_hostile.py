"""Hostile detections for the object tracker's parity tests (tests/test_inst_hostile.py): ROIs on the level-count boundaries of the ROI pyramid, ROIs smaller than the
tracking window or the erosion kernel, size changes between frames, objects that come and go, more objects than the tracker's tables start with, empty and saturated
contents, the caps, the configuration switches, the 2-D / 3-D box association's ties, and the detector's limits.  After the pattern of tests/front_hostile.py: the
generators return plain inputs (a Case), the conditions are asserted on the ORACLE ALONE or on the numpy restatements below, and prove that a case reaches the branch it
is named for.  If a seed fails a condition, take another seed, never loosen the condition.

Restated from csrc/inst_track.hip: RoiPyr::layout's level rule, rect_iou + the association loop, the min-distance grid of the selection (csrc/gftt.hip)."""
import numpy as np

from dynamic_vins_amd.dynsim import BOX3D_DTYPE, INSTOBS_DTYPE
from tests import front_hostile as fh

LK_WIN, MAX_LEVELS = 21, 4
SMALL = (130, 70)            # level counts 1 and 2
MID = (200, 180)             # all four level counts; the grid limit at min_dynamic_dist 1
LIMIT = (320, 240)           # front_hostile's limit images
BASELINE = 0.12


# ---------------------------------------------------------------- restatements
def roi_levels(w, h):
    """RoiPyr::layout: a level is added only while the next one exceeds the window in both directions"""
    n = 1
    while n < MAX_LEVELS:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= LK_WIN or h <= LK_WIN:
            break
        n += 1
    return n


def grid_cells(w, h, min_dist):
    """cells of the selection's min-distance grid over a w x h ROI (0 below min_dist 1: no grid)"""
    if min_dist < 1:
        return 0
    c = int(np.rint(min_dist))
    return ((w + c - 1) // c) * ((h + c - 1) // c)


def rect_iou_f32(a, b):
    """Box2D::IoU on (x, y, w, h) in float32, operation by operation as rect_iou"""
    f = np.float32
    a, b = [f(v) for v in a], [f(v) for v in b]
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    x2, y2 = min(f(a[0] + a[2]), f(b[0] + b[2])), min(f(a[1] + a[3]), f(b[1] + b[3]))
    inter = f(f(x2 - x1) * f(y2 - y1)) if (x2 > x1 and y2 > y1) else f(0)
    un = f(f(f(a[2] * a[3]) + f(b[2] * b[3])) - inter)
    return f(0) if un < 2.220446049250313e-16 else f(inter / un)


def box_rect(b):
    """cv::Rect(Point2f min, Point2f max): corners rounded half to even"""
    x0, y0, x1, y1 = [int(np.rint(np.float32(v))) for v in (b["rect_min"][0], b["rect_min"][1], b["rect_max"][0], b["rect_max"][1])]
    return (x0, y0, x1 - x0, y1 - y0)


def np_associate(dets, boxes):
    """BoxAssociate2Dto3D: objects in ascending id; same class, IoU > 0.1f, the nearest centre wins (first index on a tie, a NaN never), every box used once
    -> {track_id: box index}"""
    taken, out = set(), {}
    for d in sorted(dets, key=lambda d: d["track_id"]):
        best, bi = np.inf, -1
        for i, b in enumerate(boxes):
            if i in taken or int(b["class_id"]) != int(d.get("class_id", 0)):
                continue
            if not rect_iou_f32(d["rect"], box_rect(b)) > np.float32(0.1):
                continue
            dn = float(np.sqrt(b["center"][0] * b["center"][0] + b["center"][1] * b["center"][1] + b["center"][2] * b["center"][2]))
            if dn < best:
                best, bi = dn, i
        if bi >= 0:
            taken.add(bi)
            out[int(d["track_id"])] = bi
    return out


def erode_np(mask, k=5):
    """cv::erode with a k x k rectangle: pixels outside the image do not erode (the border value is the maximum)"""
    h, w = mask.shape
    a = k // 2
    pad = np.full((h + 2 * a, w + 2 * a), 255, np.uint8)
    pad[a:a + h, a:a + w] = mask
    out = np.full((h, w), 255, np.uint8)
    for dy in range(k):
        for dx in range(k):
            out = np.minimum(out, pad[dy:dy + h, dx:dx + w])
    return out


# ---------------------------------------------------------------- frames and detections
def stereo_frames(w, h, n, seed=9, step=(1, 0), disp=2, sigma=1.2):
    """n stereo frames cut from one texture that drifts by `step` px per frame; the right image sees it `disp` px further left"""
    m = 8 + max(abs(step[0]), abs(step[1])) * n
    tex = fh.tex_u8(h + 2 * m, w + 2 * m + disp, seed, sigma)
    out = []
    for k in range(n):
        x0, y0 = m + step[0] * k, m + step[1] * k
        out.append((np.ascontiguousarray(tex[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(tex[y0:y0 + h, x0 + disp:x0 + disp + w])))
    return out


def det(track_id, rect, mask=None, class_id=0, value=255):
    x, y, w, h = rect
    m = np.full((h, w), value, np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8)
    assert m.shape == (h, w)
    return dict(track_id=int(track_id), class_id=int(class_id), rect=(int(x), int(y), int(w), int(h)), mask=m, points=None)


def rim_mask(w, h, value=255):
    """an object one pixel smaller than its box on every side"""
    m = np.zeros((h, w), np.uint8)
    m[1:h - 1, 1:w - 1] = value
    return m


def box3d(class_id, center, rect_min, rect_max):
    b = np.zeros(1, BOX3D_DTYPE)
    b["class_id"], b["score"], b["center"], b["dims"], b["yaw"] = class_id, 0.9, center, (1.5, 1.4, 3.9), 0.1
    b["rect_min"], b["rect_max"] = rect_min, rect_max
    return b


class Case:
    """one sequence: frames [(left, right)], per frame the detection list (and the 3-D boxes / the disparity map), the two trackers' parameters"""

    def __init__(self, name, size, frames, dets, boxes3d=None, disp=None, inst_max=50, inst_min=5, use_det3d=0, stereo=1, flow_back=1, times=None, bg=(30, 10)):
        self.name, (self.w, self.h), self.frames, self.dets = name, size, frames, dets
        assert len(dets) == len(frames)
        self.boxes3d = boxes3d if boxes3d is not None else [None] * len(frames)
        self.disp = disp
        self.inst_max, self.inst_min, self.use_det3d, self.stereo, self.flow_back, self.bg = inst_max, inst_min, use_det3d, stereo, flow_back, bg
        self.times = list(times) if times is not None else [0.05 * k for k in range(len(frames))]
        for dl in dets:
            for d in dl:
                x, y, w, h = d["rect"]
                assert 0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= self.w and y + h <= self.h, (name, d["rect"])

    def cam(self):
        return fh.cam_for(self.w, self.h)


def disparity_map(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(6.0 + 0.01 * xx + 0.005 * yy, np.float32)


# ---------------------------------------------------------------- the two sides
def run_oracle(oracle, case, first=0, tracker=None, frames=None):
    """-> ([(rows, insts, feats, points)] per frame, the oracle tracker); tracker / first / frames: go on with an existing background tracker and a FRESH object manager"""
    cam = case.cam()
    trk = tracker if tracker is not None else oracle.tracker(case.w, case.h, case.bg[0], case.bg[1], case.flow_back, case.stereo, cam, cam)
    oin = oracle.insts(trk, case.inst_max, case.inst_min, case.use_det3d)
    out = []
    for k in (frames if frames is not None else range(first, len(case.frames))):
        l, r = case.frames[k]
        rows = trk.track_image(l, r, case.times[k])
        if case.disp is not None:
            oin.set_disparity(case.disp, BASELINE)
        io, fo, po = oin.track(l, r, case.times[k], case.dets[k], case.boxes3d[k] if case.use_det3d else None, INSTOBS_DTYPE, BOX3D_DTYPE)
        out.append((rows, io, fo, po))
    return out, trk


def make_ctx(case):
    from dynamic_vins_amd.frontend import Context, make_cam
    cam = make_cam(*case.cam())
    ctx = Context(width=case.w, height=case.h, max_cnt=case.bg[0], min_dist=case.bg[1], flow_back=case.flow_back, stereo=case.stereo, cam0=cam, cam1=cam)
    ctx.inst_config(case.inst_max, case.inst_min, case.use_det3d)
    return ctx


def device_frame(ctx, case, k, dets=None):
    l, r = case.frames[k]
    ctx.track_stereo_enqueue(l, r, case.times[k])
    if case.disp is not None:
        ctx.inst_set_disparity(case.disp, BASELINE)
    ctx.inst_track_enqueue(case.times[k], case.dets[k] if dets is None else dets, case.boxes3d[k] if case.use_det3d else None)
    rows = ctx.track_stereo_collect()
    return (rows,) + tuple(ctx.inst_track_collect())


def run_device(case):
    ctx = make_ctx(case)
    try:
        return [device_frame(ctx, case, k) for k in range(len(case.frames))]
    finally:
        ctx.close()


def rows_equal(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} vs {len(b)} rows"
    for name in ("id", "track_cnt", "has_right"):
        assert np.array_equal(a[name], b[name]), f"{what}: {name}"
    assert np.array_equal(a["left"].view(np.uint64), b["left"].view(np.uint64)), f"{what}: left observation"
    assert np.array_equal(a["right"].view(np.uint64), b["right"].view(np.uint64)), f"{what}: right observation"


def frame_equal(dev, ref, what):
    """background rows, the instance table field by field, the object rows and the points, bit for bit"""
    rows, insts, feats, pts = dev
    rows_o, io, fo, po = ref
    rows_equal(rows, rows_o, f"{what} background")
    assert len(io) == len(insts), f"{what}: {len(insts)} vs {len(io)} objects"
    for name in ("id", "has_box3d", "first_feat", "n_feats", "first_point", "n_points"):
        assert np.array_equal(io[name], insts[name]), f"{what}: {name} {insts[name]} vs {io[name]}"
    assert np.array_equal(io["rect"].view(np.uint32), insts["rect"].view(np.uint32)), f"{what}: rect"
    assert io["box3d"].tobytes() == insts["box3d"].tobytes(), f"{what}: box3d"
    rows_equal(feats, fo, f"{what} objects")
    assert po.shape == pts.shape and np.array_equal(po.view(np.uint64), pts.view(np.uint64)), f"{what}: points"


def sequences_equal(dev, ref, name):
    assert len(dev) == len(ref)
    for k, (d, r) in enumerate(zip(dev, ref)):
        frame_equal(d, r, f"{name} frame {k}")


def obj_feats(frame, track_id):
    """the object rows of one id in one frame's output (empty when it is not in the table)"""
    _, io, fo, _ = frame
    for o in io:
        if int(o["id"]) == track_id:
            return fo[o["first_feat"]: o["first_feat"] + o["n_feats"]]
    return fo[:0]


def new_ids_in_order(frame):
    """the ids of the frame's new features (track_cnt 1): background first, then the objects in ascending object id, each block contiguous and ascending"""
    rows, io, fo, _ = frame
    blocks = [np.sort(rows["id"][rows["track_cnt"] == 1])]
    for o in sorted(io, key=lambda o: int(o["id"])):
        f = fo[o["first_feat"]: o["first_feat"] + o["n_feats"]]
        blocks.append(f["id"][f["track_cnt"] == 1])
    blocks = [b for b in blocks if len(b)]
    flat = np.concatenate(blocks) if blocks else np.zeros(0, np.uint32)
    return len(blocks), bool((np.diff(flat.astype(np.int64)) == 1).all())


# ---------------------------------------------------------------- group A: ROI geometry
A_RECTS = [(1, 1), (4, 4), (5, 5), (6, 6), (21, 21), (22, 22), (41, 41), (42, 42), (43, 43), (17, 33), (16, 16), (32, 48)]


def geometry_cases():
    """name -> (Case, claimed level count).  Masks of ones (value 1: any non-zero byte is the object); `rim_*`: the object is a pixel smaller than its box"""
    out = {}
    W, H = SMALL
    for i, (w, h) in enumerate(A_RECTS):
        fr = stereo_frames(W, H, 2, seed=200 if (w, h) == (6, 6) else 11 + i)      # (6 x 6: the first seed on which the oracle finds a corner and keeps it)
        x, y = 37 + (i % 3), 9 + (i % 5)
        out[f"ones_{w}x{h}"] = (Case(f"ones_{w}x{h}", SMALL, fr, [[det(5, (x, y, w, h), value=1)]] * 2), roi_levels(w, h))
    for w, h in ((4, 4), (5, 5), (6, 6)):
        fr = stereo_frames(W, H, 2, seed=31 + w)
        out[f"rim_{w}x{h}"] = (Case(f"rim_{w}x{h}", SMALL, fr, [[det(5, (40, 20, w, h), rim_mask(w, h, 1))]] * 2), 1)
    fr = stereo_frames(W, H, 2, seed=41)
    out["whole_frame"] = (Case("whole_frame", SMALL, fr, [[det(5, (0, 0, W, H), value=1)]] * 2), 2)
    for name, rect in (("flush_left", (0, 20, 30, 28)), ("flush_top", (50, 0, 30, 28)), ("flush_right", (W - 30, 20, 30, 28)), ("flush_bottom", (50, H - 28, 30, 28))):
        out[name] = (Case(name, SMALL, stereo_frames(W, H, 2, seed=43), [[det(5, rect, value=1)]] * 2), 1)
    for lv, s in ((1, 40), (2, 60), (3, 100), (4, 172)):
        fr = stereo_frames(MID[0], MID[1], 2, seed=50 + lv)
        out[f"levels{lv}_{s}x{s}"] = (Case(f"levels{lv}_{s}x{s}", MID, fr, [[det(5, (13, 5, s, s), value=1)]] * 2), lv)
    return out


# ---------------------------------------------------------------- group B: size change
def resize_cases():
    """name -> Case of three frames: the rectangle of frame 1 differs from frame 0's (and frame 2 returns to it), the texture drifts 1 px per frame"""
    W, H = SMALL
    pairs = {"grow_41_43": ((40, 10, 41, 41), (40, 10, 43, 43)), "shrink_43_41": ((40, 10, 43, 43), (40, 10, 41, 41)),
             "grow": ((40, 12, 30, 30), (36, 8, 44, 40)), "shrink": ((30, 6, 50, 48), (33, 9, 30, 30)),
             "shift": ((40, 14, 40, 36), (47, 19, 40, 36)), "wide_to_tall": ((30, 16, 48, 26), (32, 13, 30, 46))}
    out = {}
    for i, (name, (r0, r1)) in enumerate(sorted(pairs.items())):
        fr = stereo_frames(W, H, 3, seed=60 + i)
        out[name] = Case(name, SMALL, fr, [[det(9, r0)], [det(9, r1)], [det(9, r0)]])
    return out


def in_border(pts, rows, cols):
    """InBorder (feature_utils.h:68-74): the rounded point at least a pixel inside the image"""
    x, y = np.rint(pts[:, 0]).astype(int), np.rint(pts[:, 1]).astype(int)
    return (1 <= x) & (x < cols - 1) & (1 <= y) & (y < rows - 1)


def resize_loss_causes(oracle, case, f0, track_id=9):
    """Which rule removed the points of frame 0 (f0: the object's rows of frame 0) between frame 0 and frame 1, restated with the oracle's operators on the padded pair
    InstanceImagePadding builds (zeros right of and below each ROI, up to the common size):
      status      FeatureTrackByLK on the padded pair: what InstFeat::TrackLeft keeps (the caller checks it against the oracle's object manager)
      in_border   points that pass the forward pass, the backward pass and the 0.5 px test and are removed by InBorder alone
      padding     points FeatureTrackByLK loses on the zero-padded pair and keeps when the SAME two windows of the frames are cut at the common size with their real pixels:
                  the zero fill is what removed them
    -> dict of boolean arrays over the points of frame 0"""
    (l0, _), (l1, _) = case.frames[0], case.frames[1]
    (x0, y0, w0, h0), (x1, y1, w1, h1) = case.dets[0][0]["rect"], case.dets[1][0]["rect"]
    pw, ph = max(w0, w1), max(h0, h1)
    assert max(x0, x1) + pw <= case.w and max(y0, y1) + ph <= case.h          # the counterfactual windows lie inside the frames
    a, b = np.zeros((ph, pw), np.uint8), np.zeros((ph, pw), np.uint8)
    a[:h0, :w0] = l0[y0:y0 + h0, x0:x0 + w0]
    b[:h1, :w1] = l1[y1:y1 + h1, x1:x1 + w1]
    pts = np.ascontiguousarray(f0["left"][:, 3:5], np.float32)
    _, st = oracle.track_by_lk(a, b, pts, bool(case.flow_back), 0.5)
    pf, sf = oracle.lk(a, b, pts, 3, 30, 0.01)
    rp, rs = oracle.lk(b, a, pf, 1, 30, 0.01, initial=pts)
    d = pts - rp
    pre = (sf > 0) & (rs > 0) & (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= np.float32(0.5))
    assert np.array_equal(st > 0, pre & in_border(pf, ph, pw))               # the restatement IS FeatureTrackByLK
    _, st_real = oracle.track_by_lk(l0[y0:y0 + ph, x0:x0 + pw], l1[y1:y1 + ph, x1:x1 + pw], pts, bool(case.flow_back), 0.5)
    return dict(status=st > 0, in_border=pre & ~(st > 0), padding=(st_real > 0) & ~(st > 0))


# ---------------------------------------------------------------- group C: life cycle
LIFE_RECTS = {3: (6, 8, 34, 30), 7: (48, 30, 36, 32), 11: (92, 6, 32, 40)}


def life_case(miss, order="desc"):
    """three objects new in frame 0; id 7 is missing for `miss` frames from frame 2 on while 3 and 11 stay, then returns.  order: how the list is handed over"""
    n = min(4 + miss, 7)
    fr = stereo_frames(SMALL[0], SMALL[1], n, seed=70 + miss)
    dets = []
    for k in range(n):
        ids = [i for i in (3, 7, 11) if not (i == 7 and 2 <= k < 2 + miss)]
        ids = sorted(ids, reverse=True) if order == "desc" else ids[1 + k % 2:] + ids[:1 + k % 2]          # "shuffled": neither ascending nor descending when all three are there
        dets.append([det(i, LIFE_RECTS[i]) for i in ids])
    return Case(f"miss{miss}_{order}", SMALL, fr, dets), 2 + miss


# ---------------------------------------------------------------- group D: counts
def count_rects():
    out = []
    for k in range(17):
        i, j = k % 6, k // 6
        s = 24 + (i * 5 + j * 3) % 9
        out.append((100 - 5 * k if k else 61, (3 + 33 * i, 5 + 58 * j, s, s + (k % 3))))      # ids in no order; object 0 (id 61) is the one that stays
    return out


def count_case(with_disparity):
    """1 object, then 9, then 17, then 1 again: past 8 output slots, 16 LK jobs, 8 extra-point slots and the first arena"""
    rects = count_rects()
    fr = stereo_frames(MID[0], MID[1], 4, seed=81)
    dets = [[det(i, r) for i, r in rects[:n]] for n in (1, 9, 17, 1)]
    return Case("counts_disp" if with_disparity else "counts", MID, fr, dets, disp=disparity_map(*MID) if with_disparity else None)


# ---------------------------------------------------------------- group E: content and caps
def content_cases():
    """name -> (Case, expected per-object count of frame 0, or None)"""
    W, H = SMALL
    rect = (34, 10, 56, 48)
    x, y, w, h = rect
    out = {}

    def painted(patch, seed):
        fr = stereo_frames(W, H, 2, seed=seed)
        res = []
        for k, (l, r) in enumerate(fr):
            l, r = l.copy(), r.copy()
            l[y:y + h, x:x + w] = patch if patch.ndim == 0 else patch[:, k:k + w]
            r[y:y + h, x - 2:x - 2 + w] = patch if patch.ndim == 0 else patch[:, k:k + w]
            res.append((l, r))
        return res

    out["constant"] = (Case("constant", SMALL, painted(np.uint8(137), 90), [[det(4, rect)]] * 2), 0)
    out["zero_mask"] = (Case("zero_mask", SMALL, stereo_frames(W, H, 2, seed=91), [[det(4, rect, np.zeros((h, w), np.uint8))]] * 2), 0)
    stripe = np.zeros((h, w), np.uint8); stripe[:, 20:24] = 255
    out["stripe_mask"] = (Case("stripe_mask", SMALL, stereo_frames(W, H, 2, seed=92), [[det(4, rect, stripe)]] * 2), 0)
    out["noise2"] = (Case("noise2", SMALL, painted(fh.block_noise(h, w + 4, 3, 2), 93), [[det(4, rect)]] * 2), None)
    out["checker"] = (Case("checker", SMALL, painted(fh.checker(h, w + 4, 8), 94), [[det(4, rect)]] * 2), None)
    out["cap4"] = (Case("cap4", SMALL, stereo_frames(W, H, 3, seed=95), [[det(4, rect)]] * 3, inst_max=4, inst_min=1), 4)
    rect = (10, 4, 110, 62)
    x, y, w, h = rect
    out["cap248"] = (Case("cap248", SMALL, painted(fh.block_noise(h, w + 4, 7, 2), 96), [[det(4, rect)]] * 2, inst_max=248, inst_min=0), 248)
    return out


# ---------------------------------------------------------------- group F: configuration
def config_cases():
    W, H = SMALL
    dets = [[det(3, (8, 6, 40, 36)), det(8, (70, 20, 44, 40))]] * 3
    fr = stereo_frames(W, H, 3, seed=101, step=(3, 2), sigma=0.7)      # (fast and fine-grained: the backward check rejects points that flow_back 0 keeps)
    return {"mono": Case("mono", SMALL, fr, dets, stereo=0), "flow_back0": Case("flow_back0", SMALL, fr, dets, flow_back=0),
            "flow_back1": Case("flow_back1", SMALL, fr, dets, flow_back=1), "equal_times": Case("equal_times", SMALL, fr, dets, times=[0.0, 0.05, 0.05])}


# ---------------------------------------------------------------- group G: association
def assoc_cases():
    """name -> (Case with use_det3d, {track_id: box index} expected on frame 0).  det rectangle 60 x 50 at (5, 5); a box rectangle of the same size shifted by s px in x
    overlaps it by (60 - s) * 50: IoU 550 / 5450 = 0.1009 at s = 49, 500 / 5500 = 0.0909 at s = 50; 30 x 20 against 25 x 20 overlapping by 5 x 20 gives 100 / 1000"""
    W, H = SMALL
    fr = stereo_frames(W, H, 2, seed=111)
    d0 = (5, 5, 60, 50)

    def shifted(s, cls=0, center=(1.0, 0.5, 8.0), y=5.0):
        return box3d(cls, center, (5.0 + s, y), (65.0 + s, y + 50.0))

    def case(name, dets, boxes):
        b = np.concatenate(boxes) if boxes else np.zeros(0, BOX3D_DTYPE)
        return Case(name, SMALL, fr, [dets] * 2, boxes3d=[b] * 2, use_det3d=1)

    out = {
        "iou_above": (case("iou_above", [det(2, d0)], [shifted(49)]), {2: 0}),
        "iou_below": (case("iou_below", [det(2, d0)], [shifted(50)]), {}),
        "iou_exactly_0.1": (case("iou_exactly_0.1", [det(2, (10, 10, 30, 20))], [box3d(0, (1, 1, 9), (35.0, 10.0), (60.0, 30.0))]), {}),
        "half_to_even": (case("half_to_even", [det(2, d0)], [box3d(0, (1, 1, 9), (54.5, 5.0), (114.5, 55.0))]), {2: 0}),      # 54.5 -> 54 (s = 49); half up would give 55 (s = 50)
        "two_objects_one_box": (case("two_objects_one_box", [det(9, d0), det(2, (8, 7, 60, 50))], [shifted(3)]), {2: 0}),
        "equal_distance": (case("equal_distance", [det(2, d0)], [shifted(2, center=(0.0, 5.0, 0.0)), shifted(1, center=(3.0, 4.0, 0.0))]), {2: 0}),
        "class_mismatch": (case("class_mismatch", [det(2, d0, class_id=1)], [shifted(0, cls=2)]), {}),
        "more_boxes": (case("more_boxes", [det(2, d0)], [shifted(4, center=(0, 0, 9.0)), shifted(2, center=(0, 0, 4.0)), shifted(1, center=(0, 0, 6.0))]), {2: 1}),
        "more_objects": (case("more_objects", [det(7, d0), det(2, (9, 8, 60, 50)), det(4, (3, 6, 60, 50))], [shifted(3, center=(0, 0, 7.0)), shifted(2, center=(0, 0, 5.0))]), {2: 1, 4: 0}),
        "nan_centre": (case("nan_centre", [det(2, d0)], [shifted(1, center=(np.nan, 0.0, 3.0)), shifted(2, center=(0, 0, 50.0))]), {2: 1}),
    }
    return out


# ---------------------------------------------------------------- group H: limits
def grid_limit_case(h_roi):
    """min_dynamic_dist 1 on 200 x 180: a 190 x h_roi ROI has 190 * h_roi grid cells (172: 32680, accepted; 173: 32870, refused); four frames, the ROI of frames 1 - 3 is
    the accepted one"""
    fr = stereo_frames(MID[0], MID[1], 4, seed=121)
    dets = [[det(6, (4, 3, 190, h_roi))]] + [[det(6, (4, 3, 190, 172))]] * 3
    return Case(f"grid_190x{h_roi}", MID, fr, dets, inst_max=50, inst_min=1)


def bin_limit_case():
    """front_hostile's flag-4 image (a 4 px checkerboard, 320 x 240) as an object that covers the frame, then a benign pair"""
    chk, benign = fh.checker(LIMIT[1], LIMIT[0], 4), stereo_frames(LIMIT[0], LIMIT[1], 2, seed=5)
    full = (0, 0, LIMIT[0], LIMIT[1])
    return Case("bin_limit", LIMIT, [(chk, chk)] + benign, [[det(6, full)], [det(6, (20, 30, 120, 90))], [det(6, (20, 30, 120, 90))]], inst_max=150, inst_min=3, bg=(150, 15))


def cand_limit_case():
    """flag 1: a 2 px checkerboard over the whole 130 x 70 frame (every pixel off the image border is a non-zero local maximum: twice the candidate buffer), then a
    benign pair"""
    chk, benign = fh.checker(SMALL[1], SMALL[0], 2), stereo_frames(SMALL[0], SMALL[1], 2, seed=6)
    return Case("cand_limit", SMALL, [(chk, chk)] + benign, [[det(6, (0, 0) + SMALL)], [det(6, (20, 10, 60, 50))], [det(6, (20, 10, 60, 50))]])


def flag1_census(oracle):
    """the largest candidate census (non-zero local maxima, what the device emits) of block-noise, binary and checkerboard ROIs that cover their own frame, beside that
    frame's candidate buffer -> [(name, size, census, cap)] sorted by census / cap, largest first"""
    res = []
    for (w, h) in (SMALL, MID, LIMIT):
        imgs = {}
        for b in (1, 2, 3, 4):
            imgs[f"noise{b}"] = fh.block_noise(h, w, 3 + b, b)
            imgs[f"binary{b}"] = fh.binary(h, w, 5, plateau=b)
        for b in (1, 2, 3, 4, 8):
            imgs[f"checker{b}"] = fh.checker(h, w, b)
        for name, img in imgs.items():
            c = fh.census(oracle, img, "cpu")
            res.append((name, (w, h), c["without_zeros"], fh.cand_cap(w, h)))
    return sorted(res, key=lambda r: -r[2] / r[3])
