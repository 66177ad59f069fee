"""Hostile cases for the multi-object tracker (no GPU in here): sequences whose quantities sit exactly ON the decisions of mot_assoc_kernel / mot_feat_kernel — the
gates, the ties, the column-index quirk, the life-cycle and gallery edges, the table shapes, non-finite input — and the premise functions (exact_tracks, dots_exact,
quantity, optimal_count, order_matters) which show on tests/mot_ref.py alone that each case reaches what it is named for.  tests/test_mot_hostile.py asserts the premises (CPU) and compares the device with the float32 reference (GPU).

The yardstick at a gate is MotRef(dtype=float32): the reference computes in float and the float64 run disagrees there by construction.  So every case is exact by
construction.  Boxes are 4h x h with integer h: w h = 4 h^2, w / h = 4, sqrt(s r) = 4h and s / w = h are exact, a birth stores z exactly, a prediction with zero
velocity and an update with zero innovation keep x exact.  Embeddings hold a few dyadic components, so a dot product is exact in any summation order."""
import itertools
from collections import namedtuple

import numpy as np

from tests import mot_cases as mc
from tests import mot_ref

f32 = np.float32
Case = namedtuple("Case", "name group par frames flips mem at want")      # flips: MotRef flips that must change the outcome; at: (frame, quantity name, bit pattern)
GROUPS = ("gates", "ties", "quirk", "life", "gallery", "table", "nonfinite")


def bits(v):
    return int(np.asarray(v, f32).view(np.uint32))


def frame(rects, feats, F):
    r = np.array(rects, f32).reshape(-1, 4)
    f = np.array(feats, f32).reshape(len(r), F)
    return (r, f, np.arange(len(r)))


def empty(F):
    return frame([], [], F)


def hot(F, *pairs):
    v = np.zeros(F, f32)
    for i, a in pairs:
        v[i] = a
    return v


def box(x, y, h=10):
    return [x, y, 4 * h, h]


def iou_dist32(a, b):
    return mot_ref.MotRef(dtype=f32, feat_dim=1).iou_dist(np.array(a, f32), np.array(b, f32))


def find_boxes(target):
    """(track box 4h x h at the origin, detection box inside it) whose float32 1 - inter / union has exactly the bit pattern of `target`: integers below 2^24, so
    every product is exact and the only roundings are the division's and the subtraction's"""
    target = f32(target)
    for h in range(1, 2047):
        u = 4 * h * h
        base = int(round((1.0 - float(target)) * u))
        for i in range(max(base - 3, 1), base + 4):
            if bits(f32(1) - f32(i) / f32(u)) != bits(target):
                continue
            for hd in range(h, 0, -1):
                if i % hd == 0 and i // hd <= 4 * h:
                    t, d = [0, 0, 4 * h, h], [0, 0, i // hd, hd]
                    assert bits(iou_dist32(t, d)) == bits(target)
                    return t, d
    raise AssertionError(f"no integer boxes reach {float(target)!r}")


_BOXES = {}


def boxes_at(target):
    k = bits(target)
    if k not in _BOXES:
        _BOXES[k] = find_boxes(target)
    return _BOXES[k]


UP = lambda v: np.nextafter(f32(v), f32(2))
G08, G07, G02 = f32(0.8), f32(0.7), f32(0.2)
# 1 - dot is a multiple of 2^-24 and 0.2f = 13421773 * 2^-26 is none: the nearest reachable values on either side
FEAT_LO, FEAT_HI = f32(3355443 / 2.0 ** 24), f32(3355444 / 2.0 ** 24)
assert FEAT_LO < G02 < FEAT_HI and float(FEAT_HI) - float(FEAT_LO) == 2.0 ** -24
P0 = dict(n_init=0, max_age=3, budget=4, feat_dim=4, max_tracks=16)
FAR = 1000.0


# ---------------------------------------------------------------- group 1: gates
def gate_cases():
    out = []
    F = 4
    e0 = hot(F, (0, 1.0))
    for name, tgt, flips in (("iou1_at", G08, ("iou1",)), ("iou1_beyond", UP(G08), ())):
        T, D = boxes_at(tgt)
        out.append(Case(name, "gates", P0, [frame([T], [e0], F), frame([T], [e0], F), frame([D], [e0], F)], flips, "device", (2, "iou1", bits(tgt)), None))
    T, D = boxes_at(G08)      # passes the stage-1 IoU gate, fails stage 2's: only the appearance gate decides
    for name, v, dot in (("feat_below", FEAT_LO, 13421773), ("feat_above", FEAT_HI, 13421772)):
        f = hot(F, (0, dot / 2.0 ** 24), (1, 0.5))
        out.append(Case(name, "gates", P0, [frame([T], [e0], F), frame([T], [e0], F), frame([D], [f], F)], (), "host", (2, "feat", bits(v)), None))
    for name, tgt, flips in (("iou2_at", G07, ("iou2",)), ("iou2_beyond", UP(G07), ())):
        T, D = boxes_at(tgt)
        out.append(Case(name, "gates", P0, [frame([T], [e0], F), frame([D], [e0], F)], flips, "pinned", (1, "iou2", bits(tgt)), None))
    # a stage-1 row whose every cost is 1000: Munkres assigns it (rows <= cols: the first column), the > 100 test drops it
    T = box(0, 0)
    e1 = hot(F, (1, 1.0))
    out.append(Case("all_1000_row", "gates", P0, [frame([T], [e0], F), frame([T], [e0], F), frame([box(FAR, 0), box(2 * FAR, 0)], [e1, e1], F), frame([T], [e0], F)],
                    (), "host", None, None))
    # the union against DBL_EPSILON = 2^-52, a float32 normal: equal (kept: IoU 1), half of it (distance 1), and a denormal area
    for name, w, h, flips in (("union_at", 2.0 ** -26, 2.0 ** -26, ("union",)), ("union_beyond", 2.0 ** -27, 2.0 ** -26, ()), ("union_denormal", 2.0 ** -70, 2.0 ** -70, ())):
        t = [0, 0, w, h]
        out.append(Case(name, "gates", P0, [frame([t], [e0], F), frame([t], [e0], F), frame([t], [e0], F)], flips, "host", (1, "union", bits(f32(w) * f32(h))), None))
    # an overlap of width / height exactly 0
    out.append(Case("touch_w", "gates", P0, [frame([T], [e0], F), frame([box(40, 0)], [e0], F), frame([box(40, 0)], [e0], F)], (), "host", None, None))
    out.append(Case("touch_h", "gates", P0, [frame([T], [e0], F), frame([box(0, 10)], [e0], F), frame([box(0, 10)], [e0], F)], (), "device", None, None))
    return out


# ---------------------------------------------------------------- group 2: ties
def tie_cases():
    F = 4
    e = [hot(F, (i, 1.0)) for i in range(F)]
    T = box(0, 0)
    out = []
    # two Tentative tracks and two detections on one box: the 2 x 2 all-zero problem; frame 2's appearance match tells which gallery took which embedding
    out.append(Case("tie_tentative", "ties", P0, [frame([T, T], [e[0], e[1]], F), frame([T, T], [e[2], e[3]], F), frame([T, T], [e[3], e[2]], F)],
                    (), "device", (1, 1), [2, 1]))
    # a Confirmed row left by stage 1 and a Tentative row on one box, one detection: the Confirmed row is first
    out.append(Case("tie_confirmed_tentative", "ties", P0,
                    [frame([T], [e[0]], F), frame([T], [e[0]], F), frame([T, T], [e[1], e[2]], F), frame([T], [e[3]], F), frame([T], [e[3]], F)], (), "pinned", (3, 1), None))
    # equal appearance costs 0.125 on two Confirmed tracks
    a, b = hot(F, (0, 0.875), (1, 0.875), (2, 0.5)), hot(F, (0, 0.875), (1, 0.875), (3, 0.5))
    out.append(Case("tie_appearance", "ties", P0, [frame([T, T], [e[0], e[1]], F), frame([T, T], [e[0], e[1]], F), frame([T, T], [a, b], F),
                                                   frame([T, T], [2 * e[3], 2 * e[2]], F)], (), "host", (2, 0), [2, 1]))
    return out


# ---------------------------------------------------------------- group 3: the column-index quirk
def quirk_cases():
    F = 4
    e = [hot(F, (i, 1.0)) for i in range(F)]
    T, U, V, W = box(0, 0), box(FAR, 0), box(2 * FAR, 0), box(3 * FAR, 0)
    fr = [frame([T], [e[0]], F), frame([T, U], [e[0], e[1]], F),
          frame([T, W, U, V], [e[0], e[3], e[1], e[2]], F)]      # stage 1 takes detection 0; stage 2's columns are detections 1, 2, 3 and the Tentative track takes column 1
    fr += [frame([T, W, U, V], [e[0], e[3], e[1], e[2]], F)] * 2
    return [Case("quirk", "quirk", dict(P0, max_tracks=32), fr, (), "device", None, None),
            Case("quirk_pinned", "quirk", dict(P0, max_tracks=32, max_age=1), fr, (), "pinned", None, None)]


# ---------------------------------------------------------------- group 4: life-cycle edges
def life_cases():
    F = 4
    e = [hot(F, (i, 1.0)) for i in range(F)]
    A, B, Cx = box(0, 0), box(FAR, 0), box(2 * FAR, 0)
    out = []
    # n_init = 0: three confirm at once, detections in another order than the table: ids by stage-2 row
    out.append(Case("n_init_0_order", "life", P0, [frame([A, B, Cx], e[:3], F), frame([Cx, A, B], [e[2], e[0], e[1]], F), frame([B, Cx, A], [e[1], e[2], e[0]], F)],
                    (), "device", None, [2, 3, 1]))
    out.append(Case("max_age_0", "life", dict(P0, max_age=0), [frame([A], [e[0]], F), frame([A], [e[0]], F), frame([B], [e[1]], F), empty(F), frame([A, B], [e[0], e[1]], F)],
                    (), "host", None, None))
    # n_init 2, max_age 2: X confirms in frame 3 and misses 4, 5 (tsu == max_age in 5), Y is born in 3 and has hits + 1 == n_init in 5; empty frames age nothing
    X, Y = ([A], [e[0]]), ([B], [e[1]])
    both = ([A, B], [e[0], e[1]])
    fr = [frame(*X, F), frame(*X, F), empty(F), frame(*X, F), frame(*both, F), frame(*Y, F), empty(F), frame(*Y, F), empty(F), frame(*both, F), frame(*both, F)]
    out.append(Case("both_edges", "life", dict(P0, n_init=2, max_age=2), fr, ("n_init", "max_age"), "pinned", None, None))
    return out


# ---------------------------------------------------------------- group 5: gallery shapes
def ring_case(name, budget, rows, deciding, mem="host", stale=False):
    """two Confirmed tracks on one box: stage 1 tells them apart by appearance, stage 2 (all zero) by order.  Their galleries grow by a row per frame up to `rows`;
    row `deciding` alone carries the probe's component.  The last frame asks with the probes in the other order: ids [2, 1] only if that row is read.  stale: no row
    carries it, so the ids are [1, 2] — unless rows past the count (left by an earlier run) are read"""
    F = 8
    T = box(0, 0)
    fr = []
    for k in range(rows):
        a, b = hot(F, (0, 1.0)), hot(F, (1, 1.0))
        if stale == "fill" or (k == deciding and not stale):
            a[2], b[3] = 1.0, 1.0
        fr.append(frame([T, T], [a, b], F))
    fr.append(frame([T, T], [hot(F, (3, 1.0)), hot(F, (2, 1.0))], F))
    want = [1, 2] if stale is True else [2, 1]
    return Case(name, "gallery", dict(n_init=0, max_age=3, budget=budget, feat_dim=F, max_tracks=8), fr, (), mem, None, want)


def dim_case(F, n, mem="host"):
    """one Confirmed track whose gallery row is 0.5 e_0 + e_{F-1}; the asking box passes stage 1's IoU gate and fails stage 2's.  n - 1 detections far away with zero
    embeddings, one on the box without the last component (cost 0.75 or 1: gated), and LAST the one whose component F - 1 decides"""
    T, D = boxes_at(G08)
    g = hot(F, (0, 0.5), (F - 1, 1.0)) if F > 1 else hot(F, (0, 1.0))
    miss = hot(F, (0, 1.0)) if F > 1 else hot(F, (0, 0.5))
    rects = [[FAR * (1 + j % 8), FAR * (1 + j // 8), 40, 10] for j in range(n - 2)] + [D, D]
    feats = [np.zeros(F, f32)] * (n - 2) + [miss, g]
    want = [-1] * (n - 1) + [1]
    return Case(f"dim_F{F}_n{n}", "gallery", dict(n_init=0, max_age=3, budget=2, feat_dim=F, max_tracks=128), [frame([T], [g], F), frame([T], [g], F), frame(rects, feats, F)],
                (), mem, None, want)


def budget1_case():
    F = 4
    e = [hot(F, (i, 1.0)) for i in range(F)]
    T = box(0, 0)
    fr = [frame([T, T], [e[0], e[1]], F), frame([T, T], [e[0], e[1]], F), frame([T, T], [e[1], e[0]], F), frame([T, T], [e[2], e[3]], F), frame([T, T], [e[3], e[2]], F),
          frame([T, T], [e[1], e[0]], F)]
    return Case("budget_1", "gallery", dict(P0, budget=1), fr, (), "device", None, [1, 2])


def gallery_cases():
    out = [budget1_case()]
    out += [ring_case("ring_33_rows32_first", 33, 32, 0), ring_case("ring_33_rows32_last", 33, 32, 31, "device"), ring_case("ring_33_rows33_last", 33, 33, 32, "pinned"),
            ring_case("ring_100_rows96_last", 100, 96, 95), ring_case("ring_100_rows97_last", 100, 97, 96), ring_case("ring_100_rows100_last", 100, 100, 99),
            ring_case("ring_100_rows100_wave1_last", 100, 100, 63), ring_case("ring_100_rows97_wave2_last", 100, 97, 95)]
    out += [dim_case(F, 2) for F in (1, 7, 9, 511, 512)]
    out += [dim_case(8, 32, "device"), dim_case(8, 33, "pinned"), dim_case(9, 64)]
    return out


def stale_cases():
    """(the run that leaves 36 finite rows behind, the run behind mot_reset that asks with 33 stored: row 33, in the second wave's tile, is the stale one just past the count)"""
    return ring_case("stale_fill", 36, 36, 0, stale="fill"), ring_case("stale_row_past_count", 36, 33, 0, stale=True)


# ---------------------------------------------------------------- group 6: table shapes
def grid_box(o):
    return [FAR * (o % 10), FAR * (o // 10), 40, 10]


def wide_stage2_case():
    """100 Confirmed tracks built in turns (64 detections a frame), then 64 detections whose embeddings fail every appearance gate: stage 2 is 100 rows x 64 columns,
    and the rows with a zero are 36 .. 99"""
    F = 8
    e0 = hot(F, (0, 1.0))
    show = lambda objs, f: frame([grid_box(o) for o in objs], [f] * len(objs), F)
    turn = list(range(64, 100)) + list(range(36, 64))      # the new ones first: stage 2's column indices are then their detection ids, and the quirk stays out
    fr = [show(range(64), e0), show(range(64), e0), show(turn, e0), show(turn, e0), show(range(99, 35, -1), hot(F, (1, 1.0))), show(range(36, 100), e0)]
    return Case("wide_stage2", "table", dict(n_init=0, max_age=6, budget=4, feat_dim=F, max_tracks=128), fr, (), "device", None, None)


def table_cases():
    F = 8
    e = [hot(F, (i, 1.0)) for i in range(F)]
    T, U = box(0, 0), box(FAR, 0)
    out = [wide_stage2_case()]
    out.append(Case("r1_zero", "table", dict(P0, feat_dim=F, n_init=3), [frame([T, U], e[:2], F)] * 3, (), "host", None, None))
    # every detection taken in stage 1 while a Tentative track waits: stage 2 has a row and no column
    out.append(Case("c2_zero", "table", dict(P0, feat_dim=F), [frame([T], [e[0]], F), frame([T, U], e[:2], F), frame([T], [e[0]], F), frame([T, U], e[:2], F)], (), "pinned", None, None))
    # every track leaves through remove_nan: zero-height births have r = inf, and s r = 0 inf is a NaN one frame later
    Z = [[0, 0, 40, 0], [FAR, 0, 8, 0], [2 * FAR, 5, 1, 0]]
    out.append(Case("all_leave_by_nan", "table", dict(P0, feat_dim=F), [frame(Z, e[:3], F), frame([T, U], e[:2], F), frame([T, U], e[:2], F)], (), "host", None, None))
    for mt in (5, 65):
        out.append(slot_case(mt))
    return out


def slot_case(mt):
    """max_tracks tracks; then in ONE frame two Confirmed tracks leave (max_age 0) and two are born on one box with different embeddings; the next frames confirm the
    two and ask them apart by appearance.  A birth that took a slot still in use, or one past max_tracks, shows in frame 4's ids"""
    F = 8
    n = min(mt, 64)
    feat = lambda o: hot(F, (o % 8, 1.0))
    show = lambda objs: ([grid_box(o) for o in objs], [feat(o) for o in objs])
    N = [FAR * 5, FAR * 20, 40, 10]
    p, q = hot(F, (0, 1.0)), hot(F, (1, 1.0))
    fr = [frame(*show(range(n)), F), frame(*show(range(n)), F)]
    stay = [o for o in range(n) if o not in (1, 3)]
    r, f = show(stay)
    fr.append(frame([N, N] + r, [p, q] + f, F))      # (the two first: stage 2's column indices are then their detection ids, and the quirk stays out of this case)
    fr.append(frame([N, N] + r, [p, q] + f, F))
    fr.append(frame([N, N] + r, [q, p] + f, F))
    return Case(f"slots_max_tracks_{mt}", "table", dict(n_init=0, max_age=0, budget=2, feat_dim=F, max_tracks=mt), fr, (), "device" if mt == 5 else "host", None, None)


def capacity_frames():
    F = 8
    e = [hot(F, (i, 1.0)) for i in range(F)]
    b = [grid_box(o) for o in range(6)]
    return dict(n_init=0, max_age=3, budget=2, feat_dim=F, max_tracks=5), [frame(b[:5], e[:5], F), frame(b[:6], e[:6], F), frame(b[:5], e[:5], F)]


# ---------------------------------------------------------------- group 7: non-finite input
def nonfinite_cases():
    F = 4
    e = [hot(F, (i, 1.0)) for i in range(F)]
    T, D = boxes_at(G08)
    U, Ud = [FAR, 0] + T[2:], [FAR, 0] + D[2:]
    V = [2 * FAR, 0] + T[2:]
    nan = hot(F, (1, 1.0), (2, np.nan))
    # frame 0: U is born with a NaN in its embedding; frame 1: matched by IoU and Confirmed, gallery [NaN row, e1]; frame 2: asked with e1 on a box that only stage 1
    # would let through, beside a detection whose own embedding is a NaN: torch::min carries the NaN, so both distances are NaN and count as gated
    a = Case("nan_embedding", "nonfinite", P0, [frame([T, U], [e[0], nan], F), frame([T, U], [e[0], e[1]], F), frame([T, Ud, V], [e[0], e[1], nan], F),
                                                 frame([T, Ud, V], [e[0], e[1], e[2]], F)], (), "device", None, None)
    Z, I = [FAR, 0, 40, 0], [2 * FAR, 0, np.inf, 10]
    b = Case("zero_height_inf_width", "nonfinite", P0, [frame([T, Z, I], e[:3], F), frame([T, Z, I], e[:3], F), frame([T, Z, I], e[:3], F)], (), "pinned", None, None)
    return [a, b]


def all_cases():
    return gate_cases() + tie_cases() + quirk_cases() + life_cases() + gallery_cases() + table_cases() + nonfinite_cases()


# ---------------------------------------------------------------- running and premises
_RUNS = {}


def run(case, dtype=f32, flip=()):
    """the reference's frames of a case: computed once per (case, dtype, flip), shared, never changed"""
    key = (case.name, np.dtype(dtype).name, tuple(flip))
    if key not in _RUNS:
        with np.errstate(all="ignore"):
            _RUNS[key] = mc.run_ref(case.frames, dict(case.par, flip=tuple(flip)), dtype)
    return _RUNS[key]


def outcome(r):
    return [(list(map(int, f["ids"])), mc.discrete(f["table"])) for f in r]


def exact_tracks(case, r32):
    """per frame the table positions whose state is exact by construction: zero velocity, x[:4] the measurement of a box the case has shown, and rect() that box bit for bit"""
    m = mot_ref.MotRef(dtype=f32, feat_dim=1)
    seen, out = {}, []
    for (rects, _, _), fr in zip(case.frames, r32):
        for rc in rects:
            seen[rc.tobytes()] = rc
        ok = []
        for i, t in enumerate(fr["table"]):
            rc = seen.get(np.asarray(t["rect"], f32).tobytes())
            if rc is not None and not t["x"][4:].any() and np.asarray(t["x"][:4], f32).tobytes() == m.measure(rc).tobytes():
                ok.append(i)
        out.append(ok)
    return out


def dot_orders(g, f):
    """a dot product in float32, summed forward, reversed and pairwise"""
    p = (np.asarray(g, f32) * np.asarray(f, f32)).astype(f32)
    fwd = f32(0)
    for v in p:
        fwd = f32(fwd + v)
    rev = f32(0)
    for v in p[::-1]:
        rev = f32(rev + v)
    q = list(p)
    while len(q) > 1:
        q = [f32(q[i] + q[i + 1]) if i + 1 < len(q) else q[i] for i in range(0, len(q), 2)]
    return fwd, rev, q[0]


def dots_exact(case):
    """every finite (embedding of an earlier frame, detection) product of the case sums to the same float32 in three orders, and to the float64 sum; -> the number checked"""
    n = 0
    stored, done = {}, set()
    for _, feats, _ in case.frames:
        for g, f in itertools.product(list(stored.values()), [f for f in feats if np.isfinite(f).all()]):
            if (g.tobytes(), f.tobytes()) in done:
                continue
            done.add((g.tobytes(), f.tobytes()))
            a, b, c = dot_orders(g, f)
            assert bits(a) == bits(b) == bits(c) and float(a) == float(np.dot(g.astype(np.float64), f.astype(np.float64))), (case.name, g, f)
            n += 1
        for f in feats:
            if np.isfinite(f).all():
                stored[f.tobytes()] = f
    return n


def kept_pairs(prob, asg):
    return sorted((i, int(c)) for i, c in enumerate(asg) if c >= 0 and prob[i, c] <= mot_ref.INVALID_DIST / 10)


def optimal_count(prob):
    """the number of assignments of min(R, C) pairs with the smallest total (brute force: small problems only)"""
    R, C = prob.shape
    if R <= C:
        tot = [sum(prob[i, p[i]] for i in range(R)) for p in itertools.permutations(range(C), R)]
    else:
        tot = [sum(prob[p[j], j] for j in range(C)) for p in itertools.permutations(range(R), C)]
    return sum(t == min(tot) for t in tot)


def order_matters(prob):
    """-> (rows matter, columns matter): reversing the rows / the columns of the reference's matrix changes the pairs it keeps (mapped back)"""
    R, C = prob.shape
    base = kept_pairs(prob, mot_ref.munkres(prob))
    pr = prob[::-1]
    rows = sorted((R - 1 - i, c) for i, c in kept_pairs(pr, mot_ref.munkres(pr)))
    pc = prob[:, ::-1]
    cols = sorted((i, C - 1 - c) for i, c in kept_pairs(pc, mot_ref.munkres(pc)))
    return rows != base, cols != base


def quantity(case, r32):
    """the bit pattern of the quantity named by case.at in the float32 reference's frame"""
    k, what, _ = case.at
    info = r32[k]["info"]
    if what in ("iou1", "iou2"):
        return bits(info["iou"][0, 0])
    if what == "feat":
        return bits(info["feat"][0][0])
    if what == "union":
        a, b = info["trects"][0], case.frames[k][0][0]
        return bits(a[2] * a[3] + b[2] * b[3] - a[2] * a[3])
    raise KeyError(what)
