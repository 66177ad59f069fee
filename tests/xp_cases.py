"""Hostile clouds for the extra-point pipeline's parity tests (tests/test_extra_points_hostile.py): builders and their CPU self-checks.

Every cloud is a LATTICE with exact arithmetic: fx = fy = 512, integer cx, cy, fx * baseline = 64, and a constant disparity that makes the depth a power of two — 1.0
(depth 64) where the sampling step is 2 px, 2.0 (depth 32) where it is 4 px.  Either way two neighbouring grid nodes are exactly 0.25 m apart, every coordinate is a
multiple of 1/16 m below 2^8 and every squared distance is exact in float32: the thresholds of the radius filter (d^2 <= 0.25: two spacings, inclusive) and of the
clustering (d^2 < 1: four spacings, strict) can be hit on the nose.  The ROI sizes go through the reference's step rule, int(max(sqrt(0.8 rows cols / 1000), 2)), and the
builder asserts the step the case was designed for.  The context is the smallest that holds the ROI (the library accepts any positive size).

A builder returns a Scene (mask, (x, y), disparity, cam, baseline, image size).  check(name) runs the case's own assertions on the numpy restatement of
tests/test_extra_points.py (np_detect / np_process): the counts the case is named for, and — for the threshold cases — that the restatement with ONE comparison flipped
gives another answer, which proves that the case discriminates.  Expected outputs of the device tests never come from this module: they are the oracle's.

emulate_sweeps restates the device's label scheme (Jacobi min-label over d^2 < 1 with l = in[in[in[q]]] on the way in, csrc/extra_points.hip) for ONE purpose: to label
each convergence case with the number of sweeps that still change a label, and to assert that the set straddles the 16 sweeps the host launches.

Flag 8 (more than DV_XP_CAP = 3200 sampled points): with images up to 1280 wide the step rule bounds the grid at about 3130 nodes and the flag is unreachable; the
library accepts an 8000 x 1 context, where a 1 x 8000 ROI has step 2 and 4000 nodes: `overflow_1x8000` is that case (refused by name, context usable afterwards)."""
from collections import namedtuple

import numpy as np

from tests.test_extra_points import np_detect, np_process

F32 = np.float32
FX, CX, CY = 512.0, 16.0, 8.0
CAM = (FX, FX, CX, CY)
BASELINE = 0.125                       # fx * baseline = 64
XP_CAP, XP_SWEEPS = 3200, 16           # DV_XP_CAP (csrc/dv_internal.h), XP_SWEEPS (csrc/extra_points.hip)
Scene = namedtuple("Scene", "mask xy disp cam baseline size")


def step_rule(rows, cols):
    """InstFeat::DetectExtraPoints' sampling step (instance_feature.cpp:421-422)"""
    return int(max(np.sqrt(0.8 * rows * cols / 1000.0), 2.0))


def lattice_scene(nodes, step=2, roi=None, xy=(0, 0), size=None, values=(255,), full_mask=False):
    """nodes: bool [R, C], the grid nodes that carry a point.  roi = (rows, cols) when the ROI is larger than (R - 1) step + 1 by less than a step"""
    nodes = np.asarray(nodes, bool)
    R, C = nodes.shape
    rows, cols = roi if roi is not None else ((R - 1) * step + 1, (C - 1) * step + 1)
    assert step_rule(rows, cols) == step and (rows + step - 1) // step == R and (cols + step - 1) // step == C, (rows, cols, step_rule(rows, cols))
    val = np.asarray(values, np.uint8)[(np.arange(R)[:, None] * 5 + np.arange(C)[None, :]) % len(values)]
    mask = np.zeros((rows, cols), np.uint8)
    mask[::step, ::step] = np.where(nodes, val, 0)
    if full_mask:
        assert nodes.all()
        mask[:] = values[0]
    W, H = size if size is not None else (xy[0] + cols, xy[1] + rows)
    assert xy[0] + cols <= W and xy[1] + rows <= H
    disp = np.full((H, W), {2: 1.0, 4: 2.0}[step], F32)
    return Scene(mask, xy, disp, CAM, BASELINE, (W, H))


def block(R, C, *rects):
    """bool [R, C] with the rectangles (r0, r1, c0, c1), ends excluded, set"""
    n = np.zeros((R, C), bool)
    for r0, r1, c0, c1 in rects:
        n[r0:r1, c0:c1] = True
    return n


# ---------------------------------------------------------------- the restated pieces the self-checks need
def d2_f32(a, b):
    """flann::L2_Simple<float>: ((dx dx) + dy dy) + dz dz in float32"""
    dx = a[:, None, 0] - b[None, :, 0]; dy = a[:, None, 1] - b[None, :, 1]; dz = a[:, None, 2] - b[None, :, 2]
    return ((dx * dx + dy * dy).astype(F32) + dz * dz).astype(F32)


def survivors(p, inclusive=True):
    """the radius filter alone -> the kept points, in order"""
    if len(p) == 0:
        return p
    D = d2_f32(p, p)
    return p[((D <= F32(0.25)) if inclusive else (D < F32(0.25))).sum(1) >= 11]


def emulate_sweeps(f):
    """number of device sweeps that change a label on the filtered cloud f: Jacobi min-label over d^2 < 1, every label first replaced by its label's label, twice"""
    m = len(f)
    if m == 0:
        return 0
    A = d2_f32(f, f) < F32(1.0)
    lab, n = np.arange(m), 0
    while True:
        l = lab[lab[lab]]
        out = np.minimum(l, np.where(A, l[None, :], m).min(1))
        if np.array_equal(out, lab):
            return n
        lab, n = out, n + 1


_POINTS, _RESULT = {}, {}


def points(name):
    """the restated sampling of a case (computed once)"""
    if name not in _POINTS:
        s = CASES_ALL[name][0]()
        with np.errstate(all="ignore"):
            _POINTS[name] = np_detect(s.mask, s.xy, s.disp, s.cam, s.baseline)
    return _POINTS[name]


def result(name):
    """the restated pipeline's answer of a case (computed once)"""
    if name not in _RESULT:
        _RESULT[name] = np_process(points(name))
    return _RESULT[name]


def in_scan_order(p):
    """rows of p ascend in (y, x): the reference's row-major scan"""
    key = p[:, 1].astype(np.float64) * 4096 + p[:, 0]
    return bool((np.diff(key) > 0).all())


def counts(name):
    p = points(name)
    return len(p), len(survivors(p)), len(result(name))


# ---------------------------------------------------------------- thresholds
def radius_band_5x30():
    """inclusive radius: a band 5 node rows thick keeps its 3 inner rows (less the end columns) because the nodes two spacings away count (d^2 == 0.25)"""
    return lattice_scene(block(5, 30, (0, 5, 0, 30)))


def _check_radius_band(name):
    p = points(name)
    assert counts(name) == (150, 84, 84)
    assert len(survivors(p, inclusive=False)) == 0 and len(np_process(p, radius_inclusive=False)) == 0          # with `<` nothing has 11 neighbours


def adjacency_100():
    """strict adjacency: a 6 x 8 and a 6 x 10 block one empty node column apart; the filter takes the facing columns, the nearest SURVIVING points are four spacings
    = exactly 1.0 m apart: two clusters, the larger (32) is returned; with `<=` they would be one of 56"""
    return lattice_scene(block(6, 19, (0, 6, 0, 8), (0, 6, 9, 19)))


def adjacency_075():
    """two blocks of 8 rows whose facing columns are three spacings apart: columns 8 and 9 between them carry nodes in two rows of three, which lift the facing columns 7 and 10 to 11 neighbours and
    have only 10 themselves; the nearest survivors are 0.75 m apart: one cluster"""
    n = block(8, 20, (0, 8, 0, 8), (0, 8, 10, 20))
    n[[r for r in range(8) if r % 3 != 2], 8:10] = True
    return lattice_scene(n)


def _nearest_across(f, x_split):
    a, b = f[f[:, 0] < x_split], f[f[:, 0] > x_split]
    return float(d2_f32(a, b).min()), len(a), len(b)


def _check_adjacency(name):
    p = points(name)
    f = survivors(p)
    x0 = (0 - CX) * 64.0 / FX                                      # x of node column 0
    if name == "adjacency_100":
        gap, na, nb = _nearest_across(f, x0 + 8 * 0.25)
        assert (gap, na, nb) == (1.0, 24, 32) and counts(name) == (108, 56, 32)
        assert len(np_process(p, adjacency_strict=False)) == 56      # the flipped comparison joins them
        assert np.array_equal(result(name), f[f[:, 0] > x0 + 8 * 0.25])
    else:
        cols = np.rint((f[:, 0] - x0) / 0.25).astype(int)
        assert not np.isin(cols, (8, 9)).any() and (cols == 7).any() and (cols == 10).any()          # the filler nodes are gone, the facing columns stay
        gap, na, nb = _nearest_across(f, x0 + 8.5 * 0.25)
        assert gap == 0.5625 and len(result(name)) == na + nb == len(f)


# ---------------------------------------------------------------- count edges
def count_4x7():
    """10 survivors, the four corner ones with exactly 11 neighbours: one cluster of exactly 10, returned"""
    return lattice_scene(block(4, 7, (0, 4, 0, 7)))


def count_4x6():
    """8 survivors (>= 5, so the clustering runs) in one cluster below 10: nothing"""
    return lattice_scene(block(4, 6, (0, 4, 0, 6)))


def count_4x4():
    """4 survivors: fewer than 5, nothing"""
    return lattice_scene(block(4, 4, (0, 4, 0, 4)))


def _check_counts(name):
    p = points(name)
    want = {"count_4x7": (28, 10, 10), "count_4x6": (24, 8, 0), "count_4x4": (16, 4, 0)}[name]
    assert counts(name) == want
    if name == "count_4x7":
        nb = (d2_f32(p, p) <= F32(0.25)).sum(1)
        assert sorted(nb[nb >= 11]) == [11] * 4 + [12] * 6


# ---------------------------------------------------------------- winner rules
def tie_right_first():
    """two clusters of 24; the right one starts a grid row higher, so its first member has the lower index: it wins"""
    return lattice_scene(block(7, 20, (1, 7, 0, 8), (0, 6, 12, 20)))


def larger_later():
    """a cluster of 12 found first, one of 24 found later: the larger wins"""
    return lattice_scene(block(8, 18, (0, 5, 0, 6), (2, 8, 10, 18)))


def nine_beside_ten():
    """a cluster of 9 (found first, too small) beside one of 10"""
    return lattice_scene(block(6, 16, (0, 5, 0, 5), (2, 6, 9, 16)))


def _check_winner(name):
    p, f, res = points(name), survivors(points(name)), result(name)
    split = {"tie_right_first": 10, "larger_later": 8, "nine_beside_ten": 7}[name]
    xs = (0 - CX) * 64.0 / FX + split * 0.25
    left, right = f[f[:, 0] < xs], f[f[:, 0] > xs]
    sizes = {"tie_right_first": (24, 24), "larger_later": (12, 24), "nine_beside_ten": (9, 10)}[name]
    assert (len(left), len(right)) == sizes and _nearest_across(f, xs)[0] >= 1.0
    assert np.array_equal(res, right) and in_scan_order(res)
    first_left, first_right = np.nonzero(f[:, 0] < xs)[0][0], np.nonzero(f[:, 0] > xs)[0][0]
    assert (first_right < first_left) == (name == "tie_right_first")
    assert len(p) == {"tie_right_first": 96, "larger_later": 78, "nine_beside_ten": 53}[name]


# ---------------------------------------------------------------- block and pass edges
def sampled_1024():
    """exactly one full pass of xp_detect"""
    return lattice_scene(block(32, 32, (0, 32, 0, 32)), roi=(64, 64), full_mask=True)


def sampled_1025():
    """one point into the second pass: 32 x 33 nodes less 31 holes in the last column"""
    n = block(32, 33, (0, 32, 0, 33))
    n[1:, 32] = False
    return lattice_scene(n, roi=(64, 66))


def survivors_256():
    """the sweeps' first workgroup exactly full"""
    return lattice_scene(block(18, 18, (0, 18, 0, 18)))


def survivors_257():
    """one survivor into the second workgroup: two nodes beside the block lift one node of its edge column to 11 neighbours"""
    n = block(18, 20, (0, 18, 0, 18))
    n[8, 18:20] = True
    return lattice_scene(n)


def capacity_band():
    """the largest cloud images up to 1280 wide allow: 9 x 1249 px, full mask, 5 x 625 = 3125 points: xp_detect's fourth pass, 13 filter and sweep workgroups"""
    return lattice_scene(block(5, 625, (0, 5, 0, 625)), roi=(9, 1249), full_mask=True)


def flush_right_bottom():
    """the ROI ends on the image's last column and row"""
    return lattice_scene(block(6, 8, (0, 6, 0, 8)), xy=(25, 19), size=(40, 30))


def _check_edges(name):
    want = {"sampled_1024": (1024, 900, 900), "sampled_1025": (1025, 900, 900), "survivors_256": (324, 256, 256), "survivors_257": (326, 257, 257),
            "capacity_band": (3125, 1869, 1869), "flush_right_bottom": (48, 24, 24)}[name]
    assert counts(name) == want and in_scan_order(result(name))
    s = CASES[name][0]()
    if name == "flush_right_bottom":
        assert s.xy[0] + s.mask.shape[1] == s.size[0] and s.xy[1] + s.mask.shape[0] == s.size[1] and s.xy[0] > 0 and s.xy[1] > 0
    if name == "capacity_band":
        assert s.mask.shape == (9, 1249) and s.mask.all() and 3 * 1024 < want[0] <= XP_CAP and -(-want[0] // 256) == 13


# ---------------------------------------------------------------- disparity edges
SPECIALS = {(4, 5): np.inf, (2, 3): -0.0, (6, 8): 1e-45, (5, 2): np.nan, (7, 6): -3.0}          # +inf: depth 0; -0.0: disparity <= 0; a denormal: depth inf
MASK_HOLES = [(3, 9), (8, 1)]


def disparity_specials():
    """a 10 x 12 block with +inf, -0.0, a denormal, NaN and a negative disparity on interior nodes, two mask zeros, the other mask bytes 1, 128 and 255 in turn"""
    n = block(10, 12, (0, 10, 0, 12))
    for r, c in MASK_HOLES:
        n[r, c] = False
    s = lattice_scene(n, values=(1, 128, 255))
    for (r, c), v in SPECIALS.items():
        s.disp[2 * r, 2 * c] = v
    return s


def disparity_for_depth(target, numerator):
    """a float32 disparity d with float32(numerator / d) == target, by search around numerator / target; None if no float gives it"""
    d0 = F32(numerator / target)
    for k in range(-64, 65):
        d = np.int32(d0.view(np.int32) + k).view(F32)
        if F32(numerator / d) == target:
            return d
    return None


DEPTH_BASELINE = float(np.int32(F32(0.125).view(np.int32) + 2).view(F32))      # fx * baseline = 64.000015: with 64 no disparity gives the float above 100
DEPTH_TARGETS = [(F32(100.0), True), (np.nextafter(F32(100.0), F32(200.0)), False), (F32(0.1), True), (np.nextafter(F32(0.1), F32(0.0)), False)]


def depth_edges():
    """the comparisons `depth <= 0.1` and `depth > 100` are made in double on a float: depth exactly 100.0f is kept and the next float above it rejected; 0.1f lies
    above the double 0.1 and is kept, the next float below it is rejected.  The four disparities are found by search; fx * baseline is 64 + 2 ulp here, because with 64
    no float disparity yields the float above 100.  A 6 x 8 block beside them, at the disparity that makes its depth exactly 64 again, gives the whole pipeline
    something to return"""
    n = block(6, 16, (0, 6, 0, 8))
    spots = [(0, 12), (0, 14), (2, 12), (2, 14)]
    for r, c in spots:
        n[r, c] = True
    s = lattice_scene(n)._replace(baseline=DEPTH_BASELINE)
    num = F32(F32(FX) * F32(DEPTH_BASELINE))
    s.disp[:] = F32(num / F32(64.0))                                  # 1 + 2 ulp: the block's depth is exactly 64 again, its lattice exact
    for (r, c), (t, _) in zip(spots, DEPTH_TARGETS):
        d = disparity_for_depth(t, num)
        assert d is not None, t
        s.disp[2 * r, 2 * c] = d
    return s


def _check_disparity(name):
    p = points(name)
    if name == "disparity_specials":
        s = CASES[name][0]()
        assert len(p) == 120 - len(SPECIALS) - len(MASK_HOLES) and set(np.unique(s.mask)) == {0, 1, 128, 255}
        assert (p[:, 2] == 64.0).all() and len(result(name)) >= 10
    else:
        far = p[p[:, 2] != 64.0]
        assert len(p) == 48 + 2 and sorted(far[:, 2].tolist()) == [float(t) for t, kept in DEPTH_TARGETS if kept][::-1]
        assert float(F32(0.1)) > 0.1 and float(DEPTH_TARGETS[3][0]) <= 0.1 and float(DEPTH_TARGETS[1][0]) > 100.0
        assert len(result(name)) == 24


# ---------------------------------------------------------------- convergence
def u_nodes(arm):
    """a sideways U: two bands 5 nodes thick, 6 node rows apart, joined over the last 5 columns only; scanned row-major, the upper band's label reaches the lower band at
    its right end and has to travel left, against the scan order"""
    return block(16, arm, (0, 5, 0, arm), (11, 16, 0, arm), (5, 11, arm - 5, arm))


def serpentine_nodes(bands=4, cols=75):
    """bands 5 thick, 6 rows apart, joined at alternating ends: three turns"""
    rects = [(11 * k, 11 * k + 5, 0, cols) for k in range(bands)]
    rects += [(11 * k + 5, 11 * k + 11, cols - 5 if k % 2 == 0 else 0, cols if k % 2 == 0 else 5) for k in range(bands - 1)]
    return block(11 * bands - 6, cols, *rects)


U_ARMS = {40: (430, 254, 12), 50: (530, 314, 15), 52: (550, 326, 16), 60: (630, 374, 18), 148: (1510, 902, 48)}      # arm -> points, survivors, changing sweeps
CHANGING_SWEEPS = {}                                                  # case name -> emulated number of changing sweeps (filled by check)


def _u(arm):
    def build():
        return lattice_scene(u_nodes(arm))
    build.__doc__ = f"sideways U, arms of {arm} nodes ({arm * 0.25:g} m)"
    return build


def serpentine_4x75():
    """four bands of 75 nodes, three turns: 1590 points in a 75 x 149 px ROI"""
    return lattice_scene(serpentine_nodes())


def sweeps_of(name):
    if name not in CHANGING_SWEEPS:
        CHANGING_SWEEPS[name] = emulate_sweeps(survivors(points(name)))
    return CHANGING_SWEEPS[name]


def _check_convergence(name):
    n, m, r = counts(name)
    assert m == r and in_scan_order(result(name))                      # one component: every survivor is returned
    k = sweeps_of(name)
    if name.startswith("u_arm_"):
        assert (n, m, k) == U_ARMS[int(name[6:])]
    else:
        assert n == 1590 and k > XP_SWEEPS


def check_convergence_set():
    """the U family straddles the launched sweeps: below, the last one that fits (15), the first one whose 16th sweep still changes a label, and beyond; the friendly
    shapes stay far below"""
    got = [sweeps_of(f"u_arm_{a}") for a in sorted(U_ARMS)]
    assert got == [12, 15, 16, 18, 48] and max(got[:2]) < XP_SWEEPS <= min(got[2:])
    assert sweeps_of("capacity_band") == 6 and sweeps_of("sampled_1024") <= 5
    return got


# ---------------------------------------------------------------- flag 8
def overflow_1x8000():
    """4000 valid nodes in one row: more than DV_XP_CAP, refused with flag 8 (needs an 8000 x 1 context, which the library accepts)"""
    return lattice_scene(block(1, 4000, (0, 1, 0, 4000)), roi=(1, 8000), full_mask=True)


def _check_overflow(name):
    assert len(points(name)) == 4000 > XP_CAP


CASES = {
    "radius_band_5x30": (radius_band_5x30, _check_radius_band), "adjacency_100": (adjacency_100, _check_adjacency), "adjacency_075": (adjacency_075, _check_adjacency),
    "count_4x7": (count_4x7, _check_counts), "count_4x6": (count_4x6, _check_counts), "count_4x4": (count_4x4, _check_counts),
    "tie_right_first": (tie_right_first, _check_winner), "larger_later": (larger_later, _check_winner), "nine_beside_ten": (nine_beside_ten, _check_winner),
    "sampled_1024": (sampled_1024, _check_edges), "sampled_1025": (sampled_1025, _check_edges), "survivors_256": (survivors_256, _check_edges),
    "survivors_257": (survivors_257, _check_edges), "capacity_band": (capacity_band, _check_edges), "flush_right_bottom": (flush_right_bottom, _check_edges),
    "disparity_specials": (disparity_specials, _check_disparity), "depth_edges": (depth_edges, _check_disparity),
    "serpentine_4x75": (serpentine_4x75, _check_convergence),
}
CASES.update({f"u_arm_{a}": (_u(a), _check_convergence) for a in U_ARMS})
REFUSED = {"overflow_1x8000": (overflow_1x8000, _check_overflow)}      # raises flag 8: no output to compare
CASES_ALL = dict(CASES, **REFUSED)


def scene(name):
    return CASES_ALL[name][0]()


def check(name):
    CASES_ALL[name][1](name)


# ---------------------------------------------------------------- one frame of several objects for the tracker's device path
FRAME_SIZE = (1280, 64)
FRAME_OBJECTS = [(3, "empty", (300, 40)), (5, "tie_right_first", (200, 14)), (8, "u_arm_60", (4, 16)), (11, "capacity_band", (8, 2)), (14, "count_4x7", (400, 30))]


def frame_objects():
    """-> (disparity map of the frame, [(track id, case name, Scene moved to its place in the frame)]): an empty mask, a tie, a U whose sweeps do not converge in 16,
    the capacity band and a cluster of exactly 10, all in one launch.  Every case here samples at step 2, so one constant disparity map serves them all"""
    W, H = FRAME_SIZE
    disp = np.full((H, W), 1.0, F32)
    out = []
    for tid, name, xy in FRAME_OBJECTS:
        s = scene("count_4x6" if name == "empty" else name)
        mask = np.zeros_like(s.mask) if name == "empty" else s.mask
        assert s.disp[0, 0] == 1.0 and xy[0] + mask.shape[1] <= W and xy[1] + mask.shape[0] <= H
        out.append((tid, name, Scene(mask, xy, disp, CAM, BASELINE, FRAME_SIZE)))
    return disp, out
