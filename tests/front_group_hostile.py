"""Degenerate and unequal members for the group front end's parity tests (tests/test_front_group_hostile.py): what tests/front_hostile.py feeds one tracker, put into the
shared rounds of dv_batch_track_enqueue beside ordinary members — unequal max_cnt / min_dist, members without a row or a candidate, a tile over DISC_CAP beside sparse
ones, the three classes under masks that leave nothing, the two device limits inside a round, geometries of one tile column.  A Case is plain data: members (their frames,
masks, mode and limits) and rounds (who has a frame, in which job order, from which memory kind).  The premises are asserted on the ORACLE ALONE and printed; if a seed
misses a premise, take another seed, never loosen the premise (the pattern of tests/front_hostile.py and tests/mot_cases.py)."""
import numpy as np

from tests import front_hostile as fh

RAW, NAIVE, SEM = 0, 1, 2          # DV_MODE_RAW, DV_MODE_NAIVE, DV_MODE_SEMANTIC
DT = 0.05                          # a round's time step: frame time = DT * round, also for a member that sat a round out
LIMIT_W, LIMIT_H = 320, 240        # the size of test_front_hostile.test_limit_conditions


class Member:
    """frames: [(left, right)] in the order the member meets them (its k-th round takes frames[k]); masks: one per frame (naive / semantic) or None (raw)"""

    def __init__(self, name, max_cnt, min_dist, frames, mode=RAW, masks=None, morph=0):
        self.name, self.max_cnt, self.min_dist, self.mode, self.morph = name, max_cnt, min_dist, mode, morph
        self.frames = [(np.ascontiguousarray(l), np.ascontiguousarray(r)) for l, r in frames]
        self.masks = None if masks is None else [np.ascontiguousarray(m) for m in masks]
        self.h, self.w = self.frames[0][0].shape
        assert (mode == RAW) == (masks is None)

    def mask(self, k):
        return None if self.masks is None else self.masks[k]


class Case:
    """rounds: per round the member indices in JOB ORDER; mems: per round "host" | "pinned" | "device" (default host).  Every job of every round is built to share the
    group's launches: batched() is what dv_batch_track_info must count, and no job may run through its member's own launches"""

    def __init__(self, name, members, rounds, mems=None):
        self.name, self.members, self.rounds = name, members, [list(r) for r in rounds]
        self.mems = list(mems) if mems else ["host"] * len(rounds)
        assert all(len(r) >= 2 and len(set(r)) == len(r) for r in self.rounds) and len(self.mems) == len(self.rounds)
        for i, m in enumerate(members):
            assert len(self.met(i)) <= len(m.frames), m.name

    def met(self, i):
        """the rounds in which member i has a frame"""
        return [r for r, order in enumerate(self.rounds) if i in order]

    def frame_of(self, i, r):
        return self.met(i).index(r)

    def batched(self):
        return sum(len(r) for r in self.rounds)


def oracle_tracker(oracle, m):
    cam = fh.cam_for(m.w, m.h)
    return oracle.tracker(m.w, m.h, m.max_cnt, m.min_dist, 1, 1, cam, cam)


def oracle_frame(o, m, k, t):
    l, r = m.frames[k]
    if m.mode == RAW:
        return o.track_image(l, r, t)
    return o.track_image(l, r, t, m.masks[k], mode=m.mode, erode_k=m.morph)


def oracle_rows(oracle, case):
    """{(member, round): the oracle's rows}: every member through the oracle's tracker in its own mode, at the times of the rounds it takes part in"""
    out = {}
    for i, m in enumerate(case.members):
        o = oracle_tracker(oracle, m)
        for k, r in enumerate(case.met(i)):
            out[(i, r)] = oracle_frame(o, m, k, DT * r)
    return out


def tracked(rows):
    return int((rows["track_cnt"] > 1).sum())


def added(rows):
    return int((rows["track_cnt"] == 1).sum())


# ---------------------------------------------------------------- sequences
def drift_sequence(seed, frames=4, w=fh.W, h=fh.H):
    """a texture that drifts 1 px per frame, disparity 2 (fh.flat_sequence without the flat part)"""
    tex = fh.tex_u8(h + 8, w + 16, seed)
    assert frames <= 11
    return [(tex[2:2 + h, 4 + k:4 + k + w], tex[2:2 + h, 6 + k:6 + k + w]) for k in range(frames)]


def rolled_sequence(img, frames=3):
    """a fixed image moved 1 px per frame by a cyclic shift, disparity 1: the degenerate detector images keep their plateaus and ties in every frame"""
    return [(np.roll(img, -k, axis=1), np.roll(img, -(k + 1), axis=1)) for k in range(frames)]


# ---------------------------------------------------------------- 1. unequal members
UNEQUAL = ((8, 30), (8, 2), (50, 5), (150, 15), (1024, 2), (1, 5))


def unequal_case(reverse=False, seed0=21):
    members = [Member(f"cnt{c}_dist{d}", c, d, drift_sequence(seed0 + i, 4)) for i, (c, d) in enumerate(UNEQUAL)]
    order = list(range(len(members)))[::-1] if reverse else list(range(len(members)))
    return Case("unequal_reversed" if reverse else "unequal", members, [order] * 4)


def unequal_premises(case, ref):
    fig = {}
    for r in range(1, len(case.rounds)):
        full = [m.name for i, m in enumerate(case.members) if tracked(ref[(i, r)]) == m.max_cnt]
        adds = [m.name for i, m in enumerate(case.members) if added(ref[(i, r)]) >= 1]
        fig[r] = dict(full=full, adds=adds, rows=[len(ref[(i, r)]) for i in range(len(case.members))])
    print(f"\n[unequal] per frame after the first: {fig}")
    assert any(f["full"] and f["adds"] for f in fig.values())                   # one launch bounds a member that is asked for nothing beside one that detects
    big = [i for i, m in enumerate(case.members) if m.max_cnt == 1024][0]
    others = max(m.max_cnt for i, m in enumerate(case.members) if i != big)
    held = [len(ref[(big, r)]) for r in range(len(case.rounds))]
    print(f"[unequal] the max_cnt 1024 member holds {held} rows; the largest other max_cnt is {others}")
    assert min(held[1:]) > others
    one = [i for i, m in enumerate(case.members) if m.max_cnt == 1][0]
    assert all(len(ref[(one, r)]) == 1 for r in range(len(case.rounds)))
    return dict(big=big, big_rows=held)


# ---------------------------------------------------------------- 2. empty beside full
def empty_case(rotate=True):
    """Z never has a candidate or a row; the two saturated members overflow a candidate buffer that takes zero responses; T is ordinary.  The job list is rotated so that Z
    is first, in the middle and last in the tables; the frames come from pageable host, pinned and device memory in turn"""
    flat = np.full((fh.H, fh.W), 128, np.uint8)
    members = [Member("flat_whole", 50, 5, [(flat, flat)] * 3), Member("flat0", 50, 5, fh.flat_sequence(0)), Member("flat255", 50, 5, fh.flat_sequence(255)),
               Member("texture", 50, 5, drift_sequence(31, 3))]
    rounds = [[0, 1, 2, 3], [2, 3, 0, 1], [1, 2, 3, 0]] if rotate else [[1, 2, 3, 0]] * 3
    return Case("empty", members, rounds, ["host", "pinned", "device"])


def empty_premises(oracle, case, ref):
    assert [order.index(0) for order in case.rounds] == [0, 2, 3]               # first, in the middle, last
    for i in (1, 2):
        for rule in ("cpu", "cuda"):
            c = fh.census(oracle, case.members[i].frames[0][0], rule)
            print(f"\n[empty] {case.members[i].name} {rule}: {c}")
            assert c["with_zeros"] > c["cap"] >= c["without_zeros"]              # test_flat_sequence_condition
    rows = {m.name: [len(ref[(i, r)]) for r in range(3)] for i, m in enumerate(case.members)}
    print(f"[empty] rows per frame: {rows}")
    assert rows["flat_whole"] == [0, 0, 0]
    assert all(n >= 20 for k in ("flat0", "flat255", "texture") for n in rows[k])
    for i in (1, 2):
        assert all((ref[(i, r)]["left"][:, 3] >= 88).all() for r in range(3))    # nothing from the saturated part
    return rows


# ---------------------------------------------------------------- 3. crowded beside sparse
def crowded_case():
    """the contracting sequence at DV_MAX_FEATS / min_dist 2 beside two sparse members; member 2 sits round 3 out, which leaves S = 2, and returns"""
    members = [Member("crowded", fh.CROWD_MAX_CNT, fh.CROWD_MIN_DIST, fh.crowded_sequence()), Member("sparse_a", 30, 15, drift_sequence(41, 7)),
               Member("sparse_b", 30, 15, drift_sequence(42, 7))]
    return Case("crowded", members, [[0, 1, 2]] * 3 + [[0, 1]] + [[0, 1, 2]] * 3)


def crowded_premises(case, ref):
    n_tiles = ((fh.H + fh.TILE_H - 1) // fh.TILE_H, (fh.W + fh.TILE_W - 1) // fh.TILE_W)
    over, full_with_ties = [], []
    for r in range(len(case.rounds)):                                            # test_crowded_disc_condition, on the rows of this case
        rows = ref[(0, r)]
        old = rows[rows["track_cnt"] > 1]
        per_tile = fh.discs_per_tile(np.ascontiguousarray(old["left"][:, 3:5], np.float32), fh.W, fh.H, fh.CROWD_MIN_DIST) if r else np.zeros(n_tiles, int)
        keys = fh.order_keys(np.ascontiguousarray(rows["left"][:, 3:5], np.float32))
        ties = len(keys) - len(np.unique(keys))
        print(f"\n[crowded] frame {r}: {len(rows)} rows, {len(old)} tracked, {added(rows)} new, {ties} share a pixel, most discs on a tile {per_tile.max()}, "
              f"fewest {per_tile.min()} (DISC_CAP {fh.DISC_CAP})")
        if len(old) < fh.CROWD_MAX_CNT and added(rows) >= 1 and per_tile.max() > fh.DISC_CAP and per_tile.min() <= fh.DISC_CAP:
            over.append(r)
        if r + 1 < len(case.rounds) and len(rows) == fh.CROWD_MAX_CNT and ties >= 1:
            full_with_ties.append(r)
    assert len(over) >= 1 and len(full_with_ties) >= 1, (over, full_with_ties)
    most = 0
    for i in (1, 2):
        for r in case.met(i)[1:]:
            rows = ref[(i, r)]
            old = rows[rows["track_cnt"] > 1]
            most = max(most, int(fh.discs_per_tile(np.ascontiguousarray(old["left"][:, 3:5], np.float32), fh.W, fh.H, 15).max()))
    sparse_rows = {case.members[i].name: [len(ref[(i, r)]) for r in case.met(i)] for i in (1, 2)}
    print(f"[crowded] fallback frames {over}, full with ties {full_with_ties}; most discs on a tile of a sparse member {most}; sparse rows {sparse_rows}")
    assert most <= fh.DISC_CAP // 4                                              # nowhere near: the sparse members' tiles take the culled list
    assert case.met(2) == [0, 1, 2, 4, 5, 6] and min(len(r) for r in case.rounds) == 2
    return dict(over=over, sparse_rows=sparse_rows)


# ---------------------------------------------------------------- 4. three classes on degenerate masks
MORPH = 5


def stripes_mask(h=fh.H, w=fh.W):
    """255 in columns 3 wide, 5 columns of 0 between them and at both image borders (the erosion's border counts as 255): every MORPH x MORPH window holds a 0"""
    m = np.zeros((h, w), np.uint8)
    m[:, (np.arange(w) % 8) >= 5] = 255
    assert not m[:, 0].any() and not m[:, -1].any()
    return m


def single_pixel_mask(oracle, img, rule, h=fh.H, w=fh.W):
    """255 at the strongest corner of img under the detector's rule, 0 elsewhere"""
    x, y = oracle.gftt(img, 1, 0.01, 5, rule=rule)[0]
    m = np.zeros((h, w), np.uint8)
    m[int(y), int(x)] = 255
    return m


# which -> six members: (image, mode, mask kind, mask_morphology_size).  Two raw, two semantic, two naive in both; the masks all-0, eroded-away, single-pixel and all-255
# are spread over the two layouts so that each holds a semantic and a naive member that keeps its rows
CLASS_LAYOUTS = {
    "zero_and_eroded": (("binary", RAW, None, 0), ("checker8", RAW, None, 0), ("noise2", SEM, "all255", 0), ("tiled", SEM, "all0", 3),
                        ("flat255_54pc", NAIVE, "all255", MORPH), ("binary", NAIVE, "eroded", MORPH)),
    "single_pixel": (("noise2", RAW, None, 0), ("tiled", RAW, None, 0), ("checker8", SEM, "single", 0), ("binary", SEM, "all255", 3),
                     ("tiled", NAIVE, "single", 0), ("flat0_54pc", NAIVE, "all255", MORPH)),
}


def classes_case(oracle, which):
    imgs = fh.detector_images()
    members = []
    for k, (name, mode, kind, morph) in enumerate(CLASS_LAYOUTS[which]):
        frames = rolled_sequence(imgs[name], 3)
        if kind is None:
            masks = None
        elif kind == "single":
            masks = [single_pixel_mask(oracle, l, "cuda" if mode == NAIVE else "cpu") for l, _ in frames]
        else:
            masks = [dict(all255=np.full((fh.H, fh.W), 255, np.uint8), all0=np.zeros((fh.H, fh.W), np.uint8), eroded=stripes_mask())[kind]] * 3
        members.append(Member(f"{('raw', 'naive', 'semantic')[mode]}_{name}_{kind}", 50, 5, frames, mode, masks, morph))
    return Case(f"classes_{which}", members, [list(range(6))] * 3)


def classes_premises(oracle, case, ref, which):
    kinds = [k for _, _, k, _ in CLASS_LAYOUTS[which]]
    rows = {m.name: [(len(ref[(i, r)]), added(ref[(i, r)])) for r in range(3)] for i, m in enumerate(case.members)}
    print(f"\n[classes {which}] (rows, new corners) per frame: {rows}")
    for i, m in enumerate(case.members):
        if kinds[i] == "eroded":
            assert m.morph == MORPH and m.masks[0].any() and not oracle.erode(m.masks[0], m.morph).any()       # the member's own erosion leaves nothing
        if kinds[i] in ("all0", "eroded"):
            assert all(added(ref[(i, r)]) == 0 for r in range(3))
        if kinds[i] == "single":
            assert all(int((mk != 0).sum()) == 1 for mk in m.masks) and all(added(ref[(i, r)]) <= 1 for r in range(3))
    keeps = {mode: [m.name for i, m in enumerate(case.members) if m.mode == mode and min(len(ref[(i, r)]) for r in range(3)) >= 10] for mode in (NAIVE, SEM)}
    assert keeps[NAIVE] and keeps[SEM], keeps
    assert sorted(m.mode for m in case.members) == [RAW, RAW, NAIVE, NAIVE, SEM, SEM]
    return dict(keeps=keeps[NAIVE] + keeps[SEM], rows=rows)


# ---------------------------------------------------------------- 5. limits inside a round
def limit_members():
    """A: min_dist 3, the 4 px checkerboard first (one value bin over SEL_CAP: flag 4), benign texture from then on; B: min_dist 1, benign (the grid over SEL_MAX_CELLS:
    flag 2, every frame); C, D: min_dist 15, benign.  Four frames each"""
    chk = fh.checker(LIMIT_H, LIMIT_W, 4)
    benign = [drift_sequence(s, 4, LIMIT_W, LIMIT_H) for s in (5, 6, 7, 8)]
    return [Member("A", 150, 3, [(chk, chk)] + benign[0][1:]), Member("B", 150, 1, benign[1]), Member("C", 150, 15, benign[2]), Member("D", 150, 15, benign[3])]


def limit_premises(oracle, members):
    a = members[0]
    for rule in ("cpu", "cuda"):                                                 # test_limit_conditions
        c = fh.census(oracle, a.frames[0][0], rule)
        print(f"\n[limits] 4 px checkerboard {LIMIT_W} x {LIMIT_H} {rule}: {c}; min_dist 1 -> {LIMIT_W * LIMIT_H} cells")
        assert c["top_bin"] > fh.SEL_CAP and c["without_zeros"] > fh.SEL_CAP and c["with_zeros"] <= c["cap"]
    assert LIMIT_W * LIMIT_H > fh.SEL_MAX_CELLS                                   # B's grid
    assert ((LIMIT_W + 2) // 3) * ((LIMIT_H + 2) // 3) <= fh.SEL_MAX_CELLS         # A's grid is accepted: flag 4 stands alone
    worst = 0
    for m in members:
        for k, (l, _) in enumerate(m.frames):
            if m.name == "A" and k == 0:
                continue
            b = fh.census(oracle, l, "cpu")                                       # raw members detect by the CPU rule
            worst = max(worst, b["max_bin"])
            assert b["max_bin"] <= fh.SEL_CAP and b["with_zeros"] <= b["cap"]
    print(f"[limits] the fullest value bin of a benign frame holds {worst} candidates (SEL_CAP {fh.SEL_CAP})")


# ---------------------------------------------------------------- 6. small geometries
def small_case(w, h):
    """three raw members at 65 x 17 or 17 x 65: one tile column, 1 px ragged edges, pyramid levels below the 21 px window; two frames"""
    first = fh.partly_flat(h, w, 40, 255) if w > h else fh.tiled(h, w)
    members = [Member("named", 50, 5, rolled_sequence(first, 2)), Member("texture_a", 30, 3, drift_sequence(51, 2, w, h)), Member("texture_b", 10, 2, drift_sequence(52, 2, w, h))]
    return Case(f"small_{w}x{h}", members, [[0, 1, 2]] * 2)


def small_premises(case, ref):
    m = case.members[0]
    sizes = fh.pyramid_sizes(m.w, m.h, 3)
    rows = {mm.name: [(len(ref[(i, r)]), tracked(ref[(i, r)])) for r in range(2)] for i, mm in enumerate(case.members)}
    print(f"\n[small] {m.w} x {m.h}: levels {sizes}, (rows, tracked) per frame: {rows}")
    assert (m.w + fh.TILE_W - 1) // fh.TILE_W <= 2 and min(m.w, m.h) == 17 and all(min(s) < fh.LK_WIN for s in sizes)
    assert sum(tracked(ref[(i, 1)]) for i in range(3)) >= 5                       # the second frame does track: the small pyramids are used
    assert all(len(ref[(i, 1)]) >= 3 for i in range(3))
    return rows
