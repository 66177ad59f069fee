"""Constructed inputs for the detector head at its documented limits and at the network's own grid sizes (tests/test_solo_head_limits.py on the device,
tests/test_solo_head_ref.py on the reference alone).  solo_ref.make_case searches at random for spaced scores, which stops working once some hundred overlapping blobs decay
each other; here every score is PLACED:

  feature          channel j is +1 on tile j mod T and -1 elsewhere (T tiles = runs of consecutive pixels, each larger than the largest pixel floor unless a case wants a
                   candidate under the floor); the last channel is the constant 1.  Every channel but the last stands for a tile, so a wrong product at any k shows.
  kernel rows      a cell selects one tile or the union of two (coefficient 1 on one of the channels that stand for the tile, chosen by the cell index) with bias 1/8: the
                   logits are 9/8 | -7/8 (one tile) and 1/8 | -15/8 (two) — exact in float32 in any order, never zero.  Masks are tiles or unions of two, every IoU is 0,
                   1/3, 1/2 or 1, and sum(seg * mask) / sum_mask is sigmoid(9/8) or sigmoid(1/8).
  first-sort       the candidates are listed in the order wanted; rank r gets top / RATIO^r through its category score, the tail behind `n_ranked` lies 1 % lower and closer
                   together (never observable: asserted to lie beyond nms_pre).
  updated scores   the decay coefficient of a rank depends on the masks, labels and the ORDER only, so one float64 run with the plain grid gives every coefficient; the
                   grid is then laid again from the top with a hole of HOLE relative around every decayed score that falls inside it.
  update_thr       the geometric mean of the n_surv-th and the next updated score.
The three spacing conditions (first-sort scores up to the cut, updated scores at or above update_thr, the distance of every updated score from update_thr: 1e-3 relative,
in the float64 reference) are asserted on the result, whatever the construction did; declared ties are exempt and asserted to be exact.
No file outside the repository is read."""
import math

import numpy as np
import torch

from tests import solo_ref
from tests.solo_ref import SPACING

RATIO, HOLE = 1.0025, 1.3e-3
SEG_SCORE = {1: 1.0 / (1.0 + math.exp(-9 / 8)), 2: 1.0 / (1.0 + math.exp(-1 / 8))}
REF_GRIDS, REF_NUM_GRIDS, REF_STRIDES = (12, 16, 24, 36, 40), (40, 36, 24, 16, 12), (8, 8, 16, 32, 32)          # the network's levels and the reference's two tables
SMALL_GRIDS = (5, 4, 3, 2, 2)


def even_tiles(n_px, n_tiles):
    return [n_px // n_tiles + (t < n_px % n_tiles) for t in range(n_tiles)]


def tile_feature(channels, fh, fw, tile_px):
    T = len(tile_px)
    assert sum(tile_px) <= fh * fw and 1 <= T <= channels - 1
    tile_of = np.full(fh * fw, -1)
    tile_of[: sum(tile_px)] = np.repeat(np.arange(T), tile_px)
    feat = np.ones((channels, fh * fw), np.float32)
    for j in range(channels - 1):
        feat[j] = np.where(tile_of == j % T, 1.0, -1.0)
    return feat.reshape(channels, fh, fw)


def gaps(v, ties):
    v = np.asarray(v, np.float64)
    v = v[np.isfinite(v) & (v > 0)]
    return solo_ref.relative_gaps(np.unique(v) if ties else v)


def tile_case(channels, fh, fw, grids, n_classes, par, specs, n_ranked=None, tile_px=None, n_tiles=12, n_surv=0, top=0.74, stable=False):
    """specs: (cell, class, tiles[, "tie"]) in the first-sort order wanted ("tie": the same score as the entry before, bit for bit) -> (inputs, par with update_thr placed,
    float64 head)"""
    par = dict(par)
    tile_px = list(tile_px) if tile_px is not None else even_tiles(fh * fw, n_tiles)
    T, C = len(tile_px), channels
    n_ranked = len(specs) if n_ranked is None else n_ranked
    level_off = np.cumsum([0] + [g * g for g in grids])
    assert len({(s[0], s[1]) for s in specs}) == len(specs) and all(0 <= s[0] < level_off[-1] and 0 <= s[1] < n_classes for s in specs)
    kernels = [np.zeros((C, g, g), np.float32) for g in grids]
    cates = [np.full((n_classes, g, g), 0.01, np.float32) for g in grids]
    level = lambda cell: int(np.searchsorted(level_off, cell, side="right") - 1)
    tiles_of = {}
    for s in specs:
        cell, tiles = s[0], tuple(s[2])
        assert tiles_of.setdefault(cell, tiles) == tiles and len(set(tiles)) == len(tiles) in (1, 2), "a cell has one kernel row"
    for cell, tiles in tiles_of.items():
        l = level(cell)
        row = kernels[l].reshape(C, -1)[:, cell - level_off[l]]
        for t in tiles:
            stands = [j for j in range(C - 1) if j % T == t]
            row[stands[cell % len(stands)]] = 1.0
        row[C - 1] = 0.125

    def put(cell, cls, v):
        l = level(cell)
        cates[l].reshape(n_classes, -1)[cls, cell - level_off[l]] = v
    ties = [len(s) > 3 and s[3] == "tie" for s in specs]
    any_tie = any(ties)

    def lay(coef):
        """first-sort targets from the top: a rank steps down until it and its decayed image are clear of every image laid so far"""
        images, out = [], []
        clear = lambda v: all(abs(v - r) > HOLE * max(v, r) for r in images)
        for r in range(len(specs)):
            if ties[r]:
                assert coef[r] == 1.0 and len(specs[r][2]) == len(specs[r - 1][2])
                out.append(out[-1])
                continue
            if r < n_ranked:
                t = top if r == 0 else out[-1] / RATIO
            else:
                t = out[-1] / (1.01 if r == n_ranked else 1.00002)
            c = coef[r]
            image = r < n_ranked and np.isfinite(c) and 0.0 < c < 1.0
            assert not image or c < 1.0 - 2 * HOLE
            for _ in range(100000):
                if r >= n_ranked or (clear(t) and (not image or clear(t * c))):
                    break
                t /= 1.0 + HOLE / 4
            else:
                raise AssertionError("no room for a score")
            out.append(t)
            if image:
                images.append(t * c)
        return out

    def run(targets, p):
        for s, t in zip(specs, targets):
            v = np.float32(t / SEG_SCORE[len(s[2])])
            assert v > 1.2 * par["score_thr"], "a category score too close to score_thr: fewer ranks, or a higher top"
            put(s[0], s[1], v)
        return solo_ref.head(kernels, cates, feat, p, torch.float64, stable)
    feat = tile_feature(C, fh, fw, tile_px)
    probe = dict(par, update_thr=0.0)
    h = run(lay([1.0] * len(specs)), probe)
    assert h["n_pass"] == len(specs) and not (h["logits"] == 0).any()
    inp = dict(kernels=kernels, cates=cates, feature=feat)
    if h["n_floor"] == 0:
        return inp, par, h
    # candidate index (nonzero() order: cell, then class) of every spec, and the coefficient of every rank that was sorted
    by_cand = sorted(range(len(specs)), key=lambda i: (specs[i][0], specs[i][1]))
    spec_of_cand = np.array(by_cand)
    coef = np.ones(len(specs))
    with np.errstate(invalid="ignore", divide="ignore"):
        coef[spec_of_cand[h["sorted"][0]]] = h["updated"] / h["sorted"][1]
    h = run(lay(list(coef)), probe)
    kept = sorted(spec_of_cand[h["seg_scores"][1].numpy()].tolist())
    assert any_tie or list(spec_of_cand[h["sorted"][0]]) == kept[: par["nms_pre"]], "the first sort is not the order asked for"
    assert len(kept) <= par["nms_pre"] or sum(1 for i in kept if i < n_ranked) >= par["nms_pre"], "the tail reaches the first nms_pre"
    upd = h["updated"][np.isfinite(h["updated"])]
    if n_surv:
        u = np.sort(upd)[::-1]
        k = min(n_surv, len(u))
        lo = u[k] if k < len(u) and u[k] > 0 else u[k - 1] * 0.5
        par["update_thr"] = float(np.float32(math.sqrt(u[k - 1] * lo)))
    thr = par["update_thr"]
    h = run(lay(list(coef)), par)
    # the conditions, on the float64 reference
    first = np.sort((h["seg_scores"][0].numpy() * np.array([float(np.float32(c)) for c in _cates_of(cates, h, n_classes, level_off)])[h["seg_scores"][1].numpy()]))[::-1]
    assert gaps(first[: par["nms_pre"] + 1], any_tie) >= SPACING, "first-sort scores up to the cut are too close"
    assert gaps(upd[upd >= thr], any_tie) >= SPACING, "updated scores at or above update_thr are too close"
    assert np.min(np.abs(upd - thr)) >= SPACING * thr, "an updated score too close to update_thr"
    return inp, par, h


def _cates_of(cates, h, n_classes, level_off):
    """the category score of every candidate, in candidate order"""
    out = []
    for cell, cls in zip(*h["cand"]):
        l = int(np.searchsorted(level_off, cell, side="right") - 1)
        out.append(cates[l].reshape(n_classes, -1)[cls, cell - level_off[l]])
    return out


def scatter(rng, n_cells, n_classes, n_tiles, n, forced=(), full=None, multi=(), classes=None, two=0.15, designed=(), tiles_of=None):
    """n candidates in a random first-sort order: every cell of `forced` has at least one, `full` has every class, multi = ((cell, k), ...) have k classes, designed =
    ((rank, (cell, class, tiles[, "tie"])), ...) stand at these places of the list and their cells carry nothing else; tiles_of presets a cell's tiles"""
    classes = list(range(n_classes)) if classes is None else list(classes)
    tiles_of = dict(tiles_of or {})
    closed = {s[0] for _, s in designed}

    def tiles(cell):
        if cell not in tiles_of:
            a = int(rng.integers(n_tiles))
            tiles_of[cell] = (a,) if rng.random() >= two or n_tiles < 2 else (a, int((a + 1 + rng.integers(n_tiles - 1)) % n_tiles))
        return tiles_of[cell]
    taken, out = set(), []

    def add(cell, cls):
        if (cell, cls) in taken or cell in closed:
            return False
        taken.add((cell, cls))
        out.append((cell, cls, tiles(cell)))
        return True
    if full is not None:
        for k in range(n_classes):
            add(full, k)
    for cell, k in multi:
        for cls in rng.choice(classes, k, replace=False):
            add(cell, int(cls))
    for cell in forced:
        if not any(c == cell for c, _ in taken):
            add(cell, int(rng.choice(classes)))
    assert len(out) + len(designed) <= n
    while len(out) + len(designed) < n:
        add(int(rng.integers(n_cells)), int(rng.choice(classes)))
    out = [out[i] for i in rng.permutation(len(out))]
    for rank, s in sorted(designed, key=lambda d: d[0]):
        out.insert(rank, s)
    return out


def edge_cells(grids):
    """the first and the last cell of every level, both sides of the wave, workgroup and scan-iteration edges, the last cell"""
    off = np.cumsum([0] + [g * g for g in grids])
    n = int(off[-1])
    cells = {0, n - 1} | {int(o) for o in off[:-1]} | {int(o) - 1 for o in off[1:]}
    cells |= {c for e in (64, 256, 1024, 2048, 3072, 4096, 8192, 12288, 16384) for c in (e - 1, e) if c < n}
    return sorted(cells)


# ------------------------------------------------------------------ the cases ------------------------------------------------------------------
# name -> builder() -> dict(channels, feature, grids, classes, par, specs, further keywords of tile_case, premise(rec)); see DESIGN.md's table for the path each one reaches
SMALL = dict(channels=13, feature=(17, 31))          # 527 pixels: 12 tiles of 43 or 44, 17 mask words


def _par(origin, model, **kw):
    from dynamic_vins_amd.frontend import solo_rect
    rect = kw.pop("rect", None) or solo_rect(model[0], model[1], origin[0], origin[1])
    return solo_ref.params(rect=rect, origin=origin, **kw)


def _cells_case(grids, n_classes, num_grids=None, strides=None, seed=1):
    def build():
        rng = np.random.default_rng(seed)
        n_cells = sum(g * g for g in grids)
        edges = edge_cells(grids)
        pool = [c for c in range(n_cells) if c not in edges]
        full = pool[len(pool) // 3] if pool else None
        multi = tuple((pool[(i + 1) * len(pool) // 7], k) for i, k in enumerate((2, 3, 4, 5))) if len(pool) > 8 else ()
        n = len(edges) + (n_classes if full is not None else 0) + sum(k for _, k in multi) + 6
        specs = scatter(rng, n_cells, n_classes, 12, n, forced=edges, full=full, multi=multi)
        par = _par((67, 5), (124, 68), nms_pre=512, max_per_img=128, max_candidates=512, num_grids=num_grids or grids, strides=strides or (8,) * len(grids))

        def premise(rec):
            cells = set(rec["r64"]["cand"][0].tolist())
            assert set(edges) <= cells and rec["r64"]["n_pass"] == n
            per_cell = np.bincount(rec["r64"]["cand"][0], minlength=n_cells)
            assert full is None or per_cell[full] == n_classes
            assert all(per_cell[c] == k for c, k in multi)
        return dict(SMALL, grids=grids, classes=n_classes, par=par, specs=specs, n_surv=40, premise=premise)
    return build


def _count_case(n, extra_under_floor=3):
    """n candidates kept by the pixel floor (the sort kernel's stride of 1024) and three under it: a 12-pixel tile in cells whose floor is 16"""
    def build():
        rng = np.random.default_rng(n)
        grids, n_classes = (32, 1), 3
        tile_px = even_tiles(527 - 12, 11) + [12]
        specs = scatter(rng, 1024, n_classes, 11, n, two=0.1)
        under = [(c, 0, (11,)) for c in range(4, 1024) if not any(s[0] == c for s in specs)][:extra_under_floor]
        assert len(under) == extra_under_floor
        specs = specs[:20] + under + specs[20:]
        par = _par((67, 5), (124, 68), nms_pre=48, max_per_img=8, max_candidates=n + extra_under_floor, num_grids=(2, 40), strides=(8, 16))

        def premise(rec):
            assert rec["r64"]["n_pass"] == n + extra_under_floor and rec["r64"]["n_floor"] == n and rec["r64"]["n_sorted"] == 48
        return dict(SMALL, grids=grids, classes=n_classes, par=par, specs=specs, n_ranked=80, tile_px=tile_px, n_surv=8, premise=premise)
    return build


def _rank(rec, cell, cls):
    """place of a candidate in the float64 first sort, or None"""
    cells, labels = rec["r64"]["cand"]
    i = int(np.flatnonzero((cells == cell) & (labels == cls))[0])
    at = np.flatnonzero(rec["r64"]["sorted"][0] == i)
    return int(at[0]) if len(at) else None


def _cap4096():
    """max_candidates itself: 4096 candidates on the network's grids, 13 channels, a 33 x 67 feature (70 words, 3 pixels in the last), nms_pre 512, 131 survivors wanted of
    which max_per_img 128 stay; same-label overlaps at first-sort places 3 / 500 and 15 / 16, duplicates with the same and with another label, a chain at 350 / 360 / 370
    whose last decay is compensated by the middle one's own (a compensation above 0 in a row beyond the NMS kernel's second wave)"""
    rng = np.random.default_rng(4096)
    n_cells = sum(g * g for g in REF_GRIDS)
    edges = edge_cells(REF_GRIDS)
    free = [c for c in range(n_cells) if c not in edges]
    d = free[5::401][:9]
    designed = ((3, (d[0], 0, (0,))), (500, (d[1], 0, (0, 1))), (15, (d[2], 1, (2,))), (16, (d[3], 1, (2, 3))),
                (100, (d[4], 2, (4,))), (101, (d[4], 3, (4,))), (300, (d[5], 2, (4,))), (301, (d[5], 4, (4,))),
                (350, (d[6], 4, (6,))), (360, (d[7], 4, (6, 7))), (370, (d[8], 4, (6, 7))))
    full, multi = free[1000], tuple((free[200 * (i + 1)], k) for i, k in enumerate((2, 3, 4, 5)))
    specs = scatter(rng, n_cells, 80, 12, 4096, forced=edges, full=full, multi=multi, classes=range(5, 80), two=0.1, designed=designed, tiles_of={full: (7,)})
    par = _par((67, 5), (268, 132), nms_pre=512, max_per_img=128, max_candidates=4096, num_grids=REF_NUM_GRIDS, strides=REF_STRIDES)

    def premise(rec):
        r = rec["r64"]
        assert r["n_pass"] == 4096 and r["n_floor"] == 4096 and r["n_sorted"] == 512 and r["n"] == 128 and int((r["updated"] >= rec["par"]["update_thr"]).sum()) == 131
        assert set(edges) <= set(r["cand"][0].tolist()) and np.bincount(r["cand"][0])[full] == 80
        a, b, c, e = (_rank(rec, *designed[i][1][:2]) for i in range(4))
        assert (a, b, c, e) == (3, 500, 15, 16) and a // 64 != b // 64 and c // 16 != e // 16
        assert r["updated"][500] < 0.7 * r["sorted"][1][500] and r["updated"][16] < 0.7 * r["sorted"][1][16], "the overlaps do not decay"
        assert r["updated"][300] < 0.2 * r["sorted"][1][300] and r["updated"][301] == r["sorted"][1][301] and r["updated"][101] == r["sorted"][1][101]
        assert 0.2 < r["updated"][370] / r["sorted"][1][370] < 0.25, "exp(-2) / exp(-1/2): the compensation of a row in the sixth wave"
    return dict(channels=13, feature=(33, 67), grids=REF_GRIDS, classes=80, par=par, specs=specs, n_ranked=600, n_surv=131, premise=premise)


def _p256():
    """256 channels (48 tiles, each stood for by five or six channels), 1025 candidates of which nms_pre 512 are sorted, the LINEAR kernel: overlaps across waves and
    16-tiles, three identical same-label masks (the third column is NaN), a duplicate whose compensation is 1/2 (its score becomes exactly 0)"""
    rng = np.random.default_rng(256)
    grids, n_cells = (32, 1), 1025
    d = list(range(7, 1000, 83))
    designed = ((3, (d[0], 0, (0,))), (500, (d[1], 0, (0, 1))), (15, (d[2], 1, (2,))), (16, (d[3], 1, (2, 3))),
                (40, (d[4], 2, (4,))), (200, (d[5], 2, (4,))), (400, (d[6], 2, (4,))), (401, (d[6], 3, (4,))),
                (50, (d[7], 4, (6,))), (60, (d[8], 4, (6, 7))), (70, (d[9], 4, (6, 7))))
    specs = scatter(rng, n_cells, 80, 48, 1025, forced=(0, 1023, 1024), classes=range(5, 80), two=0.1, designed=designed)
    par = _par((64, 4), (288, 96), nms_pre=512, max_per_img=128, max_candidates=1025, num_grids=(2, 40), strides=(8, 32), nms_kernel="linear")

    def premise(rec):
        r, u32 = rec["r64"], rec["r32"]["updated"]
        assert r["n_pass"] == 1025 and r["n_floor"] > 512 and r["n_sorted"] == 512 and r["n"] == 128
        assert [_rank(rec, *s[:2]) for _, s in designed] == [k for k, _ in designed]
        assert np.isnan(u32[400]) and np.isnan(r["updated"][400]) and u32[200] == 0 and u32[40] > 0 and u32[401] > 0, "the NaN of the three identical masks"
        assert u32[70] == 0 and r["updated"][70] == 0 and 0 < u32[60] < 0.6 * rec["r32"]["sorted"][1][60], "the duplicate under a compensation of 1/2"
        assert 0 < u32[500] < 0.6 * rec["r32"]["sorted"][1][500] and 0 < u32[16] < 0.6 * rec["r32"]["sorted"][1][16]
    return dict(channels=256, feature=(24, 72), grids=grids, classes=80, par=par, specs=specs, n_ranked=600, n_tiles=48, n_surv=140, premise=premise)


def _wn137():
    """a 65 x 67 feature: 137 mask words (two chunks of 64 and one of 9, 3 pixels in the last word), 497 candidates kept (not a multiple of 16) under nms_pre 512, exactly
    max_per_img = 128 survivors, the Gaussian kernel with the overlaps of _cap4096 (the low one at place 496: the one column of the last, partial pair tile), an origin of 261 x 5 (pitch 264: a second workgroup along x; 5 rows)"""
    rng = np.random.default_rng(137)
    grids, n_cells = (33, 3, 2, 2, 1), 1107
    d = list(range(11, 1100, 97))
    designed = ((3, (d[0], 0, (0,))), (496, (d[1], 0, (0, 1))), (15, (d[2], 1, (2,))), (16, (d[3], 1, (2, 3))), (100, (d[4], 2, (4,))), (300, (d[5], 2, (4,))), (301, (d[5], 3, (4,))),
                (200, (d[6], 4, (6,))), (210, (d[7], 4, (6, 7))), (220, (d[8], 4, (6, 7))))
    specs = scatter(rng, n_cells, 128, 12, 497, forced=(1023, 1024, 1088, 1089, 1106), classes=range(5, 128), two=0.1, designed=designed)
    par = _par((261, 5), (268, 260), nms_pre=512, max_per_img=128, max_candidates=512, num_grids=(2, 2, 3, 4, 40), strides=(4, 8, 16, 32, 32))

    def premise(rec):
        r = rec["r64"]
        assert r["n_pass"] == r["n_floor"] == r["n_sorted"] == 497 and r["n"] == 128 == int((r["updated"] >= rec["par"]["update_thr"]).sum())
        assert [_rank(rec, *s[:2]) for _, s in designed] == [k for k, _ in designed]
        assert r["updated"][496] < 0.7 * r["sorted"][1][496] and r["updated"][300] < 0.2 * r["sorted"][1][300] and r["updated"][301] == r["sorted"][1][301]
        assert 0.2 < r["updated"][220] / r["sorted"][1][220] < 0.25, "exp(-2) / exp(-1/2): the compensation of a row in the fourth wave"
    return dict(channels=13, feature=(65, 67), grids=grids, classes=128, par=par, specs=specs, n_surv=128, premise=premise)


def _decay497():
    """497 sorted candidates (the last pair tile holds one column) of which all but 64 are decayed under update_thr, so that update_thr lies LOW and every decay shows: 60
    undecayed masks at the top, every other place a same-label duplicate of one of them (a duplicate wrongly left undecayed would survive), overlaps of IoU 1/2 at places
    3 / 496 and 15 / 16, and a chain at 130 / 140 / 150 whose last score is exp(-2) / exp(-1/2) of its own: the compensation of a row in the NMS kernel's third wave"""
    rng = np.random.default_rng(497)
    special = {3: (0, (0,)), 496: (0, (0, 1)), 15: (1, (2,)), 16: (1, (2, 3)), 130: (4, (6,)), 140: (4, (6, 7)), 150: (4, (6, 7))}
    specs = []
    for i in range(497):
        if i in special:
            specs.append((2 * i, special[i][0], special[i][1]))
        elif i < 60:
            specs.append((2 * i, 5 + i, (i % 6,)))
        else:
            p = int(rng.choice([q for q in range(60) if q not in special]))
            specs.append((2 * i, 5 + p, (p % 6,)))
    par = _par((67, 5), (124, 68), nms_pre=512, max_per_img=128, max_candidates=512, num_grids=(32,), strides=(32,))

    def premise(rec):
        r = rec["r64"]
        ratio = r["updated"] / r["sorted"][1]
        assert r["n_sorted"] == 497 and r["n"] == 64 and set(r["survivors"].tolist()) == set(range(60)) | {16, 496, 130, 140, 150}          # (cells ascend with the place)
        assert 0.6 < ratio[496] < 0.61 and 0.6 < ratio[16] < 0.61 and 0.6 < ratio[140] < 0.61 and 0.22 < ratio[150] < 0.23 and (ratio[[i for i in range(60, 497) if i not in special]] < 0.14).all()
    return dict(SMALL, grids=(32,), classes=80, par=par, specs=specs, n_surv=64, premise=premise)


def _upsample():
    """a 7 x 13 feature (3 channels: two tiles, an odd count) whose rectangle of 48 x 6 — laid over the feature row in which the two tiles meet, so that the planes vary along x — grows to 301 x 9: the second interpolation
    upsamples along both axes; pitch 304"""
    rng = np.random.default_rng(7)
    specs = scatter(rng, 58, 80, 2, 12, two=0.3)
    par = _par((301, 9), None, rect=(2, 10, 48, 6), nms_pre=48, max_per_img=8, max_candidates=72, strides=(8,) * 5)

    def premise(rec):
        assert rec["par"]["rect"][2] < 301 and rec["par"]["rect"][3] < 9 and rec["r64"]["n"] >= 4
    return dict(channels=3, feature=(7, 13), grids=SMALL_GRIDS, classes=80, par=par, specs=specs, n_tiles=2, n_surv=6, premise=premise)


def _tie_case(kind):
    """bit-equal scores from identical kernel rows and equal category scores in different cells and classes: two / three straddling nms_pre = 48 (every sorted candidate
    survives, so the one kept shows by its label), or two updated scores straddling max_per_img = 8"""
    def build():
        rng = np.random.default_rng(len(kind))
        at = {"two": (47, 2), "three": (46, 3), "updated": (7, 2)}[kind]
        cells = (50, 20, 35)[: at[1]]          # not in cell order: candidate order, not list order, decides
        designed = tuple((at[0] + i, (c, 70 + i, (5,)) + (("tie",) if i else ())) for i, c in enumerate(cells))
        specs = scatter(rng, 58, 80, 12, 56, classes=range(0, 60), two=0.0, designed=designed, tiles_of={c: (c % 12,) for c in range(58)})
        specs = [s if s[1] >= 70 else (s[0], i, s[2]) for i, s in enumerate(specs)]          # distinct labels: nothing decays
        par = _par((67, 5), (124, 68), nms_pre=48, max_per_img=64 if kind != "updated" else 8, max_candidates=72, strides=(8,) * 5)

        def premise(rec):
            r32, r64 = rec["r32"], rec["r64"]
            cells_, labels = r32["cand"]
            idx = [int(np.flatnonzero((cells_ == c) & (labels == 70 + i))[0]) for i, c in enumerate(cells)]
            sc = (r32["seg_scores"][0].numpy() * np.array(_cates_of(rec["inp"]["cates"], r32, 80, np.cumsum([0] + [g * g for g in SMALL_GRIDS]))))
            assert sc.dtype == np.float32 and len({sc[i].tobytes() for i in idx}) == 1, "not an exact float32 tie"
            assert int((sc > sc[idx[0]]).sum()) == at[0], "the tie does not stand where it should"
            want = sorted(idx)          # candidate order
            if kind == "updated":
                assert r32["n"] == 8 and r32["survivors"][7] == want[0] and want[1] not in r32["survivors"] and r32["scores"][7] == r32["updated"][8]
            else:
                keep = 48 - at[0]
                assert r32["n_floor"] == 56 and list(r32["sorted"][0][at[0]:]) == want[:keep] and r32["n"] == 48 and list(r32["survivors"][at[0]:]) == want[:keep]
            assert np.array_equal(r32["survivors"], r64["survivors"])
        return dict(SMALL, grids=SMALL_GRIDS, classes=80, par=par, specs=specs, n_surv=0, stable=True, premise=premise)
    return build


def _refcfg(n, n_surv):
    """the reference's configuration: grids, tables, 80 classes, nms_pre 500, max_per_img 100, the rectangle of a 1242 x 375 image in the network input — with the feature
    (24 x 72, 256 channels) and the model size (288 x 96) a quarter of the network's, so that the float64 reference stays quick.  47 tiles of 36 pixels and one of 12: its
    candidates pass the floor in the cells whose floor is 8 and fail where it is 16 or 32"""
    def build():
        rng = np.random.default_rng(n)
        n_cells = sum(g * g for g in REF_GRIDS)
        small = {c: (47,) for c in (10, 500, 1500, 2000, 2895, 2896, 3000, 3871)}
        specs = scatter(rng, n_cells, 80, 47, n, forced=tuple(small) + (0, 143, 144), two=0.15, tiles_of=small)
        par = _par((1242, 375), (288, 96), nms_pre=500, max_per_img=100, max_candidates=2048, num_grids=REF_NUM_GRIDS, strides=REF_STRIDES)

        def premise(rec):
            r = rec["r64"]
            under = n - r["n_floor"]
            assert r["n_pass"] == n and under == sum(1 for s in specs if s[2] == (47,) and s[0] >= 2896) > 0 and r["n"] == min(n_surv, 100)
            assert n < 500 or (r["n_floor"] > 500 and r["n_sorted"] == 500)
            x, y, w, h = rec["par"]["rect"]
            assert x == 0 and w == 288 and 0 < y and y + h < 96 and h % 2 == 0
        return dict(channels=256, feature=(24, 72), grids=REF_GRIDS, classes=80, par=par, specs=specs, n_ranked=min(n, 560), tile_px=[36] * 47 + [12], n_surv=n_surv, premise=premise)
    return build


BUILDERS = {
    "cells_g32": _cells_case((32,), 80, seed=1),
    "cells_g32_1": _cells_case((32, 1), 128, num_grids=(2, 40), strides=(8, 16), seed=2),
    "cells_g33": _cells_case((33, 3, 2, 2, 1), 80, num_grids=(2, 2, 3, 4, 40), strides=(4, 8, 16, 32, 32), seed=3),
    "cells_ref": _cells_case(REF_GRIDS, 80, num_grids=REF_NUM_GRIDS, strides=REF_STRIDES, seed=4),
    "cells_g64": _cells_case((64,) * 5, 128, num_grids=(64,) * 5, strides=(8, 8, 16, 32, 32), seed=5),
    "kept_1023": _count_case(1023), "kept_1024": _count_case(1024), "kept_1025": _count_case(1025),
    "cap4096": _cap4096, "p256": _p256, "wn137": _wn137, "decay497": _decay497, "upsample": _upsample,
    "tie_two": _tie_case("two"), "tie_three": _tie_case("three"), "tie_updated": _tie_case("updated"),
    "refcfg_100": _refcfg(104, 30), "refcfg_500": _refcfg(520, 104),
}
_REC = {}


def over_capacity_by_one():
    """`cap4096` with one more category score over score_thr -> (inputs, par): 4097 candidates against max_candidates 4096"""
    rec = get("cap4096")
    cates = [c.copy() for c in rec["inp"]["cates"]]
    at = np.flatnonzero(cates[2].reshape(-1) == np.float32(0.01))[17]
    cates[2].reshape(-1)[at] = 0.5
    return dict(rec["inp"], cates=cates), rec["par"]


def every_cell_passes():
    """five 64 x 64 grids whose 128 classes all pass in every cell -> (inputs, par, 2 621 440): the scan's sums at scale; the frame is refused for max_candidates"""
    grids = (64,) * 5
    par = _par((67, 5), (124, 68), nms_pre=512, max_per_img=128, max_candidates=4096, num_grids=grids, strides=(8,) * 5)
    kernels = [np.zeros((13, 64, 64), np.float32) for _ in grids]
    cates = [np.full((128, 64, 64), 0.5, np.float32) for _ in grids]
    return dict(kernels=kernels, cates=cates, feature=tile_feature(13, 17, 31, even_tiles(527, 12))), par, sum(int((c > np.float32(par["score_thr"])).sum()) for c in cates)


def get(name):
    """inputs, parameters, both references and delta of a case — computed once, shared, never changed"""
    if name not in _REC:
        b = dict(BUILDERS[name]())
        premise, (fh, fw), stable = b.pop("premise"), b.pop("feature"), b.get("stable", False)
        inp, par, _ = tile_case(b.pop("channels"), fh, fw, b.pop("grids"), b.pop("classes"), b.pop("par"), b.pop("specs"), **b)
        r64, r32 = solo_ref.reference(inp, par, torch.float64, stable), solo_ref.reference(inp, par, torch.float32, stable)
        assert r64["n"] == r32["n"] > 0
        delta = float(np.abs(r64["values"] - r32["values"].astype(np.float64)).max())
        _REC[name] = dict(name=name, inp=inp, par=par, r64=r64, r32=r32, delta=delta, stable=stable, premise=premise)
    return _REC[name]
