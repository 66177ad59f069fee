"""Scenario builders for the line tracker's tests, with their coverage ASSERTED on the reference run (tests/line_track_ref.py) before anything is compared: a builder
that stops producing a condition fails loudly.  Random 256-bit descriptors sit about 128 bits apart and exercise nothing, so a descriptor is a base code per landmark
with a few controlled bit flips."""
import math

import numpy as np

from tests import line_track_ref as lr

F32 = np.float32
DV_LINE_MAX = 512


def flip(desc, bits):
    """a copy of the 32-byte row with the given bit indices flipped (bit i lives in byte i // 8)"""
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def base_codes(n, rng, min_apart=70):
    codes = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n > 1:
        bits = np.unpackbits(codes, axis=1).astype(np.int32)
        d = bits @ (1 - bits).T + (1 - bits) @ bits.T
        np.fill_diagonal(d, 999)
        assert d.min() >= min_apart, "base codes too close: change the seed"
    return codes


# ---------------------------------------------------------------- the match step alone ----------------------------------------------------------------
def match_case(seed=5):
    """-> (query [nq, 32], train [nt, 32], tags): crafted rows among unrelated ones.  tags[name] = query index"""
    rng = np.random.default_rng(seed)
    base = base_codes(24, rng)
    train, query, tags = [], [], {}

    def add_train(row):
        train.append(row)
        return len(train) - 1

    for k in range(6):                                         # unrelated rows first, so that crafted indices are not 0
        add_train(base[16 + k])
    # distance exactly 29 and exactly 30: one flip in each of bytes 0 .. h - 1
    q = base[0]; add_train(flip(q, [8 * i + 3 for i in range(29)])); query.append(q); tags["d29"] = len(query) - 1
    q = base[1]; add_train(flip(q, [8 * i + 5 for i in range(30)])); query.append(q); tags["d30"] = len(query) - 1
    # a tie at the minimum with different first equal bytes: the LOWER index has its first equal byte later and loses
    q = base[2]
    lo = add_train(flip(q, [1, 9, 17]))                        # bytes 0, 1, 2 differ: first equal byte 3
    hi = add_train(flip(q, [41, 49, 57]))                      # bytes 5, 6, 7 differ: first equal byte 0
    query.append(q); tags["tie_key"] = len(query) - 1; tags["tie_key_rows"] = (lo, hi)
    # a tie with the same first equal byte: the lower index wins
    q = base[3]
    lo = add_train(flip(q, [80, 90]))
    hi = add_train(flip(q, [83, 95]))
    query.append(q); tags["tie_idx"] = len(query) - 1; tags["tie_idx_rows"] = (lo, hi)
    # flips occupying bytes 0 .. h - 1: the first equal byte is h
    q = base[4]; add_train(flip(q, [0, 15, 16, 31, 36])); query.append(q); tags["lead"] = len(query) - 1
    # duplicate train rows
    q = base[5]; row = flip(q, [100, 200]); a = add_train(row); b = add_train(row.copy()); query.append(q); tags["dup"] = len(query) - 1; tags["dup_rows"] = (a, b)
    # nothing near (about 128 away), an exact copy, and a row at distance 1 whose only flip is in byte 0
    query.append(base[6]); tags["far"] = len(query) - 1
    q = base[7]; add_train(q.copy()); query.append(q); tags["exact"] = len(query) - 1
    q = base[8]; add_train(flip(q, [7])); query.append(q); tags["byte0"] = len(query) - 1
    return np.array(query, np.uint8), np.array(train, np.uint8), tags


def match_conditions(query, train, tags, idx, dist):
    """the required conditions, on the literal restatement's own answer (idx, dist)"""
    def d(i, j):
        return lr.hamming(query[i], train[j])
    assert dist[tags["d29"]] == 29 and dist[tags["d30"]] == 30
    i = tags["tie_key"]; lo, hi = tags["tie_key_rows"]
    assert d(i, lo) == d(i, hi) == dist[i] and lo < hi and lr.first_equal_byte(query[i], train[lo]) > lr.first_equal_byte(query[i], train[hi]) and idx[i] == hi
    i = tags["tie_idx"]; lo, hi = tags["tie_idx_rows"]
    assert d(i, lo) == d(i, hi) == dist[i] and lr.first_equal_byte(query[i], train[lo]) == lr.first_equal_byte(query[i], train[hi]) and idx[i] == lo
    i = tags["lead"]
    assert dist[i] == 5 and lr.first_equal_byte(query[i], train[idx[i]]) == 5
    i = tags["dup"]; a, b = tags["dup_rows"]
    assert np.array_equal(train[a], train[b]) and idx[i] == a
    assert dist[tags["far"]] >= 64 or dist[tags["far"]] < 0
    assert dist[tags["exact"]] == 0 and dist[tags["byte0"]] == 1


def near_pairs(n, seed):
    """n seeded (query, train set) problems of near duplicates: 2 - 6 train rows within 0 .. 34 flips of the query, among a few unrelated rows"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q = rng.integers(0, 256, 32, dtype=np.uint8)
        rows = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(int(rng.integers(0, 4)))]
        h = int(rng.integers(0, 35))
        for _ in range(int(rng.integers(2, 7))):
            k = max(0, h + int(rng.integers(0, 3)) - (1 if rng.random() < 0.2 else 0))
            if rng.random() < 0.5:                             # flips packed into the leading bytes: late first equal bytes
                bits = rng.choice(min(256, 8 * max(k, 1) + 16), k, replace=False)
            else:
                bits = rng.choice(256, k, replace=False)
            rows.append(flip(q, [int(b) for b in bits]))
        order = rng.permutation(len(rows))
        out.append((q, np.array([rows[i] for i in order], np.uint8)))
    return out


# ---------------------------------------------------------------- tracking scenarios ----------------------------------------------------------------
class Scene:
    """landmarks with a base descriptor, end points and an angle; obs() = one detection of a landmark: <= `flips` bit flips and a small jitter"""

    def __init__(self, n, seed):
        self.rng = np.random.default_rng(seed)
        self.base = base_codes(n, self.rng)
        r = self.rng
        self.s = r.uniform(50, 600, (n, 2))
        self.e = self.s + r.uniform(-60, 60, (n, 2))
        self.angle = np.where(np.arange(n) % 2 == 0, r.uniform(1.0, 2.0, n), r.uniform(-0.5, 0.5, n))      # even landmarks "h", odd ones "v"

    def obs(self, k, flips=5, jitter=1.0, shift=(0.0, 0.0), angle=None):
        r = self.rng
        nf = int(r.integers(0, flips + 1))
        desc = flip(self.base[k], [int(b) for b in r.choice(256, nf, replace=False)])
        j = r.uniform(-jitter, jitter, 4)
        a = self.angle[k] if angle is None else angle
        line = np.array([self.s[k, 0] + j[0] + shift[0], self.s[k, 1] + j[1] + shift[1], self.e[k, 0] + j[2] + shift[0], self.e[k, 1] + j[3] + shift[1],
                         a, math.hypot(*(self.e[k] - self.s[k]))], F32)
        return line, desc

    def frame(self, left, right=None):
        """left / right: lists of landmark indices or (index, dict of obs keywords) -> (L [n, 6], Ld [n, 32], R, Rd); right None = no right image"""
        def side(items, shift):
            rows = [self.obs(it[0], shift=shift, **it[1]) if isinstance(it, tuple) else self.obs(it, shift=shift) for it in items]
            if not rows:
                return np.zeros((0, 6), F32), np.zeros((0, 32), np.uint8)
            return np.array([r[0] for r in rows], F32), np.array([r[1] for r in rows], np.uint8)
        L, Ld = side(left, (0.0, 0.0))
        if right is None:
            return L, Ld, None, None
        R, Rd = side(right, (-12.0, 0.0))
        return L, Ld, R, Rd


def fused_straddle():
    """(dx, dy) float32 whose unfused float32 dx dx + dy dy and BOTH single-FMA forms fall on different sides of 40000"""
    for i in range(1, 400):
        dx = F32(37.0 + 0.37 * i)
        dy0 = F32(math.sqrt(40000.0 - float(dx) ** 2))
        dy = dy0
        for _ in range(40):
            dy = np.nextafter(dy, F32(0))
        for _ in range(80):
            dy = np.nextafter(dy, F32(1e9))
            un = F32(F32(dx * dx) + F32(dy * dy)) < F32(40000)
            fa = F32(np.float64(dx) * np.float64(dx) + np.float64(F32(dy * dy))) < F32(40000)
            fb = F32(np.float64(dy) * np.float64(dy) + np.float64(F32(dx * dx))) < F32(40000)
            if un != fa and un != fb:
                return dx, dy, bool(un)
    raise AssertionError("no straddling pair found")


def small_scenario(seed=21):
    """8 frames, 0 .. 80 lines: every required condition of the tracker (see conditions())"""
    sc = Scene(140, seed)
    A = list(range(20))                      # 10 h, 10 v
    B = [20, 21, 22, 23, 24, 25]             # top-ups of frame 1: 3 h, 3 v
    G, Q = 26, 27                            # the gate landmark and the angle landmark
    C = list(range(30, 110))                 # 40 h, 40 v: the quota frame
    E = list(range(110, 115))
    dx, dy, _ = fused_straddle()
    sc.s[G], sc.e[G] = (100.0, 100.0), (0.0, 0.0)
    frames = []
    frames.append(sc.frame(A + [G, Q], right=A[:12]))                                                   # 0: first frame
    frames.append(sc.frame(A[:3] + [A[0]] + A[3:] + B + [(G, dict(jitter=0.0)), Q], right=A[:6] + [A[2], A[2]] + B[:2]))      # 1: two queries take one train line; top-ups; right lines share an id
    # 2: the h top-ups read 1, the v top-ups 2; G's start sits (dx, dy) from its previous END; Q's angle is off by 0.5; empty right image
    L, Ld, R, Rd = sc.frame(A + B + [(G, dict(jitter=0.0)), (Q, dict(angle=sc.angle[Q] + 0.5))], right=[])
    g = len(A) + len(B)
    L[g, 0], L[g, 1], L[g, 2], L[g, 3] = dx, dy, F32(10.0), F32(10.0)
    frames.append((L, Ld, R, Rd))
    frames.append(sc.frame([], right=A[:4]))                                                            # 3: an empty current frame (with a right image)
    # 4: after the empty frame nothing matches and the quota applies: 40 new h, 40 new v -> 35 + 35; angles around 3.14 / 4
    L, Ld, R, Rd = sc.frame(C, right=C[:20])
    L[1, 4], L[3, 4], L[5, 4] = F32(0.7849), F32(0.7852), F32(0.7856)                                   # v | h, between 3.14 / 4 and pi / 4 | h
    frames.append((L, Ld, R, Rd))
    frames.append(sc.frame(C[:30] + E, right=C[10:30]))                                                 # 5: fresh ids skip what the quota dropped
    frames.append(sc.frame(C[:30] + E, right=None))                                                     # 6: no right image at all
    frames.append(sc.frame(C[:30] + E + A[:5], right=C[:5] + E))                                        # 7
    return frames


def wave_scenario(n, seed=33):
    """3 frames of n lines, all tracked from the second on, right image of the same size: the sizes around a wave (63 / 64 / 65)"""
    sc = Scene(n, seed)
    ids = list(range(n))
    return [sc.frame(ids, right=ids) for _ in range(3)]


def cap_scenario(seed=44):
    """2 frames of DV_LINE_MAX lines on both sides"""
    sc = Scene(DV_LINE_MAX, seed)
    ids = list(range(DV_LINE_MAX))
    return [sc.frame(ids, right=ids) for _ in range(2)]


def run_ref(frames, reset_before=(), **kw):
    ref = lr.LineTrackerRef(**kw)
    out = []
    for k, (L, Ld, R, Rd) in enumerate(frames):
        if k in reset_before:
            ref.reset()
        out.append(ref.frame(L, Ld, R, Rd))
    return out


def conditions(frames, res):
    """the small scenario's required conditions on the reference run `res`"""
    # first frame: ids 0 .. n - 1 in order, no counts
    assert np.array_equal(res[0]["left_ids"], np.arange(len(frames[0][0]))) and not res[0]["left_cnt"].any()
    # two queries taking one train line
    assert any(len({t for _, t in r["info"]["good"]}) < len(r["info"]["good"]) for r in res)
    assert any(len(set(r["left_ids"].tolist())) < len(r["left_ids"]) for r in res)
    # an h top-up (count 0) whose count reads 1 when tracked next frame, a v top-up (count 1) reading 2
    ok_h = ok_v = False
    for a, b in zip(res[:-1], res[1:]):
        nxt = dict(zip(b["left_ids"].tolist(), b["left_cnt"].tolist()))
        nt = a["info"].get("h_tracked", 0) + a["info"].get("v_tracked", 0)
        if "h_tracked" not in a["info"]:
            continue
        for i, c in list(zip(a["left_ids"].tolist(), a["left_cnt"].tolist()))[nt:]:
            ok_h |= c == 0 and nxt.get(i) == 1
            ok_v |= c == 1 and nxt.get(i) == 2
    assert ok_h and ok_v
    # more than 35 new h and more than 35 new v in one frame, behind an EMPTY frame; the next frame's fresh ids skip the dropped ones
    k = next(k for k, r in enumerate(res) if r["info"]["h_new"] > 35 and r["info"]["v_new"] > 35)
    assert len(frames[k - 1][0]) == 0 and len(res[k - 1]["left_ids"]) == 0 and res[k]["info"]["dropped"] > 0 and len(res[k]["left_ids"]) == 70
    fresh = sorted(set(res[k + 1]["left_ids"].tolist()) - set(res[k]["left_ids"].tolist()))
    assert fresh and fresh[0] > int(res[k]["left_ids"].max()) + 1
    # angles on each side of 3.14 / 4 and between 3.14 / 4 and pi / 4
    a = frames[k][0][[1, 3, 5], 4]
    assert float(a[0]) < 3.14 / 4 <= float(a[1]) < math.pi / 4 < float(a[2]) and [lr.is_h(x) for x in a] == [False, True, True]
    # empty right image, right lines sharing an id, a frame without a right image
    assert any(f[2] is not None and len(f[2]) == 0 for f in frames) and any(f[2] is None for f in frames)
    assert any(len(set(r["right_ids"].tolist())) < len(r["right_ids"]) for r in res)
    assert any(len(r["right_ids"]) > 0 and len(r["right_ids"]) < len(f[2]) for f, r in zip(frames, res) if f[2] is not None)
    # the gate: a fused sum and the int abs() each change the outcome
    ids = [r["left_ids"].tolist() for r in res]
    assert [r["left_ids"].tolist() for r in run_ref(frames, fused=True)] != ids
    assert [r["left_ids"].tolist() for r in run_ref(frames, int_abs=True)] != ids
