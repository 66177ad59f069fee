"""The line tracker's rule in plain Python / numpy, written from the reference's lines: the yardstick of tests/test_line_track*.py.

(a) `Mihasher`: a LITERAL restatement of the path BinaryDescriptorMatcher::match takes (thirdparty/line_descriptor/src/binary_descriptor_matcher.cpp:197-254) with
    Mihasher(256, 32), K = 1: the constructor (:756-784), populate (:800-819), split (bitops_custom.hpp:99-123), SparseHashtable / BucketGroup with the buckets' order
    (:851-860,874-967), query's (s, k, bitstr) enumeration with its stop rule (:635-753), checkKDistances (:107-123).
(b) `nearest_closed_form`: the closed form the kernel evaluates: least by (distance, first equal byte, train index), nothing from distance 30 on.
(c) `LineTrackerRef`: TrackLeftLine / TrackLine / TrackRightLine (line_detector/line_detector.cpp:101-297) with numpy float32 where the reference has float, then
    SetOutputFeats' `lines` map (front_end/background_tracker.cpp:373-389) as ids and source indices.

Unpinned for lack of OpenCV and of the reference's build: (1) the SparseHashtable's BucketGroups are calloc()ed, never constructed (:838): the restatement takes the
zero-filled std::vector as the EMPTY vector it is in libstdc++ / libc++, so the first insert goes through push_value; (2) whether cv::Point2f::dot is contracted to
an FMA by the reference's compiler (taken unfused) and (3) which abs() overload line_detector.cpp:123 resolves to (taken float); (4) above distance 128 the reference
leaves results[] unwritten: the restatement reports index -1 there."""
import math

import numpy as np

NO_ID = 0xFFFFFFFF
MATCH_DIST = 30
F32 = np.float32


def popcnt(x):
    return bin(x).count("1")


def hamming(p, q):
    """cv::line_descriptor::match (bitops_custom.hpp:83-96) on two 32-byte rows"""
    return int(np.unpackbits(np.bitwise_xor(p, q)).sum())


def split(code, m, mplus, b):
    """bitops_custom.hpp:99-123"""
    chunks, temp, nbits, nbyte = [0] * m, 0, 0, 0
    mask = (1 << b) - 1
    for i in range(m):
        while nbits < b:
            temp |= int(code[nbyte]) << nbits
            nbyte += 1
            nbits += 8
        chunks[i] = temp & mask
        temp = 0 if b == 64 else temp >> b
        nbits -= b
        if i == mplus - 1:
            b -= 1
            mask = (1 << b) - 1
    return chunks


ARRAY_RESIZE_FACTOR, ARRAY_RESIZE_ADD_FACTOR = 1.1, 4      # binary_descriptor_matcher.cpp:45-46


class BucketGroup:
    """:862-967 on a calloc()ed object: empty = 0, group = the empty vector.  group = [count, capacity, offsets[0 .. totones], data ...]"""

    def __init__(self):
        self.empty, self.group = 0, []

    @staticmethod
    def insert_value(vec, index, data):      # :874-898
        if len(vec) > 1:
            if vec[0] == vec[1]:
                vec[1] = int(math.ceil(vec[0] * 1.1))
                for _ in range(2 + vec[1] - len(vec)):      # (int) of the difference: negative runs no iteration
                    vec.append(0)
            vec.insert(2 + index, data)
            vec[2 + index] = data
            vec[0] += 1
        else:
            vec[:] = [1, 1, data]

    @staticmethod
    def push_value(vec, data):               # :900-923
        if len(vec) > 0:
            if vec[0] == vec[1]:
                vec[1] = int(max(math.ceil(vec[1] * ARRAY_RESIZE_FACTOR), vec[1] + ARRAY_RESIZE_ADD_FACTOR))
                for _ in range(2 + vec[1] - len(vec)):
                    vec.append(0)
            vec[2 + vec[0]] = data
            vec[0] += 1
        else:
            vec[:] = [0] * (2 + int(ARRAY_RESIZE_ADD_FACTOR))
            vec[0], vec[1], vec[2] = 1, 1, data

    def insert(self, subindex, data):        # :926-947
        g = self.group
        if len(g) == 0:
            self.push_value(g, 0)
        lowerbits = (1 << subindex) - 1
        end = popcnt(self.empty & lowerbits)
        if not (self.empty & (1 << subindex)):
            self.insert_value(g, end, g[end + 2])
            self.empty |= 1 << subindex
        totones = popcnt(self.empty)
        self.insert_value(g, totones + 1 + g[2 + end + 1], data)
        for i in range(end + 1, totones + 1):
            g[2 + i] += 1

    def query(self, subindex):               # :950-967 -> the bucket's entries in stored order
        if self.empty & (1 << subindex):
            lowerbits = (1 << subindex) - 1
            end = popcnt(self.empty & lowerbits)
            totones = popcnt(self.empty)
            size = self.group[2 + end + 1] - self.group[2 + end]
            start = 2 + totones + 1 + self.group[2 + end]
            return self.group[start:start + size]
        return []


class SparseHashtable:
    def __init__(self, b):                   # :830-842
        assert 5 <= b <= 37
        self.table = {}                      # calloc(1 << (b - 5)) BucketGroups, made on first touch

    def insert(self, index, data):           # :851-854
        self.table.setdefault(index >> 5, BucketGroup()).insert(index % 32, data)

    def query(self, index):                  # :857-860
        g = self.table.get(index >> 5)
        return g.query(index % 32) if g is not None else []


class Mihasher:
    def __init__(self, B=256, m=32):         # :756-784
        self.B, self.B_over_8, self.m = B, B // 8, m
        self.b = int(math.ceil(B / m))
        self.D = int(math.ceil(B / 2.0))
        self.d = int(math.ceil(self.D / m))
        self.mplus = B - m * (self.b - 1)
        self.H = [SparseHashtable(self.b if i < self.mplus else self.b - 1) for i in range(m)]
        self.K = 1                           # setK(1), :220

    def populate(self, codes):               # :800-819
        self.codes, self.N = codes, len(codes)
        for i in range(self.N):
            chunks = split(codes[i], self.m, self.mplus, self.b)
            for k in range(self.m):
                self.H[k].insert(chunks[k], i)

    def query(self, q):
        """:635-753 -> (results[0] or None when it stays unwritten, numres)"""
        K, m, D = self.K, self.m, self.D
        maxres = K if K else self.N
        n = 0
        seen = set()                         # counter (bitarray)
        numres = [0] * (self.B + 1)
        res = [None] * (K * (D + 1))
        chunks = split(q, m, self.mplus, self.b)
        s = 0
        while s <= self.d and n < maxres:
            for k in range(m):
                curb = self.b if k < self.mplus else self.b - 1
                chunksk = chunks[k]
                bitstr = 0
                power = list(range(s)) + [curb + 1] + [0] * 4
                bit = s - 1
                while True:
                    if bit != -1:
                        bitstr ^= (1 << power[bit]) if power[bit] == bit else (3 << (power[bit] - 1))
                        power[bit] += 1
                        bit -= 1
                    else:
                        for index in self.H[k].query(chunksk ^ bitstr):
                            if index not in seen:
                                seen.add(index)
                                hammd = hamming(self.codes[index], q)
                                if hammd <= D and numres[hammd] < maxres:
                                    res[hammd * K + numres[hammd]] = index + 1
                                numres[hammd] += 1
                        bit += 1
                        while bit < s and power[bit] == power[bit + 1] - 1:
                            bitstr ^= 1 << (power[bit] - 1)
                            power[bit] = bit
                            bit += 1
                        if bit == s:
                            break
                n = n + numres[s * m + k]
                if n >= maxres:
                    break
            s += 1
        n, results = 0, [None] * max(K, 1)
        s = 0
        while s <= D and n < K:
            c = 0
            while c < numres[s] and n < K:
                results[n] = res[s * K + c]
                n += 1
                c += 1
            s += 1
        return results[0], numres


def check_k_distances(numres, k, string_length=256):
    """:107-123 for one row"""
    out = []
    for j in range(string_length + 1):
        if len(out) >= k:
            break
        for _ in range(numres[j]):
            if len(out) >= k:
                break
            out.append(j)
    return out


def match_literal(query, train):
    """BinaryDescriptorMatcher::match (:197-254) -> (trainIdx [nq], distance [nq]); trainIdx -1 where results[] stays unwritten, distance -1 where k_distances is empty.
    None when either matrix has no rows (:201-205: no matches at all)."""
    query, train = np.asarray(query, np.uint8).reshape(-1, 32), np.asarray(train, np.uint8).reshape(-1, 32)
    if len(query) == 0 or len(train) == 0:
        return None
    mh = Mihasher(256, 32)
    mh.populate(train)
    idx, dist = np.full(len(query), -1, np.int64), np.full(len(query), -1, np.int64)
    for i, q in enumerate(query):
        r, numres = mh.query(q)
        kd = check_k_distances(numres, 1)
        if r is not None:
            idx[i] = r - 1
        if kd:
            dist[i] = kd[0]
    return idx, dist


def first_equal_byte(q, t):
    eq = np.flatnonzero(np.asarray(q) == np.asarray(t))
    return int(eq[0]) if len(eq) else 32


def nearest_closed_form(query, train):
    """(b): per query the train row least by (distance, first equal byte, index) among those nearer than 30; (-1, 0) when there is none"""
    query, train = np.asarray(query, np.uint8).reshape(-1, 32), np.asarray(train, np.uint8).reshape(-1, 32)
    idx, dist = np.full(len(query), -1, np.int64), np.zeros(len(query), np.int64)
    if len(train) == 0:
        return idx, dist
    for i, q in enumerate(query):
        d = np.unpackbits(np.bitwise_xor(train, q[None, :]), axis=1).sum(1)
        h = int(d.min())
        if h >= MATCH_DIST:
            continue
        cand = np.flatnonzero(d == h)
        keys = [(first_equal_byte(q, train[j]), int(j)) for j in cand]
        idx[i], dist[i] = min(keys)[1], h
    return idx, dist


def match_for_tracking(query, train, literal):
    """the matches TrackLine reads: [(queryIdx, trainIdx, distance)] with distance < 30 only (everything else fails the first test of :116)"""
    if len(query) == 0 or len(train) == 0:
        return []
    if literal:
        idx, dist = match_literal(query, train)
        return [(i, int(idx[i]), int(dist[i])) for i in range(len(query)) if 0 <= dist[i] < MATCH_DIST]
    idx, dist = nearest_closed_form(query, train)
    return [(i, int(idx[i]), int(dist[i])) for i in range(len(query)) if idx[i] >= 0]


def gate(q, t, fused=False, int_abs=False):
    """line_detector.cpp:118-123 in float32: q, t = (sx, sy, ex, ey, angle, length) rows.  fused / int_abs: the two readings the tests must tell apart from the declared one"""
    q, t = np.asarray(q, F32), np.asarray(t, F32)

    def dot(x, y):
        if fused:
            return F32(np.float64(x) * np.float64(x) + np.float64(F32(y * y)))      # fma(x, x, y * y): one rounding of the exact x * x + fl(y * y)
        return F32(F32(x * x) + F32(y * y))
    s = dot(F32(q[0] - t[2]), F32(q[1] - t[3]))
    e = dot(F32(q[2] - t[2]), F32(q[3] - t[3]))
    da = F32(q[4] - t[4])
    a = abs(int(da)) if int_abs else float(F32(abs(da)))
    return bool(s < F32(40000.0)) and bool(e < F32(40000.0)) and a < 0.1


def is_h(angle):
    a = float(F32(angle))
    return (a >= 3.14 / 4 and a <= 3 * 3.14 / 4) or (a <= -3.14 / 4 and a >= -3 * 3.14 / 4)


class LineTrackerRef:
    """(c).  frame(left_lines, left_desc, right_lines, right_desc) -> dict of the frame's left / right sets and the `lines` map"""

    def __init__(self, literal=False, fused=False, int_abs=False):
        self.literal, self.fused, self.int_abs = literal, fused, int_abs
        self.reset()

    def reset(self):
        self.prev = None                     # bg.prev_lines: None before the first frame
        self.global_line_id = 0

    def _matches(self, q_lines, q_desc, t_lines, t_desc):
        good = []
        for qi, ti, _ in match_for_tracking(q_desc, t_desc, self.literal):
            if gate(q_lines[qi], t_lines[ti], self.fused, self.int_abs):
                good.append((qi, ti))
        return good

    def frame(self, left_lines, left_desc, right_lines=None, right_desc=None):
        L = np.asarray(left_lines, F32).reshape(-1, 6)
        Ld = np.asarray(left_desc, np.uint8).reshape(-1, 32)
        n = len(L)
        info = {"h_new": 0, "v_new": 0, "dropped": 0, "good": []}
        if self.prev is None:                # TrackLeftLine :229-234
            ids = [self.global_line_id + i for i in range(n)]
            self.global_line_id += n
            src, cnt_map = list(range(n)), {}
        else:
            P = self.prev
            ids = [NO_ID] * n
            good = self._matches(L, Ld, P["lines"], P["desc"])
            info["good"] = good
            cnt_map = {}
            for qi, ti in good:
                line_id = P["ids"][ti]
                ids[qi] = line_id
                cnt_map.setdefault(line_id, P["cnt_map"].get(line_id, 0) + 1)      # map::insert keeps the first
            tracked, new = [], []
            for i in range(n):
                if ids[i] == NO_ID:
                    ids[i] = self.global_line_id & 0xFFFFFFFF
                    self.global_line_id += 1
                    new.append(i)
                else:
                    tracked.append(i)
            h_new = [i for i in new if is_h(L[i, 4])]
            v_new = [i for i in new if not is_h(L[i, 4])]
            h_line = sum(1 for i in tracked if is_h(L[i, 4]))
            v_line = len(tracked) - h_line
            diff_h, diff_v = 35 - h_line, 35 - v_line
            src = list(tracked)
            if diff_h > 0:
                diff_h = min(diff_h, len(h_new))
                src += h_new[:diff_h]
            if diff_v > 0:
                diff_v = min(diff_v, len(v_new))
                for i in v_new[:diff_v]:
                    src.append(i)
                    cnt_map.setdefault(ids[i], 1)
            info.update(h_new=len(h_new), v_new=len(v_new), dropped=n - len(src), h_tracked=h_line, v_tracked=v_line)
        out_ids = [ids[i] for i in src]
        cur = {"lines": L[src].copy(), "desc": Ld[src].copy(), "ids": out_ids, "cnt_map": cnt_map}
        self.prev = cur
        left_cnt = [cnt_map.get(i, 0) for i in out_ids]
        # TrackRightLine :246-297
        r_ids, r_src = [], []
        if right_lines is not None:
            R = np.asarray(right_lines, F32).reshape(-1, 6)
            Rd = np.asarray(right_desc, np.uint8).reshape(-1, 32)
            rid = [NO_ID] * len(R)
            rgood = self._matches(R, Rd, cur["lines"], cur["desc"])
            for qi, ti in rgood:
                rid[qi] = out_ids[ti]
            r_src = [i for i in range(len(R)) if rid[i] != NO_ID]
            r_ids = [rid[i] for i in r_src]
            info["right_good"] = rgood
        # SetOutputFeats :373-389 and feature_manager.cpp:127-128: per id the first left line and the first right line
        lines_map = {}
        for k, i in enumerate(out_ids):
            lines_map.setdefault(i, [k, -1])
        for k, i in enumerate(r_ids):
            if lines_map[i][1] < 0:
                lines_map[i][1] = k
        rows = [(i, lines_map[i][0], lines_map[i][1]) for i in sorted(lines_map)]      # (id, position in the left set, position in the right set or -1)
        return {"left_ids": np.array(out_ids, np.uint32), "left_src": np.array(src, np.int32), "left_cnt": np.array(left_cnt, np.int32),
                "right_ids": np.array(r_ids, np.uint32), "right_src": np.array(r_src, np.int32), "rows": rows, "info": info}
