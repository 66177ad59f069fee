"""The multi-object tracker's rule in numpy, written from the reference's lines (mot/deep_sort.cpp:72-139, mot/tracker_manager.h:40-156, mot/tracker_manager.cpp:20-69,
mot/kalman_tracker.cpp:20-96, mot/feature_bundle.h:40-50, mot/feature_metric.h:32-61): the yardstick of tests/test_mot*.py.  The filter and cost arithmetic run in the
dtype given (float32 as the reference, or float64); Munkres (mot/hungarian.cpp, restated step by step below) is always double.

Kept as the reference computes it: AssociateDetectionsToTrackersIdx subtracts the assigned COLUMN INDICES from the detection ids (tracker_manager.cpp:62-68), which
differ in stage 2 once stage 1 has matched something.  predict / correct are OpenCV 3.4's KalmanFilter from memory (include/dvins.h).

The library's declared rule (include/dvins.h) is applied in front of the Munkres call, which need not end on a NaN: a NaN appearance or IoU distance
counts as gated in both stages.  torch::min carries a NaN (feature_metric.h:59-61), so one NaN row in a gallery makes that track's appearance distance a NaN for every
detection.  MotRef(flip={...}) turns single comparisons from `>` into `>=` (`<` into `<=`): the mutants that tests/mot_hostile.py shows its cases to tell apart."""
import copy

import numpy as np

TENTATIVE, CONFIRMED, DELETED = 0, 1, 2
INVALID_DIST = 1000.0
DBL_EPSILON = float(np.finfo(np.float64).eps)


def munkres(dist):
    """HungarianAlgorithm::Solve -> assignment[row] = column or -1.  dist: [rows, cols]; worked on in double, column by column as assignmentoptimal holds it."""
    dist = np.asarray(dist, np.float64)
    if dist.shape[0] == 0:
        return np.zeros(0, np.int64)
    R, C = dist.shape
    d = dist.copy()
    star = np.zeros((R, C), bool)
    prime = np.zeros((R, C), bool)
    cov_c = np.zeros(C, bool)
    cov_r = np.zeros(R, bool)
    assignment = np.full(R, -1, np.int64)
    if C == 0:
        return assignment
    if R <= C:
        min_dim = R
        d -= d.min(axis=1, keepdims=True)
        for row in range(R):
            for col in range(C):
                if abs(d[row, col]) < DBL_EPSILON and not cov_c[col]:
                    star[row, col] = True
                    cov_c[col] = True
                    break
    else:
        min_dim = C
        d -= d.min(axis=0, keepdims=True)
        for col in range(C):
            for row in range(R):
                if abs(d[row, col]) < DBL_EPSILON and not cov_r[row]:
                    star[row, col] = True
                    cov_c[col] = True
                    cov_r[row] = True
                    break
        cov_r[:] = False
    while True:
        # step 2b
        if int(cov_c.sum()) == min_dim:
            for row in range(R):
                cols = np.flatnonzero(star[row])
                if len(cols):
                    assignment[row] = cols[0]
            return assignment
        # step 3
        found = None
        zeros_found = True
        while zeros_found and found is None:
            zeros_found = False
            for col in range(C):
                if cov_c[col]:
                    continue
                rows = np.flatnonzero(~cov_r & (np.abs(d[:, col]) < DBL_EPSILON))      # the first row of the reference's inner scan
                if not len(rows):
                    continue
                row = int(rows[0])
                prime[row, col] = True
                star_cols = np.flatnonzero(star[row])
                if not len(star_cols):
                    found = (row, col)
                    break
                cov_r[row] = True
                cov_c[star_cols[0]] = False
                zeros_found = True
        if found is not None:
            # step 4
            row, col = found
            new_star = star.copy()
            new_star[row, col] = True
            star_col = col
            star_rows = np.flatnonzero(star[:, star_col])
            while len(star_rows):
                star_row = int(star_rows[0])
                new_star[star_row, star_col] = False
                prime_col = int(np.flatnonzero(prime[star_row])[0])
                new_star[star_row, prime_col] = True
                star_col = prime_col
                star_rows = np.flatnonzero(star[:, star_col])
            prime[:] = False
            star = new_star
            cov_r[:] = False
            # step 2a
            cov_c |= star.any(axis=0)
        else:
            # step 5
            h = d[~cov_r][:, ~cov_c].min()
            d[cov_r, :] += h
            d[:, ~cov_c] -= h


class Track:
    def __init__(self, dt):
        self.x = np.zeros(7, dt)
        self.P = np.eye(7, dtype=dt)
        self.state, self.id, self.hits, self.tsu = TENTATIVE, -1, 0, 0
        self.store, self.next, self.full = None, 0, False

    def n_feats(self):
        return len(self.store) if self.full else self.next


class MotRef:
    FLIPS = ("iou1", "feat", "iou2", "invalid", "n_init", "max_age", "union")

    def __init__(self, n_init=3, max_age=5, budget=100, feat_dim=512, max_tracks=128, dtype=np.float64, flip=()):
        """flip: names out of FLIPS whose comparison is taken with equality on the other side (`a > b` becomes `a >= b`, the union's `un < eps` becomes `un <= eps`);
        empty is the reference's behaviour"""
        self.n_init, self.max_age, self.budget, self.feat_dim, self.max_tracks, self.dt = n_init, max_age, budget, feat_dim, max_tracks, np.dtype(dtype).type
        self.flip = frozenset(flip)
        assert self.flip <= set(self.FLIPS), self.flip
        dt = self.dt
        self.A = np.eye(7, dtype=dt)
        self.A[0, 4] = self.A[1, 5] = self.A[2, 6] = 1
        self.H = np.eye(4, 7, dtype=dt)
        self.Q = np.eye(7, dtype=dt) * dt(1e-2)
        self.Rm = np.eye(4, dtype=dt) * dt(1e-1)
        self.reset()

    def reset(self):
        self.tracks, self.next_id = [], 1
        self.log = []          # per frame: dict of what happened (events, the Munkres problems, the gate distances)

    def gt(self, name, a, b):
        """a > b as the reference has it; a >= b when `name` is flipped"""
        with np.errstate(invalid="ignore"):
            return a >= b if name in self.flip else a > b

    # ---- KalmanTracker ----
    def rect(self, t):
        dt = self.dt
        with np.errstate(all="ignore"):
            cx, cy, s, r = (dt(v) for v in t.x[:4])
            w = np.sqrt(s * r)
            h = s / w
            return np.array([cx - w / dt(2), cy - h / dt(2), w, h], dt)

    def measure(self, rc):
        dt = self.dt
        x, y, w, h = (dt(v) for v in rc)
        return np.array([x + w / dt(2), y + h / dt(2), w * h, w / h], dt)

    def iou_dist(self, a, b):
        dt = self.dt
        x1, y1 = max(a[0], b[0]), max(a[1], b[1])
        w = min(a[0] + a[2], b[0] + b[2]) - x1
        h = min(a[1] + a[3], b[1] + b[3]) - y1
        if w <= 0 or h <= 0:
            w = h = dt(0)
        inter = w * h
        un = a[2] * a[3] + b[2] * b[3] - inter
        if float(un) < DBL_EPSILON or ("union" in self.flip and float(un) == DBL_EPSILON):
            return dt(1)
        with np.errstate(all="ignore"):
            return dt(1) - inter / un

    def _associate(self, cost, trks, dets, matched, info):
        """AssociateDetectionsToTrackersIdx: cost [len(trks), len(dets)] in the working dtype; trks / dets are updated in place as the reference leaves them"""
        dist = np.asarray(cost, np.float64).reshape(len(trks), len(dets))
        assignment = munkres(dist) if len(trks) else np.zeros(0, np.int64)
        info["problems"].append(dist.copy())
        assignment = assignment.copy()
        for i in range(len(assignment)):
            if assignment[i] == -1:
                continue
            if self.gt("invalid", dist[i, assignment[i]], INVALID_DIST / 10):
                assignment[i] = -1
            else:
                matched.append((trks[i], dets[assignment[i]]))
        new_trks = [t for i, t in enumerate(trks) if assignment[i] == -1]
        assigned_cols = set(int(a) for a in assignment)       # COLUMN INDICES, subtracted from the detection ids (tracker_manager.cpp:62-68)
        new_dets = [d for d in dets if d not in assigned_cols]
        trks[:] = new_trks
        dets[:] = new_dets

    def update(self, rects, feats):
        """one frame -> track id per detection (int array).  A frame with no detections does not reach the tracker (dynamic_tracker.cpp:795-796)."""
        dt = self.dt
        rects = np.asarray(rects, dt).reshape(-1, 4)
        feats = np.asarray(feats, dt).reshape(len(rects), self.feat_dim)
        n = len(rects)
        info = {"n": n, "events": set(), "problems": [], "gates": [], "stages": []}
        self.log.append(info)
        if n == 0:
            return np.zeros(0, np.int64)
        saved = self.tracks
        self.tracks = copy.deepcopy(self.tracks)
        data = self.tracks
        # predict
        for t in data:
            t.tsu += 1
            t.x = self.A @ t.x
            t.P = self.A @ t.P @ self.A.T + self.Q
        # remove_nan
        keep = [t for t in data if not np.isnan(self.rect(t)).any()]
        if len(keep) != len(data):
            info["events"].add("nan_removed")
        data[:] = keep
        trects = [self.rect(t) for t in data]
        iou = np.array([[self.iou_dist(tr, dr) for dr in rects] for tr in trects], dt).reshape(len(data), n)
        info["iou"], info["trects"] = iou.copy(), np.array(trects, dt).reshape(len(data), 4)
        # stage 1
        trks = [i for i, t in enumerate(data) if t.state == CONFIRMED]
        dets = list(range(n))
        matched = []
        cost = np.zeros((len(trks), n), dt)
        for k, i in enumerate(trks):
            t = data[i]
            g = t.store if t.full else t.store[: t.next]
            with np.errstate(all="ignore"):
                feat = (dt(1) - g @ feats.T).min(axis=0)
            info["gates"] += [abs(float(v) - 0.2) for v in feat] + [abs(float(v) - 0.8) for v in iou[i]]
            gated = self.gt("iou1", iou[i], np.float32(0.8)) | self.gt("feat", feat, np.float32(0.2)) | np.isnan(iou[i]) | np.isnan(feat)      # NaN: the declared rule
            cost[k] = np.where(gated, dt(INVALID_DIST), feat)
            info.setdefault("feat", {})[i] = feat.copy()
        info["stages"].append(dict(rows=list(trks), cols=list(dets), cost=cost.copy()))
        self._associate(cost, trks, dets, matched, info)
        n1 = len(matched)
        for (ti, dj) in matched:
            if data[ti].tsu > 1:
                info["events"].add("rematch_by_appearance_after_gap")
        # stage 2
        trks += [i for i, t in enumerate(data) if t.state == TENTATIVE]
        cost = np.zeros((len(trks), len(dets)), dt)
        for k, i in enumerate(trks):
            for c, j in enumerate(dets):
                info["gates"].append(abs(float(iou[i, j]) - 0.7))
                cost[k, c] = dt(INVALID_DIST) if self.gt("iou2", iou[i, j], np.float32(0.7)) or np.isnan(iou[i, j]) else iou[i, j]
        info["stages"].append(dict(rows=list(trks), cols=list(dets), cost=cost.copy()))
        self._associate(cost, trks, dets, matched, info)
        info["born"] = list(dets)
        for (ti, dj) in matched[n1:]:
            if data[ti].state == CONFIRMED:
                info["events"].add("stage2_confirmed")
        # miss
        for i in trks:
            t = data[i]
            if t.state == TENTATIVE:
                t.state = DELETED
                info["events"].add("tentative_death")
            elif self.gt("max_age", t.tsu, self.max_age):
                t.state = DELETED
                info["events"].add("death_by_age")
        # update
        next_id = self.next_id
        for (ti, dj) in matched:
            t = data[ti]
            if t.tsu > 1 and t.state == CONFIRMED:
                info["events"].add("survived_gap")
            t.tsu = 0
            t.hits += 1
            if t.state == TENTATIVE and self.gt("n_init", t.hits, self.n_init):
                t.state, t.id = CONFIRMED, next_id
                next_id += 1
                info["events"].add("confirmation")
            z = self.measure(rects[dj])
            S = self.H @ t.P @ self.H.T + self.Rm
            HP = self.H @ t.P
            K = np.linalg.solve(S, HP).T.astype(dt)
            t.x = t.x + K @ (z - self.H @ t.x)
            t.P = t.P - K @ HP
        # birth
        for dj in dets:
            matched.append((len(data), dj))
            t = Track(dt)
            t.x[:4] = self.measure(rects[dj])
            t.store = np.full((self.budget, self.feat_dim), np.nan, dt)
            data.append(t)
            info["events"].add("birth")
        # gallery
        for (ti, dj) in matched:
            t = data[ti]
            if t.next == self.budget:
                t.full, t.next = True, 0
                info["events"].add("ring_wrap")
            t.store[t.next] = feats[dj]
            t.next += 1
        # answer (visible_tracks_info): a Confirmed track updated in this frame hands its id to its detection
        ids = np.full(n, -1, np.int64)
        for (ti, dj) in matched:
            t = data[ti]
            if t.state == CONFIRMED and t.tsu == 0:
                ids[dj] = t.id
        # remove_deleted
        data[:] = [t for t in data if t.state != DELETED]
        if len(data) > self.max_tracks:      # the library's rule, not the reference's: the frame is refused and the tracker is as it was
            self.tracks = saved
            info["events"] = {"capacity"}
            raise OverflowError(f"{len(data)} tracks, more than max_tracks {self.max_tracks}")
        self.next_id = next_id
        info["matched"] = list(matched)
        return ids

    def table(self):
        """what dv_mot_get_tracks reports, in table order"""
        return [dict(x=t.x.copy(), p_diag=np.diag(t.P).copy(), rect=self.rect(t), state=t.state, id=t.id, hits=t.hits, time_since_update=t.tsu, n_feats=t.n_feats())
                for t in self.tracks]
