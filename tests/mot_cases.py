"""Scenarios for the multi-object tracker's tests: boxes on straight paths with jitter, entries and exits, occlusion gaps, detections shuffled per frame, embeddings
normalise(prototype + small noise).  A scenario is a list of frames (rects [n, 4] float32 x y w h, feats [n, feat_dim] float32, object index per detection); an empty
frame has n = 0.  run_ref() runs tests/mot_ref.py over one and keeps ids, tables and the log per frame; conditions() asserts on the REFERENCE ALONE what makes a
scenario a fair test of a float32 device (tests/test_mot.py): if a seed fails one, take another seed, never loosen the condition."""
import numpy as np

from tests import mot_ref


def normalise(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make(seed, n_frames, n_obj, feat_dim, noise=0.02, gaps=(), switches=(), lifetimes=None, one_hot=False, spacing=(150.0, 120.0), cols=8, empty=()):
    """gaps: (object, first frame, length) without a detection; switches: (object, frame) from which the object's prototype is another one (the appearance gate fails,
    the box goes on); lifetimes: per object (first, last) frame; empty: frames without any detection"""
    rng = np.random.default_rng(seed)
    proto = normalise(np.eye(feat_dim)[np.arange(n_obj) % feat_dim] + (0.0 if one_hot else 1.0) * rng.standard_normal((n_obj, feat_dim)))
    proto2 = normalise(rng.standard_normal((n_obj, feat_dim)) if not one_hot else np.eye(feat_dim)[(np.arange(n_obj) + feat_dim // 2) % feat_dim])
    pos = np.stack([(np.arange(n_obj) % cols) * spacing[0] + 20, (np.arange(n_obj) // cols) * spacing[1] + 20], 1) + rng.uniform(0, 10, (n_obj, 2))
    vel = rng.uniform(-3, 3, (n_obj, 2))
    size = rng.uniform(40, 90, (n_obj, 2))
    if lifetimes is None:
        lifetimes = [(0, n_frames - 1)] * n_obj
    frames = []
    for k in range(n_frames):
        rects, feats, who = [], [], []
        for o in range(n_obj):
            if k in empty or not (lifetimes[o][0] <= k <= lifetimes[o][1]) or any(g[0] == o and g[1] <= k < g[1] + g[2] for g in gaps):
                continue
            p = pos[o] + vel[o] * k + rng.uniform(-0.5, 0.5, 2)
            s = size[o] + rng.uniform(-0.5, 0.5, 2)
            pr = proto2[o] if any(sw[0] == o and k >= sw[1] for sw in switches) else proto[o]
            rects.append([p[0], p[1], s[0], s[1]])
            feats.append(normalise(pr + noise * rng.standard_normal(feat_dim) / np.sqrt(feat_dim) * 4))
            who.append(o)
        order = rng.permutation(len(rects))
        frames.append((np.array(rects, np.float32).reshape(-1, 4)[order], np.array(feats, np.float32).reshape(-1, feat_dim)[order], np.array(who, np.int64)[order]))
    return frames


def run_ref(frames, par, dtype):
    m = mot_ref.MotRef(dtype=dtype, **par)
    out = []
    for rects, feats, _ in frames:
        ids = m.update(rects, feats)
        out.append(dict(ids=ids, table=m.table(), info=m.log[-1]))
    return out


def discrete(table):
    return [(t["state"], t["id"], t["hits"], t["time_since_update"], t["n_feats"]) for t in table]


def conditions(frames, par, need=()):
    """-> (float64 run, delta per quantity): the float32 and float64 references agree on every discrete outcome, every cost is >= 1e-3 from its gate, every Munkres
    problem returns the same assignment under three random +-1e-4 perturbations of its finite costs, and the events in `need` occur"""
    r64, r32 = run_ref(frames, par, np.float64), run_ref(frames, par, np.float32)
    rng = np.random.default_rng(7)
    delta = dict(x=0.0, p_diag=0.0, rect=0.0)
    seen = set()
    for k, (a, b) in enumerate(zip(r64, r32)):
        assert np.array_equal(a["ids"], b["ids"]) and discrete(a["table"]) == discrete(b["table"]), f"frame {k}: float32 and float64 references disagree"
        assert a["info"].get("matched") == b["info"].get("matched"), f"frame {k}: matched pairs differ"
        for ta, tb in zip(a["table"], b["table"]):
            for q in delta:
                delta[q] = max(delta[q], float(np.abs(ta[q] - tb[q].astype(np.float64)).max()))
        gates = a["info"]["gates"]
        assert not gates or min(gates) >= 1e-3, f"frame {k}: a cost {min(gates):.2e} from its gate"
        for prob in a["info"]["problems"]:
            if prob.size == 0:
                continue
            base = mot_ref.munkres(prob)
            finite = prob < mot_ref.INVALID_DIST
            for _ in range(3):
                pert = np.where(finite, np.maximum(prob + rng.uniform(-1e-4, 1e-4, prob.shape), 0.0), prob)
                got = mot_ref.munkres(pert)
                # (pairs over 100 are dropped by the caller: only the kept pairs are an outcome)
                keep = lambda asg, m: [(i, c) for i, c in enumerate(asg) if c >= 0 and m[i, c] <= mot_ref.INVALID_DIST / 10]
                assert keep(got, pert) == keep(base, prob), f"frame {k}: the assignment depends on 1e-4 of its costs"
        seen |= a["info"]["events"]
    missing = set(need) - seen
    assert not missing, f"the scenario never shows {sorted(missing)}"
    return r64, delta


YAML = dict(n_init=3, max_age=5, budget=100, feat_dim=512, max_tracks=128)
SMALL = dict(n_init=1, max_age=2, budget=3, feat_dim=12, max_tracks=128)
WIDE = dict(n_init=1, max_age=6, budget=4, feat_dim=32, max_tracks=128)
YAML_NEED = ("birth", "confirmation", "tentative_death", "death_by_age", "survived_gap", "rematch_by_appearance_after_gap", "stage2_confirmed", "ring_wrap")


def yaml_scenario():
    """the reference's YAML: 12 objects over the first 30 frames; objects 0 and 1 alone live on to frame 129, because a ring of 100 rows wraps only at a track's 101st
    embedding and the conditions ask this parameter set for a ring wrap"""
    life = [(0, 129)] * 2 + [(0, 29)] * 6 + [(6, 29), (9, 11), (0, 14), (3, 29)]
    gaps = [(2, 12, 3), (3, 10, 8), (4, 14, 5), (5, 20, 1)]      # <= max_age, > max_age (dies, comes back as a new track), = max_age, a single frame
    return make(seed=11, n_frames=130, n_obj=12, feat_dim=512, gaps=gaps, switches=[(6, 16)], lifetimes=life)


def small_scenario(empty=()):
    life = [(0, 23), (0, 23), (2, 9), (4, 23), (0, 6), (8, 9), (10, 23), (3, 18)]
    gaps = [(0, 6, 2), (1, 8, 4), (3, 12, 1)]
    return make(seed=5, n_frames=24, n_obj=8, feat_dim=12, gaps=gaps, switches=[(7, 10)], lifetimes=life, one_hot=True, empty=empty)


def wide_scenario():
    """100 objects of which 64 are detected per frame, in turn: more than 64 tracks (rows > cols) against 64 detections"""
    n_obj, n_frames = 100, 8
    frames = make(seed=3, n_frames=n_frames, n_obj=n_obj, feat_dim=32, cols=10, noise=0.01)
    out = []
    for k, (r, f, w) in enumerate(frames):
        shown = (w + 36 * (k % 3)) % n_obj < 64 if k >= 2 else w < 64
        out.append((r[shown], f[shown], w[shown]))
    return out


def collapse_scenario():
    """remove_nan: object 1's box shrinks so fast that the area velocity carries the predicted area below zero while boxes 0 and 2 stand still"""
    frames = []
    sizes = [(120.0, 90.0), (80.0, 60.0), (40.0, 30.0), (10.0, 8.0), (2.0, 1.5), (1.0, 0.5), (0.5, 0.25), (0.3, 0.2), (0.2, 0.1), (0.1, 0.1)]
    f = np.eye(8, dtype=np.float32)[:3]
    for k, (w, h) in enumerate(sizes):
        frames.append((np.array([[20, 20, 50, 60], [300 - w / 2, 200 - h / 2, w, h], [500, 300, 70, 40]], np.float32), f, np.arange(3)))
    return frames, dict(n_init=1, max_age=3, budget=4, feat_dim=8, max_tracks=16)
