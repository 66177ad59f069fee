"""tests/mot_ref.py against independent yardsticks (CPU): its Munkres against brute force and scipy, and the tracker's life cycle against hand-derived outcomes."""
import itertools

import numpy as np
import pytest

from tests import mot_ref


def total(cost, asg):
    return sum(cost[i, c] for i, c in enumerate(asg) if c >= 0)


def brute(cost):
    R, C = cost.shape
    if R <= C:
        return min(sum(cost[i, p[i]] for i in range(R)) for p in itertools.permutations(range(C), R))
    return min(sum(cost[p[j], j] for j in range(C)) for p in itertools.permutations(range(R), C))


def test_munkres_against_brute_force():
    rng = np.random.default_rng(0)
    for R in range(1, 6):
        for C in range(1, 6):
            for _ in range(6):
                cost = rng.integers(0, 5, (R, C)).astype(np.float64)
                asg = mot_ref.munkres(cost)
                used = [c for c in asg if c >= 0]
                assert len(used) == min(R, C) == len(set(used))
                assert total(cost, asg) == brute(cost), (R, C, cost)


def test_munkres_against_scipy():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(1)
    for R, C in [(3, 7), (7, 3), (20, 20), (33, 64), (65, 64), (128, 64), (64, 64), (128, 1), (1, 64)]:
        cost = rng.random((R, C))
        asg = mot_ref.munkres(cost)
        r, c = linear_sum_assignment(cost)
        assert abs(total(cost, asg) - cost[r, c].sum()) < 1e-9 and (asg >= 0).sum() == min(R, C)


def test_munkres_edges():
    assert list(mot_ref.munkres(np.zeros((4, 0)))) == [-1] * 4
    assert len(mot_ref.munkres(np.zeros((0, 3)))) == 0
    asg = mot_ref.munkres(np.full((5, 3), 1000.0))
    assert sorted(c for c in asg if c >= 0) == [0, 1, 2]
    assert list(mot_ref.munkres(np.full((3, 5), 1000.0))) == [0, 1, 2]      # rows <= cols: by row, the first column not covered


def one(m, boxes, feats):
    return m.update(np.asarray(boxes, np.float32), np.asarray(feats, np.float32))


BOX, F = [[10, 10, 40, 60]], np.eye(4)[:1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_confirmed_on_the_fourth_update(dtype):
    m = mot_ref.MotRef(n_init=3, max_age=5, budget=100, feat_dim=4, dtype=dtype)
    got = [int(one(m, BOX, F)[0]) for _ in range(6)]      # the birth, then updates 1 .. 5
    assert got == [-1, -1, -1, -1, 1, 1]
    assert m.table()[0]["hits"] == 5 and m.table()[0]["state"] == mot_ref.CONFIRMED


def test_tentative_dies_on_its_first_miss():
    m = mot_ref.MotRef(n_init=3, max_age=5, budget=100, feat_dim=4)
    one(m, BOX, F)
    one(m, [[500, 300, 40, 60]], F)
    assert len(m.tracks) == 1 and m.tracks[0].hits == 0      # the first left, the far box was born


def test_confirmed_survives_max_age_misses_and_empty_frames_age_nothing():
    m = mot_ref.MotRef(n_init=1, max_age=2, budget=100, feat_dim=4)
    for _ in range(3):
        one(m, BOX, F)
    assert m.tracks[0].state == mot_ref.CONFIRMED
    far, g = [[500, 300, 40, 60]], np.eye(4)[1:2]
    for k in range(2):                                        # max_age frames without a match: it stays
        one(m, far, g)
        one(m, np.zeros((0, 4)), np.zeros((0, 4)))            # no detections: the tracker is not called
        assert m.tracks[0].id == 1 and m.tracks[0].tsu == k + 1
    one(m, far, g)
    assert all(t.id != 1 for t in m.tracks)


def test_ring_overwrites_from_row_zero():
    m = mot_ref.MotRef(n_init=1, max_age=2, budget=3, feat_dim=4)
    fs = [np.eye(4)[0] * (1 - 0.01 * k) + np.eye(4)[1] * 0.01 * k for k in range(5)]
    fs = [f / np.linalg.norm(f) for f in fs]
    for k in range(5):
        one(m, BOX, [fs[k]])
    t = m.tracks[0]
    assert t.full and t.next == 2 and t.n_feats() == 3
    assert np.allclose(t.store[0], fs[3]) and np.allclose(t.store[1], fs[4]) and np.allclose(t.store[2], fs[2])
