"""Group front end (dv_batch_track_enqueue) on degenerate and unequal members (cases and premises: tests/front_group_hostile.py).

CPU (`-m "not gpu"`): every case is shown, on the oracle alone, to hold what it is named for — a full member beside a detecting one, a member without a row beside
members whose candidates would overflow, a tile over DISC_CAP beside sparse tiles, masks that leave nothing or one pixel, the two device limits, one tile column —
and the figures are printed.
GPU: every member's rows out of the shared round against (1) a twin context driven through track_stereo alone and (2) the oracle's tracker in the member's mode, on
every frame, at the bar of test_front_hostile._rows_equal (ids, counts and flags exactly, observations as uint64 views); dv_batch_track_info must count every job as
batched and none as single, so a case that falls back to the members' own launches fails.  Where a premise says a member has rows, the device's count is asserted too."""
import numpy as np
import pytest

from tests import front_group_hostile as gh
from tests import front_hostile as fh
from tests.test_front_hostile import _cam, _oracle_tracker, _rows_equal

BUILDERS = {
    "unequal": lambda o: gh.unequal_case(), "unequal_reversed": lambda o: gh.unequal_case(reverse=True),
    "empty": lambda o: gh.empty_case(), "crowded": lambda o: gh.crowded_case(),
    "classes_zero_and_eroded": lambda o: gh.classes_case(o, "zero_and_eroded"), "classes_single_pixel": lambda o: gh.classes_case(o, "single_pixel"),
    "small_65x17": lambda o: gh.small_case(65, 17), "small_17x65": lambda o: gh.small_case(17, 65),
}
_REF = {}
FLAG_TEXT = r"front end device error flags=%d \(1:"      # dv_track_stereo_collect's text: the flags' value, then the legend


def _case(oracle, name):
    """the case and the oracle's rows of every member and round: computed once, shared by the premise and the device test, never changed"""
    if name not in _REF:
        case = BUILDERS[name](oracle)
        _REF[name] = (case, gh.oracle_rows(oracle, case))
    return _REF[name]


# =============================================================== premises (oracle only)
def test_unequal_members_premise(oracle):
    case, ref = _case(oracle, "unequal")
    gh.unequal_premises(case, ref)
    rev, rref = _case(oracle, "unequal_reversed")
    assert [r[::-1] for r in rev.rounds] == case.rounds and all(np.array_equal(ref[k], rref[k]) for k in ref)


def test_empty_beside_full_premise(oracle):
    case, ref = _case(oracle, "empty")
    gh.empty_premises(oracle, case, ref)
    assert case.mems == ["host", "pinned", "device"]


def test_crowded_beside_sparse_premise(oracle):
    case, ref = _case(oracle, "crowded")
    gh.crowded_premises(case, ref)
    o = _oracle_tracker(oracle, fh.CROWD_MAX_CNT, fh.CROWD_MIN_DIST)          # the member's reference is the tracker test_crowded_disc_condition runs
    for k, (l, r) in enumerate(fh.crowded_sequence()):
        assert np.array_equal(o.track_image(l, r, gh.DT * k), ref[(0, k)])


@pytest.mark.parametrize("which", sorted(gh.CLASS_LAYOUTS))
def test_three_classes_premise(oracle, which):
    case, ref = _case(oracle, f"classes_{which}")
    gh.classes_premises(oracle, case, ref, which)


def test_limits_premise(oracle):
    gh.limit_premises(oracle, gh.limit_members())


@pytest.mark.parametrize("w,h", [(65, 17), (17, 65)])
def test_small_geometries_premise(oracle, w, h):
    case, ref = _case(oracle, f"small_{w}x{h}")
    gh.small_premises(case, ref)


# =============================================================== the shared rounds against the twins and the oracle
def _contexts(factory, m):
    cam = _cam(fh.cam_for(m.w, m.h))
    kw = dict(width=m.w, height=m.h, max_cnt=m.max_cnt, min_dist=m.min_dist, cam0=cam, cam1=cam, mask_morphology_size=m.morph)
    return factory(**kw), factory(**kw)


def _place(arrays, mem):
    """the arrays as a job names them -> (values, memory kind, what must stay alive until the round is collected)"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED
    if mem == "host":
        return list(arrays), DV_MEM_HOST, []
    held = [None if a is None else (torch.from_numpy(a.copy()).cuda() if mem == "device" else torch.from_numpy(a.copy()).pin_memory()) for a in arrays]
    return [None if t is None else t.data_ptr() for t in held], (DV_MEM_DEVICE if mem == "device" else DV_MEM_PINNED), held


def _job(i, m, k, t, mem="host"):
    (l, r), mask = m.frames[k], m.mask(k)
    vals, code, held = _place([l, r, mask], mem)
    return dict(member=i, gray0=vals[0], gray1=vals[1], mask=vals[2], t=t, mode=m.mode, mem=code), held


def _equal(got, want, what):
    try:
        _rows_equal(got, want)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None


def _close(batch, pairs):
    """the group first, then its members and their twins: the session's factory would keep them all until its end"""
    batch.close()
    for pair in pairs:
        for c in pair:
            c.close()


def _drive(factory, case, ref):
    """every round of the case through one group: each member's rows against its twin's own track_stereo and against the oracle, dv_batch_track_info exactly.
    -> {(member, round): the group's rows}"""
    import torch
    from dynamic_vins_amd.backend import Batch
    pairs = [_contexts(factory, m) for m in case.members]
    batch = Batch([b for b, _ in pairs])
    got = {}
    try:
        for r, order in enumerate(case.rounds):
            t = gh.DT * r
            jobs, keep, want = [], [], {}
            for i in order:
                m, k = case.members[i], case.frame_of(i, r)
                want[i] = pairs[i][1].track_stereo(m.frames[k][0], m.frames[k][1], t, m.mask(k), m.mode)
                job, held = _job(i, m, k, t, case.mems[r])
                jobs.append(job); keep.append(held)
            torch.cuda.synchronize()
            batch.track_enqueue(jobs)
            for i in order:
                g = pairs[i][0].track_stereo_collect()
                _equal(g, want[i], f"{case.name}, round {r}, member {case.members[i].name}, group vs twin")
                _equal(g, ref[(i, r)], f"{case.name}, round {r}, member {case.members[i].name}, group vs oracle")
                got[(i, r)] = g
            del keep
        info = batch.track_info()
    finally:
        _close(batch, pairs)
    assert info == dict(rounds=len(case.rounds), members_batched=case.batched(), members_single=0), info
    assert sorted(got) == sorted(ref)                                            # every member on every frame it has
    return got


@pytest.mark.gpu
def test_unequal_members_share_a_round(gpu_ctx_factory, oracle):
    """six raw members with (max_cnt, min_dist) from (1, 5) to (1024, 2): grids sized by the largest member, each member bounded by its own limits — full members that
    ask the detector for nothing beside members that add corners.  A second group is handed the same rounds with the job order reversed: the same bytes"""
    case, ref = _case(oracle, "unequal")
    fig = gh.unequal_premises(case, ref)
    got = _drive(gpu_ctx_factory, case, ref)
    assert [len(got[(fig["big"], r)]) for r in range(4)] == fig["big_rows"] and min(fig["big_rows"]) > 150
    rev, rref = _case(oracle, "unequal_reversed")
    got_rev = _drive(gpu_ctx_factory, rev, rref)
    for key in got:
        assert got[key].tobytes() == got_rev[key].tobytes(), key


@pytest.mark.gpu
def test_empty_member_beside_full_ones(gpu_ctx_factory, oracle):
    """a member without a candidate or a row first, in the middle and last in the tables, beside two members whose frames overflow a candidate buffer that takes zero
    responses and an ordinary one; the rounds take pageable host, pinned and device frames in turn"""
    case, ref = _case(oracle, "empty")
    rows = gh.empty_premises(oracle, case, ref)
    got = _drive(gpu_ctx_factory, case, ref)
    for i, m in enumerate(case.members):
        assert [len(got[(i, r)]) for r in range(3)] == rows[m.name]
        assert all(len(got[(i, r)]) >= 20 for r in range(3)) or m.name == "flat_whole"


@pytest.mark.gpu
def test_crowded_member_beside_sparse_ones(gpu_ctx_factory, oracle):
    """the contracting sequence at max_cnt 1024 / min_dist 2 (tiles over DISC_CAP fall back to testing every disc, 1024 points with equal sort keys) beside two members
    of max_cnt 30 / min_dist 15 whose tiles take the culled list; member 2 sits round 3 out — S = 2, the smallest group that shares — and returns"""
    case, ref = _case(oracle, "crowded")
    fig = gh.crowded_premises(case, ref)
    got = _drive(gpu_ctx_factory, case, ref)
    assert len(got[(0, 5)]) == fh.CROWD_MAX_CNT and all(int((got[(0, r)]["track_cnt"] == 1).sum()) >= 1 for r in fig["over"])
    assert all(len(got[(i, r)]) >= 20 for i in (1, 2) for r in case.met(i))


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(gh.CLASS_LAYOUTS))
def test_three_classes_on_degenerate_masks(gpu_ctx_factory, oracle, which):
    """2 raw, 2 semantic and 2 naive members on 0 / 255 images, the tiled texture and a partly flat frame, three frames; the masks: all 255, all 0, one pixel of 255
    (at the strongest corner), and stripes the member's own mask_morphology_size erodes to nothing"""
    case, ref = _case(oracle, f"classes_{which}")
    fig = gh.classes_premises(oracle, case, ref, which)
    got = _drive(gpu_ctx_factory, case, ref)
    for i, m in enumerate(case.members):
        if m.name in fig["keeps"]:
            assert min(len(got[(i, r)]) for r in range(3)) >= 10, m.name


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(65, 17), (17, 65)])
def test_small_geometries_share_a_round(gpu_ctx_factory, oracle, w, h):
    """three raw members at 65 x 17 and at 17 x 65 (the single entry accepts both sizes as they are): one tile column, 1 px ragged edges, every pyramid level above 0
    smaller than the 21 px window; two frames"""
    case, ref = _case(oracle, f"small_{w}x{h}")
    gh.small_premises(case, ref)
    got = _drive(gpu_ctx_factory, case, ref)
    assert all(len(got[(i, 1)]) >= 3 for i in range(3))


def _collect_flagged(ctx, flag):
    from dynamic_vins_amd import DvinsError
    with pytest.raises(DvinsError, match=FLAG_TEXT % flag):
        ctx.track_stereo_collect()


@pytest.mark.gpu
def test_limits_inside_a_round(gpu_ctx_factory, oracle):
    """320 x 240, members A (min_dist 3), B (min_dist 1), C, D (min_dist 15) in four shared rounds.  Round 1: A meets the 4 px checkerboard — its collect raises with
    flags=4 — and B's grid is refused with flags=2, while C and D collect the oracle's rows.  Rounds 2, 3: A gets benign frames, must not raise (a stale flag) and gives
    the rows of its twin, which met the same frames through its own entry; B keeps raising flags=2 every round (a wiped flag would pass silently).  Round 4 follows
    reset() of A alone: A's rows are the oracle's first frame.  The flags are the members' own: C and D never raise"""
    from dynamic_vins_amd import DvinsError
    from dynamic_vins_amd.backend import Batch
    members = gh.limit_members()
    gh.limit_premises(oracle, members)
    pairs = [_contexts(gpu_ctx_factory, m) for m in members]
    orc = {i: gh.oracle_tracker(oracle, members[i]) for i in (2, 3)}
    batch = Batch([b for b, _ in pairs])
    try:
        for r in range(4):
            t = gh.DT * r
            if r == 3:
                for c in pairs[0]:
                    c.reset()
            want = {}
            for i, m in enumerate(members):
                try:
                    want[i] = pairs[i][1].track_stereo(m.frames[r][0], m.frames[r][1], t)
                except DvinsError as e:
                    want[i] = str(e)
            assert isinstance(want[0], str) == (r == 0) and isinstance(want[1], str), (r, want[0] if r else None)     # the single tracker's own flag path
            batch.track_enqueue([_job(i, m, r, t)[0] for i, m in enumerate(members)])
            if r == 0:
                _collect_flagged(pairs[0][0], 4)
                assert str(want[0]).startswith("front end device error flags=4 (")
            else:
                g = pairs[0][0].track_stereo_collect()                           # must not raise
                _equal(g, want[0], f"round {r}, A, group vs twin")
                assert len(g) >= 100
                if r == 3:
                    _equal(g, gh.oracle_frame(gh.oracle_tracker(oracle, members[0]), members[0], 3, t), "round 3, A after reset, group vs oracle")
            _collect_flagged(pairs[1][0], 2)
            assert want[1].startswith("front end device error flags=2 (")
            for i in (2, 3):
                g, ref = pairs[i][0].track_stereo_collect(), gh.oracle_frame(orc[i], members[i], r, t)
                _equal(g, want[i], f"round {r}, {members[i].name}, group vs twin")
                _equal(g, ref, f"round {r}, {members[i].name}, group vs oracle")
                assert len(g) >= 100
        info = batch.track_info()
    finally:
        _close(batch, pairs)
    assert info == dict(rounds=4, members_batched=16, members_single=0), info


@pytest.mark.gpu
def test_single_tracker_flag_path(gpu_ctx_factory, oracle):
    """A's and B's frames through lone contexts: the frame on the checkerboard raises flags=4 and the benign frames behind it do not raise and refill the tracker; the
    refused grid raises flags=2 on every frame; after reset() both flags are gone for good and the rows are the oracle's"""
    from dynamic_vins_amd import DvinsError
    members = gh.limit_members()
    a, b = members[0], members[1]
    ca, cb = _contexts(gpu_ctx_factory, a)[0], _contexts(gpu_ctx_factory, b)[0]
    for k in range(3):
        t = gh.DT * k
        if k == 0:
            with pytest.raises(DvinsError, match=FLAG_TEXT % 4):
                ca.track_stereo(a.frames[k][0], a.frames[k][1], t)
        else:
            assert len(ca.track_stereo(a.frames[k][0], a.frames[k][1], t)) == a.max_cnt
        with pytest.raises(DvinsError, match=FLAG_TEXT % 2):
            cb.track_stereo(b.frames[k][0], b.frames[k][1], t)
    ca.reset()
    oa = gh.oracle_tracker(oracle, a)
    for k in (1, 2, 3):
        g = ca.track_stereo(a.frames[k][0], a.frames[k][1], gh.DT * k)
        _equal(g, gh.oracle_frame(oa, a, k, gh.DT * k), f"A after reset, frame {k}")
    assert len(g) >= 100
