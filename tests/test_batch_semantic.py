"""dv_batch_track_enqueue with DV_MODE_SEMANTIC members — the background tracking of DYNAMIC sequences, on contexts that own an object tracker (`-m gpu`):
TrackSemanticImage of several sequences in the group's shared launches (TrackLeft with the raw slice, TrackRightGPU with the naive slice, the staged
dv_track_unmask_static rectangles of the whole round in one launch), the members' dv_inst_track_enqueue on their own streams behind the group's events.
The yardstick is the twin context of tests/test_batch_naive.py: the member's own dv_track_stereo_enqueue, dv_inst_track_enqueue and the two collects on the same
inputs.  Background rows, the object tracker's instances, feature rows and points are compared as bytes every frame, dv_batch_track_info is asserted exactly.
Every member has two moving detection boxes inside a mask that moves from frame to frame."""
import numpy as np
import pytest

from tests.test_batch_naive import Member, band_mask

pytestmark = pytest.mark.gpu

RAW, NAIVE, SEM = 0, 1, 2      # DV_MODE_RAW, DV_MODE_NAIVE, DV_MODE_SEMANTIC


def dets_of(w, h, f, seed, big=False):
    """the two detections of frame f: boxes of 56 x 44 (big: 96 x 80) and 40 x 60 pixels that move 6 px right and 3 px down per frame, each with a ROI mask that
    leaves a 3 px rim free; the track ids are the member's own"""
    out = []
    for n, (bw, bh) in enumerate((((96, 80) if big else (56, 44)), (40, 60))):
        x, y = (23 * seed + 40 + 110 * n + 6 * f) % (w - bw), (h // 5 + 70 * n + 3 * f + 5 * seed) % (h - bh)
        roi = np.zeros((bh, bw), np.uint8)
        roi[3:-3, 3:-3] = 1
        out.append(dict(track_id=10 * seed + n + 1, class_id=0, rect=(x, y, bw, bh), mask=roi, points=None))
    return out


def inv_mask(w, h, f, seed, border=False, big=False):
    """the inverse merged instance mask of frame f (0 = object): band_mask's moving object plus the pixels of the two detections"""
    m = band_mask(w, h, f, seed, border)
    for d in dets_of(w, h, f, seed, big):
        x, y, bw, bh = d["rect"]
        m[y: y + bh, x: x + bw][d["mask"] > 0] = 0
    return m


class SemMember(Member):
    """Member of tests/test_batch_naive.py for the three modes: a mask in every mode but RAW, and (inst) an object tracker on both contexts.  static(f) -> the track ids
    dv_track_unmask_static is given before frame f on both contexts (None: not called).  big: the first detection is 96 x 80 pixels — with min_dist 30 the image
    holds fewer corners than max_cnt, every frame detects new ones, and the pixels of that box, once unmasked, have room for some"""

    def __init__(self, factory, w, h, seed, mode=SEM, inst=True, static=None, big=False, **kw):
        super().__init__(factory, w, h, seed, mode=mode, mask_of=lambda f: inv_mask(w, h, f, seed, kw.get("border", False), big), **kw)
        self.inst, self.static, self.big = inst, static or (lambda f: None), big
        if inst:
            for c in (self.batched, self.twin):
                c.inst_config(50, 5, 0)

    def inputs(self, f):
        l, r, _, mode = super().inputs(f)
        mask = None
        if mode != RAW:
            mask = self.mask_of(f)
            if self.kind != "bgr" and self.host_stride:
                from tests.test_batch_naive import _padded
                mask = _padded(mask, self.host_stride)
        return l, r, mask, mode

    def dets(self, f):
        return dets_of(self.w, self.h, f, self.seed, self.big)

    def twin_frame(self, f, t, ctx=None, static=None):
        """the member's own launches: -> (rows, insts, object rows, points) of frame f on the twin (or ctx)"""
        c = ctx or self.twin
        l, r, mask, mode = self.inputs(f)
        ids = self.static(f) if static is None else static
        if ids is not None:
            c.track_unmask_static(self.dets(f), ids)
        c.track_stereo_enqueue(l, r, t, mask, mode, mem=self.mem_twin, stride=l.strides[0])
        if self.inst:
            c.inst_track_enqueue(t, self.dets(f))
        rows = c.track_stereo_collect()
        return (rows,) + (c.inst_track_collect() if self.inst else ())

    def stage(self, f):
        """what precedes the batched context's job of frame f"""
        ids = self.static(f)
        if ids is not None:
            self.batched.track_unmask_static(self.dets(f), ids)

    def batched_frame(self, f, t, collect_rows=True):
        """behind the group's enqueue: the object tracker of the batched context, then the collects"""
        if self.inst:
            self.batched.inst_track_enqueue(t, self.dets(f))
        rows = (self.batched.track_stereo_collect(),) if collect_rows else ()
        return rows + (self.batched.inst_track_collect() if self.inst else ())


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w_) in enumerate(zip(got, want)):
        name = ("background rows", "instances", "object rows", "object points")[k]
        assert len(g) == len(w_), f"{what}: {len(g)} vs {len(w_)} {name}"
        assert g.tobytes() == w_.tobytes(), f"{what}: {name} differ"


def run_round(batch, members, f, present=None, min_rows=20):
    """the twins track frame f with their own launches, the batch enqueues the same jobs, everything is compared.  -> {member: the twin's outputs}"""
    import torch
    t = 0.05 * f
    want, jobs = {}, []
    for i, m in enumerate(members):
        if present is not None and i not in present:
            continue
        want[i] = m.twin_frame(f, t)
        m.stage(f)
        jobs.append(m.job(i, f, t))
    torch.cuda.synchronize()
    batch.track_enqueue(jobs)
    for i in want:
        got = members[i].batched_frame(f, t)
        assert len(got[0]) > min_rows, f"frame {f}, member {i}: {len(got[0])} rows"
        same(got, want[i], f"frame {f}, member {i}")
    return want


def delta(batch, before):
    info = batch.track_info()
    return (info["members_single"] - before["members_single"], info["members_batched"] - before["members_batched"], info["rounds"] - before["rounds"]), info


def unmask_bites(factory, member, frames, ids_of):
    """on twins alone: the frames in which dv_track_unmask_static with ids_of(f) changes the member's background rows"""
    a, b = factory(**member.kw), factory(**member.kw)
    for c in (a, b):
        c.inst_config(50, 5, 0)
    out = []
    for f in range(frames):
        ra = member.twin_frame(f, 0.05 * f, ctx=a, static=ids_of(f) or [])
        rb = member.twin_frame(f, 0.05 * f, ctx=b, static=[])
        if ra[0].tobytes() != rb[0].tobytes():
            out.append(f)
    return out


@pytest.mark.parametrize("w,h", [(320, 240), (330, 250)])
def test_dynamic_members_share_the_round_with_raw_members(gpu_ctx_factory, w, h):
    """three semantic members with object trackers and two raw members, 7 frames (330 x 250: the width is no multiple of 16 and the levels have odd sizes): every round
    batches five and runs none single, and the object trackers — on their own streams behind the group's events — give the twins' instances, rows and points"""
    from dynamic_vins_amd.backend import Batch
    frames = 7
    members = [SemMember(gpu_ctx_factory, w, h, 51), SemMember(gpu_ctx_factory, w, h, 52, mode=RAW, inst=False), SemMember(gpu_ctx_factory, w, h, 53, max_cnt=70),
               SemMember(gpu_ctx_factory, w, h, 54, mode=RAW, inst=False), SemMember(gpu_ctx_factory, w, h, 55)]
    assert not np.array_equal(members[0].mask_of(1), members[0].mask_of(2)) and not np.array_equal(members[0].mask_of(1), members[2].mask_of(1))
    batch = Batch([m.batched for m in members])
    obj_rows = 0
    for f in range(frames):
        before = batch.track_info()
        want = run_round(batch, members, f)
        d, _ = delta(batch, before)
        assert d == (0, 5, 1), (f, d)
        obj_rows += sum(len(want[i][2]) for i in (0, 2, 4))
    info = batch.track_info()
    batch.close()
    print(f"{w} x {h}: {obj_rows} object rows compared")
    assert obj_rows > 10 * frames, "the object trackers must have produced rows"
    assert info == dict(rounds=frames, members_batched=5 * frames, members_single=0), info


def test_static_instances_are_unmasked_by_the_round(gpu_ctx_factory):
    """320 x 240, 7 frames.  From frame 3 on member 0 is told that its first detection is static (the device mask is copied and unmasked by the round's launch); member 1
    is handed ids none of its detections carries (nothing is staged).  On twins alone the unmasking changes member 0's rows; the batched rows equal the twin's."""
    from dynamic_vins_amd.backend import Batch
    w, h, frames = 320, 240, 7
    first = lambda seed: dets_of(w, h, 0, seed)[0]["track_id"]
    members = [SemMember(gpu_ctx_factory, w, h, 61, big=True, min_dist=30, static=lambda f: [first(61)] if f >= 3 else None),
               SemMember(gpu_ctx_factory, w, h, 62, static=lambda f: [9001, 9002] if f >= 3 else None),
               SemMember(gpu_ctx_factory, w, h, 63, mode=RAW, inst=False)]
    bites = unmask_bites(gpu_ctx_factory, members[0], frames, lambda f: [first(61)] if f >= 3 else None)
    print("frames whose rows the unmasking changes:", bites)
    assert bites and min(bites) >= 3, bites
    batch = Batch([m.batched for m in members])
    for f in range(frames):
        run_round(batch, members, f)
    info = batch.track_info()
    batch.close()
    assert info == dict(rounds=frames, members_batched=3 * frames, members_single=0), info


def test_input_kinds_in_one_group(gpu_ctx_factory):
    """330 x 250, 6 frames, four semantic members with object trackers: mask_morphology_size 5 with an object at the image border | BGR frames with a one-channel mask |
    pageable host frames and mask in rows of 352 bytes, static instances unmasked from frame 2 on (in the member's own copy of the uploaded mask) | device frames"""
    from dynamic_vins_amd.backend import Batch
    w, h, frames = 330, 250, 6
    first = dets_of(w, h, 0, 73)[0]["track_id"]
    members = [SemMember(gpu_ctx_factory, w, h, 71, morph=5, border=True), SemMember(gpu_ctx_factory, w, h, 72, kind="bgr"),
               SemMember(gpu_ctx_factory, w, h, 73, host_stride=352, big=True, min_dist=30, static=lambda f: [first] if f >= 2 else None), SemMember(gpu_ctx_factory, w, h, 74)]
    batch = Batch([m.batched for m in members])
    for f in range(frames):
        run_round(batch, members, f)
    info = batch.track_info()
    batch.close()
    assert info == dict(rounds=frames, members_batched=4 * frames, members_single=0), info


def test_mixed_classes_and_the_sharing_rules(gpu_ctx_factory):
    """320 x 240, 7 rounds over members 0, 1 raw | 2, 3 naive | 4, 5 semantic with object trackers; who has a frame in a round decides who shares.
    (single, batched, rounds counted) per round: all six (0, 6, 1) twice | one naive and one semantic share (0, 2, 1) | a lone semantic job beside two raw ones keeps its
    own launches (1, 2, 1) | a semantic job alone (1, 0, 0) | beside one raw job: nothing is left to share (2, 0, 0) | all six again (0, 6, 1)"""
    from dynamic_vins_amd.backend import Batch
    w, h = 320, 240
    members = [SemMember(gpu_ctx_factory, w, h, 81, mode=RAW, inst=False), SemMember(gpu_ctx_factory, w, h, 82, mode=RAW, inst=False),
               SemMember(gpu_ctx_factory, w, h, 83, mode=NAIVE, inst=False), SemMember(gpu_ctx_factory, w, h, 84, mode=NAIVE, inst=False, morph=3),
               SemMember(gpu_ctx_factory, w, h, 85), SemMember(gpu_ctx_factory, w, h, 86)]
    plan = [(None, (0, 6, 1)), (None, (0, 6, 1)), ([2, 4], (0, 2, 1)), ([0, 1, 4], (1, 2, 1)), ([4], (1, 0, 0)), ([0, 4], (2, 0, 0)), (None, (0, 6, 1))]
    batch = Batch([m.batched for m in members])
    for f, (present, expect) in enumerate(plan):
        before = batch.track_info()
        run_round(batch, members, f, present=present)
        d, info = delta(batch, before)
        assert d == expect, (f, d, info)
    batch.close()


def test_a_member_changes_mode_from_frame_to_frame(gpu_ctx_factory):
    """320 x 240, 8 frames: member 0 raw, member 1 semantic with an object tracker, members 2 (no object tracker) and 3 (with one) go raw, raw, semantic, semantic,
    naive, naive, semantic, semantic.  A raw or naive job of a member that owns an object tracker keeps the member's own launches, on its own stream, between frames
    on the group's stream; a naive frame behind a semantic one finds the GPU tracker's pyramid of the previous frame.  (single, batched) per round: frames 0, 1: the
    semantic job is alone (2, 2) | 2, 3: (0, 4) | 4, 5: (1, 3) | 6, 7: (0, 4)"""
    from dynamic_vins_amd.backend import Batch
    w, h = 320, 240
    modes = [RAW, RAW, SEM, SEM, NAIVE, NAIVE, SEM, SEM]
    members = [SemMember(gpu_ctx_factory, w, h, 91, mode=RAW, inst=False), SemMember(gpu_ctx_factory, w, h, 92),
               SemMember(gpu_ctx_factory, w, h, 93, mode=lambda f: modes[f], inst=False), SemMember(gpu_ctx_factory, w, h, 94, mode=lambda f: modes[f])]
    expect = [(2, 2), (2, 2), (0, 4), (0, 4), (1, 3), (1, 3), (0, 4), (0, 4)]
    batch = Batch([m.batched for m in members])
    for f, e in enumerate(expect):
        before = batch.track_info()
        run_round(batch, members, f)
        d, info = delta(batch, before)
        assert d[:2] == e, (f, d, info)
    batch.close()


def test_refused_round_changes_nothing_and_drops_its_unmask_jobs(gpu_ctx_factory):
    """320 x 240, two semantic members with object trackers and a raw one.  Member 1's rows of round 2 are left uncollected; the next call — frame 3 for everybody, with
    static-instance rectangles staged on member 0 — returns -1 with a lone context's text, no member has a frame pending or a flipped pyramid, member 1 still holds its
    rows of round 2, and rounds 3 to 5 give the rows of twins that saw neither the refused call nor its rectangles, which would have changed frame 3's rows."""
    import torch
    from dynamic_vins_amd.backend import Batch
    from dynamic_vins_amd.frontend import DvinsError
    w, h = 320, 240
    members = [SemMember(gpu_ctx_factory, w, h, 61, big=True, min_dist=30), SemMember(gpu_ctx_factory, w, h, 62), SemMember(gpu_ctx_factory, w, h, 63, mode=RAW, inst=False)]
    first = dets_of(w, h, 0, 61)[0]["track_id"]
    bites = unmask_bites(gpu_ctx_factory, members[0], 4, lambda f: [first] if f == 3 else None)
    assert bites == [3], bites
    batch = Batch([m.batched for m in members])
    run_round(batch, members, 0)
    run_round(batch, members, 1)
    want, jobs = {}, []
    for i, m in enumerate(members):
        want[i] = m.twin_frame(2, 0.1)
        jobs.append(m.job(i, 2, 0.1))
    torch.cuda.synchronize()
    batch.track_enqueue(jobs)
    same(members[0].batched_frame(2, 0.1), want[0], "round 2, member 0")
    same(members[2].batched_frame(2, 0.1), want[2], "round 2, member 2")
    inst1 = members[1].batched_frame(2, 0.1, collect_rows=False)      # its object tracker's frame is collected, its background rows are not
    held = [m.keep for m in members]
    members[0].batched.track_unmask_static(members[0].dets(3), [first])
    jobs = [m.job(i, 3, 0.15) for i, m in enumerate(members)]
    torch.cuda.synchronize()
    with pytest.raises(DvinsError) as err:
        batch.track_enqueue(jobs)
    assert "not collected" in str(err.value)
    for i in (0, 2):
        with pytest.raises(DvinsError):
            members[i].batched.track_stereo_collect()
    same((members[1].batched.track_stereo_collect(),) + inst1, want[1], "round 2, member 1")
    del held
    for f in (3, 4, 5):
        run_round(batch, members, f)
    info = batch.track_info()
    batch.close()
    assert info == dict(rounds=6, members_batched=18, members_single=0), info
