"""The line tracker on the device (`-m gpu`) against tests/line_track_ref.py: dv_line_match against the literal restatement of the Mihasher path, dv_line_track_* frame
by frame against TrackLeftLine / TrackRightLine with the input alternating between host, pinned and device memory — ids, source indices, counts and order exactly equal,
rows bit-equal to the ids joined with dv_undistort_lines' output for the same end points —, a reset in mid-sequence, and the cap."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import line_track_cases as lc
from tests import line_track_ref as lr

pytestmark = pytest.mark.gpu

CAM0 = (460.0, 458.0, 367.0, 248.0, -0.28, 0.07, 2e-4, 1e-5)
CAM1 = (457.0, 456.0, 379.0, 255.0, -0.28, 0.07, -1e-4, -2e-4)


@pytest.fixture(scope="module")
def ctx():
    from dynamic_vins_amd.frontend import Context, make_cam
    c = Context(width=752, height=480, cam0=make_cam(*CAM0), cam1=make_cam(*CAM1))
    yield c
    c.close()


class Feeder:
    """hands a frame's arrays over in host, pinned or device memory; keeps them alive until the collect"""

    def __init__(self, ctx):
        import torch
        from dynamic_vins_amd.frontend import DV_LINE_MAX
        self.ctx, self.torch, self.keep = ctx, torch, None
        self.pin = [ctx.lib.dv_pinned_alloc(DV_LINE_MAX * s) for s in (24, 32, 24, 32)]
        assert all(self.pin)

    def close(self):
        for p in self.pin:
            self.ctx.lib.dv_pinned_free(p)

    def track(self, frame, mem):
        from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED
        L, Ld, R, Rd = frame
        if mem == DV_MEM_HOST:
            return self.ctx.line_track(L, Ld, R, Rd)
        arrs = [np.ascontiguousarray(L, np.float32), np.ascontiguousarray(Ld, np.uint8)] + ([] if R is None else [np.ascontiguousarray(R, np.float32), np.ascontiguousarray(Rd, np.uint8)])
        if mem == DV_MEM_PINNED:
            for p, a in zip(self.pin, arrs):
                C.memmove(p, a.ctypes.data, a.nbytes)
            ptrs = [int(p) for p in self.pin[: len(arrs)]]
        else:
            assert mem == DV_MEM_DEVICE
            self.keep = [self.torch.from_numpy(a).cuda() for a in arrs]
            self.torch.cuda.synchronize()
            ptrs = [t.data_ptr() if t.numel() else 0 for t in self.keep]
        ptrs = [p if len(a) else None for p, a in zip(ptrs, arrs)]
        right = (None, None) if R is None else (ptrs[2], ptrs[3])
        return self.ctx.line_track(ptrs[0], ptrs[1], right[0] if R is not None and len(R) else None, right[1] if R is not None and len(R) else None,
                                   n_left=len(L), n_right=0 if R is None else len(R), mem=mem)


def expect_rows(ctx, frame, ref):
    from dynamic_vins_amd.backend import LINEROW_DTYPE
    L, _, R, _ = frame
    un_l = ctx.undistort_lines(ctx.cfg.cam0, L[ref["left_src"]][:, :4]) if len(ref["left_src"]) else np.zeros((0, 4))
    un_r = ctx.undistort_lines(ctx.cfg.cam1, R[ref["right_src"]][:, :4]) if len(ref["right_src"]) else np.zeros((0, 4))
    rows = np.zeros(len(ref["rows"]), LINEROW_DTYPE)
    for k, (i, lp, rp) in enumerate(ref["rows"]):
        rows["id"][k], rows["left"][k] = i, un_l[lp]
        if rp >= 0:
            rows["has_right"][k], rows["right"][k] = 1, un_r[rp]
    return rows


def compare(ctx, frame, got, ref, tag):
    for key in ("left_ids", "left_src", "left_cnt", "right_ids", "right_src"):
        assert np.array_equal(got[key], ref[key]), f"{tag}: {key}\n{got[key]}\n{ref[key]}"
    want = expect_rows(ctx, frame, ref)
    assert got["rows"].tobytes() == want.tobytes(), f"{tag}: rows"


@functools.lru_cache(maxsize=None)
def scenario(name):
    if name == "small":
        frames = lc.small_scenario()
        ref = lc.run_ref(frames)
        lc.conditions(frames, ref)
        return frames, ref
    frames = lc.cap_scenario() if name == "cap" else lc.wave_scenario(int(name[4:]))
    return frames, lc.run_ref(frames)


def test_line_match_equals_the_literal_restatement(ctx):
    query, train, tags = lc.match_case()
    idx_a, dist_a = lr.match_literal(query, train)
    lc.match_conditions(query, train, tags, idx_a, dist_a)
    problems = [(query, train)] + [(q[None, :], t) for q, t in lc.near_pairs(40, seed=9)]
    L, Ld, _, _ = lc.cap_scenario()[0]
    L2, Ld2, _, _ = lc.cap_scenario()[1]
    problems.append((Ld2, Ld))                       # DV_LINE_MAX x DV_LINE_MAX
    for q, t in problems:
        idx_a, dist_a = lr.match_literal(q, t)
        near = (dist_a >= 0) & (dist_a < lr.MATCH_DIST)
        want_idx, want_dist = np.where(near, idx_a, -1), np.where(near, dist_a, 0)
        idx, dist = ctx.line_match(q, t)
        assert np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)
    idx, dist = ctx.line_match(query, train[:0])     # "descriptors matrices cannot be void": no matches
    assert (idx == -1).all() and (dist == 0).all()
    assert len(ctx.line_match(query[:0], train)[0]) == 0


# the memory kind rotates host, pinned, device from a start of the scenario's own: every kind is a first frame somewhere, and the cap runs device then host, then
# pinned then device, so that DV_LINE_MAX lines are read in place on a first and on a tracked frame
@pytest.mark.parametrize("name,start", [("small", 0), ("wave63", 1), ("wave64", 2), ("wave65", 0), ("cap", 2), ("cap", 1)])
def test_tracking_equals_the_reference(ctx, name, start):
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED
    frames, ref = scenario(name)
    feed = Feeder(ctx)
    try:
        ctx.line_track_reset()
        for k, (frame, r) in enumerate(zip(frames, ref)):
            mem = (DV_MEM_HOST, DV_MEM_PINNED, DV_MEM_DEVICE)[(k + start) % 3]
            compare(ctx, frame, feed.track(frame, mem), r, f"{name} frame {k} mem {mem}")
    finally:
        feed.close()


def test_reset_in_mid_sequence(ctx):
    frames = lc.small_scenario()
    ref = lc.run_ref(frames, reset_before=(2,))
    assert np.array_equal(ref[2]["left_ids"], np.arange(len(frames[2][0])))      # a first frame again, ids from 0
    ctx.line_track_reset()
    for k, (frame, r) in enumerate(zip(frames, ref)):
        if k == 2:
            ctx.line_track_reset()
        compare(ctx, frame, ctx.line_track(*frame), r, f"frame {k}")


def test_more_than_the_cap_is_refused_at_enqueue(ctx):
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import DV_LINE_MAX
    frames = lc.small_scenario()
    ctx.line_track_reset()
    first = ctx.line_track(*frames[0])
    L, D = np.zeros((DV_LINE_MAX + 1, 6), np.float32), np.zeros((DV_LINE_MAX + 1, 32), np.uint8)
    with pytest.raises(DvinsError, match="DV_LINE_MAX"):
        ctx.line_track_enqueue(L, D)
    with pytest.raises(DvinsError, match="DV_LINE_MAX"):
        ctx.line_track_enqueue(L[:3], D[:3], L, D)
    with pytest.raises(DvinsError, match="nothing enqueued"):
        ctx.line_track_collect()
    ctx.line_track_enqueue(*frames[1])
    with pytest.raises(DvinsError, match="not collected"):
        ctx.line_track_enqueue(*frames[1])
    got = ctx.line_track_collect()                   # the refused frames left the tracker as it was
    ref = lc.run_ref(frames[:2])
    assert np.array_equal(first["left_ids"], ref[0]["left_ids"]) and np.array_equal(got["left_ids"], ref[1]["left_ids"]) and np.array_equal(got["left_cnt"], ref[1]["left_cnt"])
