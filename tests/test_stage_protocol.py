"""The enqueue / collect protocol of the per-frame stages (`-m gpu`) where no other module pins it: dv_solo_head_*, dv_reid_extract_*, dv_viode_frame_* and
dv_mot_update_*.  A collect before any enqueue is refused with "<entry>: nothing enqueued", a second enqueue with "<entry>: previous frame not collected"; the frame
in flight is not disturbed by the refusal, and the stage goes on: the next frame of a known small case gives what the frame before the refusals gave and what the
stage's own reference asks.  The tracker's empty frame (n = 0: nothing is launched, collect does not wait) between two real frames changes neither counts nor ids.
(dv_solo_input_*, dv_inst_stack_frame_*, dv_lbd_describe_* and dv_line_track_* have theirs in their own modules.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def fresh_ctx(w, h):
    """a context none of whose stages exists yet"""
    from dynamic_vins_amd.frontend import Context, make_cam
    cam = make_cam(100.0, 100.0, w / 2, h / 2)
    return Context(width=w, height=h, max_cnt=30, min_dist=10, cam0=cam, cam1=cam)


def test_solo_head():
    from dynamic_vins_amd._abi import DvinsError
    from tests import solo_cases
    from tests.test_solo_head import check_against, device_outputs, planes_of, to_params
    rec = solo_cases.get("upsample")          # the smallest constructed case: 3 channels, a 7 x 13 feature, 58 cells, 12 candidates
    w, h = rec["par"]["origin"]
    ctx, keep = fresh_ctx(w, h), []
    try:
        with pytest.raises(DvinsError, match="dv_solo_head_collect: nothing enqueued"):
            ctx.solo_head_collect()
        out, par = device_outputs(rec["inp"], "host", keep), to_params(rec["par"])
        ctx.solo_head_enqueue(out, par)
        with pytest.raises(DvinsError, match="dv_solo_head_enqueue: previous frame not collected"):
            ctx.solo_head_enqueue(out, par)
        labels, scores, st, n_pass = ctx.solo_head_collect()
        first = (labels, scores, planes_of(st, len(labels), w, h).copy(), n_pass)
        with pytest.raises(DvinsError, match="dv_solo_head_collect: nothing enqueued"):
            ctx.solo_head_collect()
        planes, st2, labels2, scores2 = check_against(ctx, rec["inp"], rec["par"], rec["r64"], rec["delta"], "host", keep, "upsample after the refusals")
        assert np.array_equal(first[0], labels2) and first[1].tobytes() == scores2.tobytes() and np.array_equal(first[2], planes) and first[3] == rec["r64"]["n_pass"]
        assert st2.data != st.data          # the two plane sets alternate: the refused enqueue did not flip them
    finally:
        ctx.close()


def test_reid():
    from dynamic_vins_amd._abi import DvinsError
    from tests import reid_cases as rc
    from tests import reid_ref as rr
    from tests.test_reid import H, NAMED, PAD, W
    ctx = fresh_ctx(W, H)
    try:
        ctx.reid_load(rc.weights(0))          # 64 x 128 crops
        with pytest.raises(DvinsError, match="dv_reid_extract_collect: nothing enqueued"):
            ctx.reid_extract_collect()
        img, rects = rc.image(W, H, pad=PAD), NAMED[2:3]
        want = rr.prepare(img, rects)
        ctx.reid_extract_enqueue(img, rects)
        with pytest.raises(DvinsError, match="dv_reid_extract_enqueue: previous frame not collected"):
            ctx.reid_extract_enqueue(img, rects)
        with pytest.raises(DvinsError, match="dv_reid_load: a frame is in flight"):
            ctx.reid_load(rc.weights(0))
        ptr, n = ctx.reid_extract_collect()
        assert ptr != 0 and n == 1
        first = ctx.reid_feats(1)
        assert np.array_equal(ctx.reid_input(1).view(np.uint32), want.view(np.uint32))
        with pytest.raises(DvinsError, match="dv_reid_extract_collect: nothing enqueued"):
            ctx.reid_extract_collect()
        again = ctx.reid_extract(img, rects)          # the kernels sum in a fixed order (no atomics, no split-K): the same frame gives the same bits
        assert np.isfinite(first).all() and first.any() and again.tobytes() == first.tobytes()
        assert np.array_equal(ctx.reid_input(1).view(np.uint32), want.view(np.uint32))
    finally:
        ctx.close()


def viode_case(w=33, h=17):
    """a w x h label image pair with one dynamic key -> (left, right, keys)"""
    from dynamic_vins_amd import viode
    from tests.test_viode_live import label_scene
    rgb = [(10, 1, 2)]
    keys = viode.pixel_to_key(np.array([10]), np.array([1]), np.array([2])).astype(np.uint32)
    s0, s1 = label_scene(w, h, rgb, 10), label_scene(w, h, rgb, 20)
    s0[3:9, 5:16] = (2, 1, 10)          # the key's box is at least 11 x 6, whatever the random blob
    return s0, s1, keys


def viode_expect(ctx, s0, s1, keys, min_size=4):
    from dynamic_vins_amd import viode
    _, inv, k0, bx = ctx.viode_mask(s0, keys)
    k1 = ctx.viode_mask(s1, keys)[2]
    return [(d["track_id"], d["rect"]) for d in viode.detections(k0, bx, keys, min_size)], inv, k0, k1


def viode_check(got, want, w, h):
    from tests.test_viode_live import download
    dets, inv, k0, k1 = got
    assert [(d["track_id"], d["rect"]) for d in dets] == want[0] and len(dets) == 1
    assert np.array_equal(download(inv, w * h).reshape(h, w), want[1])
    assert np.array_equal(download(k0, 4 * w * h).view(np.uint32).reshape(h, w), want[2])
    assert np.array_equal(download(k1, 4 * w * h).view(np.uint32).reshape(h, w), want[3])


def test_viode_frame():
    from dynamic_vins_amd._abi import DvinsError
    w, h = 33, 17
    ctx = fresh_ctx(w, h)
    try:
        s0, s1, keys = viode_case(w, h)
        with pytest.raises(DvinsError, match="dv_viode_frame_collect: nothing enqueued"):
            ctx.viode_frame_collect(4)
        want = viode_expect(ctx, s0, s1, keys)
        ctx.viode_frame_enqueue(s0, s1, keys)
        with pytest.raises(DvinsError, match="dv_viode_frame_enqueue: previous frame not collected"):
            ctx.viode_frame_enqueue(s1, s0, keys)
        first = ctx.viode_frame_collect(4)
        viode_check(first, want, w, h)
        with pytest.raises(DvinsError, match="dv_viode_frame_collect: nothing enqueued"):
            ctx.viode_frame_collect(4)
        ctx.viode_frame_enqueue(s0, s1, keys)
        second = ctx.viode_frame_collect(4)
        viode_check(second, want, w, h)
        assert second[1] != first[1] and second[2] != first[2]          # the two buffer sets alternate: the refused enqueue did not flip them
        viode_check(first, want, w, h)
    finally:
        ctx.close()


def test_mot_empty_frame_between_two_real_ones():
    from dynamic_vins_amd._abi import DvinsError
    from tests.test_mot import ref_of
    frames, par, r64, _ = ref_of("small")          # the smallest scenario; its reference run has no empty frame
    ctx = fresh_ctx(64, 48)
    try:
        ctx.mot_config(**par)
        with pytest.raises(DvinsError, match="dv_mot_update_collect: nothing enqueued"):
            ctx.mot_update_collect()
        at = len(frames) // 2
        assert len(frames[at - 1][0]) > 0 and len(frames[at][0]) > 0
        for k, ((rects, feats, _), ref) in enumerate(zip(frames, r64)):
            if k == at:
                before = ctx.mot_tracks()
                ctx.mot_update_enqueue(np.zeros((0, 4), np.float32), np.zeros((0, par["feat_dim"]), np.float32), n=0)
                with pytest.raises(DvinsError, match="dv_mot_update_enqueue: previous frame not collected"):
                    ctx.mot_update_enqueue(rects, feats)
                with pytest.raises(DvinsError, match="dv_mot_get_tracks: a frame is in flight"):
                    ctx.mot_tracks()
                ids, nt, nc = ctx.mot_update_collect()
                assert len(ids) == 0 and (nt, nc) == counts, "the empty frame changed the counts"
                assert ctx.mot_tracks().tobytes() == before.tobytes(), "the empty frame changed the table"
                with pytest.raises(DvinsError, match="dv_mot_update_collect: nothing enqueued"):
                    ctx.mot_update_collect()
            ids, nt, nc = ctx.mot_update(rects, feats)
            counts = (nt, nc)
            assert np.array_equal(ids, ref["ids"]), f"frame {k}: ids {ids}, reference {ref['ids']}"
            assert nt == len(ref["table"]), f"frame {k}"
    finally:
        ctx.close()
