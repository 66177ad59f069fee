"""dv_destroy with a frame in flight on every per-frame stage (`-m gpu`): label images, mask stack, detector input, detector head, ReID, multi-object tracker, LBD (both
cams) and line tracker each run one collected frame on one 33 x 17 context, then each gets a frame that is enqueued and NOT collected, then the context is destroyed.
dv_destroy drains the context's stream before it frees anything, so this is a legal sequence: the stages' buffers, pinned blocks and events go with their structs.  A
second context then runs the label-image stage and gives what dv_viode_mask and the host rule give.  Run in a child process under a time limit, so that a teardown that
hangs or takes the process down fails this test alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 33, 17


def frames():
    """every stage's smallest input -> dict of name: (enqueue, collect) closures over a context"""
    from tests import mot_cases, reid_cases, solo_cases
    from tests.test_solo_head import device_outputs, to_params
    from tests.test_stage_protocol import viode_case
    rng = np.random.default_rng(3)
    s0, s1, keys = viode_case(W, H)
    stack = np.zeros((2, H, W), np.uint8); stack[0, 2:9, 3:14] = 1; stack[1, 8:15, 20:31] = 1
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, (H, W), dtype=np.uint8)
    head = solo_cases.get("upsample")
    keep = []
    head_out, head_par = device_outputs(head["inp"], "host", keep), to_params(head["par"])
    rect = np.array([[3, 4, 10, 8]], np.float32)
    (m_rects, m_feats, _), m_par = mot_cases.small_scenario()[0], mot_cases.SMALL
    lines = np.array([[2, 3, 28, 12, 0.33, 27.5], [30, 2, 4, 14, 2.7, 28.6]], np.float32)          # sx, sy, ex, ey, angle, length
    desc = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    keep += [s0, s1, keys, stack, bgr, gray, rect, m_rects, m_feats, lines, desc]

    def setup(c):
        c.reid_load(reid_cases.weights(0))
        c.mot_config(**m_par)
    stages = {
        "viode": (lambda c: c.viode_frame_enqueue(s0, s1, keys), lambda c: c.viode_frame_collect(4)),
        "inst_stack": (lambda c: c.inst_stack_frame_enqueue(stack), lambda c: c.inst_stack_frame_collect(4)),
        "solo_input": (lambda c: c.solo_input_enqueue(bgr, 64, 32), lambda c: c.solo_input_collect()),
        "solo_head": (lambda c: c.solo_head_enqueue(head_out, head_par), lambda c: c.solo_head_collect()),
        "reid": (lambda c: c.reid_extract_enqueue(bgr, rect), lambda c: c.reid_extract_collect()),
        "mot": (lambda c: c.mot_update_enqueue(m_rects, m_feats), lambda c: c.mot_update_collect()),
        "lbd0": (lambda c: c.lbd_describe_enqueue(0, gray, lines, min_length=1.0), lambda c: c.lbd_describe_collect(0)),
        "lbd1": (lambda c: c.lbd_describe_enqueue(1, gray, lines, min_length=1.0), lambda c: c.lbd_describe_collect(1)),
        "line_track": (lambda c: c.line_track_enqueue(lines, desc, lines, desc), lambda c: c.line_track_collect()),
    }
    return setup, stages, (s0, s1, keys), keep


def child():
    from tests.test_stage_protocol import fresh_ctx, viode_check, viode_expect
    setup, stages, (s0, s1, keys), keep = frames()
    ctx = fresh_ctx(W, H)
    setup(ctx)
    for name, (enqueue, collect) in stages.items():          # one collected frame each
        enqueue(ctx)
        collect(ctx)
    for name, (enqueue, _) in stages.items():                # and one in flight on every stage at once
        enqueue(ctx)
    ctx.close()                                              # dv_destroy
    print("destroyed with %d frames in flight" % len(stages), flush=True)
    second = fresh_ctx(W, H)
    want = viode_expect(second, s0, s1, keys)
    second.viode_frame_enqueue(s0, s1, keys)
    viode_check(second.viode_frame_collect(4), want, W, H)
    assert second.lib.dv_last_error(second.h) == b""
    second.close()
    print("second context ok", flush=True)


def test_destroy_with_a_frame_in_flight_on_every_stage():
    r = subprocess.run([sys.executable, "-c", "from tests.test_stage_teardown import child; child()"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "destroyed with 9 frames in flight" in r.stdout and "second context ok" in r.stdout, r.stdout[-2000:]
