"""The LBD stage on the device (`-m gpu`) against tests/lbd_ref.py: gradients equal to the integer oracle, borders included; the 72 floats and the 32 bytes of every
kind of line in tests/lbd_cases.py bit-equal to the float32 reference (a NaN compared as a NaN: lbd_ref.same_floats says why); selection, order and src exact; the three
memory kinds, both cam slots, the in-flight refusal; and lbd_track chained into the line tracker equal to line_track fed the host copies of the same rows."""
import ctypes as C

import numpy as np
import pytest

from tests import lbd_cases as lc
from tests import lbd_ref

pytestmark = pytest.mark.gpu

CAM = (460.0, 458.0, 367.0, 248.0, -0.28, 0.07, 2e-4, 1e-5)


@pytest.fixture(scope="module")
def ctx():
    from dynamic_vins_amd.frontend import Context, make_cam
    c = Context(width=752, height=480, cam0=make_cam(*CAM), cam1=make_cam(*CAM))
    yield c
    c.close()


@pytest.mark.parametrize("name", ["a", "b", "border5", "border6x1", "flat", "step"])
def test_gradients_equal_the_integer_oracle(ctx, name):
    img = lc.images()[name]
    h, w = img.shape
    assert img.strides[0] > w
    ctx.lbd_describe(img, np.zeros((0, 6), np.float32), cam=1)          # an empty frame still has gradients
    dx, dy, _ = ctx.lbd_debug(1, w, h, 0)
    rx, ry = lbd_ref.gradients(img)
    assert np.array_equal(dx, rx) and np.array_equal(dy, ry)


@pytest.mark.parametrize("name", ["pixels", "angles", "sides", "outside", "one", "many", "flat", "step"])
def test_descriptors_equal_the_float32_reference(ctx, name):
    r = lc.reference(name)
    img, lines = r["img"], r["lines"]
    h, w = img.shape
    out = ctx.lbd_describe(img, lines, min_length=-1.0)
    _, _, fd = ctx.lbd_debug(0, w, h, len(lines))
    bad = [i for i in range(len(lines)) if not lbd_ref.same_floats(fd[i], r["des"][i])]
    assert not bad, f"{name}: the 72 floats of lines {bad[:8]} differ"
    assert out["n"] == len(lines) and np.array_equal(out["src"], np.arange(len(lines)))
    assert np.array_equal(out["desc"], r["rows"]) and out["lines"].tobytes() == lines.tobytes()


def test_selection_order_and_src(ctx):
    lines, mask, min_length = lc.selection_lines()
    img = lc.images()["a"]
    dx, dy = lbd_ref.gradients(img)
    _, rows = lbd_ref.describe(dx, dy, lines)
    smask = lc.strided(mask, 8)
    for m, ml in ((smask, min_length), (None, min_length), (smask, 2e9)):
        keep = lbd_ref.select(lines, ml, m)
        out = ctx.lbd_describe(img, lines, mask=m, min_length=ml)
        assert out["n"] == len(keep) and np.array_equal(out["src"], keep)
        assert np.array_equal(out["desc"], rows[keep]) and out["lines"].tobytes() == lines[keep].tobytes()
    assert ctx.lbd_describe(img, lines, mask=smask, min_length=2e9)["n"] == 0


def test_memory_kinds_cam_slots_and_the_in_flight_refusal(ctx):
    import torch
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED
    ra, rb = lc.reference("sides"), lc.reference("one")
    want = {}
    for r, cam in ((ra, 0), (rb, 1)):
        keep = lbd_ref.select(r["lines"], 10.0)
        want[cam] = (keep, r["rows"][keep])
    pins = []

    def feed(r, cam, img_mem, lines_mem, explicit):
        img, lines = r["img"], r["lines"]
        npix = r["npix"].astype(np.int32) if explicit else None
        h, w = img.shape
        kw = dict(min_length=10.0, size=(w, h), stride=img.strides[0], mem=img_mem, lines_mem=lines_mem, n=len(lines))
        if img_mem == DV_MEM_HOST:
            pi = img
        elif img_mem == DV_MEM_PINNED:
            p = ctx.lib.dv_pinned_alloc(img.strides[0] * h)
            pins.append(p)
            C.memmove(p, img.base.ctypes.data, img.strides[0] * h)
            pi = int(p)
        else:
            t = torch.from_numpy(np.ascontiguousarray(img.base)).cuda()
            pins.append(t)
            pi = t.data_ptr()
        if lines_mem == DV_MEM_HOST:
            pl, pn = lines, npix
            kw.pop("n")
        elif lines_mem == DV_MEM_PINNED:
            p = ctx.lib.dv_pinned_alloc(lines.nbytes + 4 * len(lines))
            pins.append(p)
            C.memmove(p, lines.ctypes.data, lines.nbytes)
            pl, pn = int(p), None
            if explicit:
                C.memmove(p + lines.nbytes, npix.ctypes.data, npix.nbytes)
                pn = int(p) + lines.nbytes
        else:
            tl = torch.from_numpy(lines.copy()).cuda()
            pins.append(tl)
            pl, pn = tl.data_ptr(), None
            if explicit:
                tn = torch.from_numpy(npix).cuda()
                pins.append(tn)
                pn = tn.data_ptr()
        torch.cuda.synchronize()
        ctx.lbd_describe_enqueue(cam, pi, pl, pn, None, **kw)

    kinds = (DV_MEM_HOST, DV_MEM_PINNED, DV_MEM_DEVICE)
    for k, (im, lm) in enumerate([(a, b) for a in kinds for b in kinds]):
        c0 = k & 1                                  # which cam slot goes first alternates; both are in flight together
        feed(ra if c0 == 0 else rb, c0, im, lm, explicit=bool(k & 2))
        feed(rb if c0 == 0 else ra, c0 ^ 1, lm, im, explicit=not (k & 2))
        if k == 0:
            with pytest.raises(DvinsError, match="not collected"):
                ctx.lbd_describe_enqueue(c0, ra["img"], ra["lines"])
        for cam in (c0 ^ 1, c0):
            out = ctx.lbd_describe_collect(cam)
            keep, rows = want[cam]
            assert np.array_equal(out["src"], keep) and np.array_equal(out["desc"], rows), (k, cam)
    with pytest.raises(DvinsError, match="nothing enqueued"):
        ctx.lbd_describe_collect(0)
    nan = ra["lines"].copy()
    nan[1, 4] = np.nan
    t = torch.from_numpy(nan).cuda()
    torch.cuda.synchronize()
    with pytest.raises(DvinsError, match="non-finite"):          # device lines get their value checks at the enqueue
        ctx.lbd_describe_enqueue(0, ra["img"], t.data_ptr(), n=len(nan), lines_mem=DV_MEM_DEVICE)
    assert ctx.lbd_describe(ra["img"], ra["lines"], min_length=10.0)["n"] == len(want[0][0])          # and leave nothing in flight
    for p in pins:
        if not hasattr(p, "data_ptr"):
            ctx.lib.dv_pinned_free(p)


def test_lbd_track_equals_line_track_fed_the_host_rows(ctx):
    from dynamic_vins_amd.frontend import Context, make_cam
    base = lc.images()["a"]
    L0 = np.array([lc.line(20, 12, 60, 14), lc.line(30, 30, 70, 22), lc.line(50, 5, 52, 35), lc.line(10, 20, 25, 21), lc.line(70, 10, 90, 30)], np.float32)
    other = Context(width=752, height=480, cam0=make_cam(*CAM), cam1=make_cam(*CAM))
    try:
        ctx.line_track_reset()
        other.line_track_reset()
        matched = 0
        for k in range(3):
            left, right = lc.strided(np.roll(base, k, axis=1)), lc.strided(np.roll(base, k - 2, axis=1))
            Ll, Lr = L0.copy(), L0[:4].copy()
            Ll[:, [0, 2]] += k
            Lr[:, [0, 2]] += k - 2
            got = ctx.lbd_track(left, Ll, right, Lr, min_length=16.0)
            a, b = other.lbd_describe(left, Ll, min_length=16.0, cam=0), other.lbd_describe(right, Lr, min_length=16.0, cam=1)
            want = other.line_track(a["lines"], a["desc"], b["lines"], b["desc"])
            assert np.array_equal(got["left_kept"], a["src"]) and np.array_equal(got["right_kept"], b["src"]) and len(a["src"]) == 4      # the 15-pixel line is dropped
            for key in ("left_ids", "left_src", "left_cnt", "right_ids", "right_src"):
                assert np.array_equal(got[key], want[key]), (k, key)
            assert got["rows"].tobytes() == want["rows"].tobytes() and len(got["rows"]) > 0
            matched += int((got["left_cnt"] > 0).sum()) + len(got["right_ids"])
        assert matched > 0, "no line was ever matched: the chain was not exercised"
    finally:
        other.close()
