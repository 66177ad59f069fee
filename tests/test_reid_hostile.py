"""The ReID extractor on the device (`-m gpu`) at its limits, against the cases and references of tests/reid_hostile.py (their premises: tests/test_reid_hostile_ref.py).

Prepared input at camera geometry: bit for bit against rr.prepare.  dv_reid_layer and dv_reid_stem on real-valued data: the bound of tests/test_reid.py unchanged (device
error against float64 at most 4 x the CPU float32 error on the same case, floor one float32 ulp of the largest output).  On integer data, on one-hot inputs, on flat images
and across batch positions: equality in every bit.

Largest ratios device error / float32 error measured on the MI355X (none is asserted beyond the 4 x rule):
  limit shapes (c_in 32, 96, 160, 512 into c_out 64, 192, 320, 192; the net's maps up to 128 x 128 and n = 64)   1.74 (96 -> 192 stride 1 at 9 x 7; 1.47 at 64 -> 128 on 64 x 32; 1.17 at n = 64)
  working regime (non-negative activations and weights, c_in 64 and 512)                                          1.07 at c_in = 64, 0.75 at c_in = 512
  stem                                                                                                            2.05 at 1 x 2 (4.7e-7 absolute), 1.31 at 121 x 57"""
import numpy as np
import pytest

from tests import reid_cases as rc
from tests import reid_hostile as rh
from tests import reid_ref as rr
from tests.test_reid import bound, make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded():
    c = make_ctx()
    c.reid_load(rc.weights(0))
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def prepared(c, img, rects, size):
    c.reid_load(rc.weights(0), *size)
    c.reid_extract_enqueue(img, rects)
    _, n = c.reid_extract_collect()
    assert n == len(rects)
    return c.reid_input(n)


# ---- A. crops at camera geometry ----
@pytest.mark.parametrize("frame", rh.CONTEXTS, ids=lambda f: "%dx%d" % f)
def test_camera_crops_bit_for_bit(frame):
    c = make_ctx(*frame)
    try:
        for size in rh.SIZES:
            img, names, rects, want = rh.camera_case(*frame, *size)
            got = prepared(c, img, rects, size)
            bad = [names[i] for i in range(len(names)) if not np.array_equal(bits(got[i]), bits(want[i]))]
            assert got.shape == want.shape and not bad, (size, bad, int((got != want).sum()))
    finally:
        c.close()


def test_flat_and_checkerboard_frames_bit_for_bit():
    c = make_ctx(*rh.BIG)
    try:
        for size in rh.SIZES:
            rects = rh.extreme_rects(*size)
            for u in (0, 255):
                got = prepared(c, rh.flat_image(*rh.BIG, u), rects, size)
                t = rh.table_values(u)
                assert all((got[:, ch] == t[ch]).all() for ch in range(3)), (size, u)
            img = rh.checker_image(*rh.BIG)
            got = prepared(c, img, rects, size)
            assert np.array_equal(bits(got), bits(rr.prepare(img, rects, *size))), size
    finally:
        c.close()


# ---- B. dv_reid_layer at the limits of what it accepts ----
def layer_ratio(ctx, case, regime, with_res, relu, per_image=False):
    (x, wt, scale, shift, res), r64, r32 = rh.layer_reference(case, regime, with_res, relu)
    got = ctx.reid_layer(x, wt, scale, shift, residual=res if with_res else None, stride=case[2], relu=relu)
    assert got.shape == r64.shape
    err, e32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    print("layer %s %s res%d relu%d: device %.3e float32 %.3e bound %.3e ratio %.2f" % (rh.case_id(case), regime, with_res, relu, err, e32, bound(r64, r32), err / max(e32, 1e-30)))
    assert err <= bound(r64, r32), (case, regime, with_res, relu, err, e32)
    if per_image:
        for b in range(len(got)):
            assert np.abs(got[b] - r64[b]).max() <= bound(r64[b], r32[b]), (case, b)
    return err / max(e32, 1e-30), got, r64, r32


@pytest.mark.parametrize("case", rh.LIMIT_CASES + rh.NET_CASES, ids=rh.case_id)
def test_layer_at_the_limits_against_float64(ctx, case):
    """one or three chunks of 32 input channels, five (not a power of two); c_out = 192 and 320 through the two-wave kernel with blockIdx.y > 0; 3 x 4 tiles partial on both
    axes; the net's own maps with 8 to 16 tiles per axis; the 128 x 128 maximum; n = 64, where image 63 is held to its own bound like image 0.  Largest ratio measured on the
    MI355X: 1.74 (96 -> 192, stride 1, 9 x 7), 1.47 at 64 -> 128 on the 64 x 32 map, 1.18 at 128 x 128, 1.17 at n = 64"""
    worst = max(layer_ratio(ctx, case, "normal", wr, relu, per_image=True)[0] for wr, relu in ((True, True), (False, False)))
    print("limit %s: largest ratio %.2f" % (rh.case_id(case), worst))


@pytest.mark.parametrize("case", rh.WORKING_CASES, ids=rh.case_id)
def test_layer_in_the_working_regime(ctx, case):
    """x = max(N(0, 1), 0) against weights | N(0, 2 / (k^2 c_in)) |, residual and ReLU on: every product is non-negative, nothing cancels, the sums are the largest the
    net's statistics give.  The 4 x rule unchanged.  Largest ratio measured on the MI355X: 1.07 (64 -> 64 at 9 x 7), 0.75 at c_in = 512"""
    ratio, got, r64, _ = layer_ratio(ctx, case, "working", True, True, per_image=True)
    print("working %s: ratio %.2f" % (rh.case_id(case), ratio))
    assert got.min() > 0


# ---- C. exact checks ----
@pytest.mark.parametrize("case", rh.EXACT_CASES, ids=rh.case_id)
def test_layer_on_integer_data_in_every_bit(ctx, case):
    """every (c_in, c_out, stride, k) of the net and of the limit pairs on integer-valued data: all partial sums are exact in float32 in any order, so the device equals
    the float64 reference in every bit, with the residual before and after the ReLU switch and without either"""
    for with_res, relu in ((True, True), (True, False), (False, True)):
        (x, wt, scale, shift, res), r64, _ = rh.layer_reference(case, "integer", with_res, relu)
        got = ctx.reid_layer(x, wt, scale, shift, residual=res if with_res else None, stride=case[2], relu=relu)
        wrong = np.argwhere(got.astype(np.float64) != r64)
        assert got.shape == r64.shape and len(wrong) == 0, "%s res%d relu%d: %d of %d differ, first at %s: %r against %r" % (
            rh.case_id(case), with_res, relu, len(wrong), got.size, tuple(wrong[0]), got[tuple(wrong[0])], r64[tuple(wrong[0])])


@pytest.mark.parametrize("shape", rh.IMPULSE_SHAPES, ids=lambda s: "%d-%d-s%d-k%d" % s)
def test_layer_impulse_names_the_weight_it_used(ctx, shape):
    """one 1 per image against w[co, ci, ky, kx] = (co * 512 + ci) * 9 + ky * k + kx + 1: every output element is the one weight that met the 1, or 0"""
    x, where, wt, ref = rh.impulse_case(*shape)
    co = shape[1]
    got = ctx.reid_layer(x, wt, np.ones(co, np.float32), np.zeros(co, np.float32), stride=shape[2], relu=False)
    wrong = np.argwhere(got.astype(np.float64) != ref)
    if len(wrong):
        b, o, oy, ox = wrong[0]
        raise AssertionError("%s: %d of %d outputs differ; first at image %d (input channel %d at pixel (%d, %d)), output channel %d at (%d, %d): used (co, ci, tap) = %s, "
                             "the reference %s" % (shape, len(wrong), got.size, b, *where[b], o, oy, ox, rh.impulse_decode(got[b, o, oy, ox]), rh.impulse_decode(ref[b, o, oy, ox])))
    assert got.shape == ref.shape


# ---- D. the stem ----
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("size", rh.STEM_SIZES, ids=lambda s: "%dx%d" % s)
def test_stem_against_float64(ctx, size, n):
    """conv1 + scale / shift + ReLU + max_pool2d(3, 2, 1) from 1 x 1 to 128 x 64, odd and even last rows and columns.  Largest ratio measured on the MI355X: 2.05 (1 x 2, n = 3: device 4.7e-7), 1.73 at 3 x 5, 1.31 at 121 x 57, 0.99 at 128 x 64"""
    (x, wt, scale, shift), r64, r32 = rh.stem_reference(*size, n)
    got = ctx.reid_stem(x, wt, scale, shift)
    err, e32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    print("stem %dx%d n%d: device %.3e float32 %.3e bound %.3e ratio %.2f" % (*size, n, err, e32, bound(r64, r32), err / max(e32, 1e-30)))
    assert got.shape == r64.shape and err <= bound(r64, r32) and got.min() >= 0
    # the last pooled row and column on their own: a slip there is not outvoted by the rest of the map
    for edge, e64, e32_ in ((got[:, :, -1], r64[:, :, -1], r32[:, :, -1]), (got[:, :, :, -1], r64[:, :, :, -1], r32[:, :, :, -1])):
        assert np.abs(edge - e64).max() <= bound(e64, e32_)


@pytest.mark.parametrize("size", rh.STEM_SIZES, ids=lambda s: "%dx%d" % s)
def test_stem_on_integer_data_in_every_bit(ctx, size):
    (x, wt, scale, shift), r64, _ = rh.stem_reference(*size, 3, "integer")
    got = ctx.reid_stem(x, wt, scale, shift)
    wrong = np.argwhere(got.astype(np.float64) != r64)
    assert got.shape == r64.shape and len(wrong) == 0, "%d of %d differ, first at (image, channel, row, column) %s: %r against %r" % (
        len(wrong), got.size, tuple(wrong[0]), got[tuple(wrong[0])], r64[tuple(wrong[0])])


def test_stem_all_negative_is_all_zero_and_nan_stays_where_it_is(ctx):
    import torch
    (x, wt, scale, shift), r64, r32 = rh.stem_reference(9, 7, 3)
    dead = ctx.reid_stem(x, wt, scale, np.full(64, -1e3, np.float32))
    assert dead.shape == r64.shape and not bits(dead).any()          # + 0.0 in every bit
    xn = rh.stem_nan_case()[0]
    n64, n32 = rh.stem(xn, wt, scale, shift, dtype=torch.float64), rh.stem(xn, wt, scale, shift, dtype=torch.float32)
    got = ctx.reid_stem(xn, wt, scale, shift)
    nan = np.isnan(n64)
    assert np.array_equal(np.isnan(got), nan) and nan.sum() == 64 * 6
    assert np.abs(got[~nan] - n64[~nan]).max() <= bound(n64[~nan], n32[~nan])


def test_stem_refusals(ctx):
    from dynamic_vins_amd._abi import DvinsError
    z = lambda *s: np.zeros(s, np.float32)
    for x, why in ((z(65, 3, 4, 4), "1..64 images"), (z(1, 3, 129, 4), "height and width"), (z(1, 3, 4, 129), "height and width")):
        with pytest.raises(DvinsError, match="dv_reid_stem: " + why):
            ctx.reid_stem(x, z(64, 3, 3, 3), z(64), z(64))
    with pytest.raises(ValueError):
        ctx.reid_stem(z(1, 4, 4, 4), z(64, 3, 3, 3), z(64), z(64))


def test_operators_are_refused_while_a_frame_is_in_flight(loaded):
    from dynamic_vins_amd._abi import DvinsError
    z = lambda *s: np.zeros(s, np.float32)
    loaded.reid_load(rc.weights(0))
    loaded.reid_extract_enqueue(rc.image(*rh.SMALL, pad=7), rh.batch_rects()[:2])
    try:
        with pytest.raises(DvinsError, match="dv_reid_stem: a frame is in flight"):
            loaded.reid_stem(z(1, 3, 4, 4), z(64, 3, 3, 3), z(64), z(64))
        with pytest.raises(DvinsError, match="dv_reid_layer: a frame is in flight"):
            loaded.reid_layer(z(1, 64, 4, 4), z(64, 64, 3, 3), z(64), z(64))
    finally:
        loaded.reid_extract_collect()


# ---- E. the whole extractor ----
@pytest.mark.parametrize("size", rh.SIZES, ids=lambda s: "%dx%d" % s)
def test_every_batch_position_equals_the_crop_alone(loaded, size):
    """one frame of 64 distinct crops, the same 64 reversed, and each crop in a frame of its own: a workgroup's M tile belongs to one image at every slot, so the row of a
    crop is the same bits wherever it stands and whatever stands beside it"""
    loaded.reid_load(rc.weights(0), *size)
    img, rects = rc.image(*rh.SMALL, pad=7), rh.batch_rects()
    batch = loaded.reid_extract(img, rects)
    back = loaded.reid_extract(img, rects[::-1].copy())[::-1]
    solo = np.concatenate([loaded.reid_extract(img, rects[i: i + 1]) for i in range(64)])
    assert batch.shape == solo.shape == (64, 512) and np.isfinite(solo).all() and len({r.tobytes() for r in solo}) == 64
    for name, got in (("in order", batch), ("reversed", back)):
        bad = [i for i in range(64) if not np.array_equal(bits(got[i]), bits(solo[i]))]
        assert not bad, "%s: crops %s differ from their solo runs" % (name, bad)


@pytest.mark.parametrize("size", rh.SIZES, ids=lambda s: "%dx%d" % s)
def test_flat_image_gives_one_embedding_64_times(loaded, size):
    x, e64, e32 = rh.flat_reference(*size)
    loaded.reid_load(rc.weights(0), *size)
    got = loaded.reid_extract(rh.flat_colour_image(), rh.flat_rects())
    inp = loaded.reid_input(64)
    assert np.array_equal(bits(inp), bits(x)) and all(np.array_equal(bits(inp[i]), bits(inp[0])) for i in range(64))
    bad = [i for i in range(64) if not np.array_equal(bits(got[i]), bits(got[0]))]
    assert not bad, "embeddings %s differ from embedding 0" % bad
    err = np.abs(got[0] - e64[0]).max()
    print("flat image %s: device %.3e float32 %.3e bound %.3e" % (size, err, np.abs(e32 - e64).max(), bound(e64, e32)))
    assert err <= bound(e64, e32)


@pytest.mark.parametrize("size", rh.SIZES, ids=lambda s: "%dx%d" % s)
def test_camera_frame_embeddings_against_float64(size):
    rects, e64, e32 = rh.camera_embeddings(*size)
    c = make_ctx(*rh.BIG)
    try:
        c.reid_load(rc.weights(0), *size)
        got = c.reid_extract(rh.camera_image(*rh.BIG), rects)
        inp = c.reid_input(len(rects))
    finally:
        c.close()
    _, _, all_rects, x = rh.camera_case(*rh.BIG, *size)
    assert np.array_equal(bits(inp), bits(x[rh.downscaling(all_rects, *size)]))          # what the net was given: the exact half and its four neighbours among them
    err, d32, b = np.abs(got - e64).max(), np.abs(e32 - e64).max(), bound(e64, e32)
    off =np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max()
    print("camera frame %s: %d crops, device %.3e float32 %.3e bound %.3e ratio %.2f, largest | norm - 1 | %.3e" % (size, len(rects), err, d32, b, err / d32, off))
    assert got.shape == e64.shape and err <= b and off <= b


def test_dead_embedding_is_nan_and_leaves_no_trace():
    """conv2.7.conv.4.bias at -1e3: the last map is all zero, the reference row 0 / 0 in every component, and so is the device's; the next frame under the normal weights is
    the bits of a ctx that never saw the dead ones"""
    img, rects = rc.image(*rh.SMALL, pad=7), rh.batch_rects()[:3]
    c = make_ctx()
    try:
        c.reid_load(rh.dead_weights())
        dead = c.reid_extract(img, rects)
        c.reid_load(rc.weights(0))
        after = c.reid_extract(img, rects)
    finally:
        c.close()
    fresh = make_ctx()
    try:
        fresh.reid_load(rc.weights(0))
        want = fresh.reid_extract(img, rects)
    finally:
        fresh.close()
    assert dead.shape == (3, 512) and np.isnan(dead).all()
    assert np.isfinite(want).all() and np.array_equal(bits(after), bits(want))
