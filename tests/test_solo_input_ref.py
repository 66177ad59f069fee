"""The restatement of the detector's input stage (tests/solo_input_ref.py) against the reference's own lines on CPU torch — (t - mean) / std, F.interpolate(bilinear,
align_corners=True), the zero cat — and the refusals of dv_solo_input_check.  No GPU.  torch must stay inside the bar the device is held to, so the bar cannot hide a
wrong restatement; the identity case is bit-equal."""
import numpy as np
import pytest

from tests import solo_input_ref as sr

# the device test's five pairs, then further shapes: an odd image, the reference's KITTI frame into its 1152 x 384 network
PAIRS = list(sr.CASES.values()) + [((67, 21), (96, 48)), ((1242, 375), (1152, 384))]


def test_rectangles_are_the_librarys():
    from dynamic_vins_amd.frontend import solo_rect
    for name, ((w, h), (mw, mh)) in sr.CASES.items():
        assert sr.rect(mw, mh, w, h) == solo_rect(mw, mh, w, h) == sr.RECTS[name], name
    assert sr.rect(1152, 384, 1242, 375) == solo_rect(1152, 384, 1242, 375) == (0, 18, 1152, 348)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_restatement_equals_torch(pair):
    (w, h), (mw, mh) = pair
    _, img = sr.image(w, h, seed=w + h)
    r = sr.solo_input(img, mw, mh)
    t = sr.torch_reference(img, mw, mh)
    assert t.shape == (3, mh, mw) and t.dtype == np.float32
    d = float(np.abs(t.astype(np.float64) - r["out"]).max())
    print("torch - restatement, image %dx%d model %dx%d: %.3g" % (w, h, mw, mh, d))
    assert d <= sr.BAR
    pad = ~r["inside"]
    assert np.array_equal(t[:, pad].view(np.uint32), np.zeros((3, int(pad.sum())), np.uint32))           # +0.0, bit for bit
    assert np.array_equal(r["out"][:, pad], np.zeros((3, int(pad.sum()))))
    ex = r["exact"]
    assert ex.any() and np.array_equal(t[:, ex], r["source"][:, ex]) and np.array_equal(r["out"][:, ex], r["source"][:, ex].astype(np.float64))
    if (w, h) == (mw, mh):
        assert ex.all() and np.array_equal(t.view(np.uint32), sr.normalise(img).view(np.uint32))


def test_axis_rule():
    i0, i1, l0, l1 = sr.axis(23, 22)
    assert i0[0] == 0 and l1[0] == 0 and i0[-1] + (l1[-1] > 0.5) == 22 and (i1 - i0 <= 1).all() and (i1 <= 22).all()
    assert np.array_equal(l0, (np.float32(1) - l1).astype(np.float32)) and (l1 >= 0).all() and (l1 < 1).all()
    i0, i1, l0, l1 = sr.axis(32, 32)
    assert np.array_equal(i0, np.arange(32)) and (l1 == 0).all() and i1[-1] == 31


REFUSALS = [
    (dict(img=(0, 23)), "sizes must be positive"),
    (dict(model=(64, -1)), "sizes must be positive"),
    (dict(img=(1, 23)), "image sides under 2"),
    (dict(img=(2000, 2), model=(64, 32)), "rectangle sides under 2"),
    (dict(std=(58.395, 0.0, 57.375)), "std must not be zero"),
    (dict(mean=(float("nan"), 116.28, 103.53)), "must be finite"),
    (dict(std=(58.395, 57.12, float("inf"))), "must be finite"),
    (dict(stride=3 * 70 - 1), "row stride below 3 \\* width"),
    (dict(model=(64, 33)), "is odd"),                # rect_h 22: the two pads of 5 leave 32 rows
    (dict(img=(23, 70), model=(65, 32)), "is odd"),
    (dict(img=(20000, 23)), "up to 16384"),
]


def refusal_args(kw):
    (w, h), (mw, mh) = kw.get("img", (70, 23)), kw.get("model", (64, 32))
    return dict(img_w=w, img_h=h, model_w=mw, model_h=mh, mean=kw.get("mean", sr.MEAN), std=kw.get("std", sr.STD), stride=kw.get("stride", 3 * w))


@pytest.mark.parametrize("kw,why", REFUSALS, ids=[w.replace(" ", "_").replace("\\", "") + str(i) for i, (_, w) in enumerate(REFUSALS)])
def test_check_refuses_without_a_device(kw, why):
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import solo_input_check
    solo_input_check(70, 23, 64, 32)
    solo_input_check(70, 23, 64, 32, stride=3 * 70 + 5)
    with pytest.raises(DvinsError, match="dv_solo_input_check: .*" + why):
        solo_input_check(**refusal_args(kw))
