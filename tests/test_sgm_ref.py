"""Premises of the stereo matcher's restatement (tests/sgm_ref.py), asserted on the restatement alone (CPU): the vectorised form equals the naive form on every
intermediate; the subpixel division is a mathematical floor; a shifted texture comes back as its shift; semi-global smoothing is no worse than plain
winner-takes-all on a rendered scene; and every refusal of dv_stereo_sgm_check, which needs no device."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import sgm_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (sgm_params keywords [+ stride], the refusal's text)
REFUSALS = {
    "n_disp": (dict(n_disp=96), "n_disp must be 64, 128 or 256"),
    "p1_negative": (dict(n_disp=64, p1=-1), "p1 must not be negative"),
    "p2_below_p1": (dict(n_disp=64, p1=30, p2=29), "p2 must not be below p1"),
    "p2_above_255": (dict(n_disp=64, p1=10, p2=256), "p2 above 255"),
    "uniqueness_negative": (dict(n_disp=64, uniqueness=-1), r"uniqueness must lie in \[0, 100\)"),
    "uniqueness_100": (dict(n_disp=64, uniqueness=100), r"uniqueness must lie in \[0, 100\)"),
    "reserved": (dict(n_disp=64, reserved=(0, 0, 1)), "reserved words must be zero"),
    "stride": (dict(n_disp=64, stride=71), "row stride below width"),
}


@pytest.mark.parametrize("kind", ["random", "flat", "checker"])
@pytest.mark.parametrize("size", [(12, 7), (20, 9)])
def test_vectorised_form_equals_naive_form(size, kind):
    w, h = size
    l, r = sr.images(kind, w, h, seed=5)
    a, b = sr.sgm(l, r, n_disp=64), sr.sgm_naive(l, r, n_disp=64)
    for item in ("codes_l", "codes_r", "S", "dstar", "dr"):
        assert a[item].dtype == b[item].dtype and np.array_equal(a[item], b[item]), item
    assert np.array_equal(a["out"].view(np.uint32), b["out"].view(np.uint32))
    if kind == "flat":
        assert not a["dstar"].any() and not a["dr"].any()


def test_subpixel_division_is_a_floor():
    """(Sm, S0, Sp) tables with negative numerators (Sp - Sm > den / 16) against exact rational arithmetic, in the scalar and in the vectorised form"""
    table = [(10, 5, 30), (30, 5, 10), (7, 7, 7), (100, 0, 101), (101, 0, 100), (0, 0, 2552), (2552, 0, 0), (5, 5, 6), (6, 5, 5), (40, 39, 90), (12, 3, 13), (3, 3, 4), (9, 2, 200)]
    negatives = 0
    D = 64
    for sm, s0, sp in table:
        den = max(sm + sp - 2 * s0, 1)
        num = 16 * (sm - sp) + den
        negatives += num < 0
        want = 16 * 7 + math.floor(Fraction(num, 2 * den))
        assert sr.subpixel_naive(7, D, sm, s0, sp) == want
        S = np.full((1, 8, D), 3000, np.uint16)          # column 7: the winner at d = 7 with these neighbours, nothing else near
        S[0, 7, 6], S[0, 7, 7], S[0, 7, 8] = sm, s0, sp
        S[0, 7, 7] = s0
        if not (s0 < sm and s0 < sp):
            continue          # not a winner at d = 7: the scalar form above covers it
        _, _, out = sr.decide(S, 0, -1)
        assert out[0, 7] == np.float32(want) / np.float32(16)
    assert negatives >= 4
    assert sr.subpixel_naive(0, D, 0, 5, 9) == 0 and sr.subpixel_naive(D - 1, D, 9, 5, 0) == 16 * (D - 1)


# valid interior pixels of the shifted texture per shift, as the restatement gives them (deterministic: seed 4, 160 x 24, D = 64, default parameters)
SHIFT_COUNTS = {1: 1144, 17: 1016, 63: 648}          # of 1144, 1016, 648: every interior pixel


@pytest.mark.parametrize("k", [1, 17, 63])
def test_shifted_texture_comes_back_as_its_shift(k):
    w, h = 160, 24
    l, r = sr.images("shifted", w, h, seed=4, shift=k)
    out = sr.sgm(l, r, n_disp=64)["out"]
    x0 = max(8, k + 8)
    inner = out[8:h - 8, x0:w - 8]
    valid = inner > 0
    print("shift %d: %d of %d interior pixels valid" % (k, int(valid.sum()), inner.size))
    assert np.abs(inner[valid] - k).max() <= 0.5
    assert int(valid.sum()) == SHIFT_COUNTS[k]
    assert int(valid.sum()) > inner.size // 2


def quality_scene():
    """a rendered 320 x 180 rectified pair (no distortion) with moving boxes, and the true disparity fx * baseline / depth of the left image (all below 64)"""
    from dynamic_vins_amd import dynsim, sim
    from dynamic_vins_amd.render import DynRoomRenderer
    w, h, baseline = 320, 180, 0.12
    cam = dict(fx=200.0, fy=200.0, cx=160.0, cy=90.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0)
    rr = DynRoomRenderer(cam, w, h, device="cpu")
    left, right, _, depth = rr.stereo_dynamic(sim.Trajectory(), 1.0, dynsim.default_boxes(), sim.rig(baseline)["t_ic1"])
    truth = cam["fx"] * baseline / depth.numpy()
    return left.numpy(), right.numpy(), truth


def test_smoothing_is_no_worse_than_winner_takes_all():
    """the share of ALL pixels that are valid and within 1 px of the truth: semi-global (default penalties) against the same census cost with p1 = p2 = 0"""
    left, right, truth = quality_scene()
    assert np.isfinite(truth).all() and 0 < truth.min() and truth.max() < 64
    res = {}
    for name, pen in (("sgm", dict(p1=10, p2=120)), ("wta", dict(p1=0, p2=0))):
        out = sr.sgm(left, right, n_disp=64, **pen)["out"]
        valid = out > 0
        res[name] = dict(valid_share=float(valid.mean()), good_share=float((valid & (np.abs(out - truth) <= 1.0)).mean()))
    print(res)
    path = os.path.join(ROOT, "profiles", "sgm_quality.json")
    if os.access(os.path.dirname(path), os.W_OK):
        with open(path, "w") as f:
            json.dump(dict(scene="DynRoomRenderer 320x180, fx 200, baseline 0.12 m, default boxes, t = 1.0; truth = fx * baseline / depth", n_disp=64,
                           rule="share of all pixels valid and within 1 px of the truth", **res), f, indent=1)
            f.write("\n")
    assert res["sgm"]["good_share"] >= res["wta"]["good_share"]


@pytest.mark.parametrize("name", list(REFUSALS))
def test_every_refusal_without_a_device(name):
    from dynamic_vins_amd import _abi
    from dynamic_vins_amd.frontend import sgm_check
    kw, text = REFUSALS[name]
    sgm_check(72, 10, n_disp=64)          # the same frame is accepted with sound parameters
    with pytest.raises(_abi.DvinsError, match=text):
        sgm_check(72, 10, **kw)


def test_size_refusals_and_loading_without_a_gpu():
    from dynamic_vins_amd import _abi
    from dynamic_vins_amd.frontend import sgm_check
    lib = _abi.load()
    for n in ("dv_stereo_sgm_check", "dv_stereo_sgm_enqueue", "dv_stereo_sgm_collect", "dv_stereo_sgm_debug"):
        assert n in _abi.SIGNATURES and getattr(lib, n) is not None
    with pytest.raises(_abi.DvinsError, match="image sizes must be positive"):
        sgm_check(0, 10, n_disp=64)
    assert lib.dv_stereo_sgm_check(72, 10, 72, None) != 0 and b"null parameters" in lib.dv_last_error(None)
