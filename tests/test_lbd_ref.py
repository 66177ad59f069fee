"""The premises of tests/test_lbd.py's cases, asserted on the reference alone (tests/lbd_ref.py), and the refusals of dv_lbd_check — none of it needs a device.
The float64 evaluation of the same formulas is REPORTED beside the float32 one (printed, not gated): the distance says how far a byte is from flipping."""
import numpy as np
import pytest

from tests import lbd_cases as lc
from tests import lbd_ref


def test_tables_pairs_and_pixel_rule():
    gg, gl = lbd_ref.tables()
    assert gg[31] == 1.0 and gl[10] == 1.0 and np.array_equal(gg, gg[::-1]) and np.array_equal(gl, gl[::-1])
    assert abs(gg[0] - np.exp(-0.5)) < 1e-15 and abs(gl[0] - np.exp(-100 / 98)) < 1e-15          # u = sigma = 31; u = 10, sigma = 7: the integer divisions
    assert len(set(lbd_ref.PAIRS)) == 32 and all(a < b for a, b in lbd_ref.PAIRS)
    L = np.array([lc.line(0, 0, 0, 0), lc.line(0.5, 0, 1.5, 0), lc.line(2.5, 7, 3.5, 1), lc.line(10.4, 3, 2.6, 5.5)], np.float32)
    assert lbd_ref.num_pixels(L).tolist() == [1, 3, 7, 8]          # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 5.5 -> 6: ties to even


def test_gradient_oracle_on_hand_computed_images():
    ramp = np.tile(np.arange(0, 120, 10, dtype=np.uint8), (9, 1))          # a ramp survives a symmetric blur away from the border
    dx, dy = lbd_ref.gradients(ramp)
    assert (dx[:, 3:-3] == 80).all() and (dy == 0).all() and (dx[:, 0] == 0).all() and (dx[:, -1] == 0).all()          # reflect-101: the border column's difference is 0
    one = np.full((1, 6), 9, np.uint8)
    assert all((g == 0).all() for g in lbd_ref.gradients(one))
    assert np.array_equal(lbd_ref.blur(np.full((5, 5), 255, np.uint8)), np.full((5, 5), 255, np.uint8))          # the weights sum to 256


def test_flat_image_gives_zero_rows():
    r = lc.reference("flat")
    assert (r["dx"] == 0).all() and (r["dy"] == 0).all()
    assert np.isnan(r["des"]).all() and (r["rows"] == 0).all()


def test_the_tie_case_really_ties():
    r = lc.reference("step")
    d = r["des"][0].reshape(9, 8)
    assert not np.isnan(d).any()
    ties = [(a, b, i) for a, b in lbd_ref.PAIRS for i in range(8) if d[a, i] == d[b, i] and d[a, i] != 0]
    assert (2, 6, 0) in ties, ties                     # opposite bands, equal to the bit, non-zero: f1 > f2 is false and so is f2 > f1
    k = lbd_ref.PAIRS.index((2, 6))
    assert r["rows"][0, k] & 1 == 0
    assert (d[:, [2, 3, 6, 7]] == 0).all()             # dy = 0 and sin = 0: the orthogonal half is exactly zero, another tie in every pair


def test_the_clamped_cases_really_leave_the_image():
    r = lc.reference("sides")
    (X0, Y0), (C, S) = r["parts"]["x_raw"], r["parts"]["y_raw"]
    n = r["npix"][:, None].astype(np.float32)
    xe, ye = X0 + C * (n - 1), Y0 + S * (n - 1)          # where a row ends, up to rounding
    lo_x, hi_x = np.minimum(X0, xe).min(1), np.maximum(X0, xe).max(1)
    lo_y, hi_y = np.minimum(Y0, ye).min(1), np.maximum(Y0, ye).max(1)
    assert lo_x[0] < -1 and hi_x[1] > 96 and lo_y[2] < -1 and hi_y[3] > 40 and lo_x[4] < -1 and lo_y[4] < -1          # left, right, top, bottom, corner
    o = lc.reference("outside")
    for li in range(2):
        xs = np.array([x[li] for x in o["parts"]["x"]])
        ys = np.array([y[li] for y in o["parts"]["y"]])
        xs, ys = xs[xs >= 0], ys[ys >= 0]
        assert len(set(xs.tolist())) == 1 and len(set(ys.tolist())) == 1 and xs[0] in (0, 95) and ys[0] in (0, 39)          # every sample is one corner pixel


def test_kinds_cover_the_lengths_and_angles():
    assert lc.reference("pixels")["npix"].tolist() == [1, 2, 63, 64, 65, 130]
    a = lc.reference("angles")["lines"][:, 4]
    c, s = lbd_ref.directions(lc.reference("angles")["lines"])
    assert a[0] == 0 and c[0] == 1 and s[0] == 0
    # NOT the issue's denormal cosine, which no float angle reaches: its substitute, the smallest non-zero cosine one does (lbd_cases.SMALLEST_COS_ANGLE), 4.37e-8
    assert a[1] == np.float32(lc.SMALLEST_COS_ANGLE) and 4e-8 < abs(c[1]) < 5e-8 and 4e-8 < abs(c[2]) < 5e-8 and s[1] == 1 and s[2] == -1
    assert c[3] == -1 and c[4] == -1 and 0 < abs(s[3]) < 1e-7 and s[3] == -s[4]
    assert len(lc.reference("many")["lines"]) == 512 and len(lc.reference("one")["lines"]) == 1


def test_float64_yardstick_is_reported():
    for name in lc.kinds():
        r = lc.reference(name)
        ok = ~np.isnan(r["des"])
        delta = float(np.abs(r["des"][ok] - r["des64"][ok]).max()) if ok.any() else float("nan")
        print(f"{name}: max |float32 - float64| = {delta:.3g}; bytes that differ = {int((r['rows'] != r['rows64']).sum())} of {r['rows'].size}")


def test_selection_reference():
    lines, mask, min_length = lc.selection_lines()
    assert lbd_ref.select(lines, min_length, mask).tolist() == [0, 5, 6, 7, 10, 12]
    assert lbd_ref.select(lines, min_length, None).tolist() == [i for i in range(13) if i != 1]
    assert lbd_ref.select(lines, 2e9, mask).tolist() == []


def test_refusals_need_no_device():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import lbd_check, lbd_num_pixels
    good = np.array([lc.line(3, 4, 30, 9)], np.float32)
    lbd_check(96, 40, 120, good)
    lbd_check(96, 40, 96, good, np.array([136], np.int32))
    lbd_check(96, 40, 96, np.zeros((0, 6), np.float32))
    assert lbd_num_pixels(good).tolist() == lbd_ref.num_pixels(good).tolist() == [28]
    nan_angle = good.copy(); nan_angle[0, 4] = np.nan
    inf_x = good.copy(); inf_x[0, 2] = np.inf
    for kw, why in ((dict(lines=np.tile(good, (513, 1))), "DV_LINE_MAX"), (dict(lines=nan_angle), "non-finite"), (dict(lines=inf_x), "non-finite"), (dict(w=32768, stride=32768), "32767"),
                    (dict(h=32768), "32767"), (dict(num_pixels=np.array([0], np.int32)), "num_pixels"), (dict(num_pixels=np.array([137], np.int32)), "num_pixels"),
                    (dict(stride=95), "stride"), (dict(mem=7), "memory kind"), (dict(mask=np.zeros((40, 96), np.uint8), mask_stride=64), "mask stride")):
        args = dict(w=96, h=40, stride=96, lines=good)
        args.update(kw)
        with pytest.raises(DvinsError, match="dv_lbd_check.*" + why):
            lbd_check(**args)
    with pytest.raises(DvinsError, match="null key lines"):
        lbd_check(96, 40, 96, None, n=3)
    with pytest.raises(DvinsError, match="aligned"):
        lbd_check(96, 40, 96, good.ctypes.data + 2, n=1, mem=2)
