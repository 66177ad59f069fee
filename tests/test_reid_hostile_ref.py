"""Premises of the ReID extractor's hostile cases (tests/reid_hostile.py), asserted on tests/reid_ref.py alone, on the CPU: every case reaches what it was built for, so
that a later change of a builder or of a seed cannot hollow tests/test_reid_hostile.py out silently.  Every premise prints its count."""
import os
import subprocess

import numpy as np
import pytest

from tests import reid_cases as rc
from tests import reid_hostile as rh
from tests import reid_ref as rr
from tests.test_reid_ref import resize_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clamp_counts(src, dst):
    """destination indices whose source index is left of the crop, at or past its last pixel, and whose fraction is exactly 0.5"""
    s, f = rh.raw_coef(src, dst)
    return int((s < 0).sum()), int((s >= src - 1).sum()), int((f == np.float32(0.5)).sum())


@pytest.mark.parametrize("name", list(rh.LOOP_CASES))
def test_every_scale_class_agrees_with_the_pixel_loop(name):
    """rr.resize_u8 against the pixel loop of tests/test_reid_ref.py on a 16 x 24 destination, and what makes the class a class"""
    (sw, sh), (dw, dh) = rh.LOOP_CASES[name], rh.LOOP_DST
    crop = np.random.default_rng(sw * 1000 + sh).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    a = rr.resize_u8(crop, dw, dh)
    area = sw == 2 * dw and sh == 2 * dh
    lx, rx, hx = clamp_counts(sw, dw)
    ly, ry, hy = clamp_counts(sh, dh)
    print("%s %d x %d -> %d x %d: area path %d; columns left clamp %d right clamp %d f = 0.5 at %d; rows above %d at or past the last %d f = 0.5 at %d"
          % (name, sw, sh, dw, dh, area, lx, rx, hx, ly, ry, hy))
    assert area == (name == "area2")
    if area:
        v = crop.astype(int)
        assert np.array_equal(a, (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2)
        # the bilinear rule at f = 0.5 in both axes gives the same bytes: 1024 * ((1024 (a + b)) >> 4) >> 16 = a + b without loss.  The two paths differ in what they
        # read (the area path never computes a coefficient), not in what they return: only a slip inside one of them tells them apart
        assert np.array_equal(a, resize_loop(crop, dw, dh))
    else:
        assert np.array_equal(a, resize_loop(crop, dw, dh))
    assert (lx > 0) == (sw < dw) and (ly > 0) == (sh < dh)              # only an upscale reaches left of the crop
    want_half = {"s4": (dw, dh), "s4x_s3y": (dw, 0), "s2x": (dw, 0), "s2y": (0, dh), "area2": (dw, dh), "w-1": (0, dh), "w+1": (0, dh), "h-1": (dw, 0), "h+1": (dw, 0)}
    if name in want_half:
        assert (hx, hy) == want_half[name]
    if name in ("s3", "identity"):
        assert (hx, hy) == (0, 0) and all((rh.raw_coef(s, d)[1] == 0).all() for s, d in ((sw, dw), (sh, dh)))      # whole source pixels: a copy
    if name == "identity":
        assert np.array_equal(a, crop) and (rx, ry) == (1, 1)
    if name in ("strip_col", "pixel"):
        assert lx + rx == dw and (a == a[:, :1]).all()                  # one source column: every destination column clamps onto it, from the left or the right
    if name in ("strip_row", "pixel"):
        # one source row: both row indices clamp onto it, but the fraction is kept and each of the two products is truncated on its own: rows may differ by one
        assert ly + ry == dh and np.abs(a.astype(int) - a[:1].astype(int)).max() <= 1
    if name == "s1.5":
        assert sorted(set(rh.raw_coef(sw, dw)[1].tolist())) == [0.25, 0.75]
    if name == "ratio":
        assert len(set(rh.raw_coef(sw, dw)[1].tolist())) >= dw // 2 and len(set(rh.raw_coef(sh, dh)[1].tolist())) >= dh // 2
    if name in ("up", "half_lo"):
        assert lx > 0 and rx > 0 and ly > 0 and ry > 0


@pytest.mark.parametrize("ctx", rh.CONTEXTS)
@pytest.mark.parametrize("size", rh.SIZES)
def test_camera_rectangles_are_the_classes_they_claim(ctx, size):
    W, H = ctx
    iw, ih = size
    img, names, rects, want = rh.camera_case(W, H, iw, ih)
    assert img.shape == (H, W, 3) and img.strides == (3 * W + rh.PAD, 3, 1) and want.shape == (len(names), 3, ih, iw)
    assert set(rh.ALL_NAMES) - set(names) == rh.MISSING[(ctx, size)] and len(names) <= 64
    q = {n: rr.round_rect(r) for n, r in zip(names, rects)}
    assert all(rr.rect_ok(v, W, H) for v in q.values())
    scale = {n: (v[2] / iw, v[3] / ih) for n, v in q.items()}
    for n, s in (("s3", (3, 3)), ("s4", (4, 4)), ("s4x_s3y", (4, 3)), ("s2x", (2, 1)), ("s2y", (1, 2)), ("area2", (2, 2)), ("identity", (1, 1))):
        assert n not in scale or scale[n] == s
    area = [n for n, v in q.items() if v[2] == 2 * iw and v[3] == 2 * ih]
    assert area == ["area2"]
    assert (q["w-1"][2], q["w+1"][2], q["h-1"][3], q["h+1"][3]) == (2 * iw - 1, 2 * iw + 1, 2 * ih - 1, 2 * ih + 1)
    if size == (64, 128):
        assert (q["w-1"][2], q["w+1"][2], q["h-1"][3], q["h+1"][3]) == (127, 129, 255, 257) and scale["s1.5"] == (1.5, 1.5)
    assert q["ratio"][2:] == [200, 333] and q["whole"] == [0, 0, W, H] and q["pixel"] == [W - 1, H - 1, 1, 1]
    assert q["strip_col"] == [W - 1, 0, 1, H] and q["strip_row"] == [0, H - 1, W, 1]
    corners = [q["corner_" + c] for c in ("tl", "tr", "bl", "br")]
    assert [c[0] for c in corners] == [0, W - 150, 0, W - 150] and [c[1] for c in corners] == [0, 0, H - 290, H - 290]
    # the .5 fields: round half to even moves them ONTO the border, where round half up would leave the image or fall short of it
    r = dict(zip(names, rects))
    halves = sum(int(float(v) % 1 == 0.5) for n in ("half_hi", "half_lo", "half_whole") for v in r[n])
    assert q["half_hi"][0] + q["half_hi"][2] == W and q["half_hi"][1] + q["half_hi"][3] == H and float(r["half_hi"][0]) % 1 == 0.5 and float(r["half_hi"][2]) % 1 == 0.5
    assert q["half_lo"] == [0, 0, 2, 4] and q["half_whole"][:3] == [0, 0, W]
    flush = sum(int(v[0] + v[2] == W) + int(v[1] + v[3] == H) + int(v[0] == 0) + int(v[1] == 0) for v in q.values())
    down = rh.downscaling(rects, iw, ih)
    print("%d x %d at %d x %d: %d rectangles (missing %s), %d downscaling in both axes, %d fields at .5, %d rectangle edges on the image border, largest byte offset %d"
          % (W, H, iw, ih, len(names), sorted(rh.MISSING[(ctx, size)]), len(down), halves, flush, (H - 1) * img.strides[0] + 3 * W - 1))
    assert halves >= 9 and len(down) >= 10
    # the prepared crops differ from each other and are no constant
    assert len({want[i].tobytes() for i in range(len(names))}) == len(names) - (1 if q["whole"] == q["half_whole"] else 0)
    # identity is a copy with the channel swap
    x, y = q["identity"][:2]
    u = img[y: y + ih, x: x + iw, ::-1].astype(np.float32) * (np.float32(1) / np.float32(255))
    assert np.array_equal(want[names.index("identity")], ((u - rr.MEAN) / rr.STD).transpose(2, 0, 1))


def test_flat_and_checkerboard_frames_reach_the_extremes():
    W, H = rh.BIG
    for iw, ih in rh.SIZES:
        rects = rh.extreme_rects(iw, ih)
        for u in (0, 255):
            x = rr.prepare(rh.flat_image(W, H, u), rects, iw, ih)
            t = rh.table_values(u)
            assert all((x[:, c] == t[c]).all() for c in range(3))
        x = rr.prepare(rh.checker_image(W, H), rects, iw, ih)
        lo, hi = rh.table_values(0), rh.table_values(255)
        vals = [sorted(set(np.rint((x[i, 0] * rr.STD[0] + rr.MEAN[0]) * 255).astype(int).ravel().tolist())) for i in range(len(rects))]
        print("checkerboard at %d x %d: bytes per crop (identity, 1.5, exact half at even and odd origin, 1 x 1, whole) %s" % (iw, ih, [v if len(v) < 9 else len(v) for v in vals]))
        assert vals[0] == [0, 255] and ((x[0, 0] == lo[0]) | (x[0, 0] == hi[0])).all()
        assert vals[2] == [128] and vals[3] == [128] and len(vals[4]) == 1          # the area path: (0 + 255 + 255 + 0 + 2) >> 2
        assert len(vals[1]) >= 2 and min(vals[1]) > 0 and max(vals[1]) < 255


@pytest.mark.parametrize("case", rh.EXACT_CASES, ids=rh.case_id)
def test_integer_data_is_exact_in_float32_on_the_cpu_too(case):
    """the premise of the bit-equal layer tests: | sum | <= 8 * 4 * K <= 147456 < 2^24, so the float32 CPU reference equals the float64 one in every bit"""
    ci, co, s, k, h, w, n = case
    (x, wt, scale, shift, res), r64, r32 = rh.layer_reference(case, "integer", True, True)
    assert k * k * ci <= 4608 and np.abs(x).max() <= 8 and np.abs(wt).max() <= 4 and set(scale.tolist()) <= {0.5, 1.0, 2.0}
    assert all((a == np.rint(a)).all() for a in (x, wt, shift, res))
    assert np.array_equal(r32.astype(np.float64), r64) and np.abs(r64).max() < 2 ** 24 and (r64 * 2 == np.rint(r64 * 2)).all()
    assert 0.2 < (r64 == 0).mean() < 0.8 and len(np.unique(r64)) > 20          # the ReLU bites, and the rest is no constant


def test_exact_cases_cover_the_net_and_the_limit_pairs():
    shapes = {c[:4] for c in rh.EXACT_CASES}
    assert shapes == set(rh.LAYERS) | {(ci, co, s, k) for ci, co in rh.LIMIT_PAIRS for s, k in rh.KS} and len(shapes) == 22
    assert {c[4:] for c in rh.EXACT_CASES} == {(9, 7, 3), (17, 13, 3)}
    assert {c[:2] for c in rh.LIMIT_CASES} == {(32, 64), (96, 192), (160, 320), (512, 192)} and len(rh.LIMIT_CASES) == 24
    assert [c[4:] for c in rh.NET_CASES] == [(128, 128, 1), (61, 29, 2), (61, 29, 2), (64, 32, 2), (31, 15, 2), (16, 8, 2), (8, 4, 64)]
    tiles = lambda c: tuple(-(-v // t) for v, t in zip(rh.out_hw(c[4], c[5], c[3], c[2]), (8, 4)))
    print("tiles per axis (rows, columns): limit maps %s, net maps %s" % (sorted({tiles(c) for c in rh.LIMIT_CASES}), [tiles(c) for c in rh.NET_CASES]))
    assert (3, 4) in {tiles(c) for c in rh.LIMIT_CASES} and max(tiles(c) for c in rh.NET_CASES) == (16, 32) and (8, 8) in [tiles(c) for c in rh.NET_CASES]
    for c in rh.LIMIT_CASES + rh.NET_CASES + rh.WORKING_CASES + rh.EXACT_CASES:
        assert c[6] * c[4] * c[5] * max(c[0], c[1]) <= 2 ** 24


@pytest.mark.parametrize("case", rh.WORKING_CASES, ids=rh.case_id)
def test_working_regime_has_no_cancellation(case):
    (x, wt, scale, shift, res), r64, r32 = rh.layer_reference(case, "working", True, True)
    assert x.min() == 0 and wt.min() >= 0 and res.min() == 0 and scale.min() > 0
    zeros = float((x == 0).mean())
    e32 = np.abs(r32 - r64).max()
    print("working regime %s: %.0f %% of the input zero, outputs %.2f .. %.2f, float32 error %.3e (%.2f ulp of the largest)" % (rh.case_id(case), 100 * zeros, r64.min(), r64.max(), e32,
                                                                                                                                 e32 / np.spacing(np.float32(r64.max()))))
    assert 0.45 < zeros < 0.55 and r64.min() > 0 and e32 > 0


@pytest.mark.parametrize("shape", rh.IMPULSE_SHAPES)
def test_impulse_reference_names_every_weight_once(shape):
    ci, co, s, k = shape
    x, where, wt, ref = rh.impulse_case(*shape)
    assert wt.max() < 2 ** 24 and len(np.unique(wt)) == wt.size and (x.sum(axis=(1, 2, 3)) == 1).all()
    assert [rh.impulse_decode(wt[c, i, ky, kx]) for c, i, ky, kx in ((0, 0, 0, 0), (co - 1, ci - 1, k - 1, k - 1))] == [(0, 0, 0), (co - 1, ci - 1, (k - 1) * k + k - 1)]
    assert {c for c, _, _ in where} == set(rh.impulse_channels(ci)) >= {0, 3, 4, 31, ci - 1} and {(y, xx) for _, y, xx in where} == set(rh.IMPULSE_PIXELS)
    hit = 0
    for b, (c, py, px) in enumerate(where):
        nz = np.argwhere(ref[b] != 0)
        hit += len(nz)
        for o, oy, ox in nz:
            dco, dci, tap = rh.impulse_decode(ref[b, o, oy, ox])
            pad = 1 if k == 3 else 0
            assert (dco, dci) == (o, c) and (oy * s - pad + tap // k, ox * s - pad + tap % k) == (py, px)
    taps = {rh.impulse_decode(v)[2] for v in ref[ref != 0]}
    print("impulse %s: %d images, %d non-zero outputs, taps seen %s" % (shape, len(where), hit, sorted(taps)))
    assert hit > 0 and (taps == set(range(k * k)) or s == 2)
    if k == 1:          # stride 2 without padding reads even pixels only: (7, 3) is never read, (8, 4) is
        assert not ref[[b for b, (_, y, xx) in enumerate(where) if (y, xx) == (7, 3)]].any() and ref[[b for b, (_, y, xx) in enumerate(where) if (y, xx) == (8, 4)]].any()


def test_stem_reference_cases():
    import torch
    for h, w in rh.STEM_SIZES:
        for n in (1, 3):
            (x, wt, scale, shift), r64, r32 = rh.stem_reference(h, w, n)
            assert r64.shape == (n, 64, (h + 1) // 2, (w + 1) // 2) and r64.min() >= 0 and r64.max() > 0
        (x, wt, scale, shift), i64, i32 = rh.stem_reference(h, w, 3, "integer")
        assert np.array_equal(i32.astype(np.float64), i64) and (i64 * 2 == np.rint(i64 * 2)).all() and i64.max() > 0
    assert {h % 2 for h, _ in rh.STEM_SIZES} == {0, 1} and {w % 2 for _, w in rh.STEM_SIZES} == {0, 1}
    # a shift below every pre-activation: all zero
    (x, wt, scale, shift), _, _ = rh.stem_reference(9, 7, 3)
    top = float(np.abs(rh.stem(x, wt, scale, np.zeros(64, np.float32), dtype=torch.float64)).max())
    dead = rh.stem(x, wt, scale, np.full(64, -1e3, np.float32), dtype=torch.float64)
    assert top < 1e3 and not dead.any()
    # one NaN pixel: NaN in every channel of the pooled pixels whose 5 x 5 input window holds it, in that image alone
    xn = rh.stem_nan_case()[0]
    nan = np.isnan(rh.stem(xn, wt, scale, shift, dtype=torch.float64))
    b, _, y, xx = rh.NAN_AT
    want = np.zeros_like(nan)
    for py in range(5):
        for px in range(4):
            want[b, :, py, px] = abs(2 * py - y) <= 2 and abs(2 * px - xx) <= 2
    print("stem: largest pre-activation without shift %.2f; NaN at %d of %d outputs (%d pooled pixels x 64 channels)" % (top, int(nan.sum()), nan.size, int(nan.sum()) // 64))
    assert np.array_equal(nan, want) and nan.sum() == 64 * 6 and np.array_equal(np.isnan(rh.stem(xn, wt, scale, shift, dtype=torch.float32)), nan)


def test_whole_extractor_premises():
    import torch
    r = rh.batch_rects()
    assert r.shape == (64, 4) and len({tuple(rr.round_rect(q)) for q in r}) == 64
    x = rr.prepare(rc.image(*rh.SMALL, pad=7), r)
    assert len({x[i].tobytes() for i in range(64)}) == 64
    fr = rh.flat_rects()
    q = [rr.round_rect(v) for v in fr]
    assert len({tuple(v) for v in q}) == 64 and [1, 1] in [v[2:] for v in q] and [0, 0, 70, 41] in q and sum(int(float(v) % 1 == 0.5) for row in fr for v in row) >= 12
    for iw, ih in rh.SIZES:
        fx, e64, e32 = rh.flat_reference(iw, ih)
        t = [rh.table_values(u)[c] for c, u in enumerate(rh.FLAT_COLOUR[::-1])]
        assert all((fx[:, c] == t[c]).all() for c in range(3)) and np.isfinite(e64).all() and abs(np.linalg.norm(e64) - 1) < 1e-12
        rects, c64, c32 = rh.camera_embeddings(iw, ih)
        print("whole extractor at %d x %d: flat image float32 error %.3e; %d camera crops, float32 error %.3e, largest component %.3f"
              % (iw, ih, np.abs(e32 - e64).max(), len(rects), np.abs(c32 - c64).max(), np.abs(c64).max()))
        assert len(rects) >= 10 and np.isfinite(c64).all() and 0 < np.abs(c32 - c64).max() < 1e-6
    # the dead embedding: one tensor changed, the last map all zero, 0 / 0 in every component
    dead, live = rh.dead_weights(), rc.weights(0)
    diff = np.flatnonzero(dead != live)
    P = rr.split(dead)
    assert len(diff) == 512 and (P[rh.DEAD_TENSOR] == -1e3).all() and diff[-1] == rr.n_floats() - 1025
    e = rr.forward(dead, x[:2], torch.float64)
    print("dead embedding: %d of %d reference components NaN" % (int(np.isnan(e).sum()), e.size))
    assert np.isnan(e).all() and np.isnan(rr.forward(dead, x[:2], torch.float32)).all()


def test_host_program_walks_the_same_rectangles():
    """tests/host/reid_host.cpp under AddressSanitizer + UBSan prints every rectangle it walked, rounded: the list is tests/reid_hostile.py's"""
    host = os.path.join(ROOT, "tests", "host")
    subprocess.run(["make", "-s", "-C", host, "-f", "reid.mk", "reid"], check=True, capture_output=True, text=True)
    r = subprocess.run([os.path.join(host, "_build", "reid_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "reid_host ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("rect ")]
    want = [(W, H, iw, ih) + tuple(rr.round_rect(q)) for W, H in rh.CONTEXTS for iw, ih in rh.SIZES for _, q in rh.camera_rects(W, H, iw, ih)]
    print("host program: %d rectangles walked under the sanitizers" % len(got))
    assert got == want and len(got) > 120
