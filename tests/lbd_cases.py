"""The images and key lines of tests/test_lbd.py, built once, with their reference results (tests/lbd_ref.py) computed once and never modified.
tests/test_lbd_ref.py asserts the premise of every case on the reference alone."""
import functools
import math

import numpy as np

from tests import lbd_ref

PI32 = float(np.float32(math.pi))
# SUBSTITUTE for the issue's "angle whose float cos is denormal-small": dL is (float) cos((double) angle) of a FLOAT angle, and no float lies nearer to a zero of the cosine
# than the float nearest pi / 2, whose cosine is -4.37e-8 — a denormal dL cannot be reached through the interface.  This is the smallest cosine that can.
SMALLEST_COS_ANGLE = float(np.float32(math.pi / 2))


def strided(img, extra=24):
    """the same pixels in rows of width + extra bytes; the padding holds 255s a kernel must never read as pixels"""
    h, w = img.shape
    buf = np.full((h, w + extra), 255, np.uint8)
    buf[:, :w] = img
    return buf[:, :w]


def line(sx, sy, ex, ey, angle=None, length=None):
    sx, sy, ex, ey = (float(np.float32(v)) for v in (sx, sy, ex, ey))
    if angle is None:
        angle = math.atan2(ey - sy, ex - sx)
    if length is None:
        length = math.hypot(ex - sx, ey - sy)
    return [sx, sy, ex, ey, float(np.float32(angle)), float(np.float32(length))]


def centred(cx, cy, angle, npix):
    """a line of npix pixels by the library's rule through (cx, cy) at `angle`"""
    c, s = math.cos(angle), math.sin(angle)
    m = max(abs(c), abs(s))
    half = (npix - 1) / (2 * m)
    return line(cx - half * c, cy - half * s, cx + half * c, cy + half * s, angle)


@functools.lru_cache(None)
def images():
    rng = np.random.default_rng(20261020)
    tex = lambda w, h: strided(rng.integers(0, 256, (h, w), dtype=np.uint8))
    step = np.zeros((40, 96), np.uint8)
    step[:, :48], step[:, 48:] = 40, 200
    return {"a": tex(96, 40), "b": tex(70, 23), "flat": strided(np.full((40, 96), 77, np.uint8)), "step": strided(step),
            "border5": tex(5, 5), "border6x1": tex(6, 1)}


def kinds():
    """name -> (image name, [lines]): every kind of line the issue lists, on the 96 x 40 image unless said otherwise"""
    k = {}
    k["pixels"] = ("a", [line(10, 20, 10, 20, 0.0), line(10, 20, 11, 20), line(5, 21, 67, 21), line(5, 19, 68, 19), line(5, 18, 69, 18), line(-20, 20, 109, 20)])
    k["angles"] = ("a", [centred(48, 20, a, 21) for a in (0.0, SMALLEST_COS_ANGLE, -SMALLEST_COS_ANGLE, PI32, -PI32, float(np.float32(math.pi / 4)))])
    k["sides"] = ("a", [line(2, 20, 2, 30), line(93, 8, 93, 28), line(30, 1, 60, 1), line(30, 38, 60, 38), line(1, 1, 9, 9)])
    k["outside"] = ("a", [line(200, 100, 260, 100), line(-300, -50, -240, -90)])
    k["one"] = ("b", [line(8, 11, 50, 14)])
    rng = np.random.default_rng(7)
    many = []
    for _ in range(512):
        a = float(rng.uniform(-math.pi, math.pi))
        many.append(centred(float(rng.uniform(0, 70)), float(rng.uniform(0, 23)), a, int(rng.integers(1, 25))))
    k["many"] = ("b", many)
    k["flat"] = ("flat", [line(20, 20, 70, 20), line(48, 5, 48, 35), line(10, 5, 60, 30)])
    k["step"] = ("step", [line(30, 20, 66, 20, 0.0), line(48, 4, 48, 36)])
    return k


@functools.lru_cache(None)
def reference(name):
    """-> dict(img, lines [n, 6] float32, npix, des, rows, des64, parts) of a kind"""
    img_name, lines = kinds()[name]
    img = images()[img_name]
    lines = np.array(lines, np.float32).reshape(-1, 6)
    dx, dy = lbd_ref.gradients(img)
    parts = {}
    des, rows = lbd_ref.describe(dx, dy, lines, parts=parts)
    des64, rows64 = lbd_ref.describe(dx, dy, lines, dtype=np.float64)
    for a in (lines, des, rows, des64, dx, dy):
        a.setflags(write=False)
    return {"img": img, "lines": lines, "npix": lbd_ref.num_pixels(lines), "dx": dx, "dy": dy, "des": des, "rows": rows, "des64": des64, "rows64": rows64, "parts": parts}


def selection_lines():
    """(lines, mask, min_length) on the 96 x 40 image: lengths at and one float below the threshold, end points at x.5, on the mask's last row / column and one past it,
    a mask byte of 1, a zero byte"""
    mask = np.full((40, 96), 255, np.uint8)
    mask[10, 20] = 1          # a byte of 1 keeps
    mask[12, 30] = 0          # a zero drops
    mask[5, 2] = 0            # (2.5, 5) rounds to x = 2: dropped; (3.5, 5) rounds to 4: kept
    below = float(np.nextafter(np.float32(15.0), np.float32(0.0)))
    L = [line(20, 10, 40, 10, length=15.0),            # 0  exactly min_length, start on the byte of 1: kept
         line(20, 11, 40, 11, length=below),            # 1  one float below: dropped
         line(30, 12, 50, 12, length=20.0),             # 2  start on a zero byte: dropped
         line(50, 13, 30, 12, length=20.0),             # 3  end on the zero byte: dropped
         line(2.5, 5, 40, 6, length=30.0),              # 4  2.5 -> 2 (ties to even), a zero byte: dropped
         line(3.5, 5, 40, 6, length=30.0),              # 5  3.5 -> 4: kept
         line(95, 39, 10, 39, length=30.0),             # 6  on the last column and row: kept
         line(95.4, 39.4, 10, 3, length=30.0),          # 7  rounds to the last column and row: kept
         line(95.5, 20, 10, 3, length=30.0),            # 8  95.5 -> 96, one past the last column: dropped
         line(10, 39.5, 50, 3, length=30.0),            # 9  39.5 -> 40, one past the last row: dropped
         line(-0.5, 20, 50, 3, length=30.0),            # 10 -0.5 -> -0 = column 0: kept
         line(-0.6, 20, 50, 3, length=30.0),            # 11 -1: dropped
         line(60, 20, 80, 25, length=1e9)]              # 12 kept
    return np.array(L, np.float32), mask, 15.0
