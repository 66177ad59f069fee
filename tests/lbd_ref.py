"""The LBD descriptor of cv::line_descriptor::BinaryDescriptor at octave 0, restated in numpy in the reference's own order of operations
(thirdparty/line_descriptor/src/binary_descriptor_custom.cpp: computeSobel :373-398, computeLBD :1026-1372, binaryConversion :401-412, the constructor's tables
:217-259) and Detect's selection (line_detector/line_detector.cpp:82-96).  It is the yardstick of tests/test_lbd.py.

Every running sum is sequential: the row starts, the samples along a row, the row sums, the band sums (the reference's literal row loop: own band, band above, band
below) and the sums of the tail are Python loops over the summed index; numpy only vectorises over lines and over the 63 rows, which are independent.  A masked term of
+0.0 is an exact no-op on a sum that is never -0.0, so the conditional sums and the lines' different lengths vectorise.  float32 arrays make every operation round once
to float32 (numpy fuses nothing); dtype=np.float64 evaluates the same formulas in double as a distance yardstick.

The blur is the project's declared rule (separable, weights 14 62 104 62 14 / 256, exact sums, one rounding); the Sobel half is cv::Sobel's exact integers."""
import math

import numpy as np

BANDS, BAND_W = 9, 7
ROWS, FLOATS = BANDS * BAND_W, BANDS * 8
BLUR_W = np.array([14, 62, 104, 62, 14], np.int64)
# combinations[32][2] by its rule: the pairs a < b of the 9 bands in lexicographic order without (0, 7), (0, 8), (1, 7), (1, 8)
PAIRS = [(a, b) for a in range(BANDS) for b in range(a + 1, BANDS) if not (a <= 1 and b >= 7)]
assert len(PAIRS) == 32 and PAIRS[0] == (0, 1) and PAIRS[5] == (0, 6) and PAIRS[6] == (1, 2) and PAIRS[15] == (2, 7) and PAIRS[31] == (7, 8)


def reflect101(p, n):
    p = np.asarray(p).copy()
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def blur(img):
    h, w = img.shape
    a = img.astype(np.int64)[np.ix_(reflect101(np.arange(-2, h + 2), h), reflect101(np.arange(-2, w + 2), w))]
    rows = sum(BLUR_W[k] * a[:, k:k + w] for k in range(5))
    acc = sum(BLUR_W[j] * rows[j:j + h, :] for j in range(5))
    return ((acc + 32768) >> 16).astype(np.uint8)


def gradients(img):
    """(dx, dy) int16 of the blurred image: cv::Sobel(CV_16SC1, 1, 0, 3) and (0, 1, 3), BORDER_REFLECT_101"""
    h, w = img.shape
    b = blur(img).astype(np.int64)[np.ix_(reflect101(np.arange(-1, h + 1), h), reflect101(np.arange(-1, w + 1), w))]
    col = b[:, 2:] - b[:, :-2]
    dx = col[:-2] + 2 * col[1:-1] + col[2:]
    row = b[2:, :] - b[:-2, :]
    dy = row[:, :-2] + 2 * row[:, 1:-1] + row[:, 2:]
    return dx.astype(np.int16), dy.astype(np.int16)


def tables():
    """gaussCoefG_ [63], gaussCoefL_ [21] in double, with the constructor's integer divisions"""
    u, sigma = float((BAND_W * 3 - 1) // 2), float((BAND_W * 2 + 1) // 2)
    inv = -1 / (2 * sigma * sigma)
    gl = np.array([math.exp((i - u) * (i - u) * inv) for i in range(3 * BAND_W)])
    u = float((ROWS - 1) // 2)
    inv = -1 / (2 * u * u)
    gg = np.array([math.exp((i - u) * (i - u) * inv) for i in range(ROWS)])
    return gg, gl


def num_pixels(lines):
    lines = np.asarray(lines, np.float32).reshape(-1, 6)
    r = np.rint(lines[:, :4]).astype(np.float64)          # ties to even
    return (np.maximum(np.abs(r[:, 2] - r[:, 0]), np.abs(r[:, 3] - r[:, 1])) + 1).astype(np.int64)


def coord(v, hi):
    """(short) round(v) clamped to [0, hi]: half away from zero, through int32 with the low 16 bits kept (x86-64); outside int32, or NaN: 0"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5))
        ok = (r > -2147483648.0) & (r < 2147483648.0)
    t = np.where(ok, r, 0.0).astype(np.int64) & 0xFFFF
    t = np.where(t >= 32768, t - 65536, t)
    return np.clip(t, 0, hi)


def directions(lines, dtype=np.float32):
    ang = np.asarray(lines, np.float32).reshape(-1, 6)[:, 4]
    c = np.array([math.cos(float(a)) for a in ang]).astype(dtype)
    s = np.array([math.sin(float(a)) for a in ang]).astype(dtype)
    return c, s


def describe(dx, dy, lines, npix=None, dtype=np.float32, parts=None):
    """-> (des [n, 72] dtype, rows [n, 32] uint8).  parts: a dict that receives the clamped sample coordinates of every line for the premises of the cases"""
    f = dtype
    lines = np.asarray(lines, np.float32).reshape(-1, 6)
    n = len(lines)
    h, w = dx.shape
    if npix is None:
        npix = num_pixels(lines)
    npix = np.asarray(npix, np.int64).reshape(-1)
    ln = ((npix & 0xFFFF) ^ 0x8000) - 0x8000                                     # (short) numOfPixels
    half_w = np.trunc((ln - 1) / 2.0).astype(np.int64)                          # C division truncates
    half_h = (ROWS - 1) // 2
    gg, gl_tab = tables()
    gg, gl_tab = (gg.astype(np.float32).astype(f), gl_tab.astype(np.float32).astype(f)) if f == np.float32 else (gg, gl_tab)
    c, s = directions(lines, f)
    sx, sy, ex, ey = (lines[:, k].astype(f) for k in range(4))
    mx, my = (0.5 * (sx + ex).astype(np.float64)).astype(f), (0.5 * (sy + ey).astype(np.float64)).astype(f)
    gxi, gyi = dx.astype(f), dy.astype(f)
    with np.errstate(all="ignore"):
        x0 = (-c) * half_w.astype(f) + s * f(half_h) + mx
        y0 = (-s) * half_w.astype(f) - c * f(half_h) + my
        X0, Y0 = np.zeros((n, ROWS), f), np.zeros((n, ROWS), f)
        for r in range(ROWS):
            X0[:, r], Y0[:, r] = x0, y0
            x0 = x0 - s
            y0 = y0 + c
        C, S = c[:, None], s[:, None]
        O0, O1 = -S, C
        x, y = X0.copy(), Y0.copy()
        pl, nl, po, no = (np.zeros((n, ROWS), f) for _ in range(4))
        zero = f(0)
        xs, ys = [], []
        for k in range(int(ln.max()) if n else 0):
            on = (k < ln)[:, None]
            xc, yc = coord(x, w - 1), coord(y, h - 1)
            if parts is not None:
                xs.append(np.where(on, xc, -1)); ys.append(np.where(on, yc, -1))
            gx, gy = gxi[yc, xc], gyi[yc, xc]
            g_l = gx * C + gy * S
            g_o = gx * O0 + gy * O1
            pl = pl + np.where(on & (g_l > 0), g_l, zero)
            nl = nl - np.where(on & ~(g_l > 0), g_l, zero)
            po = po + np.where(on & (g_o > 0), g_o, zero)
            no = no - np.where(on & ~(g_o > 0), g_o, zero)
            x = x + C
            y = y + S
        if parts is not None:
            parts["x"], parts["y"], parts["x_raw"], parts["y_raw"] = xs, ys, (X0, Y0), (C, S)
        G = gg[None, :]
        pl, nl, po, no = G * pl, G * nl, G * po, G * no
        rowv = [pl, nl, pl * pl, nl * nl, po, no, po * po, no * no]
        band = [np.zeros((n, BANDS), f) for _ in range(8)]
        for hid in range(ROWS):                                                 # the literal row loop (:1201-1240)
            b = hid // BAND_W
            for bb, cf in ((b, gl_tab[hid % BAND_W + BAND_W]), (b - 1, gl_tab[hid % BAND_W + 2 * BAND_W]), (b + 1, gl_tab[hid % BAND_W])):
                if 0 <= bb < BANDS:
                    for q in range(8):
                        v = rowv[q][:, hid]
                        band[q][:, bb] = band[q][:, bb] + ((cf * cf) * v if q in (2, 3, 6, 7) else cf * v)
        des = np.zeros((n, FLOATS), f)
        inv2, inv3 = (f(np.float32(1.0 / (BAND_W * 2.0))), f(np.float32(1.0 / (BAND_W * 3.0)))) if f == np.float32 else (1.0 / (BAND_W * 2.0), 1.0 / (BAND_W * 3.0))
        for b in range(BANDS):
            inv = inv2 if b in (0, BANDS - 1) else inv3
            for mean_at, std_at, q1, q2 in ((0, 4, 0, 2), (1, 5, 1, 3), (2, 6, 4, 6), (3, 7, 5, 7)):
                t = band[q1][:, b] * inv
                des[:, b * 8 + mean_at] = t
                des[:, b * 8 + std_at] = np.sqrt(band[q2][:, b] * inv - t * t)
        tm, ts = np.zeros(n, f), np.zeros(n, f)
        for b in range(BANDS):
            for k in range(4):
                tm = tm + des[:, b * 8 + k] * des[:, b * 8 + k]
            for k in range(4, 8):
                ts = ts + des[:, b * 8 + k] * des[:, b * 8 + k]
        tm, ts = f(1) / np.sqrt(tm), f(1) / np.sqrt(ts)
        for b in range(BANDS):
            des[:, b * 8:b * 8 + 4] = des[:, b * 8:b * 8 + 4] * tm[:, None]
            des[:, b * 8 + 4:b * 8 + 8] = des[:, b * 8 + 4:b * 8 + 8] * ts[:, None]
        des = np.where(des.astype(np.float64) > 0.4, f(np.float32(0.4)) if f == np.float32 else 0.4, des).astype(f)
        t = np.zeros(n, f)
        for i in range(FLOATS):
            t = t + des[:, i] * des[:, i]
        t = f(1) / np.sqrt(t)
        des = (des * t[:, None]).astype(f)
        rows = np.zeros((n, 32), np.uint8)
        for k, (a, b) in enumerate(PAIRS):
            bits = des[:, 8 * a:8 * a + 8] > des[:, 8 * b:8 * b + 8]
            rows[:, k] = (bits.astype(np.uint32) << np.arange(8, dtype=np.uint32)).sum(axis=1).astype(np.uint8)
    return des, rows


def select(lines, min_length, mask=None):
    """Detect's selection -> the kept indices in input order.  A rounded end point outside the mask drops the line (the project's declared deviation)"""
    lines = np.asarray(lines, np.float32).reshape(-1, 6)
    keep = lines[:, 5] >= np.float32(min_length)
    if mask is not None:
        h, w = mask.shape
        for xk, yk in ((0, 1), (2, 3)):
            rx, ry = np.rint(lines[:, xk]), np.rint(lines[:, yk])
            inside = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
            xi, yi = np.where(inside, rx, 0).astype(np.int64), np.where(inside, ry, 0).astype(np.int64)
            keep &= inside & (mask[yi, xi] != 0)
    return np.flatnonzero(keep).astype(np.int32)


def same_floats(a, b):
    """bit equality of two float32 arrays, NaN matching NaN: IEEE 754 leaves the sign and payload of an invalid operation's NaN to the implementation (x86 sets the
    sign bit, the GPU does not), so a NaN is compared as a NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
