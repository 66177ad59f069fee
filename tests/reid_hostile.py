"""The ReID extractor at its limits: the case builders and read-only references shared by tests/test_reid_hostile_ref.py (CPU: every case reaches what it was built
for, on tests/reid_ref.py alone) and tests/test_reid_hostile.py (the device against them).  Every reference is computed once and left read-only.  Families:
  camera      crops of 752 x 480 and 1242 x 375 frames (and of a 480 x 752 one, the only one of the three that holds a crop of 4 x the input in both axes: 4 x 128 rows
              are more than either camera has): integer scales, scale 2 in one axis only, exactly 2 x and one pixel off it, 1.5, a non-terminating ratio, identity, the
              whole image, the corners, strips, one pixel, fields at .5 that round to even onto the border; flat and checkerboard images
  layer       dv_reid_layer at the channel counts, map sizes and batch the net never runs but the operator accepts, on normal data, on data of the net's working regime
              (non-negative activations against non-negative weights: no cancellation) and on integer data whose every partial sum is exact
  impulse     a one-hot input against a weight that names its own index: every output element names the weight it used
  stem        dv_reid_stem (conv1 + scale / shift + ReLU + max-pool) at odd and even sizes
  whole       64 crops of one frame, a flat image, a dead last map"""
import functools

import numpy as np

from tests import reid_cases as rc
from tests import reid_ref as rr
from tests.test_reid import LAYERS

SIZES = [(64, 128), (57, 121)]                      # in_w, in_h
BIG, WIDE, TALL = (752, 480), (1242, 375), (480, 752)      # W, H
CONTEXTS = [BIG, WIDE, TALL]
PAD = 5                                             # unused bytes behind every image row
ORIGIN = (37, 11)                                   # where the scale-class crops start: odd, off every alignment


def frozen(a):
    a.setflags(write=False)
    return a


# ---- crops at camera geometry ----
def camera_rects(W, H, in_w, in_h):
    """[(name, (x, y, w, h))] of one frame: every class of the module docstring that fits a W x H image (tests/host/reid_host.cpp builds the same list)"""
    gx, gy = ORIGIN
    cand = [("s3", gx, gy, 3 * in_w, 3 * in_h), ("s4", gx, gy, 4 * in_w, 4 * in_h), ("s4x_s3y", gx, gy, 4 * in_w, 3 * in_h),
            ("s2x", gx, gy, 2 * in_w, in_h), ("s2y", gx, gy, in_w, 2 * in_h), ("area2", gx, gy, 2 * in_w, 2 * in_h),
            ("w-1", gx, gy, 2 * in_w - 1, 2 * in_h), ("w+1", gx, gy, 2 * in_w + 1, 2 * in_h), ("h-1", gx, gy, 2 * in_w, 2 * in_h - 1), ("h+1", gx, gy, 2 * in_w, 2 * in_h + 1),
            ("s1.5", gx, gy, (3 * in_w + 1) // 2, (3 * in_h + 1) // 2), ("ratio", gx, gy, 200, 333), ("identity", gx, gy, in_w, in_h), ("whole", 0, 0, W, H),
            ("corner_tl", 0, 0, 150, 290), ("corner_tr", W - 150, 0, 150, 290), ("corner_bl", 0, H - 290, 150, 290), ("corner_br", W - 150, H - 290, 150, 290),
            ("strip_col", W - 1, 0, 1, H), ("strip_row", 0, H - 1, W, 1), ("pixel", W - 1, H - 1, 1, 1),
            ("half_hi", W - 100.5, H - 200.5, 100.5, 200.5 if H % 2 == 0 else 201), ("half_lo", 0.5, 0.5, 2.5, 3.5), ("half_whole", 0.5, 0.5, W - 0.5, H - 0.5)]
    return [(name, (x, y, w, h)) for name, x, y, w, h in cand if rr.rect_ok(rr.round_rect([x, y, w, h]), W, H)]


ALL_NAMES = [n for n, _ in camera_rects(*TALL, 64, 128)]
# what a frame is too small for: 4 x the input's rows are more than either camera has, 3 x 128 rows more than the wide one's 375
MISSING = {(BIG, (64, 128)): {"s4"}, (BIG, (57, 121)): {"s4"}, (WIDE, (64, 128)): {"s3", "s4", "s4x_s3y"}, (WIDE, (57, 121)): {"s4"}, (TALL, (64, 128)): set(), (TALL, (57, 121)): set()}


@functools.lru_cache(maxsize=None)
def camera_image(W, H):
    return frozen(rc.image(W, H, seed=11, pad=PAD))


@functools.lru_cache(maxsize=None)
def camera_case(W, H, in_w, in_h):
    """-> (image, names, rects [n, 4] float32, prepared [n, 3, in_h, in_w] by rr.prepare)"""
    img = camera_image(W, H)
    named = camera_rects(W, H, in_w, in_h)
    rects = frozen(np.array([r for _, r in named], np.float32))
    return img, [n for n, _ in named], rects, frozen(rr.prepare(img, rects, in_w, in_h))


def downscaling(rects, in_w, in_h):
    """indices of the rectangles larger than the input in both axes"""
    return [i for i, r in enumerate(rects) if rr.round_rect(r)[2] > in_w and rr.round_rect(r)[3] > in_h]


def flat_image(W, H, value):
    buf = np.full((H, 3 * W + PAD), value, np.uint8)
    return frozen(np.lib.stride_tricks.as_strided(buf, (H, W, 3), (buf.strides[0], 3, 1)))


def checker_image(W, H):
    buf = np.zeros((H, 3 * W + PAD), np.uint8)
    img = np.lib.stride_tricks.as_strided(buf, (H, W, 3), (buf.strides[0], 3, 1))
    yy, xx = np.mgrid[0:H, 0:W]
    img[:] = np.where((xx + yy) % 2, 255, 0).astype(np.uint8)[:, :, None]
    return frozen(img)


def table_values(u):
    """the three prepared values of byte u, tensor channel order"""
    return (np.float32(u) * (np.float32(1) / np.float32(255)) - rr.MEAN) / rr.STD


def extreme_rects(in_w, in_h):
    """on the 752 x 480 frame: identity, scale 1.5 (where a checkerboard runs the fixed-point chain at 0, 255 and the mixes between), the exact half, a 1 x 1 crop"""
    gx, gy = ORIGIN
    return frozen(np.array([[gx, gy, in_w, in_h], [gx, gy, (3 * in_w + 1) // 2, (3 * in_h + 1) // 2], [gx, gy, 2 * in_w, 2 * in_h], [gx + 1, gy, 2 * in_w, 2 * in_h], [5, 7, 1, 1],
                            [0.5, 0.5, BIG[0] - 0.5, BIG[1] - 0.5]], np.float32))


# scale classes of the pixel-loop comparison: source (w, h) against a 16 x 24 destination
LOOP_DST = (16, 24)
LOOP_CASES = {"s3": (48, 72), "s4": (64, 96), "s4x_s3y": (64, 72), "s2x": (32, 24), "s2y": (16, 48), "area2": (32, 48), "w-1": (31, 48), "w+1": (33, 48), "h-1": (32, 47),
              "h+1": (32, 49), "s1.5": (24, 36), "ratio": (50, 62), "identity": (16, 24), "whole": (188, 90), "corner": (37, 54), "strip_col": (1, 90), "strip_row": (188, 1),
              "pixel": (1, 1), "half_lo": (2, 4), "up": (7, 5)}


def raw_coef(src, dst):
    """source index and fraction of every destination index BEFORE the clamps, as rr.coef computes them"""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (src / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, f - s.astype(np.float32)


# ---- dv_reid_layer ----
def out_hw(h, w, k, stride):
    pad = 2 if k == 3 else 0
    return (h + pad - k) // stride + 1, (w + pad - k) // stride + 1


LIMIT_PAIRS = [(32, 64), (96, 192), (160, 320), (512, 192)]
KS = [(1, 3), (2, 3), (2, 1)]                       # stride, k
# c_in, c_out, stride, k, h, w, n (the order of LAYERS in tests/test_reid.py, then the map and the batch)
LIMIT_CASES = [(ci, co, s, k, h, w, 2) for ci, co in LIMIT_PAIRS for s, k in KS for h, w in ((9, 7), (17, 13))]
NET_CASES = [(64, 64, 1, 3, 128, 128, 1), (64, 64, 1, 3, 61, 29, 2), (64, 128, 2, 3, 61, 29, 2), (64, 128, 2, 3, 64, 32, 2), (128, 256, 2, 3, 31, 15, 2), (256, 512, 2, 3, 16, 8, 2), (512, 512, 1, 3, 8, 4, 64)]
WORKING_CASES = [(c, c, 1, 3, h, w, 2) for c in (64, 512) for h, w in ((8, 4), (9, 7))]
EXACT_CASES = [(ci, co, s, k, h, w, 3) for ci, co, s, k in LAYERS + [(ci, co, s, k) for ci, co in LIMIT_PAIRS for s, k in KS] for h, w in ((9, 7), (17, 13))]
IMPULSE_SHAPES = [(64, 64, 1, 3), (64, 128, 2, 3), (64, 128, 2, 1), (32, 64, 1, 3), (96, 192, 1, 3), (160, 320, 2, 3), (160, 320, 2, 1), (512, 192, 1, 3), (512, 512, 1, 3)]
IMPULSE_MAP = (17, 13)                              # 3 x 4 tiles at stride 1, 2 x 2 at stride 2, partial on both axes
IMPULSE_PIXELS = [(0, 0), (7, 3), (8, 4), (16, 12)]      # a tile's first and last pixel, the seam (row 8, column 4), the map's last row and column


def case_id(case):
    return "%d-%d-s%d-k%d-%dx%d-n%d" % case


def layer_inputs(case, regime):
    """x, weight, scale, shift, residual of one case.  regime: normal (the distributions of tests/test_reid.py), working (x = max(N(0, 1), 0), weights | N(0, 2 / (k^2
    c_in)) |, a non-negative residual) or integer (x in [-8, 8], weights in [-4, 4], scale a power of two, integer shift and residual: every partial sum is an integer below
    2^24, so float32 holds it exactly in whatever order it is summed)"""
    ci, co, s, k, h, w, n = case
    rng = np.random.default_rng([ci, co, s, k, h, w, n, {"normal": 0, "working": 1, "integer": 2}[regime]])
    ho, wo = out_hw(h, w, k, s)
    if regime == "integer":
        x = rng.integers(-8, 9, (n, ci, h, w)).astype(np.float32)
        wt = rng.integers(-4, 5, (co, ci, k, k)).astype(np.float32)
        scale, shift = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), co), rng.integers(-8, 9, co).astype(np.float32)
        res = rng.integers(-8, 9, (n, co, ho, wo)).astype(np.float32)
    else:
        x = rng.standard_normal((n, ci, h, w)).astype(np.float32)
        wt = (rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (k * k * ci))).astype(np.float32)
        scale, shift = rng.uniform(0.75, 1.25, co).astype(np.float32), (rng.standard_normal(co) * 0.1).astype(np.float32)
        res = rng.standard_normal((n, co, ho, wo)).astype(np.float32)
        if regime == "working":
            x, wt, res = np.maximum(x, 0), np.abs(wt), np.maximum(res, 0)
    return tuple(frozen(a) for a in (x, wt, scale, shift, res))


@functools.lru_cache(maxsize=None)
def layer_reference(case, regime, with_res, relu):
    """-> (inputs, float64 result, float32 result) of rr.layer"""
    import torch
    inp = layer_inputs(case, regime)
    x, wt, scale, shift, res = inp
    kw = dict(residual=res if with_res else None, stride=case[2], relu=relu)
    return inp, frozen(rr.layer(x, wt, scale, shift, dtype=torch.float64, **kw)), frozen(rr.layer(x, wt, scale, shift, dtype=torch.float32, **kw))


def impulse_channels(c_in):
    """both sides of the channel quad (3 | 4), of the half-wave pair and the chunk (31 | 32), and the last channel"""
    return sorted({c for c in (0, 3, 4, 31, 32, c_in - 1) if c < c_in})


def impulse_weight(c_in, c_out, k):
    """w[co, ci, ky, kx] = (co * 512 + ci) * 9 + ky * k + kx + 1: at most 512 * 512 * 9 < 2^24, exact in float32"""
    co, ci, ky, kx = np.meshgrid(np.arange(c_out), np.arange(c_in), np.arange(k), np.arange(k), indexing="ij")
    return frozen(((co * 512 + ci) * 9 + ky * k + kx + 1).astype(np.float32))


def impulse_decode(v):
    """a weight value -> (co, ci, tap), or the value itself where it is no weight"""
    if v != v or v < 1 or v != int(v):
        return float(v)
    q, tap = divmod(int(v) - 1, 9)
    return (q // 512, q % 512, tap)


@functools.lru_cache(maxsize=None)
def impulse_case(c_in, c_out, stride, k):
    """-> (x [n, c_in, 17, 13] with ONE 1 per image, the (channel, row, column) of each image, weight, float64 result).  scale 1, shift 0, no residual, no ReLU"""
    import torch
    h, w = IMPULSE_MAP
    where = [(c, y, x) for c in impulse_channels(c_in) for y, x in IMPULSE_PIXELS]
    x = np.zeros((len(where), c_in, h, w), np.float32)
    for b, (c, py, px) in enumerate(where):
        x[b, c, py, px] = 1
    wt = impulse_weight(c_in, c_out, k)
    ref = rr.layer(x, wt, np.ones(c_out, np.float32), np.zeros(c_out, np.float32), stride=stride, relu=False, dtype=torch.float64)
    return frozen(x), where, wt, frozen(ref)


# ---- dv_reid_stem ----
STEM_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (9, 7), (16, 8), (121, 57), (128, 64)]      # h, w


def stem(x, weight, scale, shift, dtype=None):
    """the operator dv_reid_stem computes, in torch on the CPU: conv2d(pad 1) * scale + shift, ReLU, max_pool2d(3, 2, 1)"""
    import torch
    import torch.nn.functional as F
    dt = dtype or torch.float64
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    y = F.conv2d(t(x), t(weight), padding=1) * t(scale).view(1, -1, 1, 1) + t(shift).view(1, -1, 1, 1)
    return F.max_pool2d(torch.relu(y), 3, 2, 1).numpy()


def stem_inputs(h, w, n, regime="normal"):
    rng = np.random.default_rng([h, w, n, regime == "integer"])
    if regime == "integer":
        x, wt = rng.integers(-8, 9, (n, 3, h, w)).astype(np.float32), rng.integers(-4, 5, (64, 3, 3, 3)).astype(np.float32)
        scale, shift = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), 64), rng.integers(-8, 9, 64).astype(np.float32)
    else:
        x = (rng.standard_normal((n, 3, h, w)) * 1.2).astype(np.float32)                     # the prepared input's spread
        wt = (rng.standard_normal((64, 3, 3, 3)) * np.sqrt(2.0 / 27)).astype(np.float32)
        scale, shift = rng.uniform(0.75, 1.25, 64).astype(np.float32), (rng.standard_normal(64) * 0.1).astype(np.float32)
    return tuple(frozen(a) for a in (x, wt, scale, shift))


@functools.lru_cache(maxsize=None)
def stem_reference(h, w, n, regime="normal"):
    import torch
    inp = stem_inputs(h, w, n, regime)
    return inp, frozen(stem(*inp, dtype=torch.float64)), frozen(stem(*inp, dtype=torch.float32))


NAN_AT = (1, 2, 4, 3)                               # image, channel, row, column of the one NaN pixel on a 9 x 7 map, n = 3


def stem_nan_case():
    inp, _, _ = stem_reference(9, 7, 3)
    x = inp[0].copy()
    x[NAN_AT] = np.nan
    return (frozen(x),) + inp[1:]


# ---- the whole extractor ----
SMALL = (70, 41)


@functools.lru_cache(maxsize=None)
def batch_rects():
    """64 rectangles on the 70 x 41 image whose rounded forms are all different"""
    from tests.test_reid import all_rects
    r = all_rects(64)
    assert len({tuple(rr.round_rect(q)) for q in r}) == 64
    return frozen(r.copy())


@functools.lru_cache(maxsize=None)
def flat_rects():
    """64 different rectangles for the constant image: 1 x 1, the whole image and .5 fields among them"""
    from tests.test_reid import NAMED
    return frozen(np.concatenate([NAMED, rc.rects(53, *SMALL, seed=9, min_w=1, min_h=1)]).astype(np.float32))


FLAT_COLOUR = (31, 142, 250)                        # B, G, R


def flat_colour_image():
    buf = np.zeros((SMALL[1], 3 * SMALL[0] + PAD), np.uint8)
    img = np.lib.stride_tricks.as_strided(buf, (SMALL[1], SMALL[0], 3), (buf.strides[0], 3, 1))
    img[:] = np.array(FLAT_COLOUR, np.uint8)
    return frozen(img)


@functools.lru_cache(maxsize=None)
def flat_reference(in_w, in_h):
    """-> (prepared [64, ...], float64 and float32 embedding of crop 0)"""
    import torch
    x = rr.prepare(flat_colour_image(), flat_rects(), in_w, in_h)
    return frozen(x), frozen(rr.forward(rc.weights(0), x[:1], torch.float64)), frozen(rr.forward(rc.weights(0), x[:1], torch.float32))


@functools.lru_cache(maxsize=None)
def camera_embeddings(in_w, in_h):
    """the downscaling rectangles of the 752 x 480 frame -> (rects, float64 embeddings, float32 embeddings)"""
    import torch
    img, _, rects, x = camera_case(*BIG, in_w, in_h)
    idx = downscaling(rects, in_w, in_h)
    return frozen(rects[idx].copy()), frozen(rr.forward(rc.weights(0), x[idx], torch.float64)), frozen(rr.forward(rc.weights(0), x[idx], torch.float32))


DEAD_TENSOR = "conv2.7.conv.4.bias"


@functools.lru_cache(maxsize=1)
def dead_weights():
    """rc.weights(0) with the last batch-norm's bias at -1e3: the last ReLU leaves an all-zero map, the mean is 0 and the normalisation 0 / 0"""
    flat = rc.weights(0).copy()
    off = 0
    for name, shape in rr.tensors():
        n = int(np.prod(shape))
        if name == DEAD_TENSOR:
            flat[off: off + n] = -1e3
        off += n
    return frozen(flat)
