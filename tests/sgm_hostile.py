"""The stereo matcher at its limits: the cases shared by tests/test_sgm_hostile_ref.py (CPU: every case reaches what it was built for, on the restatement alone) and
tests/test_stereo_sgm_hostile.py (the device against tests/sgm_ref.py, bit for bit).  A case is a name -> (left, right, params, layout); its reference result is computed
once by the parts of sgm_ref.sgm and left read-only.  Families:
  narrow      w < n_disp: whole lanes of a path wave never have a pixel at x - d, dR's gather has no x + d < w but at d = 0, `d* <= x` decides most of the image
  thin        h = 1, w = 1, 1 x 1, 2 x 2: chains of one pixel, w + h - 1 = w, 63 of the census wave's lanes retired
  seams       the census tile (256 x 4, four columns per lane) and the path kernels' four chains per workgroup at, and one past, their multiples
  planted     bands of three rows with right(x) = left(x + s): winners at both ends of the disparity range, in every lane slot, and a shift outside the range
  corners_256 the parameter corners at four disparities per lane; uniqueness = 0 with no left-right test (nearly every pixel valid) on every shape
  saturated   the largest sums the rules can produce, flat images, long runs of equal neighbours
  layout      padded rows and a base off a dword, from host, pinned and device memory"""
import functools
from collections import namedtuple

import numpy as np

from tests import sgm_ref as sr

Case = namedtuple("Case", "family w h D par extra lead mems pair")      # par: keywords over sr.params' defaults; rows of w + extra bytes starting `lead` bytes in; pair: the key of its images
ITEMS = ("codes_l", "codes_r", "S", "dstar", "dr")
CORNERS = {"p_zero": dict(p1=0, p2=0), "p_max": dict(p1=255, p2=255), "uniq_0": dict(uniqueness=0), "uniq_99": dict(uniqueness=99), "lr_off": dict(lr_max_diff=-1),
           "lr_0": dict(lr_max_diff=0)}          # tests/test_stereo_sgm.py's
WIDE_OPEN = dict(uniqueness=0, lr_max_diff=-1)      # nearly every pixel with d* <= x is valid: the subpixel arithmetic over the widest spread of d*
# the texture seed of the planted case per n_disp: the first seeds at which every premise of tests/test_sgm_hostile_ref.py holds on the restatement (at least 8 valid
# winners at every shift below n_disp, valid pixels in the band whose shift is outside the range)
PLANTED_SEEDS = {64: 2, 128: 2, 256: 1}
PLANTED_BAND = 3
CASES, _BUILD = {}, {}          # _BUILD: pair key -> the function that makes (left, right); cases that share a key share the images and, with p1 and p2, S


def planted_shifts(D):
    K = D // 64
    return [0, 1, K, K + 1, D // 2 - 1, D - 2, D - 1, D + 3]


def planted_bands(w, h, shifts, seed, top=255):
    """bands of three rows (the last one cut at h); in band i right(x) = left(x + shifts[i]) over a random texture of its own with values in [0, top]"""
    rng = np.random.default_rng(seed)
    l, r = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for i, s in enumerate(shifts):
        rows = slice(PLANTED_BAND * i, min(PLANTED_BAND * (i + 1), h))
        tex = rng.integers(0, top + 1, (PLANTED_BAND, w + s), dtype=np.uint8)[:rows.stop - rows.start]
        l[rows], r[rows] = tex[:, :w], tex[:, s:s + w]
    assert PLANTED_BAND * len(shifts) >= h
    return l, r


def planted(D, seed):
    """n_disp + 24 columns, 24 rows: one band per shift of planted_shifts"""
    return planted_bands(D + 24, PLANTED_BAND * 8, planted_shifts(D), seed)


PROPERTY_SHAPES = [(70, 23, 64), (130, 9, 128)]          # w, h, n_disp
PROPERTY_KINDS = ("random", "planted")
PROPERTY_TOP, PROPERTY_ADD = 200, 55                     # images in [0, 200]; adding 55 to both moves no pixel out of [0, 255]


def property_pair(kind, w, h, D):
    """the pairs of the tests that compare the matcher with itself (a vertical flip, a constant added to both images)"""
    if kind == "random":
        rng = np.random.default_rng(31)
        return rng.integers(0, PROPERTY_TOP + 1, (h, w), dtype=np.uint8), rng.integers(0, PROPERTY_TOP + 1, (h, w), dtype=np.uint8)
    K = D // 64
    shifts = [D // 2 - 1, D - 1, K + 1, 1, D - 2, 0, K, D + 3][:(h + PLANTED_BAND - 1) // PLANTED_BAND]
    return planted_bands(w, h, shifts, 32, top=PROPERTY_TOP)


def anti_checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    l = np.where((xx + yy) % 2, 255, 0).astype(np.uint8)
    return l, (255 - l).astype(np.uint8)


def ramp(w, h, shift):
    x = np.arange(w + shift) % 256
    tex = np.broadcast_to(x.astype(np.uint8), (h, w + shift))
    return np.ascontiguousarray(tex[:, :w]), np.ascontiguousarray(tex[:, shift:shift + w])


def _add(name, family, w, h, D, pair, par=None, extra=0, lead=0, mems=("host",)):
    key, build = pair
    assert name not in CASES, name
    _BUILD.setdefault(key, build)
    CASES[name] = Case(family, w, h, D, dict(par or {}), extra, lead, tuple(mems), key)


def _kind(kind, w, h, seed):
    return (kind, w, h, seed), lambda: sr.images(kind, w, h, seed=seed)


def _register():
    for w, h, D in [(37, 6, 64), (37, 6, 128), (5, 3, 256), (63, 2, 64)]:
        for kind in ("random", "checker"):
            _add("narrow_%dx%d_d%d_%s" % (w, h, D, kind), "narrow", w, h, D, _kind(kind, w, h, 21))
    for w, h, D in [(70, 1, 64), (130, 1, 128), (1, 9, 128), (1, 1, 64), (1, 1, 256), (2, 2, 64)]:
        for kind in ("random", "checker"):
            _add("thin_%dx%d_d%d_%s" % (w, h, D, kind), "thin", w, h, D, _kind(kind, w, h, 22))
    for w, h in [(256, 4), (257, 5), (253, 4), (254, 4), (255, 4), (71, 22), (70, 24), (70, 22)]:
        for kind in ("random", "checker"):
            _add("seams_%dx%d_d64_%s" % (w, h, kind), "seams", w, h, 64, _kind(kind, w, h, 23))
    for D in (64, 128, 256):
        build = ("planted", D), functools.partial(planted, D, PLANTED_SEEDS[D])
        _add("planted_d%d_default" % D, "planted", D + 24, PLANTED_BAND * 8, D, build)
        _add("planted_d%d_wide_open" % D, "planted", D + 24, PLANTED_BAND * 8, D, build, WIDE_OPEN)
    for corner, par in CORNERS.items():
        for kind in ("random", "shifted"):
            _add("corners_260x6_d256_%s_%s" % (corner, kind), "corners_256", 260, 6, 256, _kind(kind, 260, 6, 11), par)
    for w, h, D, extra, lead in [(70, 23, 64, 0, 0), (130, 9, 128, 0, 0), (67, 5, 64, 4, 1), (260, 6, 256, 0, 0)]:      # tests/test_stereo_sgm.py's four shapes
        for kind in ("random", "shifted"):
            _add("corners_%dx%d_d%d_wide_open_%s" % (w, h, D, kind), "corners_256", w, h, D, _kind(kind, w, h, 11), WIDE_OPEN, extra, lead)
    for kind in ("random", "shifted"):
        _add("corners_70x23_d64_lr_300_%s" % kind, "corners_256", 70, 23, 64, _kind(kind, 70, 23, 11), dict(lr_max_diff=300))
    w, h = 70, 8
    _add("saturated_anti_checker", "saturated", w, h, 64, (("anti_checker", w, h), lambda: anti_checker(w, h)), dict(p1=255, p2=255))
    _add("saturated_all_0", "saturated", w, h, 64, (("all_0", w, h), lambda: (np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8))))
    _add("saturated_all_255", "saturated", w, h, 64, (("all_255", w, h), lambda: (np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8))))
    _add("saturated_ramp", "saturated", 300, h, 64, (("ramp", 300, h), lambda: ramp(300, h, 3)))
    _add("saturated_zero_against_random", "saturated", w, h, 64, (("zero_random", w, h), lambda: (np.zeros((h, w), np.uint8), sr.images("random", w, h, seed=24)[1])))
    _add("layout_narrow_37x6_d64", "layout", 37, 6, 64, _kind("random", 37, 6, 21), None, 5, 3, ("host", "pinned", "device"))
    _add("layout_seams_257x5_d64", "layout", 257, 5, 64, _kind("random", 257, 5, 23), None, 5, 3, ("host", "pinned", "device"))


_register()


def names(family=None):
    return [n for n, c in CASES.items() if family is None or c.family == family]


@functools.lru_cache(None)
def _pair(key):
    l, r = _BUILD[key]()
    l, r = np.ascontiguousarray(l, np.uint8), np.ascontiguousarray(r, np.uint8)
    l.setflags(write=False); r.setflags(write=False)
    return l, r


@functools.lru_cache(None)
def _aggregated(key, D, p1, p2):
    """codes and S of a pair: shared by the cases that differ in the decision's parameters alone"""
    l, r = _pair(key)
    cl, cr = sr.census(l), sr.census(r)
    return cl, cr, sr.aggregate(sr.cost_volume(cl, cr, D), p1, p2)


def case(name):
    """-> (left, right, params, layout): params = sr.params(...) complete, layout = (bytes per row beyond w, offset of the base)"""
    c = CASES[name]
    l, r = _pair(c.pair)
    assert l.shape == (c.h, c.w) and r.shape == (c.h, c.w), name
    return l, r, sr.params(n_disp=c.D, **c.par), (c.extra, c.lead)


@functools.lru_cache(None)
def reference(name):
    """the restatement's intermediates and map of a case (sr.sgm's dict, by sr.sgm's own steps), computed once and read-only"""
    _, _, p, _ = case(name)
    cl, cr, S = _aggregated(CASES[name].pair, p["n_disp"], p["p1"], p["p2"])
    dstar, dr, out = sr.decide(S, p["uniqueness"], p["lr_max_diff"])
    res = dict(codes_l=cl, codes_r=cr, S=S, dstar=dstar, dr=dr, out=out)
    for v in res.values():
        v.setflags(write=False)
    return res
