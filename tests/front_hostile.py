"""Degenerate inputs for the front end's parity tests (tests/test_front_hostile.py): flat and partly flat frames, exact ties of the corner response, binary images,
dense feature fields, tiny pyramids, wrong initial flows, aperture-problem and no-convergence pairs, repeated points.  Every generator returns plain inputs; the
conditions are asserted on the ORACLE ALONE (or on the numpy restatements below where the oracle's own behaviour is the question) and prove that a case reaches the
branch it is named for.  If a seed fails a condition, take another seed, never loosen the condition (the pattern of tests/mot_cases.py).

Device limits restated here (csrc/gftt.hip, csrc/dv_context.hip dv_ensure_cand; documented beside dv_gftt in include/dvins.h)."""
import numpy as np

from dynamic_vins_amd import synth

W, H = 130, 70              # 3 x 5 tiles of 64 x 16: an interior tile, a ragged right column (2 px) and a ragged bottom row (6 px)
TILE_W, TILE_H = 64, 16
DISC_CAP = 128              # culled disc centres a tile keeps before it falls back to testing every disc
SEL_CAP = 8192              # candidates of ONE value bin the selection can sort
SEL_BINS = 2048
SEL_MAX_CELLS = 32768       # min-distance grid cells
SEL_MAX_ACC = 1024
LK_WIN = 21
ZED_DIST = (-0.17198906485492285, 0.024624053031210322, 0.0003391614313509814, -0.00045583634752113735)


def cand_cap(w, h):
    return max(4096, (w * h) // 4)


def cam_for(w, h):
    return (w * 0.55, w * 0.55, w / 2 - 3.1, h / 2 + 2.2) + ZED_DIST


# ---------------------------------------------------------------- images
def tex_u8(h, w, seed, sigma=1.5):
    return np.ascontiguousarray((synth.texture(h, w, seed, sigma) * 255).astype(np.uint8))


def tiled(h=H, w=W, seed=5):
    """a 16 x 32 texture repeated: every response value of the interior occurs once per period"""
    t = tex_u8(16, 32, seed)
    return np.ascontiguousarray(np.tile(t, ((h + 15) // 16, (w + 31) // 32))[:h, :w])


def mirrored(img):
    return np.ascontiguousarray(img[::-1, ::-1])


def partly_flat(h, w, cols, value, seed=5):
    """texture whose left `cols` columns are `value`"""
    img = tex_u8(h, w, seed)
    img[:, :cols] = value
    return img


def binary(h, w, seed=5, sigma=1.5, plateau=1):
    """a texture thresholded to 0 / 255; plateau: side of the square blocks it is made of (2: every corner is a corner of 2 px blocks, and equal responses abound)"""
    t = np.where(synth.texture((h + plateau - 1) // plateau, (w + plateau - 1) // plateau, seed, sigma) > 0.5, 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.kron(t, np.ones((plateau, plateau), np.uint8))[:h, :w])


def checker(h, w, block=8):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray((((yy // block) + (xx // block)) % 2 * 255).astype(np.uint8))


def block_noise(h, w, seed, block=2):
    """binary noise in block x block cells: as dense in corners as an image gets"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.kron(b, np.ones((block, block), np.uint8))[:h, :w])


def detector_images():
    """name -> image; the partly flat ones cover more than 1/4 and more than 3/4 of the frame, with both flat values"""
    d = {
        "tiled": tiled(),
        "tiled_mirror": mirrored(tiled()),
        "flat0_54pc": partly_flat(H, W, 70, 0),
        "flat255_54pc": partly_flat(H, W, 70, 255),
        "flat255_69pc": partly_flat(H, W, 90, 255),          # the frame the defect was predicted on
        "flat0_80pc": partly_flat(H, W, 104, 0),
        "flat255_80pc": partly_flat(H, W, 104, 255),
        "flat_whole": np.full((H, W), 128, np.uint8),
        "binary": binary(H, W, 5, plateau=2),
        "checker8": checker(H, W, 8),
        "noise2": block_noise(H, W, 3, 2),
        "tiled_17x65": tiled(65, 17),                         # w 17, h 65: one tile column, a 1 px bottom row
        "flat255_65x17": partly_flat(17, 65, 40, 255),        # w 65, h 17: a 1 px right column and a 1 px bottom row
    }
    return d


PARTLY_FLAT = ("flat0_54pc", "flat255_54pc", "flat255_69pc", "flat0_80pc", "flat255_80pc", "flat_whole")
MIN_DISTS = (1, 2, 2.5, 3.5, 0.4, 0.99)


# ---------------------------------------------------------------- numpy restatements (detector)
def local_maxima(eig, mask=None):
    """interior, unmasked pixels with v >= all eight neighbours -> boolean image (what gftt_tile_body emits before any exclusion of zeros)"""
    h, w = eig.shape
    c = eig[1:-1, 1:-1]
    ok = np.ones_like(c, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                ok &= c >= eig[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    out = np.zeros((h, w), bool)
    out[1:-1, 1:-1] = ok
    if mask is not None:
        out &= mask != 0
    return out


def threshold_of(eig, quality, mask, rule):
    sel = eig[mask != 0] if (mask is not None and rule == "cpu") else eig.reshape(-1)          # rule "cuda": the maximum of the whole map
    max_val = float(sel.max()) if sel.size else 0.0
    return max_val, np.float32(max_val * quality)


def census(oracle, img, rule, quality=0.01, mask=None):
    """the candidates the device would emit, counted from the oracle's response map, beside the device's limits"""
    eig = oracle.min_eigen(img, rule=rule)
    lm = local_maxima(eig, mask)
    max_val, thr = threshold_of(eig, quality, mask, rule)
    alive = lm & (eig > thr)
    vals = eig[alive]
    top = np.float32(max_val)
    bscale = np.float32(SEL_BINS) / np.float32(top - thr) if top > thr else np.float32(0)
    bins = np.clip(((vals - thr) * bscale).astype(np.int64), 0, SEL_BINS - 1)
    h, w = img.shape
    return dict(with_zeros=int(lm.sum()), without_zeros=int((lm & (eig != 0)).sum()), surviving=int(alive.sum()),
                top_bin=int((bins == SEL_BINS - 1).sum()) if vals.size else 0,
                max_bin=int(np.bincount(bins).max()) if vals.size else 0,
                max_same_value=int(np.unique(vals, return_counts=True)[1].max()) if vals.size else 0,
                cap=cand_cap(w, h))


def np_gftt(oracle, img, max_n, quality, min_dist, mask=None, rule="cpu", reverse_ties=False, stats=None):
    """thresholded local maxima sorted by (value desc, linear address desc) and the greedy min-distance loop, from the oracle's response map only.
    reverse_ties: address ASCENDING (the wrong order).  stats (a dict): receives `in_step_conflicts`, the candidates that pass every corner accepted in earlier
    groups of 64 consecutive sorted candidates and are suppressed by one accepted inside their own group."""
    eig = oracle.min_eigen(img, rule=rule)
    h, w = eig.shape
    _, thr = threshold_of(eig, quality, mask, rule)
    alive = local_maxima(eig, mask) & (eig > thr)
    addr = np.flatnonzero(alive.reshape(-1))
    vals = eig.reshape(-1)[addr]
    order = np.lexsort((addr if reverse_ties else -addr, -vals.astype(np.float64)))
    addr = addr[order]
    cx, cy = (addr % w).astype(np.float32), (addr // w).astype(np.float32)
    max_n = max_n if max_n > 0 else SEL_MAX_ACC
    out, src = [], []
    conflicts = 0
    md2 = float(min_dist) * float(min_dist)
    ax, ay = np.zeros(len(addr), np.float32), np.zeros(len(addr), np.float32)
    for i in range(len(addr)):
        n = len(out)
        if n == max_n:
            break
        if min_dist >= 1 and n:
            d2 = ((cx[i] - ax[:n]) ** 2 + (cy[i] - ay[:n]) ** 2).astype(np.float64)
            hit = np.flatnonzero(d2 < md2)
            if hit.size:
                if all(src[q] // 64 == i // 64 for q in hit):
                    conflicts += 1
                continue
        ax[n], ay[n] = cx[i], cy[i]
        out.append((cx[i], cy[i])); src.append(i)
    if stats is not None:
        stats["in_step_conflicts"] = conflicts
        stats["values"] = eig[np.array([int(p[1]) for p in out], int), np.array([int(p[0]) for p in out], int)] if out else np.zeros(0, np.float32)
    return np.array(out, np.float32).reshape(-1, 2)


def tie_cut_max_ns(oracle, img, min_dist, rule, upto=48):
    """the max_n in [1, upto] for which the address-ascending order returns another SET of corners: the cut falls inside a group of equal values"""
    good = []
    full_a = np_gftt(oracle, img, upto, 0.01, min_dist, rule=rule)
    full_b = np_gftt(oracle, img, upto, 0.01, min_dist, rule=rule, reverse_ties=True)
    for n in range(1, upto + 1):
        a = {tuple(p) for p in full_a[:n]}
        b = {tuple(p) for p in full_b[:n]}
        if a != b:
            good.append(n)
    return good


def discs_per_tile(pts, w, h, radius):
    """the cull test of gftt_tile_body: disc centres (rounded half to even) whose bounding square reaches the tile -> count per tile [rows, cols]"""
    cx, cy = np.rint(pts[:, 0]).astype(int), np.rint(pts[:, 1]).astype(int)
    ny, nx = (h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W
    out = np.zeros((ny, nx), int)
    for ty in range(ny):
        for tx in range(nx):
            x0, y0 = tx * TILE_W, ty * TILE_H
            out[ty, tx] = int(((cx + radius >= x0) & (cx - radius < x0 + TILE_W) & (cy + radius >= y0) & (cy - radius < y0 + TILE_H)).sum())
    return out


# ---------------------------------------------------------------- sequences for the whole-frame entries
def flat_sequence(value, cols=90, frames=3, seed=9):
    """three stereo frames, the left `cols` columns saturated (a sky that does not move), the rest a texture that drifts 1 px per frame, disparity 2"""
    tex = tex_u8(H + 8, W + 16, seed)
    out = []
    for k in range(frames):
        l = tex[2:2 + H, 4 + k:4 + k + W].copy()
        r = tex[2:2 + H, 6 + k:6 + k + W].copy()
        l[:, :cols] = value; r[:, :cols] = value
        out.append((np.ascontiguousarray(l), np.ascontiguousarray(r)))
    return out


def crowded_sequence(seed=3, frames=7, rate=0.87):
    """a texture that contracts about the image centre by `rate` per frame (disparity 1): the tracked points move together while the detector fills the gaps, so the
    discs on a tile, the feature count and the number of features that share a pixel all grow from frame to frame"""
    m = 80
    t = synth.texture(H + 2 * m, W + 2 * m, seed, 1.0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    out = []
    for k in range(frames):
        s = rate ** k
        X, Y = cx + (xx - cx) / s + m, cy + (yy - cy) / s + m
        out.append((synth.sample(t, X, Y), synth.sample(t, X + 1.0, Y)))
    return out


def order_keys(pts):
    """the sort key of lk_order_kernel: the pixel a point truncates to, row major"""
    return (np.clip(pts[:, 1].astype(int), 0, 8191) << 13) | np.clip(pts[:, 0].astype(int), 0, 8191)


CROWD_MAX_CNT, CROWD_MIN_DIST = 1024, 2          # DV_MAX_FEATS: the most points a tracker holds and lk_order_kernel ranks


# ---------------------------------------------------------------- tracker cases
class LkCase:
    """a, b: the image pair; pts: previous points; inits: initial flows (name -> array) used by the calls with an initial flow; levels: the max_level values run"""

    def __init__(self, a, b, pts, inits=None, levels=(3, 1, 0)):
        self.a, self.b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        self.pts = np.ascontiguousarray(pts, np.float32)
        self.inits = inits if inits is not None else {"init": (self.pts + np.float32([1.5, -0.75])).astype(np.float32)}
        self.levels = levels


def shifted_pair(h, w, dx, dy, seed=3, tex=None, margin=24):
    """a, b = a moved by (dx, dy): b(x, y) = a(x - dx, y - dy), both sampled from one larger float texture"""
    t = synth.texture(h + 2 * margin, w + 2 * margin, seed) if tex is None else tex
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return synth.sample(t, xx + margin, yy + margin), synth.sample(t, xx + margin - dx, yy + margin - dy)


def lattice(w, h, n=5, lo=0.0, hi=None):
    xs = np.linspace(lo, (w - 1 - lo) if hi is None else hi, n)
    ys = np.linspace(lo, (h - 1 - lo) if hi is None else hi, n)
    return np.array([[x, y] for y in ys for x in xs], np.float32)


def pyramid_sizes(w, h, max_level=3):
    s = [(w, h)]
    for _ in range(max_level):
        w, h = (w + 1) // 2, (h + 1) // 2
        s.append((w, h))
    return s


def tiny_case(w, h, seed=4):
    a, b = shifted_pair(h, w, 0.8, -0.6, seed, margin=8)
    corners = np.array([[0.4, 0.4], [w - 1 - 0.4, 0.4], [0.4, h - 1 - 0.4], [w - 1 - 0.4, h - 1 - 0.4],
                        [-0.4, -0.4], [w - 1 + 0.4, -0.4], [-0.4, h - 1 + 0.4], [w - 1 + 0.4, h - 1 + 0.4]], np.float32)
    return LkCase(a, b, np.vstack([lattice(w, h, 5), corners]))


def edge_case():
    """points 0 .. 12 px from each edge of a 96 x 128 (h x w) image: the window leaves the image at the coarse levels, and at level 0 for the nearest"""
    h, w = 96, 128
    a, b = shifted_pair(h, w, 2.3, -1.4, 6)
    pts = []
    for d in (0, 1.5, 3, 5, 7.25, 9, 10.5, 12):
        for t in (0.13, 0.37, 0.62, 0.88):
            pts += [[d, t * (h - 1)], [w - 1 - d, t * (h - 1)], [t * (w - 1), d], [t * (w - 1), h - 1 - d]]
    return LkCase(a, b, np.array(pts, np.float32))


def drift_case(repetitive):
    """true shift 3 px, initial flows wrong by 6, 9 and 12 px towards each of the four directions; max_level 0 and 1"""
    h, w = 96, 128
    if repetitive:
        t = np.tile(synth.texture(16, 32, 5), (9, 6)).astype(np.float32)
        a, b = shifted_pair(h, w, 3.0, 0.0, tex=t, margin=16)
    else:
        a, b = shifted_pair(h, w, 3.0, 0.0, 8)
    pts = lattice(w, h, 6, lo=20.0)
    inits = {}
    for e in (6, 9, 12):
        for name, (ux, uy) in (("r", (1, 0)), ("l", (-1, 0)), ("d", (0, 1)), ("u", (0, -1))):
            inits[f"{name}{e}"] = (pts + np.float32([3.0 + e * ux, e * uy])).astype(np.float32)
    return LkCase(a, b, pts, inits, levels=(1, 0))


def reject_case(kind):
    """pairs on which the minimum-eigenvalue / determinant tests reject part of the points: vertical stripes beside texture, a half-flat frame, a 0 / 255 image"""
    h, w = 96, 128
    if kind == "stripes":
        base = synth.texture(h + 48, w + 48, 11)
        xx = np.arange(w + 48, dtype=np.float64)
        base[:, : (w + 48) // 2] = (0.5 + 0.4 * np.sin(xx[: (w + 48) // 2] / 2.5))[None, :]
        a, b = shifted_pair(h, w, 1.0, 0.0, tex=base.astype(np.float32))
    elif kind == "half_flat":
        a, b = shifted_pair(h, w, 1.0, 0.5, 12)
        a[:, : w // 2] = 255; b[:, : w // 2] = 255
    else:
        t = np.where(synth.texture(h + 48, w + 48, 13, 6.0) > 0.5, 1.0, 0.0).astype(np.float32)
        a, b = shifted_pair(h, w, 1.0, 0.0, tex=t)
        a, b = [np.ascontiguousarray(np.where(i > 127, 255, 0).astype(np.uint8)) for i in (a, b)]
    return LkCase(a, b, lattice(w, h, 8, lo=14.0))


def no_convergence_case(kind):
    h, w = 96, 128
    m = 40
    t = synth.texture(h + 2 * m, w + 2 * m, 15)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = synth.sample(t, xx + m, yy + m)
    if kind == "rotated":
        th, s, cx, cy = np.deg2rad(10.0), 1.1, (w - 1) / 2, (h - 1) / 2
        c, sn = np.cos(th) * s, np.sin(th) * s
        b = synth.sample(t, c * (xx - cx) - sn * (yy - cy) + cx + m, sn * (xx - cx) + c * (yy - cy) + cy + m)
    else:
        b = np.random.default_rng(29).integers(0, 256, (h, w), dtype=np.uint8)
    return LkCase(a, np.ascontiguousarray(b), lattice(w, h, 8, lo=6.0))


def point_set_pair():
    return shifted_pair(96, 128, 1.7, -0.9, 19)


def point_sets():
    """name -> points on point_set_pair(): the counts around a wavefront, the tracker's capacity (the operator entries check no upper bound: DV_MAX_FEATS is what
    a tracker submits), every point three times, rows descending"""
    rng = np.random.default_rng(23)
    big = rng.uniform([2, 2], [125, 93], (1024, 2)).astype(np.float32)
    d = {f"n{n}": big[:n].copy() for n in (1, 63, 64, 65, 1024)}
    d["triple"] = np.repeat(big[:21], 3, axis=0)
    by_row = big[:96]
    d["rows_desc"] = by_row[np.argsort(-by_row[:, 1], kind="stable")]
    return d


def lk_cases():
    d = {"tiny_33x47": tiny_case(33, 47), "tiny_20x24": tiny_case(20, 24), "tiny_21x21": tiny_case(21, 21), "edges": edge_case(),
         "drift": drift_case(False), "drift_tiled": drift_case(True),
         "stripes": reject_case("stripes"), "half_flat": reject_case("half_flat"), "binary": reject_case("binary"),
         "rotated": no_convergence_case("rotated"), "noise": no_convergence_case("noise")}
    return d


def oracle_lk(oracle, rule, *a, **kw):
    if rule == "cuda":
        kw.pop("eps", None)
        return oracle.lk_cuda(*a, **kw)
    return oracle.lk(*a, **kw)


def oracle_track(oracle, rule, a, b, pts, flow_back):
    return oracle.track_by_lk_gpu(a, b, pts, flow_back) if rule == "cuda" else oracle.track_by_lk(a, b, pts, flow_back, 0.5)
