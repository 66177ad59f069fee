"""The stereo matcher's specification (include/dvins.h, dv_stereo_sgm_*) in numpy with integer dtypes — the reference the device is compared with bit for bit —
and a second, deliberately naive restatement in scalar loops straight from the formulas.  Both return the same dict of intermediates:
codes_l / codes_r (uint64 [h, w]), S (uint16 [h, w, D]), dstar / dr (int16 [h, w]: the two winners before any validity test), out (float32 [h, w])."""
import numpy as np

RX, RY = 4, 3                      # census window 9 x 7
OOB_COST = 64                      # C(x, y, d) for x - d < 0
BIG = 1 << 14                      # a term left out of a minimum
DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]      # (dx, dy): p - r is the predecessor of p


def params(n_disp=64, p1=10, p2=120, uniqueness=5, lr_max_diff=1):
    return dict(n_disp=int(n_disp), p1=int(p1), p2=int(p2), uniqueness=int(uniqueness), lr_max_diff=int(lr_max_diff))


def popcount64(a):
    a = np.ascontiguousarray(a, np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(-1).astype(np.int32)


def floor_div(a, b):
    """floor(a / b) for b > 0 in Python integers"""
    return a // b


# ---------------------------------------------------------------- vectorised ----
def census(img):
    """row-major over the window, centre skipped, earlier positions in higher bits; replicate border"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    pad = np.pad(img, ((RY, RY), (RX, RX)), mode="edge")
    code = np.zeros((h, w), np.uint64)
    for dy in range(2 * RY + 1):
        for dx in range(2 * RX + 1):
            if dy == RY and dx == RX:
                continue
            code = (code << np.uint64(1)) | (pad[dy:dy + h, dx:dx + w] < img).astype(np.uint64)
    return code


def cost_volume(cl, cr, D):
    h, w = cl.shape
    C = np.full((h, w, D), OOB_COST, np.int32)
    for d in range(min(D, w)):
        C[:, d:, d] = popcount64(cl[:, d:] ^ cr[:, :w - d])
    return C


def _step(Cp, prev, has_prev, p1, p2):
    """Cp, prev [n, D]; has_prev [n]: one step of n independent paths"""
    m = prev.min(1, keepdims=True)
    lo = np.full_like(prev, BIG); lo[:, 1:] = prev[:, :-1] + p1
    hi = np.full_like(prev, BIG); hi[:, :-1] = prev[:, 1:] + p1
    L = Cp + np.minimum(np.minimum(prev, lo), np.minimum(hi, m + p2)) - m
    return np.where(has_prev[:, None], L, Cp)


def _paths(C, shift, reverse, p1, p2):
    """walks axis 0 of C [a, b, D] (backwards if reverse); the predecessor of (i, j) is (i -+ 1, j - shift)"""
    a, b, D = C.shape
    L = np.zeros_like(C)
    order = range(a - 1, -1, -1) if reverse else range(a)
    prev = None
    for i in order:
        if prev is None:
            L[i] = C[i]
        else:
            sh = np.zeros_like(prev); has = np.zeros(b, bool)
            if shift == 0:
                sh, has = prev, np.ones(b, bool)
            elif shift > 0:
                sh[shift:], has[shift:] = prev[:-shift], True
            else:
                sh[:shift], has[:shift] = prev[-shift:], True
            L[i] = _step(C[i], sh, has, p1, p2)
        prev = L[i]
    return L


def aggregate(C, p1, p2):
    S = np.zeros(C.shape, np.int32)
    for dx, dy in DIRECTIONS:
        if dy == 0:          # horizontal: walk x, vector over y
            S += _paths(C.swapaxes(0, 1), 0, dx < 0, p1, p2).swapaxes(0, 1)
        else:                # vertical and diagonal: walk y, vector over x, the predecessor's x is x - dx
            S += _paths(C, dx, dy < 0, p1, p2)
    assert S.max() < 65536
    return S.astype(np.uint16)


def decide(S, uniqueness, lr_max_diff):
    S = S.astype(np.int32)
    h, w, D = S.shape
    ds = np.arange(D)
    xs = np.arange(w)[None, :]
    dstar = S.argmin(2)                                      # the first minimum: the lowest d
    s0 = np.take_along_axis(S, dstar[..., None], 2)[..., 0]
    other = np.where(np.abs(ds[None, None, :] - dstar[..., None]) > 1, S, 1 << 16).min(2)
    valid = ~(other * (100 - uniqueness) < s0 * 100)
    SR = np.full((h, w, D), 1 << 30, np.int32)                # SR[y, x, d] = S[y, x + d, d]
    for d in range(min(D, w)):
        SR[:, :w - d, d] = S[:, d:, d]
    dr = SR.argmin(2)
    valid &= dstar <= xs
    if lr_max_diff >= 0:
        xr = np.clip(xs - dstar, 0, w - 1)
        valid &= np.abs(np.take_along_axis(dr, xr, 1) - dstar) <= lr_max_diff
    sm = np.take_along_axis(S, np.clip(dstar - 1, 0, D - 1)[..., None], 2)[..., 0]
    sp = np.take_along_axis(S, np.clip(dstar + 1, 0, D - 1)[..., None], 2)[..., 0]
    den = np.maximum(sm + sp - 2 * s0, 1)
    sub = (16 * (sm - sp) + den) // (2 * den)                 # numpy's // on integers is the mathematical floor
    d16 = 16 * dstar + np.where((dstar > 0) & (dstar < D - 1), sub, 0)
    out = np.where(valid, d16.astype(np.float32) / np.float32(16), np.float32(0)).astype(np.float32)
    return dstar.astype(np.int16), dr.astype(np.int16), out


def sgm(left, right, n_disp=64, p1=10, p2=120, uniqueness=5, lr_max_diff=1):
    cl, cr = census(left), census(right)
    S = aggregate(cost_volume(cl, cr, n_disp), p1, p2)
    dstar, dr, out = decide(S, uniqueness, lr_max_diff)
    return dict(codes_l=cl, codes_r=cr, S=S, dstar=dstar, dr=dr, out=out)


# ---------------------------------------------------------------- naive ----
def subpixel_naive(d, D, sm, s0, sp):
    if d <= 0 or d >= D - 1:
        return 16 * d
    den = max(sm + sp - 2 * s0, 1)
    return 16 * d + floor_div(16 * (sm - sp) + den, 2 * den)


def sgm_naive(left, right, n_disp=64, p1=10, p2=120, uniqueness=5, lr_max_diff=1):
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    h, w = left.shape
    D = n_disp
    clamp = lambda v, n: min(max(v, 0), n - 1)

    def census_naive(img):
        out = np.zeros((h, w), np.uint64)
        for y in range(h):
            for x in range(w):
                code = 0
                for dy in range(-RY, RY + 1):
                    for dx in range(-RX, RX + 1):
                        if dx == 0 and dy == 0:
                            continue
                        code = (code << 1) | int(img[clamp(y + dy, h), clamp(x + dx, w)] < img[y, x])
                out[y, x] = code
        return out

    cl, cr = census_naive(left), census_naive(right)
    C = [[[bin(int(cl[y, x]) ^ int(cr[y, x - d])).count("1") if x - d >= 0 else OOB_COST for d in range(D)] for x in range(w)] for y in range(h)]
    S = np.zeros((h, w, D), np.int64)
    for dx, dy in DIRECTIONS:
        L = {}
        for y in (range(h) if dy >= 0 else range(h - 1, -1, -1)):
            for x in (range(w) if dx >= 0 else range(w - 1, -1, -1)):
                px, py = x - dx, y - dy
                if not (0 <= px < w and 0 <= py < h):
                    L[(x, y)] = list(C[y][x])
                    continue
                P = L[(px, py)]
                m = min(P)
                cur = []
                for d in range(D):
                    terms = [P[d], m + p2]
                    if d - 1 >= 0:
                        terms.append(P[d - 1] + p1)
                    if d + 1 < D:
                        terms.append(P[d + 1] + p1)
                    cur.append(C[y][x][d] + min(terms) - m)
                L[(x, y)] = cur
        for (x, y), v in L.items():
            S[y, x] += v
    dstar, dr, out = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16), np.zeros((h, w), np.float32)

    def argmin_low(vals):          # (value, d) order: ties take the lowest d
        return min((v, d) for d, v in vals)[1]

    for y in range(h):
        for x in range(w):
            dstar[y, x] = argmin_low([(d, int(S[y, x, d])) for d in range(D)])
            dr[y, x] = argmin_low([(d, int(S[y, x + d, d])) for d in range(D) if x + d < w])
    for y in range(h):
        for x in range(w):
            d0 = int(dstar[y, x]); s0 = int(S[y, x, d0])
            bad = any(int(S[y, x, d]) * (100 - uniqueness) < s0 * 100 for d in range(D) if abs(d - d0) > 1)
            if d0 > x:
                bad = True
            elif lr_max_diff >= 0 and abs(int(dr[y, x - d0]) - d0) > lr_max_diff:
                bad = True
            if not bad:
                d16 = subpixel_naive(d0, D, int(S[y, x, d0 - 1]) if d0 > 0 else 0, s0, int(S[y, x, d0 + 1]) if d0 < D - 1 else 0)
                out[y, x] = np.float32(d16) / np.float32(16)
    return dict(codes_l=cl, codes_r=cr, S=S.astype(np.uint16), dstar=dstar, dr=dr, out=out)


# ---------------------------------------------------------------- inputs shared by the CPU and the GPU tests ----
def images(kind, w, h, seed=0, shift=5):
    """-> (left, right) uint8 [h, w]"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w), 97, np.uint8), np.full((h, w), 97, np.uint8)
    if kind == "checker":          # two values; the right image is the left one moved by one cell
        yy, xx = np.mgrid[0:h, 0:w]
        return (np.where(((xx // 3) + (yy // 2)) % 2, 200, 40).astype(np.uint8), np.where((((xx + 3) // 3) + (yy // 2)) % 2, 200, 40).astype(np.uint8))
    if kind == "shifted":          # right(x) = left(x + shift)
        tex = rng.integers(0, 256, (h, w + shift), dtype=np.uint8)
        return np.ascontiguousarray(tex[:, :w]), np.ascontiguousarray(tex[:, shift:shift + w])
    if kind == "bright_edges":     # a bright left column and a bright top row over a random ground
        l, r = rng.integers(0, 128, (h, w), dtype=np.uint8), rng.integers(0, 128, (h, w), dtype=np.uint8)
        for im in (l, r):
            im[:, 0] = 255; im[0, :] = 255
        return l, r
    raise ValueError(kind)
