"""The project's own definition of the ReID extractor (dv_reid_*): the crop / resize rule in numpy integers and the network in CPU torch, float32 or float64.
Written from mot/extractor.cpp:31-52, mot/reid_net.cpp:17-135, mot/mot_parameter.h:26-30 and OpenCV's 8-bit INTER_LINEAR as include/dvins.h states it (unpinned).
Nothing here touches the library."""
import numpy as np

BLOCKS = [(64, 64, 0), (64, 64, 0), (64, 128, 1), (128, 128, 0), (128, 256, 1), (256, 256, 0), (256, 512, 1), (512, 512, 0)]
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
EPS = 1e-5


def tensors():
    """(name, shape) of every tensor in the order ReIdNetImpl::load_form reads the flat file"""
    def bn(name, c):
        return [(f"{name}.{f}", (c,)) for f in ("weight", "bias", "running_mean", "running_var")]
    out = [("conv1.0.weight", (64, 3, 3, 3)), ("conv1.0.bias", (64,))] + bn("conv1.1", 64)
    for i, (ci, co, down) in enumerate(BLOCKS):
        out += [(f"conv2.{i}.conv.0.weight", (co, ci, 3, 3))] + bn(f"conv2.{i}.conv.1", co)
        out += [(f"conv2.{i}.conv.3.weight", (co, co, 3, 3))] + bn(f"conv2.{i}.conv.4", co)
        if down:
            out += [(f"conv2.{i}.downsample.0.weight", (co, ci, 1, 1))] + bn(f"conv2.{i}.downsample.1", co)
    return out


def n_floats():
    return sum(int(np.prod(s)) for _, s in tensors())


def split(flat):
    """the flat float32 file -> {name: array}"""
    flat = np.asarray(flat, np.float32).reshape(-1)
    assert flat.size == n_floats()
    out, off = {}, 0
    for name, shape in tensors():
        k = int(np.prod(shape))
        out[name] = flat[off: off + k].reshape(shape)
        off += k
    return out


def size_ok(in_w, in_h):
    def last(n):
        for _ in range(4):
            n = -(-n // 2)
        return n
    return 0 < in_w <= 64 and 0 < in_h <= 128 and last(in_w) == 4 and last(in_h) == 8


# ---- crops ----
def round_rect(r):
    """Rect2f -> Rect: cvRound per field, half to even.  None where the crop is empty or leaves the image is decided by the caller"""
    return [int(v) for v in np.rint(np.asarray(r, np.float32))]


def rect_ok(q, img_w, img_h):
    x, y, w, h = q
    return x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= img_w and y + h <= img_h


def coef(src, dst, vertical):
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (src / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if not vertical:
        lo, hi = s < 0, s >= src - 1
        s = np.where(lo, 0, np.where(hi, src - 1, s))
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
        i0, i1 = s, np.minimum(s + 1, src - 1)
    else:
        i0, i1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return i0, i1, c0, c1


def resize_u8(crop, dw, dh):
    """cv::resize(crop, {dw, dh}) of an (h, w, c) uint8 array with INTER_LINEAR -> (dh, dw, c) uint8"""
    h, w = crop.shape[:2]
    v = crop.astype(np.int64)
    if w == 2 * dw and h == 2 * dh:      # both scales exactly 2: the fast area path
        return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1 = coef(w, dw, False)
    y0, y1, b0, b1 = coef(h, dh, True)
    S = v[:, x0] * a0[None, :, None] + v[:, x1] * a1[None, :, None]      # (h, dw, c)
    out = (((b0[:, None, None] * (S[y0] >> 4)) >> 16) + ((b1[:, None, None] * (S[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def prepare(img, rects, in_w=64, in_h=128):
    """(H, W, 3) uint8 BGR image, [n, 4] rectangles -> [n, 3, in_h, in_w] float32 as Extractor::extract hands it to the net; raises ValueError on a bad rectangle"""
    H, W = img.shape[:2]
    out = np.zeros((len(rects), 3, in_h, in_w), np.float32)
    for i, r in enumerate(rects):
        q = round_rect(r)
        if not rect_ok(q, W, H):
            raise ValueError(f"rectangle {i} is empty or leaves the image")
        x, y, w, h = q
        u = resize_u8(img[y: y + h, x: x + w], in_w, in_h)[:, :, ::-1]      # the channel swap
        f = u.astype(np.float32) * (np.float32(1) / np.float32(255))
        out[i] = ((f - MEAN) / STD).astype(np.float32).transpose(2, 0, 1)
    return out


# ---- the network ----
def layer(x, weight, scale, shift, residual=None, stride=1, relu=True, dtype=None):
    """the operator dv_reid_layer computes, in torch on the CPU"""
    import torch
    import torch.nn.functional as F
    dt = dtype or torch.float64
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    y = F.conv2d(t(x), t(weight), stride=stride, padding=1 if weight.shape[-1] == 3 else 0)
    y = y * t(scale).view(1, -1, 1, 1) + t(shift).view(1, -1, 1, 1)
    if residual is not None:
        y = y + t(residual)
    return (torch.relu(y) if relu else y).numpy()


def forward(flat, x, dtype=None):
    """ReIdNetImpl::forward on a prepared [n, 3, h, w] tensor -> [n, 512], batch-norm in its eval form as torch evaluates it"""
    import torch
    import torch.nn.functional as F
    dt = dtype or torch.float64
    P = {k: torch.from_numpy(v.copy()).to(dt) for k, v in split(flat).items()}
    bn = lambda t, name: F.batch_norm(t, P[name + ".running_mean"], P[name + ".running_var"], P[name + ".weight"], P[name + ".bias"], False, 0.0, EPS)
    with torch.no_grad():
        t = torch.from_numpy(np.asarray(x)).to(dt)
        t = torch.relu(bn(F.conv2d(t, P["conv1.0.weight"], P["conv1.0.bias"], stride=1, padding=1), "conv1.1"))
        t = F.max_pool2d(t, 3, 2, 1)
        for i, (ci, co, down) in enumerate(BLOCKS):
            p = f"conv2.{i}."
            y = torch.relu(bn(F.conv2d(t, P[p + "conv.0.weight"], stride=2 if down else 1, padding=1), p + "conv.1"))
            y = bn(F.conv2d(y, P[p + "conv.3.weight"], stride=1, padding=1), p + "conv.4")
            if down:
                t = bn(F.conv2d(t, P[p + "downsample.0.weight"], stride=2), p + "downsample.1")
            t = torch.relu(t + y)
        t = F.avg_pool2d(t, (8, 4), 1)
        t = t.view(t.size(0), -1)
        t = t / t.norm(2, 1, True)
    return t.numpy()
