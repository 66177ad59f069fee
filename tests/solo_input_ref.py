"""The detector's input stage restated in numpy: Pipeline::ImageToTensor + Pipeline::ProcessInput (det2d/pipeline.cpp:370-387,204-232) by the formulas of include/dvins.h
— channel swap, (v - mean) / std in float32, upsample_bilinear2d's float32 index and weight rule with align_corners = true, zero padding — with float32 weights and the
interpolation sum evaluated in float64.  The bar the device (and torch itself) must keep to this restatement is derived here, not measured."""
import numpy as np

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)      # det2d_parameter.h:24-25, RGB order

# |device - restatement| <= BAR, absolute: a derivation, not a measurement.  With the default mean / std every operand's magnitude is <= (255 - 103.53) / 57.375 = 2.64,
# so one float32 rounding costs at most half an ulp of [2, 4), 1.2e-7.  The weights are in [0, 1] and each pair sums to 1, so no rounding error is amplified on its way
# through lh0 (lw0 a + lw1 b) + lh1 (lw0 c + lw1 d); a value passes through at most seven roundings (product, inner sum, outer product, outer sum, on both branches) plus
# the one of 1 - l1: under 16 x 1.2e-7 = 2e-6.  The restatement shares the float32 normalised values and weights and adds no rounding of its own beyond float64's.
# The device evaluates the same value as nested differences (csrc/solo_input_host.h): differences up to 5.3 cost 2.4e-7 per rounding, top and bottom carry at most
# 6e-7, the outer step 6e-7 more, and this restatement's rounded 1 - l1 moves ITS value by up to 1.6e-7 per axis: under 1.6e-6, inside the same bar.
BAR = 2e-6

# image (w, h) -> model (w, h): the issue's table, and what each covers
CASES = {
    "pad_rows": ((70, 23), (64, 32)),       # pads above and below; 21 rows rounded up to 22; rect (0, 5, 64, 22)
    "pad_cols": ((23, 70), (64, 32)),       # pads left and right; rect (27, 0, 10, 32): rect_x and rect_w off a multiple of 4
    "odd_width": ((71, 23), (66, 34)),      # model width not a multiple of 4: every second plane row starts off 16 bytes
    "upsample": ((30, 30), (64, 32)),
    "identity": ((64, 32), (64, 32)),
}
RECTS = {"pad_rows": (0, 5, 64, 22), "pad_cols": (27, 0, 10, 32), "odd_width": (0, 6, 66, 22), "upsample": (16, 0, 32, 32), "identity": (0, 0, 64, 32)}


def image(w, h, seed=0, stride=None, lead=0):
    """random bytes as an (h, w, 3) view with `stride` bytes per row, `lead` bytes into its buffer -> (flat buffer, view)"""
    stride = 3 * w if stride is None else stride
    rng = np.random.default_rng(seed)
    pixels = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)                 # the same pixels whatever the layout; the bytes between the rows are random too
    flat = rng.integers(0, 256, lead + stride * h + 16, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[lead:], (h, w, 3), (stride, 3, 1))
    view[:] = pixels
    return flat, view


def rect(model_w, model_h, img_w, img_h):
    """Pipeline::GetXYWHS (det2d/pipeline.cpp:23-48)"""
    r_w, r_h = np.float32(model_w) / np.float32(img_w), np.float32(model_h) / np.float32(img_h)
    if r_h > r_w:
        w, h = model_w, int(np.float32(r_w * np.float32(img_h)))
        h += h % 2
        return 0, (model_h - h) // 2, w, h
    w, h = int(np.float32(r_h * np.float32(img_w))), model_h
    w += w % 2
    return (model_w - w) // 2, 0, w, h


def axis(n_in, n_out):
    """per destination index: i0, i1, l0, l1 (float32) of an axis of n_in samples resampled to n_out"""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    r = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(r.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (r - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def normalise(img, mean=MEAN, std=STD):
    """(h, w, 3) uint8 BGR -> [3, h, w] float32, plane c = byte 2 - c: (v - mean[c]) / std[c] in float32, IEEE division"""
    m, s = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(std, np.float32).reshape(3, 1, 1)
    t = np.ascontiguousarray(np.asarray(img)[..., ::-1].transpose(2, 0, 1)).astype(np.float32)
    return ((t - m).astype(np.float32) / s).astype(np.float32)


def solo_input(img, model_w, model_h, mean=MEAN, std=STD):
    """-> dict(out: [3, model_h, model_w] float64 (exactly representable where the stage must be exact), rect, inside: bool [model_h, model_w], exact: bool [model_h, model_w]
    — inside the rectangle with both l1 weights 0 —, source: [3, model_h, model_w] float32, the normalised source value at (i0 row, i0 column) inside the rectangle)"""
    h, w = img.shape[:2]
    x, y, rw, rh = rect(model_w, model_h, w, h)
    n = normalise(img, mean, std)
    y0, y1, h0, h1 = axis(h, rh)
    x0, x1, w0, w1 = axis(w, rw)
    p = n.astype(np.float64)
    H0, H1 = h0.astype(np.float64)[None, :, None], h1.astype(np.float64)[None, :, None]
    W0, W1 = w0.astype(np.float64)[None, None, :], w1.astype(np.float64)[None, None, :]
    top = W0 * p[:, y0][:, :, x0] + W1 * p[:, y0][:, :, x1]
    bot = W0 * p[:, y1][:, :, x0] + W1 * p[:, y1][:, :, x1]
    out = np.zeros((3, model_h, model_w), np.float64)
    out[:, y:y + rh, x:x + rw] = H0 * top + H1 * bot
    inside = np.zeros((model_h, model_w), bool)
    inside[y:y + rh, x:x + rw] = True
    exact = np.zeros((model_h, model_w), bool)
    exact[y:y + rh, x:x + rw] = (h1 == 0)[:, None] & (w1 == 0)[None, :]
    source = np.zeros((3, model_h, model_w), np.float32)
    source[:, y:y + rh, x:x + rw] = n[:, y0][:, :, x0]
    return dict(out=out, rect=(x, y, rw, rh), inside=inside, exact=exact, source=source)


def torch_reference(img, model_w, model_h, mean=MEAN, std=STD):
    """the reference's own lines on CPU torch: ImageToTensor's swap and permute, (t - mean) / std, F.interpolate(bilinear, align_corners=True), the zero cat"""
    import torch
    import torch.nn.functional as F
    h, w = img.shape[:2]
    x, y, rw, rh = rect(model_w, model_h, w, h)
    t = torch.from_numpy(np.ascontiguousarray(img)).to(torch.float32)
    t = torch.cat([t[..., 2].unsqueeze(2), t[..., 1].unsqueeze(2), t[..., 0].unsqueeze(2)], 2).permute(2, 0, 1)
    mean_t = torch.tensor(mean, dtype=torch.float32).reshape(3, 1, 1).expand(3, h, w)
    std_t = torch.tensor(std, dtype=torch.float32).reshape(3, 1, 1).expand(3, h, w)
    t = (t - mean_t) / std_t
    t = F.interpolate(t.unsqueeze(0), size=(rh, rw), mode="bilinear", align_corners=True).squeeze(0)
    r_w, r_h = np.float32(model_w) / np.float32(w), np.float32(model_h) / np.float32(h)
    if r_h > r_w:
        cat_t = torch.zeros(3, (model_h - rh) // 2, model_w)
        t = torch.cat([cat_t, t, cat_t], 1)
    else:
        cat_t = torch.zeros(3, model_h, (model_w - rw) // 2)
        t = torch.cat([cat_t, t, cat_t], 2)
    return t.contiguous().numpy()
