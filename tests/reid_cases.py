"""Seeded inputs for the ReID extractor's tests: a weight file in the reference's order (nothing of 45 MB is committed), images and rectangles.
Conv weights N(0, 2 / (k^2 c_in)), batch-norm weight in [0.75, 1.25], variance in [0.5, 1.5], batch-norm mean and bias and conv1's bias N(0, 0.1^2)."""
import functools

import numpy as np

from tests import reid_ref as rr


@functools.lru_cache(maxsize=2)
def weights(seed=0):
    """the flat float32 file of ReIdNetImpl::load_form as an array"""
    rng = np.random.default_rng(seed)
    parts = []
    for name, shape in rr.tensors():
        n = int(np.prod(shape))
        if len(shape) == 4:
            v = rng.standard_normal(n, np.float32) * np.float32(np.sqrt(2.0 / (shape[1] * shape[2] * shape[3])))
        elif name.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, n)
        elif name.endswith(".weight"):
            v = rng.uniform(0.75, 1.25, n)
        else:      # conv1's bias, batch-norm bias and running_mean
            v = rng.standard_normal(n) * 0.1
        parts.append(np.asarray(v, np.float32))
    flat = np.concatenate(parts)
    flat.setflags(write=False)
    return flat


def write_file(path, seed=0):
    weights(seed).tofile(path)
    return path


def image(w, h, seed=1, pad=0):
    """an (h, w, 3) uint8 view with `pad` unused bytes behind every row (smooth blobs plus noise, so that neighbours differ and interpolation matters)"""
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, (h, 3 * w + pad), dtype=np.uint8)
    img = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (buf.strides[0], 3, 1))
    yy, xx = np.mgrid[0:h, 0:w]
    for c in range(3):
        img[:, :, c] = (img[:, :, c] // 4 + 96 + 90 * np.sin(xx / (5.0 + c) + c) * np.cos(yy / (7.0 - c))).clip(0, 255).astype(np.uint8)
    return img


def rects(n, img_w, img_h, seed=2, min_w=6, min_h=10):
    """n float32 rectangles that stay inside the image after rounding"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 4), np.float32)
    for i in range(n):
        w = rng.uniform(min_w, img_w * 0.6)
        h = rng.uniform(min_h, img_h * 0.9)
        out[i] = (rng.uniform(0, img_w - w - 1), rng.uniform(0, img_h - h - 1), w, h)
    return out
