"""The ReID extractor's yardstick and host rules (CPU): tests/reid_ref.py against a second statement of the resize written differently, the size rule, the float count and
the file order, dv_reid_check's refusals through ctypes, the shim's overloads compiling, and csrc/reid_host.h as a stand-alone program under AddressSanitizer + UBSan.
The yardstick tests exercise tests/reid_ref.py alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import reid_cases as rc
from tests import reid_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def rne(v):
    """round half to even on a Python float"""
    return int(round(v))


def resize_loop(crop, dw, dh):
    """the rule once more, pixel by pixel in Python ints and struct-rounded floats"""
    h, w, cn = crop.shape
    out = np.zeros((dh, dw, cn), np.uint8)
    for dy in range(dh):
        fy = f32((dy + 0.5) * (h / float(dh)) - 0.5)
        sy = int(np.floor(fy))
        fy = f32(fy - sy)
        y0, y1 = min(max(sy, 0), h - 1), min(max(sy + 1, 0), h - 1)
        b0, b1 = rne(f32(f32(1.0 - fy) * 2048.0)), rne(f32(fy * 2048.0))
        for dx in range(dw):
            fx = f32((dx + 0.5) * (w / float(dw)) - 0.5)
            sx = int(np.floor(fx))
            fx = f32(fx - sx)
            if sx < 0:
                sx, fx = 0, 0.0
            if sx >= w - 1:
                sx, fx = w - 1, 0.0
            x1 = min(sx + 1, w - 1)
            a0, a1 = rne(f32(f32(1.0 - fx) * 2048.0)), rne(f32(fx * 2048.0))
            for c in range(cn):
                S0 = int(crop[y0, sx, c]) * a0 + int(crop[y0, x1, c]) * a1
                S1 = int(crop[y1, sx, c]) * a0 + int(crop[y1, x1, c]) * a1
                out[dy, dx, c] = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
    return out


@pytest.mark.parametrize("src,dst", [((7, 5), (4, 3)), ((3, 2), (8, 16))])
def test_resize_agrees_with_the_pixel_loop(src, dst):
    crop = np.random.default_rng(5).integers(0, 256, (src[1], src[0], 3), dtype=np.uint8)
    a, b = rr.resize_u8(crop, dst[0], dst[1]), resize_loop(crop, dst[0], dst[1])
    assert a.shape == b.shape == (dst[1], dst[0], 3) and np.array_equal(a, b)
    assert len(np.unique(a)) > 4


def test_exact_half_takes_the_area_rule():
    crop = np.random.default_rng(6).integers(0, 256, (12, 8, 3), dtype=np.uint8)
    v = crop.astype(int)
    area = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
    assert np.array_equal(rr.resize_u8(crop, 4, 6), area)
    assert np.array_equal(rr.resize_u8(crop[:11], 4, 6), resize_loop(crop[:11], 4, 6))      # one scale off 2: bilinear again


def test_round_half_even_of_rectangles():
    assert rr.round_rect([2.5, 3.5, 10.5, 11.5]) == [2, 4, 10, 12] and rr.round_rect([0.5, 0.5, 69.5, 40.5]) == [0, 0, 70, 40] and rr.round_rect([1.5, 2.5, 3.5, 4.5]) == [2, 2, 4, 4]
    assert rr.rect_ok([0, 0, 70, 40], 70, 41) and not rr.rect_ok([1, 0, 70, 40], 70, 41) and not rr.rect_ok([0, 0, 0, 40], 70, 41)


def test_prepare_swaps_channels_and_refuses_bad_rectangles():
    img = rc.image(70, 41, pad=5)
    x = rr.prepare(img, np.array([[3.5, 2.5, 64, 38]], np.float32), 64, 128)      # rounds to x = 4, y = 2
    assert x.shape == (1, 3, 128, 64) and x.dtype == np.float32
    u = rr.resize_u8(img[2:40, 4:68], 64, 128)
    want = (u[5, 7, 0].astype(np.float32) * (np.float32(1) / np.float32(255)) - np.float32(0.406)) / np.float32(0.225)      # the image's B is tensor channel 2
    assert x[0, 2, 5, 7] == want
    for bad in ([[0, 0, 71, 10]], [[-1, 0, 10, 10]], [[5, 5, 0.4, 10]], [[60, 30, 10, 12]]):
        with pytest.raises(ValueError):
            rr.prepare(img, np.array(bad, np.float32))


def test_sizes_follow_the_ceil_chain():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import DV_REID_N_FLOATS, reid_check
    for w in (1, 48, 49, 57, 64, 65):
        for h in (112, 113, 121, 128, 129):
            ok = 49 <= w <= 64 and 113 <= h <= 128
            assert rr.size_ok(w, h) == ok
            if ok:
                reid_check(DV_REID_N_FLOATS, w, h)
            else:
                with pytest.raises(DvinsError, match="input size"):
                    reid_check(DV_REID_N_FLOATS, w, h)


def test_float_count_and_file_order(tmp_path):
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import DV_REID_N_FLOATS, reid_check
    count = 64 * 27 + 64 + 4 * 64
    for ci, co, down in rr.BLOCKS:
        count += co * ci * 9 + 4 * co + co * co * 9 + 4 * co + (co * ci + 4 * co if down else 0)
    assert count == rr.n_floats() == DV_REID_N_FLOATS == 11178496
    path = rc.write_file(str(tmp_path / "reid.bin"), seed=3)
    assert os.path.getsize(path) == 4 * count
    # a loader written here: sequential reads in the reference's order
    P = rr.split(rc.weights(3))
    with open(path, "rb") as fh:
        take = lambda *shape: np.frombuffer(fh.read(4 * int(np.prod(shape))), np.float32).reshape(shape)
        assert np.array_equal(take(64, 3, 3, 3), P["conv1.0.weight"]) and np.array_equal(take(64), P["conv1.0.bias"])
        for f in ("weight", "bias", "running_mean", "running_var"):
            assert np.array_equal(take(64), P["conv1.1." + f])
        for i, (ci, co, down) in enumerate(rr.BLOCKS):
            for conv, bn, shape in [("conv.0", "conv.1", (co, ci, 3, 3)), ("conv.3", "conv.4", (co, co, 3, 3))] + ([("downsample.0", "downsample.1", (co, ci, 1, 1))] if down else []):
                assert np.array_equal(take(*shape), P[f"conv2.{i}.{conv}.weight"])
                for f in ("weight", "bias", "running_mean", "running_var"):
                    assert np.array_equal(take(co), P[f"conv2.{i}.{bn}.{f}"])
        assert fh.read() == b""
    v = P["conv2.7.conv.4.running_var"]
    assert v.min() >= 0.5 and v.max() <= 1.5 and abs(float(P["conv2.7.conv.3.weight"].std()) - np.sqrt(2 / 4608)) < 1e-4
    for bad in (count - 1, count + 1, 0):
        with pytest.raises(DvinsError, match="11178496"):
            reid_check(bad)


def test_reference_float32_is_close_to_float64():
    """the yardstick's own precision: float32 against float64 on three crops, the figure the 4 x rule of tests/test_reid.py scales"""
    import torch
    img = rc.image(70, 41)
    x = rr.prepare(img, rc.rects(3, 70, 41), 64, 128)
    e64, e32 = rr.forward(rc.weights(0), x, torch.float64), rr.forward(rc.weights(0), x, torch.float32)
    assert np.abs(np.linalg.norm(e64, axis=1) - 1).max() < 1e-12
    assert 0 < np.abs(e32 - e64).max() < 1e-6


def test_reid_host_under_the_sanitizers():
    host = os.path.join(ROOT, "tests", "host")
    subprocess.run(["make", "-s", "-C", host, "-f", "reid.mk", "reid"], check=True, capture_output=True, text=True)
    r = subprocess.run([os.path.join(host, "_build", "reid_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "reid_host ok" in r.stdout, r.stdout + r.stderr


def test_pipeline_refusals_of_the_device_form():
    from dynamic_vins_amd.pipeline import DynamicPipeline
    with pytest.raises(ValueError, match=r"params\['reid_weights'\]"):
        DynamicPipeline(None, mask_stack=True, mot=("device", dict(n_init=1)))
    with pytest.raises(ValueError, match="feat_dim 512, the extractor's width"):
        DynamicPipeline(None, mask_stack=True, mot=("device", dict(reid_weights="x", feat_dim=16)))
    with pytest.raises(ValueError, match="mot must be"):
        DynamicPipeline(None, mask_stack=True, mot=("host", dict(reid_weights="x")))      # only the string "device" names the device form


def test_reid_image_takes_the_colour_image_as_it_is_and_replicates_gray():
    """DynamicPipeline.reid_image on stand-in sequences: seq.color0[k] is handed on untouched (same memory, so channel order and row stride are the sequence's), and a
    sequence without colour gives the left gray image in all three channels, packed"""
    import torch
    from types import SimpleNamespace
    from dynamic_vins_amd.pipeline import DynamicPipeline
    h, w = 5, 7
    gray = [(torch.arange(h * w, dtype=torch.uint8).reshape(h, w) + k, None) for k in range(2)]
    colour = [torch.stack([torch.full((h, w), 10 * k + c, dtype=torch.uint8) for c in (1, 2, 3)], dim=-1) for k in range(2)]      # B, G, R = 1, 2, 3 (+ 10 k)
    p = DynamicPipeline.__new__(DynamicPipeline)
    p.seq, p._reid_img = SimpleNamespace(frames=gray, color0=colour), (None, None)
    for k in (1, 0, 0):
        img = p.reid_image(k)
        assert img.data_ptr() == colour[k].data_ptr() and tuple(img.shape) == (h, w, 3) and img.stride() == (3 * w, 3, 1)
        assert img[2, 3].tolist() == [10 * k + 1, 10 * k + 2, 10 * k + 3]
    p.seq, p._reid_img = SimpleNamespace(frames=gray), (None, None)
    for k in (0, 1):
        img = p.reid_image(k)
        assert tuple(img.shape) == (h, w, 3) and img.stride() == (3 * w, 3, 1) and img.dtype == torch.uint8
        assert all(torch.equal(img[:, :, c], gray[k][0]) for c in range(3))
