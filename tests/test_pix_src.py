"""The bytes the dynamic front end's two mask kernels write (`-m gpu`): the static-instance unmasking in front of the background tracker (dv_track_unmask_static,
_keys, _planes) and the objects' ROI masks (dv_inst_track_enqueue, _keys, _planes), read back through dv_front_debug_mask and compared byte for byte with the four
membership rules written in numpy: ROI mask byte >= 1; key == id; stack byte not 0 and not 128; stack float > threshold (false for NaN).
Sizes where an index can go wrong, not the workload's: 70 x 23 (the width is no multiple of 4 or 16: the mask pitch is 80, a tight byte stack has every odd row two bytes
off a dword) and 260 x 9 (the width crosses the 256-column workgroup, the height is no multiple of 4).  Flat frames: no corner is found, only the masks matter."""
import numpy as np
import pytest

from tests.test_inst_stack import laid_out, on_memory

pytestmark = pytest.mark.gpu

SIZES = [(70, 23), (260, 9)]
THR = np.float32(0.5)
BIG = 3000000001                                                                  # an id above 2^31: the comparison is unsigned
IDS = [0, 11, BIG, 13, 14, 15, 16]                                                # id 0 is a key like any other
U8_VALUES = np.array([0, 1, 127, 128, 129, 255], np.uint8)
F32_VALUES = np.array([THR, np.nextafter(THR, np.float32(np.inf)), np.nan, np.inf, -np.inf], np.float32)
ROI_VALUES = np.array([0, 1, 128, 255], np.uint8)
# (source, extra row elements, memory kind)
CASES = [("roi", 0, "host"),
         ("key", 0, "host"), ("key", 3, "host"), ("key", 3, "device"), ("key", 0, "pinned"),
         ("u8", 0, "host"), ("u8", 3, "device"), ("u8", 0, "pinned"),
         ("f32", 0, "host"), ("f32", 3, "device"), ("f32", 3, "pinned")]


def rect_sets(W, H):
    """-> two lists of (x, y, w, h): A = single pixel at the origin, the bottom-right pixel, odd x0 with width 5, a 4-wide strip against the right edge over the full
    height, two overlapping rectangles; B = the full image and a rectangle inside it"""
    a = [(0, 0, 1, 1), (W - 1, H - 1, 1, 1), (3, 1, 5, min(4, H - 1)), (W - 4, 0, 4, H), (9, 2, 13, 5), (17, 3, 11, 6)]
    b = [(0, 0, W, H), (5, 1, 30, 7)]
    return a, b


def make_source(kind, pad, mem, W, H, rects, seed, keep):
    """detections over `rects` with ids IDS[i] and a source of `kind` filled with every value of its rule, members and non-members inside and outside every rectangle
    -> (dets, has [n, H, W] bool: the rule evaluated image-wide per detection, unmask(ctx, static_ids), objects(ctx, t))"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_PINNED
    rng = np.random.default_rng(seed)
    n = len(rects)
    dets = [dict(track_id=IDS[i], class_id=0, rect=r, points=None) for i, r in enumerate(rects)]
    has = np.zeros((n, H, W), bool)
    if kind == "roi":
        for i, d in enumerate(dets):
            x, y, w, h = d["rect"]
            d["mask"] = ROI_VALUES[rng.integers(0, len(ROI_VALUES), (h, w))]
            has[i, y:y + h, x:x + w] = d["mask"] >= 1
        return dets, has, (lambda ctx, ids: ctx.track_unmask_static(dets, ids)), (lambda ctx, t: ctx.inst_track_enqueue(t, dets, None))
    if kind == "key":
        palette = np.array(IDS[:n] + [7], np.uint32)
        kimg = np.full((H, W + pad), IDS[1], np.uint32)                           # beyond the row: a key in use, which must never be read as image
        kimg[:, :W] = palette[rng.integers(0, len(palette), (H, W))]
        for i in range(n):
            has[i] = kimg[:, :W] == np.uint32(IDS[i])
        if mem == "host":
            args = (kimg[:, :W],)
        else:
            t = torch.from_numpy(kimg.view(np.int32))
            t = t.cuda() if mem == "device" else t.pin_memory()
            torch.cuda.synchronize()
            keep.append(t)
            args = (t.data_ptr(), DV_MEM_DEVICE if mem == "device" else DV_MEM_PINNED, 4 * (W + pad))
        keep.append(kimg)
        return dets, has, (lambda ctx, ids: ctx.track_unmask_static_keys(dets, ids, *args)), (lambda ctx, t: ctx.inst_track_enqueue_keys(t, dets, *args))
    values = U8_VALUES if kind == "u8" else F32_VALUES
    vals = values[rng.integers(0, len(values), (n + 1, H, W))]                    # one plane more than detections; detection i reads plane n - i
    for i, d in enumerate(dets):
        d["plane"] = n - i
        has[i] = (vals[n - i] != 0) & (vals[n - i] != 128) if kind == "u8" else vals[n - i] > THR
    flat, view = laid_out(vals, W + pad, 7 if pad else 0, 1 if pad and kind == "u8" else 0)      # padded byte stacks start off a dword too
    stack, kw = on_memory(flat, view, mem, keep)
    keep.append(flat)
    kw["threshold"] = float(THR)
    return (dets, has, (lambda ctx, ids: ctx.track_unmask_static_planes(dets, ids, stack, **kw)),
            (lambda ctx, t: ctx.inst_track_enqueue_planes(t, dets, stack, **kw)))


def new_ctx(gpu_ctx_factory, W, H, inst):
    from dynamic_vins_amd.frontend import make_cam
    c = make_cam(100, 100, W / 2, H / 2)
    ctx = gpu_ctx_factory(width=W, height=H, max_cnt=20, min_dist=5, stereo=0, cam0=c, cam1=c)
    if inst:
        ctx.inst_config(20, 3, 0)
    return ctx


def inside(rect, W, H):
    x, y, w, h = rect
    m = np.zeros((H, W), bool)
    m[y:y + h, x:x + w] = True
    return m


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unmasking_writes_the_rule(gpu_ctx_factory, size, case):
    """working mask == where(inside any static rectangle & has, 255, input mask) at every byte, for a host input mask and for a caller's device input mask (which is
    byte-identical after the frame); a detection that is not static changes nothing"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MODE_RAW
    W, H = size
    kind, pad, mem = case
    ctx = new_ctx(gpu_ctx_factory, W, H, inst=False)
    gray = np.full((H, W), 100, np.uint8)
    gray_dev = torch.from_numpy(gray).cuda()
    keep, k = [], 0
    for rects in rect_sets(W, H):
        for device_mask in (False, True):
            dets, has, unmask, _ = make_source(kind, pad, mem, W, H, rects, 10 * k + W, keep)
            static = [d["track_id"] for d in dets[:-1]] + [99]                    # the last detection is not static; 99 is no detection
            mask = np.random.default_rng(k).integers(0, 256, (H, W)).astype(np.uint8)
            want = mask.copy()
            for i, d in enumerate(dets[:-1]):
                want[inside(d["rect"], W, H) & has[i]] = 255
            unmask(ctx, np.array(static, np.uint32))
            if device_mask:
                mask_dev = torch.from_numpy(mask).cuda()
                torch.cuda.synchronize()
                ctx.track_stereo_enqueue(gray_dev.data_ptr(), None, 0.05 * k, mask_dev.data_ptr(), DV_MODE_RAW, DV_MEM_DEVICE)
            else:
                ctx.track_stereo_enqueue(gray, None, 0.05 * k, mask, DV_MODE_RAW, DV_MEM_HOST)
            ctx.track_stereo_collect()
            got, w = ctx.front_debug_mask(0)
            assert w == W and got.shape == (H, (W + 15) // 16 * 16)
            bad = np.argwhere(got[:, :W] != want)
            assert len(bad) == 0, f"frame {k}: {len(bad)} bytes differ, first at (row, col) {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
            assert (want != mask).any() and (want == mask).any()
            if device_mask:
                assert mask_dev.cpu().numpy().tobytes() == mask.tobytes(), "the caller's device mask was written"
            k += 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_roi_masks_write_the_rule(gpu_ctx_factory, size, case):
    """every byte of every object's slice up to its pitch: 255 / 0 by the rule for c < w, 0 in the padding columns; the same objects in a second frame with smaller
    rectangles, so a byte that survived from the first frame shows.  (Host masks are copied, not cut: their slice carries the caller's bytes, the padding is not defined.)"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MODE_RAW
    W, H = size
    kind, pad, mem = case
    ctx = new_ctx(gpu_ctx_factory, W, H, inst=True)
    gray_dev = torch.from_numpy(np.full((H, W), 100, np.uint8)).cuda()
    a, _ = rect_sets(W, H)
    frames = [[(0, 0, W, H), (W - 4, 0, 4, H), (9, 2, 13, 5), (17, 3, 11, 6), (2, 0, 37, H)],          # large first ...
              [a[0], a[1], a[2], (19, 4, 3, 2), (W - 4, 0, 4, H)]]                                      # ... then smaller (and the strip, moved to another object)
    keep = []
    for k, rects in enumerate(frames):
        dets, has, _, objects = make_source(kind, pad, mem, W, H, rects, 77 + k + W, keep)
        ctx.track_stereo_enqueue(gray_dev.data_ptr(), None, 0.05 * k, None, DV_MODE_RAW, DV_MEM_DEVICE)
        objects(ctx, 0.05 * k)
        ctx.track_stereo_collect()
        insts, _, _ = ctx.inst_track_collect()
        assert len(insts) == len(dets)
        seen = set()
        for i, d in enumerate(dets):
            x, y, w, h = d["rect"]
            got, gw = ctx.front_debug_mask(1, d["track_id"])
            p = (w + 15) // 16 * 16
            assert gw == w and got.shape == (h, p)
            if kind == "roi":
                assert got[:, :w].tobytes() == d["mask"].tobytes(), f"frame {k}, object {d['track_id']}"
                continue
            want = np.zeros((h, p), np.uint8)
            want[:, :w] = np.where(has[i, y:y + h, x:x + w], 255, 0)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, f"frame {k}, object {d['track_id']} {d['rect']}: {len(bad)} bytes differ, first at (row, col) {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
            seen |= set(np.unique(want[:, :w]).tolist())
        assert kind == "roi" or seen == {0, 255}
