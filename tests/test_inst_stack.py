"""Dynamic mode from a detector's instance-mask stack on the device (`-m gpu`): thread T1's stage (dv_inst_stack_frame_enqueue / _collect), the objects' masks and the static
unmasking straight from the stack (dv_inst_track_enqueue_planes, dv_track_unmask_static_planes), the runner's and the pipeline's mask-stack sequences
(dv_runner_set_inst_stack, DynamicPipeline(mask_stack=True)).  The stage is checked against the reference's own formulas written with
CPU torch (detector2d.cpp:58-97, semantic_image.cpp:20-93); the two *_planes entries against the host-mask path of the same build.  Everything is bit equality.
Sizes: the label-image tests' operator sizes (70 x 23, 64 x 4) plus 67 x 5 with an odd row stride; 640 x 360 where the tracker runs."""
import ctypes as C

import numpy as np
import pytest

from tests.test_viode_live import FRAMES, H, W, download, new_ctx, rows_equal, sequence

pytestmark = pytest.mark.gpu

_CACHE = {}
THR = np.float32(0.5)
U8_HIT = np.array([1, 127, 129, 255], np.uint8)          # what mask_tensor.to(kInt8).abs().clamp(0, 1) keeps; 128 it does not
F32_HIT = np.array([np.nextafter(THR, np.float32(np.inf)), 0.9, 1e30, np.inf], np.float32)
F32_MISS = np.array([THR, np.nextafter(THR, np.float32(-np.inf)), np.nan, -1.0, 0.0], np.float32)


def encode(member, kind, rng, decoys=None):
    """bool [n, h, w] -> the element values of a stack: members get every value that counts, the others every value that must not (decoys: non-members that carry the
    value a naive `!= 0` / `>= threshold` test would take)"""
    if kind == "u8":
        out = np.where(member, U8_HIT[rng.integers(0, len(U8_HIT), member.shape)], 0).astype(np.uint8)
        if decoys is not None:
            out[decoys & ~member] = 128
        return out
    out = np.where(member, F32_HIT[rng.integers(0, len(F32_HIT), member.shape)], F32_MISS[rng.integers(0, len(F32_MISS), member.shape)]).astype(np.float32)
    return out


def laid_out(vals, row_elems, plane_extra, lead):
    """the stack in a flat buffer: rows of row_elems elements (>= w), planes h * row_elems + plane_extra elements apart, `lead` elements in front; everything between and
    around the image rows holds a value that WOULD count, so a read outside a row shows -> (flat buffer, strided [n, h, w] view of it)"""
    n, h, w = vals.shape
    plane = h * row_elems + plane_extra
    flat = np.full(lead + n * plane + 8, 255 if vals.dtype == np.uint8 else 1.0, vals.dtype)
    view = np.lib.stride_tricks.as_strided(flat[lead:], (n, h, w), (plane * vals.itemsize, row_elems * vals.itemsize, vals.itemsize))
    view[...] = vals
    return flat, view


def torch_reference(view, kind):
    """the reference's formulas on the CPU: membership, merged mask, its complement, boxes from nonzero() min / max (None: an empty plane, where torch::max throws)"""
    import torch
    m = torch.from_numpy(np.ascontiguousarray(view))
    if kind == "f32":
        m = m > float(THR)                                                        # Detector2D::Launch: seg_label > kSoloMaskThr
    bel = m.to(torch.int8).abs().clamp(0, 1)
    merged = (bel.sum(0).clamp(0, 1) * 255).to(torch.uint8).numpy()
    boxes = []
    for p in range(bel.shape[0]):
        nz = bel[p].nonzero()
        boxes.append(None if nz.numel() == 0 else (int(nz[:, 0].min()), int(nz[:, 0].max()), int(nz[:, 1].min()), int(nz[:, 1].max())))
    return bel.numpy().astype(bool), merged, (~torch.from_numpy(merged)).numpy(), boxes


def expected_dets(boxes, min_size):
    out = []
    for p, b in enumerate(boxes):
        if b is None:
            continue
        r0, r1, c0, c1 = b
        if c1 - c0 >= max(min_size, 1) and r1 - r0 >= max(min_size, 1):
            out.append((p, p, (c0, r0, c1 - c0, r1 - r0)))                       # plane, track id, cv::Rect(min_pt, max_pt)
    return out


def scene(w, h, n, seed):
    """membership [n, h, w]: plane 0 touches all four image edges; with n >= 3 plane 1 is empty and plane n - 1 a single pixel; the others random overlapping blobs"""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, h, w), bool)
    bh, bw = max(h // (2 if n < 8 else 6), 3), max(w // (3 if n < 8 else 24), 3)      # (many planes: small blobs, so that some pixels stay background)
    for p in range(n):
        x0, y0 = int(rng.integers(0, w - 2)), int(rng.integers(0, max(h - 2, 1)))
        m[p, y0:y0 + int(rng.integers(2, bh)), x0:x0 + int(rng.integers(2, bw))] = True
    m[0, 0, :] = m[0, h - 1, :] = True; m[0, :, 0] = m[0, :, w - 1] = True
    if seed % 2:
        m[0] = False; m[0, 1:3, 5:9] = True                                       # the second frame: plane 0 shrinks — no box may survive from the first
    if n >= 3:
        m[1] = False
        m[n - 1] = False; m[n - 1, h // 2, w - 1 - seed % 2] = True
    decoys = rng.random((n, h, w)) < 0.08
    return m, decoys, rng


def stage_ctx(gpu_ctx_factory, w, h):
    if ("ctx", w, h) not in _CACHE:
        from dynamic_vins_amd.frontend import make_cam
        _CACHE[("ctx", w, h)] = gpu_ctx_factory(width=w, height=h, max_cnt=50, min_dist=10, cam0=make_cam(100, 100, w / 2, h / 2), cam1=make_cam(100, 100, w / 2, h / 2))
    return _CACHE[("ctx", w, h)]


def on_memory(flat, view, mem, keep):
    """the flat buffer in the asked memory kind -> keyword arguments of frontend.mask_stack beside the pointer"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED, DV_STACK_F32, DV_STACK_U8
    if mem == "host":
        return view, {}
    t = torch.from_numpy(flat.view(np.uint8))
    t = t.cuda() if mem == "device" else t.pin_memory()
    torch.cuda.synchronize()
    keep.append(t)
    off = view.__array_interface__["data"][0] - flat.__array_interface__["data"][0]
    return t.data_ptr() + off, dict(mem=DV_MEM_DEVICE if mem == "device" else DV_MEM_PINNED, n_planes=view.shape[0], kind=DV_STACK_F32 if view.dtype == np.float32 else DV_STACK_U8,
                                    row_stride=view.strides[1], plane_stride=view.strides[0])


# ------------------------------------------------------------------ 1. the stage ------------------------------------------------------------------
# (w, h, row elements, extra elements between planes, elements in front): 67 x 5 with rows of 71 elements, planes further apart than rows x stride, and — for bytes — a base
# address that is no multiple of 4, so the tail and the unaligned paths are taken; 70 x 23 tight: every other row starts off a dword; 64 x 4: everything aligned
LAYOUTS = [(70, 23, 70, 0, 0), (64, 4, 64, 0, 0), (67, 5, 71, 13, 1), (301, 5, 303, 5, 1)]          # the last: two workgroup columns (the kernel's are 256 pixels wide)


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("n_planes", [1, 3, 64])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l[0]}x{l[1]}s{l[2]}")
def test_stage_equals_the_reference_formulas(gpu_ctx_factory, layout, n_planes, kind):
    """dv_inst_stack_frame_enqueue / _collect against (m.to(int8).abs().clamp(0, 1).sum(0).clamp(0, 1) * 255).to(uint8), its complement and nonzero() min / max per plane,
    in host, device and pinned memory: merged and inverse mask byte for byte, detections (ascending plane, max row / column excluded, size floor, empty plane dropped),
    the planes[] array.  Two consecutive frames of different content: no box leaks, and frame k's masks are intact after frame k + 1 was enqueued and collected."""
    w, h, row, extra, lead = layout
    if kind == "f32":
        extra, lead = extra + 3, 0                                                # (float planes: 4-byte aligned by construction; rows of 284 bytes are not 16-byte aligned)
    ctx = stage_ctx(gpu_ctx_factory, w, h)
    min_size = 2
    for mem in ("host", "device", "pinned"):
        keep, frames = [], []
        for f in range(2):
            member, decoys, rng = scene(w, h, n_planes, 40 + f)
            flat, view = laid_out(encode(member, kind, rng, decoys), row, extra, lead)
            bel, merged, inv, boxes = torch_reference(view, kind)
            assert np.array_equal(bel, member), "the torch rule and the scene's membership disagree: the value tables above are wrong"
            if kind == "u8":
                assert ((view == 128).any(0) & (merged == 0)).any(), "no pixel that only a naive != 0 test would take"
            frames.append((flat, view, merged, inv, expected_dets(boxes, min_size), boxes))
        if n_planes >= 3:
            assert frames[0][5][1] is None and frames[0][5][n_planes - 1][0] == frames[0][5][n_planes - 1][1], "no empty / single-pixel plane"
        assert frames[0][5][0] == (0, h - 1, 0, w - 1), "no plane touching all four edges"
        got = []
        for flat, view, *_ in frames:
            stack, kw = on_memory(flat, view, mem, keep)
            ctx.inst_stack_frame_enqueue(stack, threshold=float(THR), **kw)
            got.append(ctx.inst_stack_frame_collect(min_size))
        for f in (1, 0):                                                          # frame 0 is read AFTER frame 1 was enqueued and collected
            dets, inv_p, mrg_p = got[f]
            assert [(d["plane"], d["track_id"], d["rect"]) for d in dets] == frames[f][4], f"{mem}, frame {f}: detections"
            assert all(d["mask"] is None and d["class_id"] == 0 for d in dets)
            assert np.array_equal(download(mrg_p, w * h).reshape(h, w), frames[f][2]), f"{mem}, frame {f}: merged mask"
            assert np.array_equal(download(inv_p, w * h).reshape(h, w), frames[f][3]), f"{mem}, frame {f}: inverse mask"
        assert got[0][1] != got[1][1] and got[0][2] != got[1][2]


def test_int8_rule_byte_by_byte(gpu_ctx_factory):
    """what to(kInt8).abs().clamp(0, 1) does to every byte value, on this machine's CPU torch, against the kernel: 128 -> int8 -128 -> abs wraps to -128 -> 0"""
    import torch
    w, h = 64, 4
    ctx = stage_ctx(gpu_ctx_factory, w, h)
    plane = np.arange(256, dtype=np.uint8).reshape(1, h, w)
    want = torch.from_numpy(plane[0]).to(torch.int8).abs().clamp(0, 1).numpy().astype(bool)
    assert not want[2, 0] and want[0, 1] and want[1, 63] and want[2, 1] and want[3, 63] and not want[0, 0]          # 128, 1, 127, 129, 255, 0
    ctx.inst_stack_frame_enqueue(plane)
    dets, inv_p, mrg_p = ctx.inst_stack_frame_collect(1)
    assert np.array_equal(download(mrg_p, w * h).reshape(h, w), np.where(want, 255, 0).astype(np.uint8))
    assert np.array_equal(download(inv_p, w * h).reshape(h, w), np.where(want, 0, 255).astype(np.uint8))
    assert [d["rect"] for d in dets] == [(0, 0, 63, 3)]


# ------------------------------------------------------------------ 2. naive form ------------------------------------------------------------------
def test_naive_form_remaps_the_merged_mask(gpu_ctx_factory):
    """SetBackgroundMask: with maps from dv_undistort_setup the inverse mask equals ~dv_remap(merged) byte for byte (and the merged pointer holds the remapped mask); the
    dynamic form on the same context does not remap; without maps the flag is refused"""
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import make_cam
    w, h = 70, 23
    cam = make_cam(60.0, 61.0, 34.0, 12.0, -0.25, 0.06, 1e-3, -2e-3)
    ctx = gpu_ctx_factory(width=w, height=h, max_cnt=50, min_dist=10, cam0=cam, cam1=cam)
    member, decoys, rng = scene(w, h, 3, 40)
    stack = encode(member, "u8", rng, decoys)
    merged = torch_reference(stack, "u8")[1]
    with pytest.raises(DvinsError, match="dv_inst_stack_frame_enqueue: DV_STACK_REMAP_MERGED needs installed undistortion maps"):
        ctx.inst_stack_frame_enqueue(stack, remap_merged=True)
    ctx.undistort_setup(0.0)
    m1, m2 = ctx.undistort_maps(0)
    want = ctx.remap(merged, m1, m2)
    assert not np.array_equal(want, merged), "the maps move nothing in this scene"
    ctx.inst_stack_frame_enqueue(stack, remap_merged=True)
    dets, inv_p, mrg_p = ctx.inst_stack_frame_collect(2)
    assert np.array_equal(download(inv_p, w * h).reshape(h, w), ~want)
    assert np.array_equal(download(mrg_p, w * h).reshape(h, w), want)
    ctx.inst_stack_frame_enqueue(stack)                                            # SetMaskAndRoi does not remap
    _, inv_p, _ = ctx.inst_stack_frame_collect(2)
    assert np.array_equal(download(inv_p, w * h).reshape(h, w), ~merged)


# ------------------------------------------------------------------ 3. object masks ------------------------------------------------------------------
# track id, plane, (x, y, w, h): widths 33 / 17 / 15 / 1, x not a multiple of 4, one rectangle flush with the right and bottom edges, the first two overlap; plane 2 is unused
RECTS = [(901, 5, (37, 50, 33, 60)), (902, 0, (61, 70, 17, 50)), (903, 3, (W - 15, H - 40, 15, 40)), (904, 1, (201, 100, 1, 80)), (3000000001, 4, (300, 120, 121, 90))]
N_OBJ_PLANES = 6


def object_frame(k):
    """membership [6, H, W] of frame k and its detections with numpy-cut masks; the scene drifts by k pixels"""
    m = np.zeros((N_OBJ_PLANES, H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    dets = []
    for tid, p, (x, y, w, h) in RECTS:
        x += k if x + w + FRAMES < W and w > 1 else 0                             # (the flush rectangle stays flush)
        if p == 4:                                                                # an ellipse inside its rectangle: mask != rectangle
            m[p][((yy - (y + h / 2)) / (0.5 * h)) ** 2 + ((xx - (x + w / 2)) / (0.5 * w)) ** 2 < 1] = True
        else:
            m[p, y:y + h, x:x + w] = True
        if p == 5:
            m[p, y + 20:y + 26, x + 3:x + 9] = False                              # a hole
            m[2, y + 20:y + 26, x + 3:x + 9] = True                               # ... that belongs to another plane only
        dets.append(dict(track_id=tid, class_id=0, rect=(x, y, w, h), plane=p, points=None))
    m[4, 10:30, 500:520] = True                                                   # pixels of the own plane outside the rectangle
    m[5, 300:320, 20:40] = True
    for d in dets:
        x, y, w, h = d["rect"]
        d["mask"] = np.ascontiguousarray(np.where(m[d["plane"], y:y + h, x:x + w], 255, 0).astype(np.uint8))
    return m, dets


def run_objects(kind, mem, n_frames=5):
    """-> per frame (insts, feats, points).  kind None: dv_inst_track_enqueue with the numpy-cut masks (the reference); else the plane form"""
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MODE_RAW
    from tests.test_viode_live import cam
    seq = sequence()
    ctx = new_ctx(morph=0)
    c = cam()
    disp = np.full((H, W), np.float32(np.float32(c["fx"]) * np.float32(0.12) / np.float32(6.0)), np.float32)      # a wall 6 m away: every masked sample yields a point
    out, keep = [], []
    for k in range(n_frames):
        member, dets = object_frame(k)
        l, r = seq.frames[k]
        ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[k], None, DV_MODE_RAW, DV_MEM_DEVICE)
        ctx.inst_set_disparity(disp, 0.12)
        if kind is None:
            ctx.inst_track_enqueue(seq.times[k], dets, None)
        else:
            rng = np.random.default_rng(k)
            flat, view = laid_out(encode(member, kind, rng, rng.random(member.shape) < 0.05), W + 5, 7 if kind == "u8" else 8, 1 if kind == "u8" else 0)
            stack, kw = on_memory(flat, view, mem, keep)
            keep.append(flat)
            ctx.inst_track_enqueue_planes(seq.times[k], dets, stack, threshold=float(THR), **kw)
        ctx.track_stereo_collect()
        out.append(ctx.inst_track_collect())
    ctx.close()
    return out


@pytest.mark.parametrize("kind,mem", [("u8", "host"), ("u8", "device"), ("f32", "pinned"), ("f32", "device")])
def test_plane_masks_equal_host_masks(kind, mem):
    """dv_inst_track_enqueue_planes against dv_inst_track_enqueue with the ROI masks cut in numpy from the same stack, 5 frames, a disparity map set (the extra-point
    sampling reads the mask): instances, feature rows, ids and extra points identical.  Rectangles 1 / 15 / 17 / 33 wide, flush with the image edge, overlapping, with pixels
    of another plane only inside and pixels of the own plane outside; rows of W + 5 elements, planes further apart than that.  The 1-pixel-wide object cannot carry a corner
    in any implementation (tests/test_viode_live.py): it is witnessed by its extra points."""
    if "objref" not in _CACHE:
        _CACHE["objref"] = run_objects(None, None)
    ref = _CACHE["objref"]
    got = run_objects(kind, mem)
    for k, ((ia, fa, pa), (ib, fb, pb)) in enumerate(zip(ref, got)):
        print(f"frame {k}: rows per object {dict(zip(ia['id'].tolist(), ia['n_feats'].tolist()))}, points {dict(zip(ia['id'].tolist(), ia['n_points'].tolist()))}")
        assert len(ia) == len(RECTS)
        for o in ia:
            if int(o["rect"][2]) > 1:
                assert o["n_feats"] >= 1, f"frame {k}: the reference has no feature on object {o['id']}"
            else:
                assert o["n_points"] >= 1, f"frame {k}: the reference has no extra point on the 1-pixel-wide object"
        assert ia.tobytes() == ib.tobytes(), f"frame {k}: instances"
        rows_equal(fa, fb, f"frame {k}: object rows")
        assert pa.tobytes() == pb.tobytes() and len(pa) > 0, f"frame {k}: extra points"
    assert any(f["track_cnt"].max() > 1 for _, f, _ in ref[1:]), "no object feature survived a frame: the temporal path was not exercised"


# ------------------------------------------------------------------ 4. static unmasking ------------------------------------------------------------------
def scene_stack(seq, k, kind):
    """frame k of the rendered escort scene as a mask stack, one plane per dynamic key of its key image -> (values [n, H, W], detections with their planes)"""
    from tests.test_viode_live import ctx_free_key_image
    kimg = ctx_free_key_image(seq, k)
    keys = [int(v) for v in seq.dyn_keys]
    member = np.stack([kimg == key for key in keys])
    rng = np.random.default_rng(100 + k)
    dets = [dict(d, plane=keys.index(int(d["track_id"]))) for d in seq.dets[k]]
    return encode(member, kind, rng, rng.random(member.shape) < 0.02), dets


def run_background(variant, n_frames=8):
    """TrackSemanticImage over the scene with a fixed list of static ids -> per frame the background rows.  variant: "masks" (dv_track_unmask_static, host masks),
    "u8" (plane form, host stack), "f32_dev" (plane form, float stack on the device), "none" """
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MODE_SEMANTIC, DV_STACK_F32
    seq = sequence()
    ctx = new_ctx(inst=False)
    static_ids = np.array([seq.dyn_keys[0], seq.dyn_keys[2], 99], np.uint32)
    out, keep = [], []
    for k in range(n_frames):
        l, r = seq.frames[k]
        if variant == "masks":
            ctx.track_unmask_static(seq.dets[k], static_ids)
        elif variant == "u8":
            vals, dets = scene_stack(seq, k, "u8")
            keep.append(vals)
            ctx.track_unmask_static_planes(dets, static_ids, vals)
        elif variant == "f32_dev":
            vals, dets = scene_stack(seq, k, "f32")
            t = torch.from_numpy(vals).cuda(); torch.cuda.synchronize(); keep.append(t)
            ctx.track_unmask_static_planes(dets, static_ids, t.data_ptr(), mem=DV_MEM_DEVICE, n_planes=vals.shape[0], kind=DV_STACK_F32, threshold=float(THR))
        ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[k], seq.inv_mask_dev[k].data_ptr(), DV_MODE_SEMANTIC, DV_MEM_DEVICE)
        out.append(ctx.track_stereo_collect())
    ctx.close()
    return out


def test_static_unmasking_from_the_stack():
    """the same sequence tracked with dv_track_unmask_static (host masks) and with the plane form (host byte stack, device float stack), a fixed list of static ids,
    8 frames: the rows of dv_track_stereo_collect identical on every frame — and a run without unmasking differs, so the unmasking mattered"""
    a, b, c, n = run_background("masks"), run_background("u8"), run_background("f32_dev"), run_background("none")
    for k in range(len(a)):
        assert len(a[k]) > 20
        rows_equal(a[k], b[k], f"frame {k}: host byte stack")
        rows_equal(a[k], c[k], f"frame {k}: device float stack")
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, n)), "unmasking changed nothing in this scene"


# ------------------------------------------------------------------ 5. refusals ------------------------------------------------------------------
def full_frame(ctx, seq, k, static_ids):
    """stage -> collect -> static unmasking -> background + object tracking of frame k, all from ONE host stack (staged once, by the stage) -> (background rows, object rows)"""
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MODE_SEMANTIC
    vals, want = scene_stack(seq, k, "u8")
    ctx.inst_stack_frame_enqueue(vals)
    dets, inv, _ = ctx.inst_stack_frame_collect(8)
    assert [(d["plane"], d["rect"]) for d in dets] == [(d["plane"], tuple(d["rect"])) for d in sorted(want, key=lambda d: d["plane"])]
    keys = [int(v) for v in seq.dyn_keys]
    for d in dets:
        d["track_id"] = keys[d["plane"]]                                          # the upstream tracker's answer
    l, r = seq.frames[k]
    ctx.track_unmask_static_planes(dets, static_ids, vals)
    ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[k], inv, DV_MODE_SEMANTIC, DV_MEM_DEVICE)
    ctx.inst_track_enqueue_planes(seq.times[k], dets, vals)
    return ctx.track_stereo_collect(), ctx.inst_track_collect()[1]


def test_refusals_name_the_entry_and_leave_nothing_staged():
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MODE_SEMANTIC, dv_mask_stack, mask_stack
    seq = sequence()
    ctx = new_ctx()
    lib, h = ctx.lib, ctx.h
    static_ids = np.array([seq.dyn_keys[0]], np.uint32)

    def fails(rc, name):
        assert rc == -1
        assert name in lib.dv_last_error(h).decode(), lib.dv_last_error(h).decode()

    vals, dets = scene_stack(seq, 0, "u8")
    assert len(dets) >= 2
    st = mask_stack(vals)
    n, p0, p1 = C.c_int(0), C.c_void_p(0), C.c_void_p(0)
    arr, planes = ctx._det_array(dets), ctx._plane_array(dets)
    fails(lib.dv_inst_stack_frame_collect(h, 8, C.addressof(arr), C.addressof(planes), len(arr), C.byref(n), C.byref(p0), C.byref(p1)), "dv_inst_stack_frame_collect")
    for bad_n in (0, 65):
        bad = dv_mask_stack(st.data, bad_n, st.kind, st.mem, st.row_stride, st.plane_stride, 0.0, 0)
        fails(lib.dv_inst_stack_frame_enqueue(h, C.addressof(bad), W, H, 0), "dv_inst_stack_frame_enqueue: 1..64 planes")
        fails(lib.dv_inst_track_enqueue_planes(h, 0.0, C.addressof(arr), C.addressof(planes), len(dets), C.addressof(bad), None, 0), "dv_inst_track_enqueue_planes: 1..64 planes")
        fails(lib.dv_track_unmask_static_planes(h, C.addressof(arr), C.addressof(planes), len(dets), static_ids.ctypes.data, 1, C.addressof(bad)), "dv_track_unmask_static_planes: 1..64 planes")
    fails(lib.dv_inst_stack_frame_enqueue(h, C.addressof(st), W - 1, H, 0), "dv_inst_stack_frame_enqueue")                      # size mismatch
    fails(lib.dv_inst_stack_frame_enqueue(h, C.addressof(st), W, H, 1), "DV_STACK_REMAP_MERGED needs installed undistortion maps")
    ctx.inst_stack_frame_enqueue(vals)
    fails(lib.dv_inst_stack_frame_enqueue(h, C.addressof(st), W, H, 0), "dv_inst_stack_frame_enqueue: previous frame not collected")      # a second _enqueue
    got, inv, _ = ctx.inst_stack_frame_collect(8)
    # a plane index out of range and a rectangle outside the image, on both entries: refused before anything is staged
    l, r = seq.frames[0]
    bad_rect = [dict(d) for d in dets]; bad_rect[0] = dict(bad_rect[0], rect=(W - 4, 10, 30, 30))
    bad_plane = [dict(d) for d in dets]; bad_plane[1] = dict(bad_plane[1], plane=len(vals))
    ids = np.array([d["track_id"] for d in dets], np.uint32)
    for bad, why in ((bad_rect, "detection rectangle outside the image"), (bad_plane, "plane index out of range")):
        a_bad, p_bad = ctx._det_array(bad), ctx._plane_array(bad)
        fails(lib.dv_track_unmask_static_planes(h, C.addressof(a_bad), C.addressof(p_bad), len(bad), ids.ctypes.data, len(ids), C.addressof(st)), "dv_track_unmask_static_planes: " + why)
    ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[0], inv, DV_MODE_SEMANTIC, DV_MEM_DEVICE)
    for bad, why in ((bad_rect, "detection rectangle outside the image"), (bad_plane, "plane index out of range")):
        a_bad, p_bad = ctx._det_array(bad), ctx._plane_array(bad)
        fails(lib.dv_inst_track_enqueue_planes(h, seq.times[0], C.addressof(a_bad), C.addressof(p_bad), len(bad), C.addressof(st), None, 0), "dv_inst_track_enqueue_planes: " + why)
    ctx.inst_track_enqueue_planes(seq.times[0], dets, vals)
    rows0 = ctx.track_stereo_collect()
    f0 = ctx.inst_track_collect()[1]
    # the frame on the context that saw the refusals equals a fresh context's: nothing was left staged
    assert len(rows0) > 20 and len(f0) > 0
    ref = new_ctx()
    ref.inst_stack_frame_enqueue(vals)
    _, inv2, _ = ref.inst_stack_frame_collect(8)
    ref.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[0], inv2, DV_MODE_SEMANTIC, DV_MEM_DEVICE)
    ref.inst_track_enqueue_planes(seq.times[0], dets, vals)
    rows_equal(rows0, ref.track_stereo_collect(), "background rows after the refused calls")
    rows_equal(f0, ref.inst_track_collect()[1], "object rows after the refused calls")
    # staged unmask jobs are dropped by a refused dv_track_stereo_enqueue (wrong size): the next frame is not unmasked by them
    ctx.track_unmask_static_planes(dets, ids, vals)
    fails(lib.dv_track_stereo_enqueue(h, l.data_ptr(), r.data_ptr(), W - 1, H, W, seq.times[1], inv, DV_MODE_SEMANTIC, DV_MEM_DEVICE), "dv_track_stereo")
    # frames 1 and 2 through the whole chain from one host stack on both contexts
    for k in (1, 2):
        a_rows, a_obj = full_frame(ctx, seq, k, static_ids)
        b_rows, b_obj = full_frame(ref, seq, k, static_ids)
        assert len(a_rows) > 20 and len(a_obj) > 0
        rows_equal(a_rows, b_rows, f"frame {k}: background rows"); rows_equal(a_obj, b_obj, f"frame {k}: object rows")
    ctx.close(); ref.close()


# ------------------------------------------------------------------ 6. runner ------------------------------------------------------------------
RUN_FRAMES = 30
KW = dict(max_cnt=150, min_dist=20, max_iters=8, use_det3d=0, mask_morphology_size=5, static_inst_threshold=10.0, extra_from_disparity=False, static_as_background=True)


def runner_sequence():
    """the rendered escort scene of the label-image tests, 30 frames (a run cut into 7 + 1 + 13 + 8), WITHOUT the right key images: a detector's stack has no counterpart of
    VIODE's right-image key test, so the pre-computed reference must not apply it either"""
    if "rseq" not in _CACHE:
        from dynamic_vins_amd.viode import ViodeSequence
        from tests.test_viode_live import cam
        masker = new_ctx(inst=False)
        s = ViodeSequence(W, H, cam(), RUN_FRAMES, masker, rate=20.0)
        masker.close()
        s.right_keys = None
        _CACHE["rseq"] = s
    return _CACHE["rseq"]


def run_runner(stack, tracker_thread, calls):
    from dynamic_vins_amd.backend import Runner
    from dynamic_vins_amd.pipeline import DynamicPipeline
    from tests.test_viode_live import record
    p = DynamicPipeline(runner_sequence(), mask_stack=stack, **KW)
    r = Runner([p], group_size=0, threads=1)
    r.set("tracker_thread", tracker_thread)
    for c in calls:
        r.run(c)
    out = record(r, p)
    r.close(); p.ctx.close()
    return out


@pytest.mark.parametrize("tracker_thread,calls", [(0, (RUN_FRAMES - 1,)), (1, (RUN_FRAMES - 1,)), (0, (7, 1, 13, 8)), (1, (7, 1, 13, 8))])
def test_runner_mask_stacks_equal_precomputed_masks(tracker_thread, calls):
    """dv_runner_set_inst_stack (the key image of every frame turned into a stack, one plane per key; T1's stage per frame) against dv_runner_set_dynamic fed the
    pre-computed masks and detections of the same stacks: row log, window and trajectory, iteration totals, object states, static report and dv_runner_dynamic_stats
    identical; one-thread order and T2 beside T3; uncut and cut into (7, 1, 13, 8)"""
    key = ("runner", tracker_thread)
    if key not in _CACHE:
        _CACHE[key] = run_runner(False, tracker_thread, (RUN_FRAMES - 1,))
    ref = _CACHE[key]
    assert ref["stats"]["object_features"] > 100 and ref["stats"]["frames_with_objects"] >= RUN_FRAMES - 3 and ref["n_instances"] >= 2 and ref["state"][1] == 1, ref["stats"]
    got = run_runner(True, tracker_thread, calls)
    for name in ref:
        assert got[name] == ref[name], name


def test_pipeline_mask_stacks_equal_precomputed_masks():
    """DynamicPipeline(mask_stack=True) stepped from Python against the pre-computed pipeline: the same entries in the same order as the runner's one-thread loop"""
    from dynamic_vins_amd.pipeline import DynamicPipeline
    out = []
    for stack in (False, True):
        p = DynamicPipeline(runner_sequence(), mask_stack=stack, **KW)
        for _ in range(12):
            p.step()
        I, S = p.est.instances()
        out.append((np.asarray(p.poses).tobytes(), I.tobytes(), np.asarray(S).tobytes(), dict(p.stat)))
        p.ctx.close()
    assert out[0][3]["object_features"] > 50
    assert out[0] == out[1]


def test_runner_refuses_a_grouped_mask_stack_sequence():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.backend import Runner
    from dynamic_vins_amd.pipeline import DynamicPipeline
    seq = runner_sequence()
    a, b = DynamicPipeline(seq, **KW), DynamicPipeline(seq, **KW)
    r = Runner([a, b], group_size=2, threads=1)
    st = DynamicPipeline.stack_input(a)
    with pytest.raises(DvinsError, match="dv_runner_set_inst_stack: a sequence of a dv_batch group is not supported"):
        r.set_inst_stack(0, st["stacks"], st["track_ids"], st["class_ids"])
    r.run(3)                                           # the runner stays usable: both members go on as pre-computed dynamic sequences
    assert r.get(0)[3] == 3 and r.get(1)[3] == 3
    r.close(); a.ctx.close(); b.ctx.close()
