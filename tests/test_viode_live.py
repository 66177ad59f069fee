"""Dynamic mode from label images on the device, one frame at a time (`-m gpu`): the key-image entries (dv_inst_track_enqueue_keys, dv_track_unmask_static_keys), thread
T1's per-frame stage (dv_viode_frame_enqueue / _collect), the runner's label-image sequences (dv_runner_set_viode) and the node's --live-masks.  The reference of every
comparison is the existing host-mask path of the same build (itself pinned to the oracle by tests/test_dynamic_pipeline.py, test_node.py, test_runner.py): equality
means bit for bit, no tolerance anywhere.  Image size: 640 x 360, the smallest at which the dynamic tests run; operator-level sizes for the frame stage."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dynamic_vins_amd import sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 640, 360, 15
_CACHE = {}


def cam():
    return sim.scaled_cam(sim.ZED, W, H, 1280, 720)


def new_ctx(morph=5, inst=True):
    from dynamic_vins_amd.frontend import Context, make_cam
    c = make_cam(*sim.cam_tuple(cam()))
    ctx = Context(width=W, height=H, max_cnt=150, min_dist=20, cam0=c, cam1=c, mask_morphology_size=morph)
    if inst:
        ctx.inst_config(50, 5, 0)
    return ctx


def sequence():
    """the VIODE-style scene (frames resident, label images, pre-computed masks / detections / key images through dv_viode_mask) — rendered once"""
    if "seq" not in _CACHE:
        from dynamic_vins_amd.viode import ViodeSequence
        masker = new_ctx(inst=False)
        _CACHE["seq"] = ViodeSequence(W, H, cam(), FRAMES, masker, rate=20.0)
        masker.close()
    return _CACHE["seq"]


def download(ptr, nbytes):
    """nbytes of device memory -> numpy uint8 (through a torch tensor on the same device)"""
    import torch
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)      # the HIP runtime this process has loaded already
    hip = C.CDLL(path)
    out = np.zeros(nbytes, np.uint8)
    torch.cuda.synchronize()
    rc = hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(ptr)), C.c_size_t(nbytes), C.c_int(2))      # hipMemcpyDeviceToHost
    assert rc == 0
    return out


def rows_equal(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} vs {len(b)} rows"
    assert a.tobytes() == b.tobytes(), what


# ------------------------------------------------------------------ 1. key masks ------------------------------------------------------------------
BIG = 3000000001          # a key above 2^31: the comparison is unsigned
KSTRIDE = W + 5           # key-image rows of 4 * (W + 5) bytes: stride larger than 4 w
# id, (x, y, w, h): widths 33 / 17 / 15 / 1, x not a multiple of 4, one rectangle flush with the right and bottom edges, 101 and 102 overlap
RECTS = [(101, (37, 50, 33, 60)), (102, (61, 70, 17, 50)), (103, (W - 15, H - 40, 15, 40)), (104, (201, 100, 1, 80)), (BIG, (300, 120, 121, 90))]


def key_frame(k):
    """the frame's key image [H, KSTRIDE] (columns >= W are filler that must never be read as image) and its detections with numpy-cut masks; the scene drifts by k pixels"""
    kimg = np.full((H, KSTRIDE), 7, np.uint32)
    kimg[:, W:] = 101                                  # beyond the row: another object's key
    yy, xx = np.mgrid[0:H, 0:W]
    dets = []
    for key, (x, y, w, h) in RECTS:
        dx = k if x + w + FRAMES < W and w > 1 else 0  # (the flush rectangle stays flush)
        x += dx
        if key == BIG:                                 # an ellipse inside its rectangle: mask != rectangle
            kimg[:, :W][((yy - (y + h / 2)) / (0.5 * h)) ** 2 + ((xx - (x + w / 2)) / (0.5 * w)) ** 2 < 1] = key
        elif key == 101:
            kimg[y:y + h, x:x + w] = key
            kimg[y + 20:y + 26, x + 3:x + 9] = 7       # a hole
        else:
            kimg[y:y + h, x:x + w] = key               # 102 overwrites part of 101's rectangle: another object's key inside it
    kimg[10:30, 500:520] = BIG                         # the object's key also present outside its rectangle
    kimg[300:320, 20:40] = 101
    for key, (x, y, w, h) in RECTS:
        dx = k if x + w + FRAMES < W and w > 1 else 0
        x += dx
        mask = np.ascontiguousarray(np.where(kimg[y:y + h, x:x + w] == key, 255, 0).astype(np.uint8))
        dets.append(dict(track_id=key, class_id=0, rect=(x, y, w, h), mask=mask, points=None))
    return kimg, dets


def run_objects(mem, n_frames=5):
    """-> per frame (insts, feats, points).  mem None: dv_inst_track_enqueue with the numpy-cut masks (the reference); else the key form with that memory kind"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED, DV_MODE_RAW
    seq = sequence()
    ctx = new_ctx(morph=0)
    c = cam()
    disp = np.full((H, W), np.float32(np.float32(c["fx"]) * np.float32(0.12) / np.float32(6.0)), np.float32)      # a wall 6 m away: every masked sample yields a point
    out, keep = [], []
    for k in range(n_frames):
        kimg, dets = key_frame(k)
        l, r = seq.frames[k]
        ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[k], None, DV_MODE_RAW, DV_MEM_DEVICE)
        ctx.inst_set_disparity(disp, 0.12)
        if mem is None:
            ctx.inst_track_enqueue(seq.times[k], dets, None)
        elif mem == DV_MEM_HOST:
            ctx.inst_track_enqueue_keys(seq.times[k], dets, kimg[:, :W])
        else:
            t = torch.from_numpy(kimg.view(np.int32))
            t = t.cuda() if mem == DV_MEM_DEVICE else t.pin_memory()
            torch.cuda.synchronize()
            keep.append(t)
            ctx.inst_track_enqueue_keys(seq.times[k], dets, t.data_ptr(), mem, 4 * KSTRIDE)
        ctx.track_stereo_collect()
        out.append(ctx.inst_track_collect())
    ctx.close()
    return out


def key_reference():
    if "keyref" not in _CACHE:
        _CACHE["keyref"] = run_objects(None)
    return _CACHE["keyref"]


@pytest.mark.parametrize("mem", ["host", "device", "pinned"])
def test_key_masks_equal_host_masks(mem):
    """dv_inst_track_enqueue_keys against dv_inst_track_enqueue with the masks cut in numpy from the same key image, 5 frames, a disparity map set (the extra-point sampling
    reads the mask): instances, feature rows, ids and extra points identical.  The host-mask run must have rows on every object, otherwise equality says nothing — every
    object but the 1-pixel-wide one: a 1 x h ROI has no horizontal gradient, Shi-Tomasi's smaller eigenvalue is identically zero there and no implementation can place a
    corner on it; that object's mask is witnessed by its extra points instead (sampled under the mask), which must be there.  Measured on an MI355X, host-mask run, per
    frame: rows 28 - 37 / 16 / 11 - 14 / 0 / 50 on the objects 33 / 17 / 15 / 1 / 121 wide, extra points 401 / 225 / 160 / 40 / 2128."""
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MEM_PINNED
    ref = key_reference()
    got = run_objects(dict(host=DV_MEM_HOST, device=DV_MEM_DEVICE, pinned=DV_MEM_PINNED)[mem])
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


# ------------------------------------------------------------------ 2. frame stage ------------------------------------------------------------------
def label_scene(w, h, keys_rgb, seed, second=False, skip=()):
    """random blobs of the given colours on a background colour -> B G R label image"""
    rng = np.random.default_rng(seed)
    img = np.empty((h, w, 3), np.uint8); img[...] = (60, 120, 90)
    for i, (r, g, b) in enumerate(keys_rgb):
        if (second and i % 2) or i in skip:
            continue                                   # the second frame lacks every other key: its boxes must not survive from the first
        x0, y0 = int(rng.integers(0, max(w - 3, 1))), int(rng.integers(0, max(h - 2, 1)))
        img[y0:y0 + int(rng.integers(1, max(h // 2, 2))), x0:x0 + int(rng.integers(1, max(w // 3, 2)))] = (b, g, r)
    return img


@pytest.mark.parametrize("w,h,nkeys", [(70, 23, 1), (70, 23, 64), (64, 4, 64), (W, H, 5)])
def test_frame_stage_equals_viode_mask_and_the_host_rule(gpu_ctx_factory, w, h, nkeys):
    """dv_viode_frame_enqueue / _collect against dv_viode_mask + viode.detections: detections, inverse mask and both key images (downloaded) identical; sizes the 64 x 4
    launch tile does not divide; nkeys 1 and 64; a key absent from the image, one whose box is below min_inst_size, one touching all four borders; two consecutive frames of
    different content (no box may leak), the first frame's buffers intact after the second is enqueued (the two buffer sets)."""
    from dynamic_vins_amd import viode
    from dynamic_vins_amd.frontend import make_cam
    ctx = gpu_ctx_factory(width=w, height=h, max_cnt=50, min_dist=10, cam0=make_cam(100, 100, w / 2, h / 2), cam1=make_cam(100, 100, w / 2, h / 2))
    rgb = [(10 + 3 * i, 1 + i, 2 + (i % 5)) for i in range(nkeys)]
    keys = np.sort(viode.pixel_to_key(np.array([c[0] for c in rgb]), np.array([c[1] for c in rgb]), np.array([c[2] for c in rgb])))
    assert len(np.unique(keys)) == nkeys
    min_size = 2 if h < 16 else 4
    frames = []
    for f in range(2):
        s0, s1 = label_scene(w, h, rgb[: max(nkeys - 1, 1)] if nkeys > 1 else rgb, 10 + f, second=bool(f), skip=(1,)), label_scene(w, h, rgb, 20 + f)
        if nkeys > 1:                                  # (the last colour is never drawn: a key absent from the image)
            b = rgb[0]
            if f == 0:                                 # the first key touches all four borders
                s0[0, :] = (b[2], b[1], b[0]); s0[h - 1, :] = (b[2], b[1], b[0]); s0[:, 0] = (b[2], b[1], b[0]); s0[:, w - 1] = (b[2], b[1], b[0])
            t = rgb[1]
            s0[h // 2, w // 2] = (t[2], t[1], t[0])    # at least one pixel of the second key: alone, its box is below min_inst_size
        frames.append((s0, s1))

    def expect(s0, s1):
        _, inv, k0, bx = ctx.viode_mask(s0, keys)
        k1 = ctx.viode_mask(s1, keys)[2]
        return [(d["track_id"], d["rect"]) for d in viode.detections(k0, bx, keys, min_size)], inv, k0, k1, bx

    want = [expect(*fr) for fr in frames]
    if nkeys > 1:
        assert (want[0][4][:, 1] < 0).any(), "no absent key in the scene"
        assert any(0 <= b[1] - b[0] < min_size for b in want[0][4] if b[1] >= 0), "no box below min_inst_size in the scene"
        assert any(tuple(b) == (0, h - 1, 0, w - 1) for b in want[0][4]), "no key touching all four borders"
        assert not np.array_equal(want[0][4], want[1][4])
    got = []
    for s0, s1 in frames:
        ctx.viode_frame_enqueue(s0, s1, keys)
        got.append(ctx.viode_frame_collect(min_size))
    for f in (1, 0):                                   # frame 0 is read AFTER frame 1 was enqueued and collected: its buffers must still hold it
        dets, inv, k0, k1 = got[f]
        assert [(d["track_id"], d["rect"]) for d in dets] == want[f][0], f"frame {f}: detections"
        assert all(d["mask"] is None for d in dets)
        assert np.array_equal(download(inv, w * h).reshape(h, w), want[f][1]), f"frame {f}: inverse mask"
        assert np.array_equal(download(k0, 4 * w * h).view(np.uint32).reshape(h, w), want[f][2]), f"frame {f}: left key image"
        assert np.array_equal(download(k1, 4 * w * h).view(np.uint32).reshape(h, w), want[f][3]), f"frame {f}: right key image"
    assert got[0][1] != got[1][1] and got[0][2] != got[1][2]


# ------------------------------------------------------------------ 3. static unmasking ------------------------------------------------------------------
def run_background(variant, n_frames=8):
    """TrackSemanticImage over the scene with a fixed list of static ids -> per frame the background rows.  variant: "masks" (dv_track_unmask_static, host masks), "keys"
    (dv_track_unmask_static_keys, host key image), "keys_dev" (device key image), "none" (no unmasking)"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MODE_SEMANTIC
    seq = sequence()
    ctx = new_ctx(inst=False)
    static_ids = np.array([seq.dyn_keys[0], seq.dyn_keys[2], 99], np.uint32)
    out, keep = [], []
    for k in range(n_frames):
        l, r = seq.frames[k]
        dets = seq.dets[k]
        kimg = ctx_free_key_image(seq, k)
        if variant == "masks":
            ctx.track_unmask_static(dets, static_ids)
        elif variant == "keys":
            ctx.track_unmask_static_keys(dets, static_ids, kimg)
        elif variant == "keys_dev":
            t = torch.from_numpy(kimg.view(np.int32)).cuda(); torch.cuda.synchronize(); keep.append(t)
            ctx.track_unmask_static_keys(dets, static_ids, t.data_ptr(), DV_MEM_DEVICE)
        ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[k], seq.inv_mask_dev[k].data_ptr(), DV_MODE_SEMANTIC, DV_MEM_DEVICE)
        out.append(ctx.track_stereo_collect())
    ctx.close()
    return out


def ctx_free_key_image(seq, k):
    """the left key image of frame k (VIODE::PixelToKey per pixel) in numpy"""
    from dynamic_vins_amd import viode
    s = seq.seg0[k]
    return np.ascontiguousarray(viode.pixel_to_key(s[..., 2], s[..., 1], s[..., 0]))


def test_static_unmasking_from_the_key_image():
    """the same sequence tracked with dv_track_unmask_static (host masks) and with the key form (host and device key image), a fixed list of static ids, 8 frames: the rows
    of dv_track_stereo_collect identical on every frame — and a run without unmasking differs, so the unmasking mattered"""
    a, b, c, n = run_background("masks"), run_background("keys"), run_background("keys_dev"), run_background("none")
    for k in range(len(a)):
        assert len(a[k]) > 20
        rows_equal(a[k], b[k], f"frame {k}: host key image")
        rows_equal(a[k], c[k], f"frame {k}: device key image")
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, n)), "unmasking changed nothing in this scene"


# ------------------------------------------------------------------ 4. runner ------------------------------------------------------------------
KW = dict(max_cnt=150, min_dist=20, max_iters=8, use_det3d=0, mask_morphology_size=5, static_inst_threshold=10.0, extra_from_disparity=False, static_as_background=True)


def record(runner, pipe):
    st, poses, iters, fr = runner.get(0)
    I, S = pipe.est.instances()
    return dict(window=np.ctypeslib.as_array(st.window).copy().tobytes(), state=(st.frame, st.nonlinear), poses=poses.tobytes(), n_poses=len(poses), iterations=iters, frames=fr,
                row_log=runner.row_log(0).tobytes(), frames9=runner.frames(0).tobytes(), instances=I.tobytes(), n_instances=len(I), inst_summary=np.asarray(S).tobytes(),
                static=np.asarray(pipe.est.static_instances()).tobytes(), stats=runner.dynamic_stats(0))


def run_runner(live, tracker_thread, calls):
    from dynamic_vins_amd.backend import Runner
    from dynamic_vins_amd.pipeline import DynamicPipeline
    p = DynamicPipeline(sequence(), live_masks=live, **KW)
    r = Runner([p], group_size=0, threads=1)
    r.set("tracker_thread", tracker_thread)
    for c in calls:
        r.run(c)
    out = record(r, p)
    r.close(); p.ctx.close()
    return out


def runner_reference(tracker_thread):
    key = ("runner", tracker_thread)
    if key not in _CACHE:
        _CACHE[key] = run_runner(False, tracker_thread, (FRAMES - 1,))
    return _CACHE[key]


@pytest.mark.parametrize("tracker_thread,calls", [(0, (FRAMES - 1,)), (1, (FRAMES - 1,)), (0, (6, FRAMES - 7)), (1, (5, 1, FRAMES - 7))])
def test_runner_label_images_equal_precomputed_masks(tracker_thread, calls):
    """dv_runner_set_viode (label images, T1's stage per frame) against dv_runner_set_dynamic fed the pre-computed masks, detections and key images of the same label images:
    row log, window and trajectory, iteration totals, object states, static report and dv_runner_dynamic_stats identical; one-thread order and T2 beside T3; a run cut
    into several dv_runner_run calls equals the uncut run"""
    ref = runner_reference(tracker_thread)
    assert ref["stats"]["object_features"] > 100 and ref["stats"]["frames_with_objects"] >= FRAMES - 2 and ref["n_instances"] >= 2 and ref["state"][1] == 1, ref["stats"]
    got = run_runner(True, tracker_thread, calls)
    for name in ref:
        assert got[name] == ref[name], name


def test_runner_refuses_a_grouped_label_image_sequence():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.backend import Runner
    from dynamic_vins_amd.pipeline import DynamicPipeline
    seq = sequence()
    a, b = DynamicPipeline(seq, **KW), DynamicPipeline(seq, **KW)
    r = Runner([a, b], group_size=2, threads=1)
    with pytest.raises(DvinsError, match="dv_runner_set_viode: a sequence of a dv_batch group is not supported"):
        r._set_viode(0, a, 0)
    r.run(3)                                           # the runner stays usable: both members go on as pre-computed dynamic sequences
    assert r.get(0)[3] == 3 and r.get(1)[3] == 3
    r.close(); a.ctx.close(); b.ctx.close()


# ------------------------------------------------------------------ 5. node ------------------------------------------------------------------
def test_node_live_masks_writes_the_same_trajectory(tmp_path):
    from tests.test_node import NODE, _viode_setup
    seq, sd, cfg = _viode_setup(tmp_path, 24)
    outs = []
    for flag in ([], ["--live-masks"]):
        od = tmp_path / ("out" + str(len(flag)))
        od.mkdir()
        r = subprocess.run([NODE, cfg, str(sd), str(od)] + flag, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "object feature rows" in r.stdout
        outs.append(open(od / "city_day_3_high_VIO_dynamic_PointOnly_Odometry.txt", "rb").read())
    assert len(outs[0].splitlines()) >= 10 and outs[0] == outs[1]


# ------------------------------------------------------------------ 6. errors ------------------------------------------------------------------
def test_errors_name_the_entry_and_leave_the_context_usable():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_HOST, DV_MODE_SEMANTIC
    seq = sequence()
    ctx = new_ctx()
    keys = seq.dyn_keys
    s0, s1 = seq.seg0[0], seq.seg1[0]
    lib, h = ctx.lib, ctx.h

    def fails(rc, name):
        assert rc == -1
        assert name in lib.dv_last_error(h).decode(), lib.dv_last_error(h).decode()

    dets_ok = seq.dets[0]
    assert len(dets_ok) >= 2
    n, p0, p1, p2 = C.c_int(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
    arr = ctx._det_array(dets_ok)
    fails(lib.dv_viode_frame_collect(h, 8, C.addressof(arr), len(arr), C.byref(n), C.byref(p0), C.byref(p1), C.byref(p2)), "dv_viode_frame_collect")          # collect without enqueue
    fails(lib.dv_viode_frame_enqueue(h, s0.ctypes.data, s1.ctypes.data, W - 1, H, 0, DV_MEM_HOST, keys.ctypes.data, len(keys)), "dv_viode_frame_enqueue")      # size mismatch
    fails(lib.dv_viode_frame_enqueue(h, s0.ctypes.data, s1.ctypes.data, W, H, 0, DV_MEM_HOST, keys.ctypes.data, 0), "dv_viode_frame_enqueue")                 # nkeys 0
    big = np.arange(1, 66, dtype=np.uint32)
    fails(lib.dv_viode_frame_enqueue(h, s0.ctypes.data, s1.ctypes.data, W, H, 0, DV_MEM_HOST, big.ctypes.data, 65), "dv_viode_frame_enqueue")                  # nkeys 65
    fails(lib.dv_viode_frame_enqueue(h, s0.ctypes.data, s1.ctypes.data, W, H, 0, 7, keys.ctypes.data, len(keys)), "dv_viode_frame_enqueue")                    # unknown mem
    ctx.viode_frame_enqueue(s0, s1, keys)
    fails(lib.dv_viode_frame_enqueue(h, s0.ctypes.data, s1.ctypes.data, W, H, 0, DV_MEM_HOST, keys.ctypes.data, len(keys)), "dv_viode_frame_enqueue")          # enqueue twice without collect
    dets, inv, k0, k1 = ctx.viode_frame_collect(8)
    assert [d["rect"] for d in dets] == [d["rect"] for d in dets_ok]
    # the key-image entries: a rectangle outside the image, a NULL key image, an unknown mem
    l, r = seq.frames[0]
    ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[0], inv, DV_MODE_SEMANTIC, DV_MEM_DEVICE)
    bad = [dict(d) for d in dets]; bad[0] = dict(bad[0], rect=(W - 4, 10, 30, 30))
    ids = np.array([d["track_id"] for d in dets], np.uint32)
    a_bad, a_ok = ctx._det_array(bad), ctx._det_array(dets)
    fails(lib.dv_inst_track_enqueue_keys(h, seq.times[0], C.addressof(a_bad), len(bad), k0, 0, DV_MEM_DEVICE, None, 0), "dv_inst_track_enqueue_keys")
    fails(lib.dv_inst_track_enqueue_keys(h, seq.times[0], C.addressof(a_ok), len(dets), None, 0, DV_MEM_DEVICE, None, 0), "dv_inst_track_enqueue_keys")
    fails(lib.dv_inst_track_enqueue_keys(h, seq.times[0], C.addressof(a_ok), len(dets), k0, 0, 5, None, 0), "dv_inst_track_enqueue_keys")
    ctx.inst_track_enqueue_keys(seq.times[0], dets, k0, DV_MEM_DEVICE)
    rows0 = ctx.track_stereo_collect()
    i0, f0, _ = ctx.inst_track_collect()
    fails(lib.dv_track_unmask_static_keys(h, C.addressof(a_bad), len(bad), ids.ctypes.data, len(ids), k0, 0, DV_MEM_DEVICE), "dv_track_unmask_static_keys")
    fails(lib.dv_track_unmask_static_keys(h, C.addressof(a_ok), len(dets), ids.ctypes.data, len(ids), None, 0, DV_MEM_DEVICE), "dv_track_unmask_static_keys")
    fails(lib.dv_track_unmask_static_keys(h, C.addressof(a_ok), len(dets), ids.ctypes.data, len(ids), k0, 0, 9), "dv_track_unmask_static_keys")
    # a normal frame succeeds afterwards on the same context — and equals a fresh context's (nothing was left staged by the refused calls)
    assert len(rows0) > 20 and len(i0) == len(dets) and len(f0) > 0
    ref = new_ctx()
    ref.viode_frame_enqueue(s0, s1, keys)
    d2, inv2, k02, k12 = ref.viode_frame_collect(8)
    ref.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[0], inv2, DV_MODE_SEMANTIC, DV_MEM_DEVICE)
    ref.inst_track_enqueue_keys(seq.times[0], d2, k02, DV_MEM_DEVICE)
    rows_equal(rows0, ref.track_stereo_collect(), "background rows after the refused calls")
    rows_equal(f0, ref.inst_track_collect()[1], "object rows after the refused calls")
    # frame 1 on the context that saw the errors
    l, r = seq.frames[1]
    ctx.viode_frame_enqueue(seq.seg0[1], seq.seg1[1], keys)
    dets, inv, k0, k1 = ctx.viode_frame_collect(8)
    ctx.track_unmask_static_keys(dets, ids[:1], k0, DV_MEM_DEVICE)
    ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), seq.times[1], inv, DV_MODE_SEMANTIC, DV_MEM_DEVICE)
    ctx.inst_set_right_keys(k1, DV_MEM_DEVICE)
    ctx.inst_track_enqueue_keys(seq.times[1], dets, k0, DV_MEM_DEVICE)
    assert len(ctx.track_stereo_collect()) > 20 and len(ctx.inst_track_collect()[1]) > 0
    # the host-mask form.  A detection with a negative width or height is refused by the entry's own check, before anything is sized from it
    d2 = seq.dets[2]
    sid = np.array([d["track_id"] for d in d2], np.uint32)
    arr2, masks2 = ctx._det_array(d2), [np.ascontiguousarray(d["mask"], np.uint8) for d in d2]
    for a, m in zip(arr2, masks2):
        a.mask = m.ctypes.data
    w0, h0 = arr2[0].w, arr2[0].h
    for arr2[0].w, arr2[0].h in ((-w0, h0), (w0, -h0)):
        fails(lib.dv_track_unmask_static(h, C.addressof(arr2), len(d2), sid.ctypes.data, len(sid)), "dv_track_unmask_static: bad detection rectangle / mask")
    # ... and what it staged is dropped by a refused dv_track_stereo_enqueue (wrong size): the next frame's working mask is its input mask, byte for byte
    l, r = seq.frames[2]
    mask = seq.inv_mask_dev[2].cpu().numpy().reshape(H, W)
    x, y, w, hh = d2[0]["rect"]
    assert (mask[y:y + hh, x:x + w][masks2[0] >= 1] != 255).any(), "unmasking this detection would change nothing"
    ctx.track_unmask_static(d2, sid)
    fails(lib.dv_track_stereo_enqueue(h, l.data_ptr(), r.data_ptr(), W - 1, H, W, seq.times[2], seq.inv_mask_dev[2].data_ptr(), DV_MODE_SEMANTIC, DV_MEM_DEVICE), "dv_track_stereo")
    ctx.track_stereo_enqueue(l.cpu().numpy(), r.cpu().numpy(), seq.times[2], mask, DV_MODE_SEMANTIC, DV_MEM_HOST)
    ctx.track_stereo_collect()
    got, _ = ctx.front_debug_mask(0)
    assert got[:, :W].tobytes() == mask.tobytes(), "rectangles staged before a refused enqueue were applied to the next frame"
    ctx.close(); ref.close()
