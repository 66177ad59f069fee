"""cfg::is_undistort_input's set-up half (InitOneCamera, utils/camera_model.cpp:479-504): dv_optimal_new_camera (host), dv_init_undistort_map (HIP kernel),
dv_undistort_setup (both on the ctx's cameras + installation + the switch of the lifting cameras), Pipeline(undistort_input=True).

CPU part (`-m "not gpu"`): dv_optimal_new_camera against tests/undistort_ref.py, an independent float64 numpy restatement of cv::getOptimalNewCameraMatrix, and the
properties that need no restatement.  GPU part (`-m gpu`): the map kernel against the oracle's initUndistortRectifyMap bit for bit, the set-up call on a stereo ctx, and the
tracker / pipeline end to end on distorted frames.
"""
import json
import os

import numpy as np
import pytest

from dynamic_vins_amd import ref_configs, sim
from tests import undistort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDISTORT_CONFIGS = ["euroc/euroc.yaml", "custom/mynteye/custom.yaml", "custom/mynteye_vision_only/custom.yaml"]
import re
MAP_TILE = int(re.search(r"#define DV_UMAP_TILE (\d+)", open(os.path.join(ROOT, "dynamic_vins_amd", "csrc", "dv_internal.h")).read()).group(1))      # consecutive pixels per workgroup of the map kernel


def shipped_cameras():
    """the six camera files of the three shipped configurations with undistort_input: 1 -> [(name, cam 8-tuple, w, h)]"""
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_config.json")))
    out = []
    for cfg in UNDISTORT_CONFIGS:
        sc = d["configs"][cfg]["scalars"]
        assert sc["undistort_input"] == "1"
        for key in ("cam0_calib", "cam1_calib"):
            name = os.path.normpath(os.path.join(os.path.dirname(cfg), sc[key].strip('"')))
            c = d["cameras"][name]
            cam = tuple(float(c[k]) for k in ("projection_parameters.fx", "projection_parameters.fy", "projection_parameters.cx", "projection_parameters.cy",
                                              "distortion_parameters.k1", "distortion_parameters.k2", "distortion_parameters.p1", "distortion_parameters.p2"))
            out.append((name, cam, int(c["image_width"]), int(c["image_height"])))
    return out


def random_cameras(n=16, seed=20261017, w=752, h=480):
    """radtan cameras whose polynomial stays monotonic over the image (corner radius <= 0.89 on the normalised plane at the smallest focal length)"""
    rng = np.random.default_rng(seed)
    return [("random%d" % i, (rng.uniform(520, 700), rng.uniform(520, 700), w / 2 + rng.uniform(-20, 20), h / 2 + rng.uniform(-20, 20),
                              rng.uniform(-0.4, 0.1), rng.uniform(-0.02, 0.1), rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3)), w, h) for i in range(n)]


def all_cameras():
    return shipped_cameras() + [("zed", sim.cam_tuple(sim.ZED), 1280, 720)] + random_cameras()


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

def test_optimal_new_camera_matches_the_numpy_restatement():
    """Both sides evaluate the same formulas in double, in different languages and loop orders.  Worst relative difference of any of fx, fy, cx, cy over the six shipped
    cameras, the ZED, 16 random cameras and alpha in {0, 0.5, 1}, measured on the CPU: 4.2e-15 (a few ulp: the restatement divides by fx where the library multiplies by
    1 / fx).  Bound: 5e-14, a factor 12 above it."""
    from dynamic_vins_amd.frontend import optimal_new_camera
    cams = all_cameras()
    assert len(cams) == 6 + 1 + 16
    worst = 0.0
    for name, cam, w, h in cams:
        for alpha in (0.0, 0.5, 1.0):
            lib = np.array(optimal_new_camera(cam, w, h, alpha))
            ref = R.optimal_new_camera(cam, w, h, alpha)
            rel = np.abs(lib / ref - 1).max()
            worst = max(worst, rel)
            assert rel <= 5e-14, (name, alpha, lib, ref)
    print("worst relative difference %.3g" % worst)


def test_optimal_new_camera_without_distortion_is_the_closed_form():
    """D = 0: the grid maps linearly, inner == outer rectangle, and with the declared spacing w / (N - 1) the grid spans [0, w] while the viewport is [0, w - 1]:
    newK = K scaled by (w - 1) / w horizontally and (h - 1) / h vertically, for every alpha"""
    from dynamic_vins_amd.frontend import optimal_new_camera
    for cam, w, h in [((458.654, 457.296, 367.215, 248.375), 752, 480), (sim.cam_tuple(ref_configs.ZED_UN_CAM0)[:4], 1280, 720), ((100.0, 90.0, 17.0, 9.0), 33, 17)]:
        want = R.identity_closed_form(cam, w, h)
        for alpha in (0.0, 0.5, 1.0):
            got = np.array(optimal_new_camera(tuple(cam) + (0.0, 0.0, 0.0, 0.0), w, h, alpha))
            assert np.abs(got / want - 1).max() <= 1e-14, (cam, alpha, got, want)


def test_optimal_new_camera_refuses_bad_input():
    from dynamic_vins_amd.frontend import DvinsError, optimal_new_camera
    cam = sim.cam_tuple(sim.EUROC)
    for bad in [dict(w=1), dict(h=0), dict(alpha=-0.1), dict(alpha=1.5)]:
        kw = dict(w=752, h=480, alpha=0.0); kw.update(bad)
        with pytest.raises(DvinsError):
            optimal_new_camera(cam, kw["w"], kw["h"], kw["alpha"])
    with pytest.raises(DvinsError):      # a polynomial that folds inside the image: the undistorted grid has no inner rectangle
        optimal_new_camera((200.0, 200.0, 376.0, 240.0, -0.4, 0.0, 0.0, 0.0), 752, 480, 0.0)


def _source_samples(m1, m2):
    return m1[..., 0] + (m2 & 31) / 32.0, m1[..., 1] + ((m2 >> 5) & 31) / 32.0


def test_alpha_0_leaves_no_black_border_and_alpha_1_keeps_every_source_pixel(oracle):
    """The property that needs no restatement, on maps the oracle's initUndistortRectifyMap builds from the library's newK for every shipped camera.
    alpha = 0: share of destination pixels whose source sample (map1 + map2 / 32) lies outside [0, w - 1] x [0, h - 1].  It is not zero: the 9 x 9 grid spans
    [0, w] x [0, h] — one pixel more than the image (spacing w / (N - 1)) — and five fixed-point iterations leave the corner points short of convergence.  What the numpy
    restatement ALONE leaves at these cameras: 7.4e-4 (EuRoC cam0 / cam1), 3.5e-4 / 2.9e-4 (MYNT EYE cam0 / cam1).  Cap: 1e-3, and the library may leave no more than the
    restatement does.  alpha = 1: every corner of the source image lies within one pixel of some destination pixel's source sample."""
    from dynamic_vins_amd.frontend import optimal_new_camera
    for name, cam, w, h in shipped_cameras():
        share_ref = R.outside_share(*oracle.init_undistort_map(cam, R.optimal_new_camera(cam, w, h, 0.0), w, h), w, h)
        share_lib = R.outside_share(*oracle.init_undistort_map(cam, optimal_new_camera(cam, w, h, 0.0), w, h), w, h)
        print("%s: outside share restatement %.3g library %.3g" % (name, share_ref, share_lib))
        assert share_ref <= 1e-3 and share_lib <= 1e-3 and share_lib <= share_ref + 1.0 / (w * h), (name, share_ref, share_lib)
        sx, sy = _source_samples(*oracle.init_undistort_map(cam, optimal_new_camera(cam, w, h, 1.0), w, h))
        for cx, cy in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]:
            assert np.maximum(np.abs(sx - cx), np.abs(sy - cy)).min() <= 1.0, (name, cx, cy)


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

EUROC = sim.cam_tuple(sim.EUROC)
STRONG = (611.3, 598.7, 371.9, 236.2, -0.39, 0.09, 1.7e-3, -1.9e-3)          # 752x480 scale: strong barrel distortion with tangential terms


def _scaled(cam, w, h, w0=752, h0=480):
    return (cam[0] * w / w0, cam[1] * h / h0, cam[2] * w / w0, cam[3] * h / h0) + tuple(cam[4:])


def _map_cases(w, h):
    """(camera, newK) triples at size w x h: EuRoC cam0, the strongly distorted camera, D = 0; newK a zoom-out with 1 / fx that is no short binary fraction, so that the
    row walk's additions round"""
    out = []
    for cam in (EUROC, STRONG, EUROC[:4] + (0.0, 0.0, 0.0, 0.0)):
        c = _scaled(cam, w, h)
        out.append((c, (0.7754 * c[0], 0.9123 * c[1], c[2] + 0.37, c[3] - 0.61)))
    return out


@pytest.fixture(scope="module")
def map_ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=64, height=48)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(33, 17), (64, 1), (1, 64), (MAP_TILE - 1, 3), (MAP_TILE + 1, 3), (752, 480)])
def test_init_undistort_map_bit_exact(map_ctx, oracle, w, h):
    """dv_init_undistort_map == the oracle's cv::initUndistortRectifyMap, zero differing elements, host and device destinations; the device destination sits inside a
    guard band that must come back untouched.  Sizes: smaller than a workgroup's tile and odd; one row; one column; a width one less / one more than the tile with
    three rows (pixel pairs straddle the row ends); EuRoC's."""
    import torch
    from dynamic_vins_amd.frontend import optimal_new_camera
    cases = _map_cases(w, h)
    if (w, h) == (752, 480):
        cases.append((EUROC, optimal_new_camera(EUROC, w, h, 0.0)))
    G = 64      # guard elements on each side
    for cam, nk in cases:
        o1, o2 = oracle.init_undistort_map(cam, nk, w, h)
        m1, m2 = map_ctx.init_undistort_map(cam, nk, w, h)
        assert np.count_nonzero(m1 != o1) == 0 and np.count_nonzero(m2 != o2) == 0, (w, h, cam)
        for shift in ((0, 0), (1, 1)) if (w, h) == (33, 17) else ((0, 0),):      # shift (1, 1): destinations that are 2-byte aligned only (the staged path)
            d1 = torch.full((2 * G + 2 * w * h + 4,), 0x5A5A, dtype=torch.int16, device="cuda")
            d2 = torch.full((2 * G + w * h + 4,), 0x3C3C, dtype=torch.int16, device="cuda")
            a1, a2 = G + shift[0], G + shift[1]
            map_ctx.init_undistort_map(cam, nk, w, h, d1.data_ptr() + 2 * a1, d2.data_ptr() + 2 * a2)
            h1, h2 = d1.cpu().numpy(), d2.cpu().numpy()
            assert np.array_equal(h1[a1: a1 + 2 * w * h].reshape(h, w, 2), o1) and np.array_equal(h2[a2: a2 + w * h].view(np.uint16).reshape(h, w), o2)
            assert (h1[:a1] == 0x5A5A).all() and (h1[a1 + 2 * w * h:] == 0x5A5A).all() and (h2[:a2] == 0x3C3C).all() and (h2[a2 + w * h:] == 0x3C3C).all()


@pytest.mark.gpu
def test_init_undistort_map_bit_exact_1280x720(map_ctx, oracle):
    w, h = 1280, 720
    cam = sim.cam_tuple(sim.ZED)
    from dynamic_vins_amd.frontend import optimal_new_camera
    nk = optimal_new_camera(cam, w, h, 0.0)
    o1, o2 = oracle.init_undistort_map(cam, nk, w, h)
    m1, m2 = map_ctx.init_undistort_map(cam, nk, w, h)
    assert np.count_nonzero(m1 != o1) == 0 and np.count_nonzero(m2 != o2) == 0


def _rows_equal(a, b):
    assert len(a) == len(b)
    assert np.array_equal(a["id"], b["id"]) and np.array_equal(a["track_cnt"], b["track_cnt"]) and np.array_equal(a["has_right"], b["has_right"])
    assert np.array_equal(a["left"].view(np.uint64), b["left"].view(np.uint64)) and np.array_equal(a["right"].view(np.uint64), b["right"].view(np.uint64))


@pytest.mark.gpu
def test_undistort_setup_on_a_stereo_ctx(gpu_ctx_factory, oracle):
    """dv_undistort_setup at 96 x 64 with two different cameras: maps, lifting cameras, return values, removal, refusal while a frame is pending"""
    from dynamic_vins_amd import synth
    from dynamic_vins_amd.frontend import DvinsError, cam_tuple, make_cam, optimal_new_camera
    w, h = 96, 64
    cam0 = _scaled(EUROC, w, h)
    cam1 = _scaled((457.587, 456.134, 379.999, 255.238, -0.25, 0.05, -6e-4, 3e-4), w, h)
    kw = dict(width=w, height=h, max_cnt=40, min_dist=8)
    ctx = gpu_ctx_factory(cam0=make_cam(*cam0), cam1=make_cam(*cam1), **kw)
    plain = gpu_ctx_factory(cam0=make_cam(*cam0), cam1=make_cam(*cam1), **kw)
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, w, 50), rng.uniform(0, h, 50)], 1).astype(np.float32)
    lift_orig = oracle.lift_projective(cam0, pts)
    assert np.array_equal(ctx.lift_projective(ctx.cameras()[0], pts).view(np.uint32), lift_orig.view(np.uint32))
    seq = synth.PlaneSequence(w, h, seed=4, disparity=2.0, margin=20)
    l, r = seq.frame(0)
    # refused while a frame is pending, and the refusal changes nothing: the frame in flight and the next one come out as on a ctx that never saw the call
    ctx.track_stereo_enqueue(l, r, 0.0)
    with pytest.raises(DvinsError):
        ctx.undistort_setup()
    assert [cam_tuple(c) for c in ctx.cameras()] == [cam0, cam1]
    with pytest.raises(DvinsError):
        ctx.undistort_maps(0)
    _rows_equal(ctx.track_stereo_collect(), plain.track_stereo(l, r, 0.0))
    l1, r1 = seq.frame(1)
    _rows_equal(ctx.track_stereo(l1, r1, 0.05), plain.track_stereo(l1, r1, 0.05))
    ctx.reset()
    # the set-up itself
    n0, n1 = ctx.undistort_setup()
    nk0, nk1 = optimal_new_camera(cam0, w, h, 0.0), optimal_new_camera(cam1, w, h, 0.0)
    assert cam_tuple(n0) == nk0 + (0.0, 0.0, 0.0, 0.0) and cam_tuple(n1) == nk1 + (0.0, 0.0, 0.0, 0.0)
    assert nk0 != nk1
    assert [cam_tuple(c) for c in ctx.cameras()] == [cam_tuple(n0), cam_tuple(n1)]
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for c, (cam, nk) in enumerate([(cam0, nk0), (cam1, nk1)]):
        o1, o2 = oracle.init_undistort_map(cam, nk, w, h)
        i1, i2 = ctx.undistort_maps(c)
        assert np.array_equal(i1, o1) and np.array_equal(i2, o2)
        assert np.array_equal(ctx.remap(img, i1, i2), oracle.remap(img, o1, o2))
    assert np.array_equal(ctx.lift_projective(ctx.cameras()[0], pts).view(np.uint32), oracle.lift_projective(cam_tuple(n0), pts).view(np.uint32))
    segs = np.concatenate([pts[:10], pts[10:20]], 1)
    assert np.array_equal(ctx.undistort_lines(ctx.cameras()[0], segs), oracle.lift_projective(cam_tuple(n0), segs.reshape(-1, 2)).reshape(-1, 4).astype(np.float64))
    # a distorted frame through the installed maps == the remapped frame through a ctx created with (newK, 0)
    und = gpu_ctx_factory(cam0=n0, cam1=n1, **kw)
    m0, m1 = [oracle.init_undistort_map(cam, nk, w, h) for cam, nk in ((cam0, nk0), (cam1, nk1))]
    _rows_equal(ctx.track_stereo(l, r, 0.0), und.track_stereo(oracle.remap(l, *m0), oracle.remap(r, *m1), 0.0))
    # a second call starts from the original cameras again
    n0b, n1b = ctx.undistort_setup()
    assert cam_tuple(n0b) == cam_tuple(n0) and cam_tuple(n1b) == cam_tuple(n1)
    # the caller's own maps for one camera afterwards: that camera's original intrinsics hold again, the other keeps (newK, 0)
    ctx.set_undistort_maps(1, *m1)
    assert [cam_tuple(c) for c in ctx.cameras()] == [cam_tuple(n0), cam1]
    # removal: maps gone, original cameras back
    ctx.set_undistort_maps(0)
    assert [cam_tuple(c) for c in ctx.cameras()] == [cam0, cam1]
    assert np.array_equal(ctx.lift_projective(ctx.cameras()[0], pts).view(np.uint32), lift_orig.view(np.uint32))
    ctx.reset(); plain.reset()
    _rows_equal(ctx.track_stereo(l, r, 0.0), plain.track_stereo(l, r, 0.0))


@pytest.fixture(scope="module")
def euroc_sequence():
    """20 frames at 320 x 240 from the synthetic renderer through a camera with EuRoC's distortion (two slightly different cameras)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dynamic_vins_amd.pipeline import SyntheticSequence
    w, h = 320, 240
    cam = sim.scaled_cam(sim.EUROC, w, h, 752, 480)
    cam1 = sim.scaled_cam(dict(fx=457.587, fy=456.134, cx=379.999, cy=255.238, k1=-0.28368365, k2=0.07451284, p1=-0.00010473, p2=-3.555907e-05), w, h, 752, 480)
    return SyntheticSequence(w, h, cam, 20, rate=20.0, cam1=cam1)


@pytest.mark.gpu
def test_tracker_with_undistort_setup_matches_the_oracle_on_remapped_frames(gpu_ctx_factory, oracle, euroc_sequence):
    """the shape of test_undistort_input_fused_into_tracking with nothing supplied but the YAML's values: Context.undistort_setup() fed the DISTORTED frames ==
    the oracle tracker built with (newK, 0) and fed the frames the oracle's remap produces with the oracle's maps, bit for bit over 20 frames"""
    from dynamic_vins_amd.frontend import cam_tuple, make_cam, optimal_new_camera
    seq = euroc_sequence
    w, h = seq.w, seq.h
    cam0, cam1 = sim.cam_tuple(seq.cam), sim.cam_tuple(seq.cam1)
    ctx = gpu_ctx_factory(width=w, height=h, max_cnt=100, min_dist=15, cam0=make_cam(*cam0), cam1=make_cam(*cam1))
    n0, n1 = ctx.undistort_setup()
    nk0, nk1 = optimal_new_camera(cam0, w, h), optimal_new_camera(cam1, w, h)
    maps = [oracle.init_undistort_map(cam0, nk0, w, h), oracle.init_undistort_map(cam1, nk1, w, h)]
    trk = oracle.tracker(w, h, 100, 15, 1, 1, nk0 + (0.0,) * 4, nk1 + (0.0,) * 4)
    assert cam_tuple(n0) == nk0 + (0.0,) * 4
    total = stereo = 0
    for k in range(len(seq.frames)):
        l, r = seq.host_frame(k)
        rows = ctx.track_stereo(l, r, seq.times[k])
        _rows_equal(rows, trk.track_image(oracle.remap(l, *maps[0]), oracle.remap(r, *maps[1]), seq.times[k]))
        total += len(rows); stereo += int(rows["has_right"].sum())
    assert total > 20 * 20 and stereo > 20 * 10, (total, stereo)      # the comparison above is not vacuous


@pytest.mark.gpu
def test_pipeline_with_undistort_input_stays_inside_the_ate_bar(euroc_sequence):
    """Pipeline(undistort_input=True) on the distorted frames: the project's ATE bar against ground truth (tests/test_pipeline_parity.py: 0.05 m)"""
    from dynamic_vins_amd.frontend import cam_tuple, optimal_new_camera
    from dynamic_vins_amd.pipeline import Pipeline
    seq = euroc_sequence
    pipe = Pipeline(seq, max_cnt=100, min_dist=15, max_iters=8, use_imu=1, undistort_input=True)
    assert cam_tuple(pipe.cam0) == optimal_new_camera(sim.cam_tuple(seq.cam), seq.w, seq.h) + (0.0,) * 4
    assert cam_tuple(pipe.cam1) == optimal_new_camera(sim.cam_tuple(seq.cam1), seq.w, seq.h) + (0.0,) * 4
    for k in range(len(seq.frames)):
        pipe.step()
    assert len(pipe.poses) >= 5
    ate = pipe.ate()
    pipe.ctx.close()
    print("ATE %.4g m over %d poses" % (ate, len(pipe.poses)))
    assert ate < 0.05, ate


@pytest.mark.gpu
def test_ctx_without_undistort_setup_is_unchanged(gpu_ctx_factory, euroc_sequence):
    """two contexts in one run: one that never calls undistort_setup and one that called it and removed the maps again track the same 20 frames to the same bytes"""
    from dynamic_vins_amd.frontend import make_cam
    seq = euroc_sequence
    kw = dict(width=seq.w, height=seq.h, max_cnt=100, min_dist=15, cam0=make_cam(*sim.cam_tuple(seq.cam)), cam1=make_cam(*sim.cam_tuple(seq.cam1)))
    a, b = gpu_ctx_factory(**kw), gpu_ctx_factory(**kw)
    b.undistort_setup(); b.set_undistort_maps(0)
    for k in range(len(seq.frames)):
        l, r = seq.host_frame(k)
        ra, rb = a.track_stereo(l, r, seq.times[k]), b.track_stereo(l, r, seq.times[k])
        assert ra.tobytes() == rb.tobytes(), k
