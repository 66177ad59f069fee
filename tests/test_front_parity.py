"""GPU parity tests: HIP front end (through the C ABI) vs the CPU oracle on the same seeded inputs.
Bar: bit-exact — the path is u8/int16/int32/int64 arithmetic plus a handful of correctly-rounded
fp32/fp64 operations evaluated in the same order on both sides (no FMA contraction)."""
import numpy as np
import pytest

from dynamic_vins_amd import synth

pytestmark = pytest.mark.gpu

ZED = (701.406049185687, 700.7199834541797, 663.9703743586792, 362.02045484177154,
       -0.17198906485492285, 0.024624053031210322, 0.0003391614313509814, -0.00045583634752113735)


def _cam(p):
    from dynamic_vins_amd.frontend import make_cam
    return make_cam(*p)


def _img(h, w, seed):
    return np.ascontiguousarray((synth.texture(h, w, seed) * 255).astype(np.uint8))


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=320, height=240, max_cnt=150, min_dist=15, cam0=_cam(ZED), cam1=_cam(ZED))


@pytest.mark.parametrize("hw", [(240, 320), (480, 752), (375, 1242), (188, 621), (94, 311), (33, 47), (720, 1280)])
def test_pyr_down_bit_exact(ctx, oracle, hw):
    img = _img(hw[0], hw[1], 7)
    got = ctx.pyr_down(img)
    ref = oracle.pyr_down(img)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)


def _pair(h, w, dx, dy, seed=3):
    seq = synth.PlaneSequence(w, h, seed=seed, margin=64)
    X, Y = seq.u + seq.m, seq.v + seq.m
    a = synth.sample(seq.tex, X, Y)
    b = synth.sample(seq.tex, X - dx, Y - dy)
    return a, b


@pytest.mark.parametrize("hw,shift", [((240, 320), (3.3, -1.7)), ((480, 752), (-9.6, 6.2)), ((375, 1242), (14.2, 0.4)), ((120, 160), (0.6, 0.3))])
def test_lk_generic_bit_exact(ctx, oracle, hw, shift):
    a, b = _pair(hw[0], hw[1], *shift)
    pts = oracle.gftt(a, 200, 0.01, 12)
    # add points near / beyond the border to exercise the reflect path and status clearing
    extra = np.array([[1.5, 2.5], [hw[1] - 2.2, hw[0] - 1.7], [0.0, 0.0], [hw[1] - 1.0, 5.0], [hw[1] / 2, 0.4]], np.float32)
    pts = np.vstack([pts, extra])
    for ml in (3, 1, 0):
        gp, gs = ctx.lk(a, b, pts, max_level=ml)
        rp, rs = oracle.lk(a, b, pts, max_level=ml)
        assert np.array_equal(gs, rs), f"status differs at max_level {ml}"
        assert np.array_equal(gp.view(np.uint32), rp.view(np.uint32)), f"positions differ at max_level {ml}"
    # recovered flow is the true shift (sanity of the oracle itself)
    rp, rs = oracle.lk(a, b, pts[:-5], max_level=3)
    d = (rp - pts[:-5])[rs > 0]
    assert abs(np.median(d[:, 0]) - shift[0]) < 0.1 and abs(np.median(d[:, 1]) - shift[1]) < 0.1


def test_lk_initial_flow_bit_exact(ctx, oracle):
    a, b = _pair(240, 320, 2.4, 1.1)
    pts = oracle.gftt(a, 120, 0.01, 12)
    init = pts + np.float32([2.0, 1.0])
    gp, gs = ctx.lk(a, b, pts, max_level=1, initial=init)
    rp, rs = oracle.lk(a, b, pts, max_level=1, initial=init)
    assert np.array_equal(gs, rs)
    assert np.array_equal(gp.view(np.uint32), rp.view(np.uint32))


@pytest.mark.parametrize("hw,shift,thr", [((240, 320), (3.3, -1.7), 0.5), ((480, 752), (-7.6, 4.2), 0.5), ((720, 1280), (11.0, -3.0), 1.0)])
def test_track_by_lk_bit_exact(ctx, oracle, hw, shift, thr):
    """FeatureTrackByLK: fwd + bwd + distance + InBorder fused in one launch."""
    a, b = _pair(hw[0], hw[1], *shift)
    pts = oracle.gftt(a, 300, 0.01, 15)
    gp, gs = ctx.track_by_lk(a, b, pts, True, thr)
    rp, rs = oracle.track_by_lk(a, b, pts, True, thr)
    assert np.array_equal(gs, rs)
    assert np.array_equal(gp.view(np.uint32), rp.view(np.uint32))
    assert gs.sum() > 0.8 * len(pts)
    gp, gs = ctx.track_by_lk(a, b, pts, False, thr)
    rp, rs = oracle.track_by_lk(a, b, pts, False, thr)
    assert np.array_equal(gs, rs) and np.array_equal(gp.view(np.uint32), rp.view(np.uint32))


@pytest.mark.parametrize("hw", [(240, 320), (480, 752), (375, 1242), (65, 130), (16, 64), (17, 65)])
def test_min_eigen_bit_exact(ctx, oracle, hw):
    img = _img(hw[0], hw[1], 11)
    got = ctx.min_eigen(img)
    ref = oracle.min_eigen(img)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("hw,max_n,md", [((240, 320), 150, 15), ((480, 752), 150, 30), ((375, 1242), 250, 25), ((240, 320), 0, 8),
                                         ((240, 320), 40, 4), ((240, 320), 500, 0)])
def test_gftt_exact(ctx, oracle, hw, max_n, md):
    img = _img(hw[0], hw[1], 5)
    got = ctx.gftt(img, max_n, 0.01, md)
    ref = oracle.gftt(img, max_n if max_n > 0 else 1024, 0.01, md)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)


def test_gftt_masked_and_chunked(ctx, oracle):
    """720p: > 8192 surviving candidates forces the value-ordered chunk path; mask with discs."""
    img = _img(720, 1280, 9)
    rng = np.random.default_rng(2)
    mask = np.full((720, 1280), 255, np.uint8)
    mask[100:300, 200:700] = 0
    pts = rng.uniform([0, 0], [1280, 720], (120, 2)).astype(np.float32)
    mask_o = oracle.circle_mask(mask, pts, 25)
    mask_g = ctx.circle_mask(mask, pts, 25)
    assert np.array_equal(mask_o, mask_g)
    got = ctx.gftt(img, 1000, 0.001, 6, mask_g)
    ref = oracle.gftt(img, 1000, 0.001, 6, mask_o)
    assert np.array_equal(got, ref)
    assert len(got) == 1000


def test_gftt_empty_and_flat(ctx, oracle):
    flat = np.full((64, 96), 128, np.uint8)
    assert len(ctx.gftt(flat, 10, 0.01, 5)) == 0 == len(oracle.gftt(flat, 10, 0.01, 5))
    img = _img(64, 96, 1)
    zero_mask = np.zeros((64, 96), np.uint8)
    assert len(ctx.gftt(img, 10, 0.01, 5, zero_mask)) == 0 == len(oracle.gftt(img, 10, 0.01, 5, zero_mask))


@pytest.mark.parametrize("hw", [(240, 320), (480, 752), (375, 1242), (720, 1280), (65, 130), (16, 64), (17, 65)])
def test_min_eigen_cuda_bit_exact(ctx, oracle, hw):
    """cv::cuda::createMinEigenValCorner(CV_8UC1, 3, 3): the GPU detector's response map (row F5, oracle/gftt_cuda.cpp) — float multiply-add chains, bit for bit"""
    img = _img(hw[0], hw[1], 11)
    got = ctx.min_eigen(img, rule="cuda")
    ref = oracle.min_eigen(img, rule="cuda")
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not np.array_equal(ref.view(np.uint32), oracle.min_eigen(img).view(np.uint32))      # ... and not the CPU detector's map


@pytest.mark.parametrize("hw,max_n,md", [((240, 320), 150, 15), ((480, 752), 150, 30), ((375, 1242), 250, 25), ((720, 1280), 250, 25), ((240, 320), 0, 8),
                                         ((240, 320), 40, 4), ((240, 320), 500, 0)])
def test_gftt_cuda_exact(ctx, oracle, hw, max_n, md):
    """DetectShiTomasiCornersGpu (feature_utils.cpp:339-348): cv::cuda::GoodFeaturesToTrackDetector::detect, without and with a mask that hides the strongest corners
    (the threshold is 1 % of the maximum over the whole image, not of the maximum under the mask)"""
    img = _img(hw[0], hw[1], 5)
    got = ctx.gftt(img, max_n, 0.01, md, rule="cuda")
    ref = oracle.gftt(img, max_n if max_n > 0 else 1024, 0.01, md, rule="cuda")
    assert got.shape == ref.shape and np.array_equal(got, ref)
    mask = np.full(hw, 255, np.uint8)
    top = oracle.gftt(img, 30, 0.01, max(md, 4), rule="cuda")
    mask = oracle.circle_mask(mask, top, 12)                   # discs over the 30 strongest corners
    mask[hw[0] // 3: hw[0] // 2, hw[1] // 4: hw[1] // 2] = 0
    got = ctx.gftt(img, max_n, 0.01, md, mask, rule="cuda")
    ref = oracle.gftt(img, max_n if max_n > 0 else 1024, 0.01, md, mask, rule="cuda")
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert len(got) > 0 and (mask[got[:, 1].astype(int), got[:, 0].astype(int)] != 0).all()


def test_gftt_cuda_masked_720p_chunked_and_degenerate(ctx, oracle):
    """720p with a low quality level (more surviving candidates than one LDS chunk holds), the tracker's analytic discs expressed as a mask, and the degenerate inputs"""
    img = _img(720, 1280, 9)
    rng = np.random.default_rng(2)
    mask = np.full((720, 1280), 255, np.uint8)
    mask[100:300, 200:700] = 0
    pts = rng.uniform([0, 0], [1280, 720], (120, 2)).astype(np.float32)
    mask = oracle.circle_mask(mask, pts, 25)
    got = ctx.gftt(img, 1000, 0.001, 6, mask, rule="cuda")
    ref = oracle.gftt(img, 1000, 0.001, 6, mask, rule="cuda")
    assert np.array_equal(got, ref) and len(got) == 1000
    flat = np.full((64, 96), 128, np.uint8)
    assert len(ctx.gftt(flat, 10, 0.01, 5, rule="cuda")) == 0 == len(oracle.gftt(flat, 10, 0.01, 5, rule="cuda"))
    small = _img(64, 96, 1)
    zero_mask = np.zeros((64, 96), np.uint8)
    assert len(ctx.gftt(small, 10, 0.01, 5, zero_mask, rule="cuda")) == 0 == len(oracle.gftt(small, 10, 0.01, 5, zero_mask, rule="cuda"))
    # the strongest response hidden by the mask raises the threshold for everything else (the CPU detector's threshold would come from under the mask)
    hot = small.copy()
    hot[20:36, 40:56] = 0
    hot[28:36, 48:56] = 255
    m = np.full((64, 96), 255, np.uint8)
    m[12:44, 32:64] = 0
    a, b = ctx.gftt(hot, 500, 0.01, 2, m, rule="cuda"), oracle.gftt(hot, 500, 0.01, 2, m, rule="cuda")
    assert np.array_equal(a, b) and len(a) < len(ctx.gftt(hot, 500, 0.01, 2, m))


@pytest.mark.parametrize("radius", [0, 1, 4, 20, 25, 30])
def test_circle_mask_bit_exact(ctx, oracle, radius):
    rng = np.random.default_rng(radius)
    mask = np.full((120, 200), 255, np.uint8)
    pts = rng.uniform([-10, -10], [210, 130], (40, 2)).astype(np.float32)
    pts[0] = [0.5, 0.5]
    pts[1] = [199.5, 119.5]
    assert np.array_equal(ctx.circle_mask(mask, pts, radius), oracle.circle_mask(mask, pts, radius))


@pytest.mark.parametrize("k", [1, 5, 10, 20])
def test_erode_bit_exact(ctx, oracle, k):
    rng = np.random.default_rng(k)
    mask = (rng.uniform(0, 1, (97, 131)) > 0.02).astype(np.uint8) * 255
    assert np.array_equal(ctx.erode(mask, k), oracle.erode(mask, k))


def test_lift_projective_bit_exact(ctx, oracle):
    rng = np.random.default_rng(0)
    pts = rng.uniform([0, 0], [1280, 720], (500, 2)).astype(np.float32)
    got = ctx.lift_projective(_cam(ZED), pts)
    ref = oracle.lift_projective(ZED, pts)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    nod = ZED[:4] + (0.0, 0.0, 0.0, 0.0)
    assert np.array_equal(ctx.lift_projective(_cam(nod), pts).view(np.uint32), oracle.lift_projective(nod, pts).view(np.uint32))


def _rows_equal(g, r):
    assert len(g) == len(r), f"feature count {len(g)} vs {len(r)}"
    for name in ("id", "track_cnt", "has_right"):
        assert np.array_equal(g[name], r[name]), name
    assert np.array_equal(g["left"].view(np.uint64), r["left"].view(np.uint64)), "left observation"
    assert np.array_equal(g["right"].view(np.uint64), r["right"].view(np.uint64)), "right observation"


@pytest.mark.parametrize("w,h,max_cnt,min_dist,frames", [(320, 240, 80, 15, 12), (752, 480, 150, 30, 8)])
def test_track_image_sequence_bit_exact(gpu_ctx_factory, oracle, w, h, max_cnt, min_dist, frames):
    """FeatureTracker::TrackImage over a sequence: ids, track counts, stereo flags and every Vec7d
    (undistorted point, pixel, velocity) identical to the oracle, frame after frame."""
    cam = (w * 0.55, w * 0.55, w / 2 - 3.1, h / 2 + 2.2) + ZED[4:]
    c = gpu_ctx_factory(width=w, height=h, max_cnt=max_cnt, min_dist=min_dist, cam0=_cam(cam), cam1=_cam(cam))
    o = oracle.tracker(w, h, max_cnt, min_dist, 1, 1, cam, cam)
    seq = synth.PlaneSequence(w, h, seed=21, disparity=9.25)
    total_tracked = 0
    for k in range(frames):
        left, right = seq.frame(k)
        t = 0.05 * k
        g = c.track_stereo(left, right, t)
        r = o.track_image(left, right, t)
        _rows_equal(g, r)
        if k:
            total_tracked += int((g["track_cnt"] > 1).sum())
    assert total_tracked > frames * max_cnt * 0.5      # the sequence really is tracked, not re-detected
    assert g["has_right"].sum() > 0.5 * len(g)


def test_track_image_naive_masked_bit_exact(gpu_ctx_factory, oracle):
    w, h, max_cnt, min_dist = 320, 240, 90, 12
    cam = (180.0, 181.0, 158.0, 121.0) + ZED[4:]
    c = gpu_ctx_factory(width=w, height=h, max_cnt=max_cnt, min_dist=min_dist, cam0=_cam(cam), cam1=_cam(cam))
    o = oracle.tracker(w, h, max_cnt, min_dist, 1, 1, cam, cam)
    seq = synth.PlaneSequence(w, h, seed=5, disparity=6.5)
    from dynamic_vins_amd.frontend import DV_MODE_NAIVE
    for k in range(8):
        left, right = seq.frame(k)
        mask = np.full((h, w), 255, np.uint8)
        mask[60:140, 100 + 5 * k:190 + 5 * k] = 0       # a moving "object" region
        g = c.track_stereo(left, right, 0.1 * k, mask, DV_MODE_NAIVE)
        r = o.track_image(left, right, 0.1 * k, mask, naive=True)
        _rows_equal(g, r)


def test_track_image_naive_720p_uses_the_gpu_detector(gpu_ctx_factory, oracle):
    """TrackImageNaive at the headline size: temporal + right tracking by the GPU tracker's rule and NEW corners by the GPU detector's rule (DetectNewFeature(img, true, ...),
    background_tracker.cpp:445) — rows bit for bit against the oracle, and different from what the CPU detector's rule (rounds 1-5) selects under the same mask."""
    w, h, max_cnt, min_dist = 1280, 720, 250, 25
    c = gpu_ctx_factory(width=w, height=h, max_cnt=max_cnt, min_dist=min_dist, cam0=_cam(ZED), cam1=_cam(ZED))
    o = oracle.tracker(w, h, max_cnt, min_dist, 1, 1, ZED, ZED)
    o_cpu = oracle.tracker(w, h, max_cnt, min_dist, 1, 1, ZED, ZED)
    seq = synth.PlaneSequence(w, h, seed=8, disparity=9.5)
    from dynamic_vins_amd.frontend import DV_MODE_NAIVE
    differs = False
    for k in range(4):
        left, right = seq.frame(k)
        mask = np.full((h, w), 255, np.uint8)
        mask[200:520, 300 + 12 * k:760 + 12 * k] = 0
        left, right = [np.where(mask == 0, im, (im.astype(np.float32) * 0.12 + 110).astype(np.uint8)) for im in (left, right)]      # a dim scene around a bright (masked) object
        g = c.track_stereo(left, right, 0.05 * k, mask, DV_MODE_NAIVE)
        r = o.track_image(left, right, 0.05 * k, mask, naive=True)
        _rows_equal(g, r)
        oracle.lib.dvo_set_variant(b"f5_cpu_rule", 1)
        try:
            rc = o_cpu.track_image(left, right, 0.05 * k, mask, naive=True)
        finally:
            oracle.lib.dvo_set_variant(b"f5_cpu_rule", 0)
        differs = differs or len(rc) != len(r) or not np.array_equal(rc["left"], r["left"])
    assert len(g) > 100 and differs


@pytest.mark.parametrize("mode,erode_k", [(2, 0), (2, 7), (1, 5)])
def test_track_semantic_image_and_mask_erosion_bit_exact(gpu_ctx_factory, oracle, mode, erode_k):
    """TrackSemanticImage (background half of dynamic mode: temporal LK by the CPU rule, right image by the GPU rule) and the
    in-tracker erosion of the inverse instance mask (use_mask_morphology)"""
    w, h, max_cnt, min_dist = 320, 240, 90, 12
    cam = (180.0, 181.0, 158.0, 121.0) + ZED[4:]
    c = gpu_ctx_factory(width=w, height=h, max_cnt=max_cnt, min_dist=min_dist, cam0=_cam(cam), cam1=_cam(cam), mask_morphology_size=erode_k)
    o = oracle.tracker(w, h, max_cnt, min_dist, 1, 1, cam, cam)
    seq = synth.PlaneSequence(w, h, seed=6, disparity=6.5)
    for k in range(7):
        left, right = seq.frame(k)
        mask = np.full((h, w), 255, np.uint8)
        mask[50:150, 90 + 6 * k:200 + 6 * k] = 0
        mask[200:204, 10:14] = 0                           # a speck the erosion grows
        g = c.track_stereo(left, right, 0.1 * k, mask, mode)
        r = o.track_image(left, right, 0.1 * k, mask, mode=mode, erode_k=erode_k)
        _rows_equal(g, r)
    assert len(g) > 40


def test_mono_and_reset(gpu_ctx_factory, oracle):
    w, h = 320, 240
    cam = (200.0, 200.0, 160.0, 120.0, 0, 0, 0, 0)
    c = gpu_ctx_factory(width=w, height=h, max_cnt=60, min_dist=20, stereo=0, cam0=_cam(cam), cam1=_cam(cam))
    seq = synth.PlaneSequence(w, h, seed=8)
    for rep in range(2):
        o = oracle.tracker(w, h, 60, 20, 1, 0, cam, cam)
        for k in range(4):
            left, _ = seq.frame(k)
            _rows_equal(c.track_stereo(left, None, 0.05 * k), o.track_image(left, None, 0.05 * k))
        c.reset()


def test_error_behaviour(ctx):
    from dynamic_vins_amd import DvinsError
    img = _img(240, 320, 1)
    with pytest.raises(DvinsError):
        ctx.track_by_lk(img, img, np.zeros((0, 2), np.float32))      # reference: std::runtime_error on empty input
    with pytest.raises(DvinsError):
        ctx.track_stereo(_img(100, 100, 1), None, 0.0, w=100, h=100)   # size mismatch (reference: std::terminate)


def test_error_behaviour_of_the_round6_entries(gpu_ctx_factory):
    """every new entry point refuses what it cannot do and leaves the context usable: an unknown memory kind, the static-instance unmasking without a mask / behind the frame's
    enqueue / with a rectangle outside the image, a key image without an object tracker or with a bad stride, the GPU detector's argument checks"""
    import ctypes as C
    from dynamic_vins_amd import DvinsError
    from dynamic_vins_amd.frontend import DV_MODE_SEMANTIC
    w, h = 160, 120
    ctx = gpu_ctx_factory(width=w, height=h, max_cnt=40, min_dist=10, cam0=_cam(ZED), cam1=_cam(ZED))
    img = _img(h, w, 3)
    with pytest.raises(DvinsError, match="memory kind"):
        ctx.track_stereo(img, img, 0.0, None, 0, 7)
    with pytest.raises(DvinsError):
        ctx.gftt(img, 10, 0.0, 5, rule="cuda")                    # qualityLevel must be > 0 (the CUDA detector asserts the same)
    with pytest.raises(DvinsError):
        ctx.inst_set_right_keys(np.zeros((h, w), np.uint32))      # no object tracker configured
    det = dict(track_id=5, rect=(10, 10, 20, 20), mask=np.full((20, 20), 255, np.uint8))
    ctx.track_unmask_static([det], [5])
    with pytest.raises(DvinsError, match="no mask"):
        ctx.track_stereo(img, img, 0.0, None, DV_MODE_SEMANTIC)   # the unmasking was asked for a frame that carries no mask
    bad = dict(track_id=5, rect=(150, 110, 20, 20), mask=np.full((20, 20), 255, np.uint8))
    with pytest.raises(DvinsError, match="rectangle"):
        ctx.track_unmask_static([bad], [5])
    # an id that is not static, or no ids at all: nothing is staged, the frame runs as usual; and a staged unmask really clears the mask for the tracker
    mask = np.full((h, w), 255, np.uint8); mask[10:30, 10:30] = 0
    ctx.track_unmask_static([det], [6]); a = ctx.track_stereo(img, img, 0.0, mask, DV_MODE_SEMANTIC)
    ctx.reset()
    ctx.track_unmask_static([det], [5]); b = ctx.track_stereo(img, img, 0.0, mask, DV_MODE_SEMANTIC)
    ctx.reset()
    c = ctx.track_stereo(img, img, 0.0, np.full((h, w), 255, np.uint8), DV_MODE_SEMANTIC)
    inside = lambda r: int(((r["left"][:, 3] >= 10) & (r["left"][:, 3] < 30) & (r["left"][:, 4] >= 10) & (r["left"][:, 4] < 30)).sum())
    assert inside(a) == 0 and b.tobytes() == c.tobytes()          # unmasked == no object at all
    ctx.inst_config(20, 5, 0)
    with pytest.raises(DvinsError, match="stride"):
        ctx._check(ctx.lib.dv_inst_set_right_keys(ctx.h, np.zeros((h, w), np.uint32).ctypes.data, 6, 0))
    ctx.inst_set_right_keys(None)


def test_instance_tracker_bit_exact(gpu_ctx_factory, oracle):
    """one object instance through InstsFeatManager::InstsTrack (row F10): a textured box drifting and growing over a
    moving background; ROI crops of changing size, eroded instance mask, box offset, right-image tracking"""
    from dynamic_vins_amd.frontend import InstFeat
    W, H = 320, 240
    cam = (180.0, 181.0, 158.0, 121.0) + ZED[4:]
    ctx = gpu_ctx_factory(width=W, height=H, max_cnt=30, min_dist=10, cam0=_cam(cam), cam1=_cam(cam))
    seq = synth.PlaneSequence(W, H, seed=9, disparity=5.5)
    obj_tex = np.clip(synth.texture(200, 260, seed=123) * 255.0 + 0.5, 0, 255).astype(np.uint8)
    inst = InstFeat(ctx, _cam(cam), _cam(cam), max_cnt=40, min_dist=4, flow_back=True)
    InstFeat.global_id_count = 1
    o_last, o_ids, o_cnt, o_prev, gid = np.zeros((0, 2), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.int32), None, 1
    tracked = 0
    for k in range(7):
        left, right = seq.frame(k)
        left, right = left.copy(), right.copy()
        x0, y0, bw, bh = 60 + 4 * k, 50 + 2 * k, 90 + 3 * k, 70 + 2 * k                 # the 2-D box drifts and grows
        patch = obj_tex[20 + k:20 + k + bh, 30:30 + bw]
        left[y0:y0 + bh, x0:x0 + bw] = patch
        right[y0:y0 + bh, x0 - 6:x0 - 6 + bw] = patch                                       # the object is closer: disparity 6
        roi = left[y0:y0 + bh, x0:x0 + bw].copy()
        mask = np.zeros((bh, bw), np.uint8); mask[6:-6, 8:-8] = 255
        g = inst.Track(roi, mask, (x0, y0), left, right)
        r, gid = oracle.inst_track(o_prev, roi, mask, (x0, y0), left, right, cam, cam, o_last, o_ids, o_cnt, 40, 4, 1, gid)
        for key in ("curr_points", "curr_un_points", "right_points", "right_un_points"):
            assert np.array_equal(g[key].view(np.uint32), r[key].view(np.uint32)), (k, key)
        for key in ("ids", "track_cnt", "right_ids"):
            assert np.array_equal(g[key], r[key]), (k, key)
        o_last, o_ids, o_cnt, o_prev = r["curr_points"], r["ids"], r["track_cnt"], roi
        tracked += int((g["track_cnt"] > 1).sum())
        assert len(g["curr_points"]) > 10 and (k == 0 or len(g["right_points"]) > 3)
    assert tracked > 40 and InstFeat.global_id_count == gid


@pytest.mark.parametrize("w,h", [(64, 48), (333, 97), (1280, 720)])
def test_bgr2gray_and_colour_input_bit_exact(gpu_ctx_factory, oracle, w, h):
    """row N2: cvtColor(BGR2GRAY) fused into pyramid level 0 — operator parity, the mono8 -> BGR -> gray identity
    (1868 + 9617 + 4899 = 16384), and TrackImage fed BGR frames == TrackImage fed the converted gray frames"""
    from dynamic_vins_amd.frontend import DV_FMT_BGR, DV_MEM_HOST, DV_MODE_RAW
    rng = np.random.default_rng(w)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ctx = gpu_ctx_factory(width=w, height=h, max_cnt=60, min_dist=12)
    g = ctx.bgr2gray(bgr)
    assert np.array_equal(g, oracle.bgr2gray(bgr))
    ref = ((bgr[..., 0].astype(np.int64) * 1868 + bgr[..., 1].astype(np.int64) * 9617 + bgr[..., 2].astype(np.int64) * 4899 + 8192) >> 14).astype(np.uint8)
    assert np.array_equal(g, ref)
    gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
    assert np.array_equal(ctx.bgr2gray(np.repeat(gray[..., None], 3, 2)), gray)
    if w >= 320:
        return
    seq = synth.PlaneSequence(w, h, seed=4, disparity=2.5, margin=40)
    c2 = gpu_ctx_factory(width=w, height=h, max_cnt=60, min_dist=12)
    for k in range(3):
        l, r = seq.frame(k)
        lb, rb = np.repeat(l[..., None], 3, 2), np.repeat(r[..., None], 3, 2)
        lb[..., 0] = np.clip(lb[..., 0].astype(int) + 9, 0, 255); rb[..., 2] = np.clip(rb[..., 2].astype(int) - 7, 0, 255)     # real colour
        a = ctx.track_stereo(np.ascontiguousarray(lb), np.ascontiguousarray(rb), 0.05 * k, None, DV_MODE_RAW, DV_MEM_HOST | DV_FMT_BGR, stride=3 * w)
        b = c2.track_stereo(oracle.bgr2gray(lb), oracle.bgr2gray(rb), 0.05 * k)
        _rows_equal(a, b)


def _rand_maps(rng, w, h):
    """smooth warp + a band of far-out-of-range and border-straddling coordinates, every fractional cell"""
    yy, xx = np.mgrid[0:h, 0:w]
    u = xx + 6 * np.sin(yy / 17.0) + rng.uniform(-1.5, 1.5, (h, w))
    v = yy + 5 * np.cos(xx / 23.0) + rng.uniform(-1.5, 1.5, (h, w))
    u[: h // 6] -= 9; v[:, : w // 8] -= 7; u[-h // 7:] += 8; v[:, -w // 9:] += 6          # rows / columns that leave the image on each side
    iu, iv = np.rint(u * 32).astype(np.int64), np.rint(v * 32).astype(np.int64)
    m1 = np.stack([iu >> 5, iv >> 5], -1).astype(np.int16)
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    m1[0, 0] = (-300, 5); m1[0, 1] = (w + 40, h + 40); m1[1, 0] = (-1, -1); m1[1, 1] = (w - 1, h - 1); m1[1, 2] = (w, 3); m1[2, 0] = (3, h)
    m2[3, :32] = np.arange(32); m2[4, :32] = np.arange(32) * 32; m1[3, :32] = (w // 2, h // 2); m1[4, :32] = (w // 2, h // 2)
    return m1, m2


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 48), (333, 201), (1280, 720)])
def test_remap_bit_exact(gpu_ctx_factory, oracle, w, h):
    """row N2: cv::remap(INTER_LINEAR, fixed-point maps, BORDER_CONSTANT) on 1- and 3-channel images, random warps with out-of-range
    coordinates and realistic undistortion maps"""
    rng = np.random.default_rng(w + h)
    ctx = gpu_ctx_factory(width=64, height=48)
    gray = rng.integers(0, 256, (h, w), dtype=np.uint8)
    bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    cam = (0.7 * w, 0.72 * w, w / 2 + 3.3, h / 2 - 2.1, -0.28, 0.07, 1e-3, -7e-4)
    maps = [_rand_maps(rng, w, h), oracle.init_undistort_map(cam, (0.62 * w, 0.64 * w, w / 2, h / 2), w, h)]
    for m1, m2 in maps:
        assert np.array_equal(ctx.remap(gray, m1, m2), oracle.remap(gray, m1, m2))
        assert np.array_equal(ctx.remap(bgr, m1, m2), oracle.remap(bgr, m1, m2))
    # identity map: the image itself; one whole pixel to the right: shifted with a zero column
    yy, xx = np.mgrid[0:h, 0:w]
    ident = np.stack([xx, yy], -1).astype(np.int16)
    assert np.array_equal(ctx.remap(gray, ident, np.zeros((h, w), np.uint16)), gray)
    sh = ctx.remap(gray, ident + np.array([1, 0], np.int16), np.zeros((h, w), np.uint16))
    assert np.array_equal(sh[:, :-1], gray[:, 1:]) and not sh[:, -1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [True, False])
def test_undistort_input_fused_into_tracking(gpu_ctx_factory, oracle, colour):
    """cfg::is_undistort_input: the tracker fed DISTORTED (colour or gray) frames with the maps installed == the tracker fed the frames
    that cv::remap + cv::cvtColor produce (ImageProcessor::Run, image_process.cpp:109-126), bit for bit"""
    from dynamic_vins_amd.frontend import DV_FMT_BGR, DV_MEM_HOST, DV_MODE_RAW, make_cam
    w, h = 200, 152
    cam = (150.0, 151.0, 101.3, 74.2, -0.25, 0.06, 8e-4, -5e-4)
    new_k = (128.0, 129.0, 100.0, 76.0)
    undist_cam = make_cam(new_k[0], new_k[1], new_k[2], new_k[3], 0, 0, 0, 0)
    m1l, m2l = oracle.init_undistort_map(cam, new_k, w, h)
    cam_r = (151.0, 150.0, 99.1, 77.4, -0.22, 0.04, -6e-4, 3e-4)
    m1r, m2r = oracle.init_undistort_map(cam_r, new_k, w, h)
    a = gpu_ctx_factory(width=w, height=h, max_cnt=60, min_dist=12, cam0=undist_cam, cam1=undist_cam)
    b = gpu_ctx_factory(width=w, height=h, max_cnt=60, min_dist=12, cam0=undist_cam, cam1=undist_cam)
    a.set_undistort_maps(0, m1l, m2l)
    a.set_undistort_maps(1, m1r, m2r)
    seq = synth.PlaneSequence(w, h, seed=6, disparity=2.5, margin=40)
    total = 0
    for k in range(4):
        l, r = seq.frame(k)
        if colour:
            l, r = np.repeat(l[..., None], 3, 2), np.repeat(r[..., None], 3, 2)
            l[..., 0] = np.clip(l[..., 0].astype(int) + 11, 0, 255); r[..., 2] = np.clip(r[..., 2].astype(int) - 9, 0, 255)
            l, r = np.ascontiguousarray(l), np.ascontiguousarray(r)
            fa = a.track_stereo(l, r, 0.05 * k, None, DV_MODE_RAW, DV_MEM_HOST | DV_FMT_BGR, stride=3 * w)
            fb = b.track_stereo(oracle.bgr2gray(oracle.remap(l, m1l, m2l)), oracle.bgr2gray(oracle.remap(r, m1r, m2r)), 0.05 * k)
        else:
            fa = a.track_stereo(l, r, 0.05 * k)
            fb = b.track_stereo(oracle.remap(l, m1l, m2l), oracle.remap(r, m1r, m2r), 0.05 * k)
        _rows_equal(fa, fb)
        total += len(fa)
    assert total > 100
    a.set_undistort_maps(0)           # removing camera 0's maps removes both: back to the plain path
    a.reset()
    c = gpu_ctx_factory(width=w, height=h, max_cnt=60, min_dist=12, cam0=undist_cam, cam1=undist_cam)
    for k in range(2):
        l, r = seq.frame(k)
        _rows_equal(a.track_stereo(l, r, 0.05 * k), c.track_stereo(l, r, 0.05 * k))


def test_viode_mask_bit_exact(gpu_ctx_factory, oracle):
    """row N4: VIODE label image -> merge / inverse masks, key image, per-key boxes"""
    import ctypes as C
    w, h = 333, 201
    rng = np.random.default_rng(3)
    palette = np.array([[10, 20, 30], [200, 3, 77], [0, 0, 0], [255, 255, 255], [9, 250, 1], [77, 77, 77]], np.uint8)      # b g r
    seg = palette[rng.integers(0, 2, (h, w))]                      # background labels
    seg[40:90, 100:180] = palette[2]; seg[120:150, 10:60] = palette[3]; seg[5:9, 300:333] = palette[4]     # three objects
    key = lambda p: int(p[2]) * 1000000 + int(p[1]) * 1000 * int(p[0])
    dyn = np.array([key(palette[2]), key(palette[3]), key(palette[4]), key(palette[5])], np.uint32)          # the last one is absent
    ctx = gpu_ctx_factory(width=64, height=48)
    merge, inv, kimg, boxes = ctx.viode_mask(seg, dyn)
    om, oi, ok_, ob = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint32), np.zeros((4, 4), np.int32)
    oracle.lib.dvo_viode_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    segc = np.ascontiguousarray(seg)
    oracle.lib.dvo_viode_mask(segc.ctypes.data, w, h, segc.strides[0], dyn.ctypes.data, 4, om.ctypes.data, oi.ctypes.data, ok_.ctypes.data, ob.ctypes.data)
    assert np.array_equal(merge, om) and np.array_equal(inv, oi) and np.array_equal(kimg, ok_) and np.array_equal(boxes, ob)
    assert np.array_equal(inv, 255 - merge) and merge[40:90, 100:180].all() and not merge[0, 0]
    assert list(boxes[0]) == [40, 89, 100, 179] and list(boxes[2]) == [5, 8, 300, 332] and list(boxes[3]) == [-1, -1, -1, -1]
    assert kimg[45, 120] == 0 and kimg[130, 20] == 255 * 1000000 + 255 * 1000 * 255          # key = r*1e6 + g*1000*b (sic)


OPERATOR_ENTRIES = ["pyr_down", "pyr_down_cuda", "min_eigen", "min_eigen_cuda", "gftt", "gftt_cuda", "erode", "circle_mask", "bgr2gray", "remap_gray", "remap_bgr"]


@pytest.mark.parametrize("entry", OPERATOR_ENTRIES)
def test_operator_entry_from_padded_device_memory_equals_tight_host_memory(ctx, entry):
    """The operator entries take DV_MEM_DEVICE arrays in place, under the caller's row stride.  A 33 x 17 image (a padded row, a ragged last 16-byte block): once from
    tight host memory, once from device memory with a row stride of width + 5 pixels (the padding holds 0xAB); the results are bit-equal."""
    import ctypes as C
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, _ptr
    w, h, pad = 33, 17, 5
    rng = np.random.default_rng(len(entry))
    lib, H = ctx.lib, ctx.h

    def padded(a):      # a's rows in device memory, width + 5 pixels apart -> (tensor, row stride in bytes)
        rows = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], 0xAB, a.dtype)
        rows[:, : a.shape[1]] = a
        return torch.from_numpy(rows).cuda(), rows.strides[0]

    dev = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    img = _img(h, w, 5)
    if entry.startswith("pyr_down"):
        want = getattr(ctx, entry)(img)
        t, stride = padded(img); out = dev(want.shape, torch.uint8)
        ctx._check(getattr(lib, "dv_" + entry)(H, _ptr(t.data_ptr()), w, h, stride, _ptr(out.data_ptr()), DV_MEM_DEVICE))
        got = out.cpu().numpy()
    elif entry.startswith("min_eigen"):
        rule = "cuda" if entry.endswith("cuda") else "cpu"
        want = ctx.min_eigen(img, rule)
        t, stride = padded(img); out = dev((h, w), torch.float32)
        ctx._check(getattr(lib, "dv_" + entry)(H, _ptr(t.data_ptr()), w, h, stride, _ptr(out.data_ptr()), DV_MEM_DEVICE))
        got, want = out.cpu().numpy().view(np.uint32), want.view(np.uint32)
    elif entry.startswith("gftt"):
        rule = "cuda" if entry.endswith("cuda") else "cpu"
        mask = np.full((h, w), 255, np.uint8); mask[:, :4] = 0
        want = ctx.gftt(img, 20, 0.01, 3, mask, rule)
        assert len(want) > 3
        t, stride = padded(img); m, _ = padded(mask); out = dev((1024, 2), torch.float32); n = C.c_int(0)
        ctx._check(getattr(lib, "dv_" + entry)(H, _ptr(t.data_ptr()), _ptr(m.data_ptr()), w, h, stride, 20, 0.01, 3.0, _ptr(out.data_ptr()), C.byref(n), DV_MEM_DEVICE))
        got, want = out.cpu().numpy()[: n.value].view(np.uint32), want.view(np.uint32)
    elif entry == "erode":
        mask = (rng.uniform(0, 1, (h, w)) > 0.05).astype(np.uint8) * 255
        want = ctx.erode(mask, 3)
        t, stride = padded(mask); out, _ = padded(np.zeros((h, w), np.uint8))      # a device destination has the source's stride
        ctx._check(lib.dv_erode(H, _ptr(t.data_ptr()), w, h, stride, 3, _ptr(out.data_ptr()), DV_MEM_DEVICE))
        got = out.cpu().numpy()
        assert (got[:, w:] == 0xAB).all()
        got = got[:, :w]
    elif entry == "circle_mask":
        mask = np.full((h, w), 255, np.uint8)
        pts = rng.uniform([-3, -3], [w + 3, h + 3], (6, 2)).astype(np.float32)
        want = ctx.circle_mask(mask, pts, 4)
        t, stride = padded(mask); p = torch.from_numpy(pts).cuda()
        ctx._check(lib.dv_circle_mask(H, _ptr(t.data_ptr()), w, h, stride, _ptr(p.data_ptr()), len(pts), 4, DV_MEM_DEVICE))
        got = t.cpu().numpy()
        assert (got[:, w:] == 0xAB).all()
        got = got[:, :w]
    elif entry == "bgr2gray":
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        want = ctx.bgr2gray(bgr)
        t, stride = padded(bgr); out = dev((h, w), torch.uint8)
        ctx._check(lib.dv_bgr2gray(H, _ptr(t.data_ptr()), w, h, stride, _ptr(out.data_ptr()), DV_MEM_DEVICE))
        got = out.cpu().numpy()
    else:
        src = rng.integers(0, 256, (h, w, 3) if entry == "remap_bgr" else (h, w), dtype=np.uint8)
        m1, m2 = _rand_maps(rng, w, h)
        want = ctx.remap(src, m1, m2)
        t, stride = padded(src); out = dev(src.shape, torch.uint8)
        ctx._check(lib.dv_remap(H, _ptr(t.data_ptr()), w, h, stride, src.ndim == 3 and 3 or 1, m1.ctypes.data, m2.ctypes.data, _ptr(out.data_ptr()), DV_MEM_DEVICE))
        got = out.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
