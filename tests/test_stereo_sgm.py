"""The stereo matcher on the device (dv_stereo_sgm_enqueue / _collect; the place of MyStereoMatcher::Launch / WaitResult, stereo/stereo.cpp) against tests/sgm_ref.py:
the float disparity map BIT FOR BIT, and through dv_stereo_sgm_debug the census codes of both images, S, d* and dR, all exactly.  Shapes: the smallest at which each
path can go wrong — 70 x 23 (D = 64: width off a multiple of 4 and of 64, most of the left band has x < d), 130 x 9 (D = 128: two disparities per lane), 67 x 5 with
rows of 71 bytes and a base off a dword (D = 64: the height is below the census window, every census row is clamped), 260 x 6 (D = 256: four disparities per lane)."""
import numpy as np
import pytest

from tests import sgm_ref as sr

pytestmark = pytest.mark.gpu

SHAPES = {"70x23_d64": (70, 23, 64, 0, 0), "130x9_d128": (130, 9, 128, 0, 0), "67x5_d64_strided": (67, 5, 64, 4, 1), "260x6_d256": (260, 6, 256, 0, 0)}      # w, h, D, stride - w, base offset
KINDS = ["random", "flat", "checker", "shifted", "bright_edges"]
CORNERS = {"p_zero": dict(p1=0, p2=0), "p_max": dict(p1=255, p2=255), "uniq_0": dict(uniqueness=0), "uniq_99": dict(uniqueness=99), "lr_off": dict(lr_max_diff=-1),
           "lr_0": dict(lr_max_diff=0)}
ITEMS = ("codes_l", "codes_r", "S", "dstar", "dr")
_REF, _CTX = {}, {}


def ctx_for(gpu_ctx_factory, w, h):
    from dynamic_vins_amd.frontend import make_cam
    if (w, h) not in _CTX:
        cam = make_cam(100, 100, w / 2, h / 2)
        _CTX[(w, h)] = gpu_ctx_factory(width=w, height=h, max_cnt=50, min_dist=10, cam0=cam, cam1=cam)
    return _CTX[(w, h)]


def laid_out(img, extra, lead):
    """-> (flat uint8 buffer, view of it with rows of w + extra bytes starting `lead` bytes in)"""
    h, w = img.shape
    flat = np.full(lead + h * (w + extra) + 8, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[lead:], (h, w), (w + extra, 1))
    view[...] = img
    return flat, view


def reference(shape, kind, seed=11, **par):
    """the case's pair and the restatement's intermediates, computed once and left unchanged"""
    key = (shape, kind, seed, tuple(sorted(par.items())))
    if key not in _REF:
        w, h, D, _, _ = SHAPES[shape]
        l, r = sr.images(kind, w, h, seed=seed)
        res = sr.sgm(l, r, **sr.params(n_disp=D, **par))
        for v in res.values():
            v.setflags(write=False)
        _REF[key] = (l, r, res)
    return _REF[key]


def run(ctx, shape, l, r, mem="host", keep=None, **par):
    """shape: a name of SHAPES, or its tuple (tests/test_stereo_sgm_hostile.py brings its own)"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_PINNED, sgm_params
    w, h, D, extra, lead = SHAPES[shape] if isinstance(shape, str) else shape
    p = sgm_params(n_disp=D, **par)
    (fl, vl), (fr, vr) = laid_out(l, extra, lead), laid_out(r, extra, lead)
    if mem == "host":
        return ctx.stereo_sgm(vl, vr, p)
    ts = [torch.from_numpy(f) for f in (fl, fr)]
    ts = [t.cuda() if mem == "device" else t.pin_memory() for t in ts]
    torch.cuda.synchronize()
    if keep is not None:
        keep.extend(ts)
    return ctx.stereo_sgm(ts[0].data_ptr() + lead, ts[1].data_ptr() + lead, p, mem=DV_MEM_DEVICE if mem == "device" else DV_MEM_PINNED, stride=w + extra)


def check_all(ctx, got, res, tag):
    from dynamic_vins_amd import frontend as fe
    dbg = dict(codes_l=fe.DV_SGM_DEBUG_CENSUS_L, codes_r=fe.DV_SGM_DEBUG_CENSUS_R, S=fe.DV_SGM_DEBUG_S, dstar=fe.DV_SGM_DEBUG_DSTAR, dr=fe.DV_SGM_DEBUG_DR)
    for item in ITEMS:
        dev = ctx.stereo_sgm_debug(dbg[item])
        bad = int((dev != res[item]).sum())
        print("%s: %s differs in %d of %d" % (tag, item, bad, dev.size))
        assert dev.dtype == res[item].dtype and bad == 0, "%s: %s" % (tag, item)
    bad = int((got.view(np.uint32) != res["out"].view(np.uint32)).sum())
    print("%s: output differs in %d of %d bit patterns; %d valid pixels" % (tag, bad, got.size, int((res["out"] > 0).sum())))
    assert got.dtype == np.float32 and bad == 0, tag


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bit_parity_with_the_restatement(gpu_ctx_factory, shape, kind):
    w, h = SHAPES[shape][:2]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    l, r, res = reference(shape, kind)
    check_all(ctx, run(ctx, shape, l, r), res, "%s %s" % (shape, kind))
    if kind == "flat":          # every cost ties: the lowest-d rule decides both winners
        assert not res["dstar"].any() and not res["dr"].any()


@pytest.mark.parametrize("corner", list(CORNERS))
@pytest.mark.parametrize("shape", ["70x23_d64", "130x9_d128"])
def test_parameter_corners(gpu_ctx_factory, shape, corner):
    w, h = SHAPES[shape][:2]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    for kind in ("random", "shifted"):
        l, r, res = reference(shape, kind, **CORNERS[corner])
        check_all(ctx, run(ctx, shape, l, r, **CORNERS[corner]), res, "%s %s %s" % (shape, kind, corner))


@pytest.mark.parametrize("shape", ["67x5_d64_strided", "70x23_d64"])
def test_memory_kinds(gpu_ctx_factory, shape):
    w, h = SHAPES[shape][:2]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    l, r, res = reference(shape, "random")
    for mem in ("host", "device", "pinned"):
        keep = []
        check_all(ctx, run(ctx, shape, l, r, mem, keep), res, "%s %s" % (shape, mem))


def test_two_frames_on_the_alternating_maps(gpu_ctx_factory):
    """the second frame runs over a first frame of different content: every element of the map, of S and of the codes is rewritten; a collected map survives one enqueue"""
    from dynamic_vins_amd.frontend import device_tensor, sgm_params
    shape = "70x23_d64"
    w, h, D = SHAPES[shape][:3]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    refs = [reference(shape, "random"), reference(shape, "bright_edges"), reference(shape, "flat")]
    ptrs = []
    for l, r, res in refs:
        ptr, stride = ctx.stereo_sgm(l, r, sgm_params(n_disp=D), host=False)
        assert stride == 4 * w
        ptrs.append(ptr)
        got = device_tensor(ptr, (h, w)).cpu().numpy()
        check_all(ctx, got, res, "frame %d" % len(ptrs))
        if len(ptrs) > 1:          # the map collected one frame ago is still that frame's
            prev = device_tensor(ptrs[-2], (h, w)).cpu().numpy()
            assert np.array_equal(prev.view(np.uint32), refs[len(ptrs) - 2][2]["out"].view(np.uint32))
    assert ptrs[0] != ptrs[1] and ptrs[2] == ptrs[0]


def test_protocol_and_parameter_refusals(gpu_ctx_factory):
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import sgm_params
    from tests.test_sgm_ref import REFUSALS
    w, h = 72, 10
    ctx = ctx_for(gpu_ctx_factory, w, h)
    l, r = sr.images("random", w, h, seed=3)
    with pytest.raises(DvinsError, match="nothing enqueued"):
        ctx.stereo_sgm_collect()
    ctx.stereo_sgm_enqueue(l, r, sgm_params(n_disp=64))
    with pytest.raises(DvinsError, match="previous frame not collected"):
        ctx.stereo_sgm_enqueue(l, r, sgm_params(n_disp=64))
    ctx.stereo_sgm_collect()
    with pytest.raises(DvinsError, match="nothing enqueued"):
        ctx.stereo_sgm_collect()
    for name, (kw, text) in REFUSALS.items():
        if "stride" in kw:
            continue          # a host array's stride is its own; the stride refusal is covered without a device
        with pytest.raises(DvinsError, match=text):
            ctx.stereo_sgm_enqueue(l, r, sgm_params(**kw))
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE
    t = torch.zeros(h * w, dtype=torch.uint8, device="cuda")
    with pytest.raises(DvinsError, match="row stride below width"):
        ctx.stereo_sgm_enqueue(t.data_ptr(), t.data_ptr(), sgm_params(n_disp=64), mem=DV_MEM_DEVICE, stride=w - 1)
    with pytest.raises(DvinsError, match="unknown memory kind"):
        ctx.stereo_sgm_enqueue(t.data_ptr(), t.data_ptr(), sgm_params(n_disp=64), mem=7, stride=w)
    ctx.stereo_sgm(l, r, sgm_params(n_disp=64))          # a refused frame leaves the stage usable
