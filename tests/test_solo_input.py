"""The detector's input stage on the device (dv_solo_input_enqueue / _collect; Pipeline::ImageToTensor + ProcessInput, det2d/pipeline.cpp:370-387,204-232) against the
restatement tests/solo_input_ref.py: |device - restatement| <= 2e-6 absolute (the derivation is in solo_input_ref.py), and bit for bit: every padding element +0.0, the
identity case equal to (v - mean) / std, every output whose two upper weights are 0 equal to the normalised source value.  Over the issue's five image x model pairs,
row strides 3 w and above, a base off by one byte, the three memory kinds, library-owned and caller-owned destinations (pre-filled with NaN, at 16- and 4-byte
alignment), and two frames on the alternating buffers.  Every refusal once through the enqueue."""
import numpy as np
import pytest

from tests import solo_input_ref as sr
from tests.test_solo_input_ref import REFUSALS, refusal_args
from tests.test_viode_live import download

pytestmark = pytest.mark.gpu
_REF = {}


def ctx_for(gpu_ctx_factory, w, h):
    from dynamic_vins_amd.frontend import make_cam
    cam = make_cam(100, 100, w / 2, h / 2)
    return gpu_ctx_factory(width=w, height=h, max_cnt=50, min_dist=10, cam0=cam, cam1=cam)


def reference(name, stride_extra=0, lead=0):
    """the case's image in the asked layout and its restatement, computed once"""
    key = (name, stride_extra, lead)
    if key not in _REF:
        (w, h), (mw, mh) = sr.CASES[name]
        flat, view = sr.image(w, h, seed=7, stride=3 * w + stride_extra, lead=lead)
        _REF[key] = (flat, view, sr.solo_input(view, mw, mh))
    return _REF[key]


def on_memory(flat, view, mem, keep):
    """-> (bgr argument, keywords) of Context.solo_input for the image in host, device or pinned memory"""
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE, DV_MEM_PINNED
    if mem == "host":
        return view, {}
    t = torch.from_numpy(flat)
    t = t.cuda() if mem == "device" else t.pin_memory()
    torch.cuda.synchronize()
    keep.append(t)
    off = view.__array_interface__["data"][0] - flat.__array_interface__["data"][0]
    return t.data_ptr() + off, dict(mem=DV_MEM_DEVICE if mem == "device" else DV_MEM_PINNED, stride=view.strides[0])


def fetch(ptr, shape):
    return download(ptr, 4 * int(np.prod(shape))).view(np.float32).reshape(shape).copy()


def check(got, r, tag):
    d = float(np.abs(got.astype(np.float64) - r["out"]).max())
    print("device - restatement, %s: %.3g" % (tag, d))
    assert d <= sr.BAR, tag
    pad = ~r["inside"]
    assert not got[:, pad].view(np.uint32).any(), tag + ": a padding element is not +0.0"
    ex = r["exact"]
    assert ex.any() and np.array_equal(got[:, ex].view(np.uint32), r["source"][:, ex].view(np.uint32)), tag + ": an output with both upper weights 0 is not the source value"
    return d


@pytest.mark.parametrize("name", list(sr.CASES))
def test_parity_over_layouts_and_memory_kinds(gpu_ctx_factory, name):
    (w, h), (mw, mh) = sr.CASES[name]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    first = None
    for stride_extra, lead in ((0, 0), (5, 1)):
        flat, view, r = reference(name, stride_extra, lead)
        for mem in ("host", "device", "pinned"):
            keep = []
            bgr, kw = on_memory(flat, view, mem, keep)
            t, rect = ctx.solo_input(bgr, mw, mh, **kw)
            assert rect == r["rect"] == sr.RECTS[name] and tuple(t.shape) == (3, mh, mw) and t.is_cuda and t.is_contiguous()
            got = t.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), fetch(t.data_ptr(), (3, mh, mw)).view(np.uint32)), "the tensor is not a view of the stage's memory"
            check(got, r, "%s stride +%d base +%d %s" % (name, stride_extra, lead, mem))
            if name == "identity":
                assert r["exact"].all() and np.array_equal(got.view(np.uint32), sr.normalise(view).view(np.uint32))
            first = got if first is None else first
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), "layout or memory kind changes the result"


@pytest.mark.parametrize("name", ["pad_cols", "odd_width"])
def test_caller_owned_destination_is_written_completely(gpu_ctx_factory, name):
    """a caller's buffer pre-filled with NaN, at a 16-byte aligned base and 4 bytes off it (the element-store path on every row): every element is written, nothing beside it"""
    import torch
    (w, h), (mw, mh) = sr.CASES[name]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    flat, view, r = reference(name)
    own, _ = ctx.solo_input(view, mw, mh)
    own = own.cpu().numpy()
    n = 3 * mh * mw
    for off in (0, 1, 2, 3):
        buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t, _ = ctx.solo_input(view, mw, mh, dst=buf.data_ptr() + 4 * (off + 1))
        assert t.data_ptr() == buf.data_ptr() + 4 * (off + 1)
        b = buf.cpu().numpy()
        got = b[off + 1: off + 1 + n].reshape(3, mh, mw)
        assert not np.isnan(got).any() and np.isnan(b[: off + 1]).all() and np.isnan(b[off + 1 + n:]).all()
        assert np.array_equal(got.view(np.uint32), own.view(np.uint32))
        check(got, r, "%s caller-owned, %d floats off 16 bytes" % (name, (off + 1) % 4))


def test_two_frames_on_the_alternating_buffers(gpu_ctx_factory):
    from dynamic_vins_amd._abi import DvinsError
    (w, h), (mw, mh) = sr.CASES["pad_rows"]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    imgs = [sr.image(w, h, seed=30 + k)[1] for k in range(3)]
    refs = [sr.solo_input(v, mw, mh) for v in imgs]
    with pytest.raises(DvinsError, match="dv_solo_input_collect: nothing enqueued"):
        ctx.solo_input_collect()
    ctx.solo_input_enqueue(imgs[0], mw, mh)
    with pytest.raises(DvinsError, match="dv_solo_input_enqueue: previous frame not collected"):
        ctx.solo_input_enqueue(imgs[1], mw, mh)
    pa, shape, _ = ctx.solo_input_collect()
    a = fetch(pa, shape)
    ctx.solo_input_enqueue(imgs[1], mw, mh)          # frame 1 is built while frame 0's tensor is still the network's
    pb, _, _ = ctx.solo_input_collect()
    assert pb != pa
    assert np.array_equal(fetch(pa, shape).view(np.uint32), a.view(np.uint32)), "frame 0's tensor changed while frame 1 was built"
    check(a, refs[0], "frame 0"); check(fetch(pb, shape), refs[1], "frame 1")
    ctx.solo_input_enqueue(imgs[2], mw, mh)
    pc, _, _ = ctx.solo_input_collect()
    assert pc == pa
    check(fetch(pc, shape), refs[2], "frame 2"); check(fetch(pb, shape), refs[1], "frame 1 after frame 2")


COLOURS = [(0, 0, 0), (255, 255, 255), (17, 130, 201)]


@pytest.mark.parametrize("name", list(sr.CASES))
def test_constant_colour_gives_the_constant(gpu_ctx_factory, name):
    """Bit for bit: every rectangle element of a constant-colour image is the normalised constant, the padding +0.0.  This is what decides the kernel's evaluation
    of the bilinear value (nested differences, csrc/solo_input_host.h): evaluated as the sum of products with a rounded 1 - l1, the same formula left up to 688 of
    1408 elements of a plane one ulp off the constant on the device (black 70 x 23 frame into 64 x 32), the counts a float32 numpy evaluation of that form leaves."""
    (w, h), (mw, mh) = sr.CASES[name]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    x, y, rw, rh = sr.RECTS[name]
    off = {}
    for col in COLOURS:
        img = np.empty((h, w, 3), np.uint8)
        img[:] = col
        t, _ = ctx.solo_input(img, mw, mh)
        got = t.cpu().numpy()
        const = sr.normalise(img)[:, 0, 0]
        inside = got[:, y:y + rh, x:x + rw]
        off[col] = [int((inside[c].view(np.uint32) != const[c].view(np.uint32)).sum()) for c in range(3)]
        assert float(np.abs(inside.astype(np.float64) - const.astype(np.float64).reshape(3, 1, 1)).max()) <= sr.BAR
        pad = np.ones((mh, mw), bool)
        pad[y:y + rh, x:x + rw] = False
        assert not got[:, pad].view(np.uint32).any()
    print("elements off the constant per plane, %s: %s" % (name, off))
    assert all(v == [0, 0, 0] for v in off.values()), off


@pytest.mark.parametrize("kw,why", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_enqueue_refuses(gpu_ctx_factory, kw, why):
    from dynamic_vins_amd._abi import DvinsError
    a = refusal_args(kw)
    ctx = ctx_for(gpu_ctx_factory, max(a["img_w"], 1), max(a["img_h"], 1)) if a["img_w"] > 0 and a["img_h"] > 0 else None
    if ctx is None:          # a ctx of a non-positive size cannot exist: the same refusal through the model's side
        ctx, a = ctx_for(gpu_ctx_factory, 70, 23), dict(a, img_w=70, img_h=23, model_w=0)
    img = np.zeros((a["img_h"], a["stride"] + 8), np.uint8)
    view = np.lib.stride_tricks.as_strided(img, (a["img_h"], a["img_w"], 3), (img.strides[0], 3, 1))
    import torch
    from dynamic_vins_amd.frontend import DV_MEM_PINNED
    pin = torch.from_numpy(img).pin_memory()
    with pytest.raises(DvinsError, match="dv_solo_input_enqueue: .*" + why):
        ctx.solo_input_enqueue(pin.data_ptr(), a["model_w"], a["model_h"], a["mean"], a["std"], mem=DV_MEM_PINNED, stride=a["stride"])
    del view


def test_enqueue_refuses_its_own_arguments(gpu_ctx_factory):
    import torch
    from dynamic_vins_amd._abi import DvinsError
    (w, h), (mw, mh) = sr.CASES["pad_rows"]
    ctx = ctx_for(gpu_ctx_factory, w, h)
    _, view = sr.image(w, h)
    buf = torch.zeros(3 * mh * mw + 1, dtype=torch.float32, device="cuda")
    with pytest.raises(DvinsError, match="dst_dev must be 4-byte aligned"):
        ctx.solo_input_enqueue(view, mw, mh, dst=buf.data_ptr() + 2)
    with pytest.raises(DvinsError, match="unknown memory kind"):
        ctx.solo_input_enqueue(buf.data_ptr(), mw, mh, mem=7, stride=3 * w)
    t, _ = ctx.solo_input(view, mw, mh)          # the stage stays usable
    check(t.cpu().numpy(), sr.solo_input(view, mw, mh), "after refusals")
