"""The stereo matcher on the device at its limits (tests/sgm_hostile.py; the premises of the cases: tests/test_sgm_hostile_ref.py): every case against tests/sgm_ref.py —
the float map BIT FOR BIT and, through dv_stereo_sgm_debug, both census images, S, d* and dR exactly; n_disp changing between the frames of one context; and two
properties of the output that go through no restatement.  Each comparison prints its count of differing elements and of valid pixels."""
import contextlib

import numpy as np
import pytest

from tests import sgm_hostile as sh
from tests import sgm_ref as sr
from tests.test_stereo_sgm import SHAPES, check_all, ctx_for, run

pytestmark = pytest.mark.gpu

SHARED = {SHAPES[s][:2] for s in SHAPES}          # the sizes tests/test_stereo_sgm.py keeps a context for


@contextlib.contextmanager
def context(gpu_ctx_factory, w, h, fresh=False):
    """the session's context of a shared size, or one of a one-off size that is closed with the test"""
    if (w, h) in SHARED and not fresh:
        yield ctx_for(gpu_ctx_factory, w, h)
        return
    from dynamic_vins_amd.frontend import make_cam
    cam = make_cam(100, 100, w / 2, h / 2)
    ctx = gpu_ctx_factory(width=w, height=h, max_cnt=50, min_dist=10, cam0=cam, cam1=cam)
    try:
        yield ctx
    finally:
        ctx.close()


def decision(par):
    return {k: v for k, v in par.items() if k != "n_disp"}


@pytest.mark.parametrize("name", sh.names())
def test_bit_parity_at_the_limits(gpu_ctx_factory, name):
    c = sh.CASES[name]
    l, r, par, (extra, lead) = sh.case(name)
    res = sh.reference(name)
    with context(gpu_ctx_factory, c.w, c.h) as ctx:
        for mem in c.mems:
            keep = []
            got = run(ctx, (c.w, c.h, c.D, extra, lead), l, r, mem, keep, **decision(par))
            assert got.shape == (c.h, c.w) and res["S"].shape == (c.h, c.w, c.D)
            check_all(ctx, got, res, "%s %s" % (name, mem))


# n_disp per frame, each on another kind of image
D_ORDERS = {"issue_order": [256, 64, 128, 256], "reversed": [256, 128, 64, 256], "growing": [64, 128, 256, 64]}
D_KINDS = ["random", "bright_edges", "shifted", "checker"]


@pytest.mark.parametrize("order", list(D_ORDERS))
def test_n_disp_changes_between_frames(gpu_ctx_factory, order):
    """S's layout follows n_disp, its buffer only grows, and nothing clears it: the first direction stores.  After every frame the map and the five debug items are that
    frame's, and the map collected one frame earlier is intact.  (`growing` starts a fresh context at 64, so that the volume really regrows twice.)"""
    from dynamic_vins_amd.frontend import device_tensor, sgm_params
    w, h = 70, 23
    frames = []
    for i, D in enumerate(D_ORDERS[order]):
        l, r = sr.images(D_KINDS[i], w, h, seed=40 + i)
        frames.append((D, l, r, sr.sgm(l, r, n_disp=D)))
    with context(gpu_ctx_factory, w, h, fresh=True) as ctx:
        ptrs = []
        for D, l, r, res in frames:
            ptr, stride = ctx.stereo_sgm(l, r, sgm_params(n_disp=D), host=False)
            assert stride == 4 * w
            ptrs.append(ptr)
            got = device_tensor(ptr, (h, w)).cpu().numpy()
            check_all(ctx, got, res, "%s frame %d (D = %d)" % (order, len(ptrs), D))
            if len(ptrs) > 1:
                prev = device_tensor(ptrs[-2], (h, w)).cpu().numpy()
                bad = int((prev.view(np.uint32) != frames[len(ptrs) - 2][3]["out"].view(np.uint32)).sum())
                print("%s frame %d: the map of frame %d differs in %d of %d" % (order, len(ptrs), len(ptrs) - 1, bad, prev.size))
                assert bad == 0
        assert ptrs[0] != ptrs[1] and ptrs[2] == ptrs[0] and ptrs[3] == ptrs[1]


def device_result(ctx, l, r, D):
    from dynamic_vins_amd import frontend as fe
    out = ctx.stereo_sgm(np.ascontiguousarray(l), np.ascontiguousarray(r), fe.sgm_params(n_disp=D))
    return dict(out=out, S=ctx.stereo_sgm_debug(fe.DV_SGM_DEBUG_S), codes_l=ctx.stereo_sgm_debug(fe.DV_SGM_DEBUG_CENSUS_L), codes_r=ctx.stereo_sgm_debug(fe.DV_SGM_DEBUG_CENSUS_R))


@pytest.mark.parametrize("kind", sh.PROPERTY_KINDS)
@pytest.mark.parametrize("shape", sh.PROPERTY_SHAPES)
def test_properties_that_go_through_no_restatement(gpu_ctx_factory, shape, kind):
    """The device against itself alone.  A vertical flip of both images flips S and the map, bit for bit: the eight directions map onto each other and every tie rule is
    in d alone — this catches a direction that differs from its mirror image, NOT one walked from the wrong border in the same way in kernel and restatement.  A constant
    added to both images (no pixel leaves [0, 255]) changes no code, so neither S nor the map.  No identity is claimed for a horizontal flip: the census bit order is not
    mirror-symmetric; dR is compared with the restatement on the planted cases instead."""
    w, h, D = shape
    l, r = sh.property_pair(kind, w, h, D)
    with context(gpu_ctx_factory, w, h) as ctx:
        a = device_result(ctx, l, r, D)
        f = device_result(ctx, l[::-1], r[::-1], D)
        c = device_result(ctx, l + sh.PROPERTY_ADD, r + sh.PROPERTY_ADD, D)
    tag = "%dx%d D = %d %s" % (w, h, D, kind)
    n_valid = int((a["out"] > 0).sum())
    assert n_valid >= 32, tag          # tests/test_sgm_hostile_ref.py: the same floor on the restatement
    bad_s, bad_o = int((f["S"] != a["S"][::-1]).sum()), int((f["out"].view(np.uint32) != a["out"][::-1].view(np.uint32)).sum())
    print("%s: flipped pair against flipped result: S differs in %d of %d, the map in %d of %d; %d valid pixels" % (tag, bad_s, a["S"].size, bad_o, a["out"].size, n_valid))
    assert bad_s == 0 and bad_o == 0, tag
    bad = {k: int((c[k].view(np.uint32) != a[k].view(np.uint32)).sum()) if k == "out" else int((c[k] != a[k]).sum()) for k in ("codes_l", "codes_r", "S", "out")}
    print("%s: both images + %d: differing elements %s" % (tag, sh.PROPERTY_ADD, bad))
    assert not any(bad.values()), tag
