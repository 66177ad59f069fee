"""The detector head on the device (`-m gpu`) at its documented limits and at the network's own grid sizes: the constructed cases of tests/solo_cases.py (whose premises and
1 % band tests/test_solo_head_ref.py asserts on the reference alone) through check_against of tests/test_solo_head.py — n_pass, n, labels and plane order exact, scores within
1e-4 relative of float64, pixels equal outside the 4 delta band, padding bytes zero.  DESIGN.md's detector-head section maps every kernel path to the case that reaches it."""
import numpy as np
import pytest

from tests import solo_cases
from tests.test_inst_stack import stage_ctx
from tests.test_solo_head import check_against, device_outputs, planes_of, to_params

pytestmark = pytest.mark.gpu

MEM = {"p256": "pinned", "upsample": "host", "kept_1024": "host", "cells_g33": "pinned"}          # every other case: device memory


def run_case(gpu_ctx_factory, name, ctx=None, keep=None):
    rec = solo_cases.get(name)
    ctx = ctx or stage_ctx(gpu_ctx_factory, *rec["par"]["origin"])
    return check_against(ctx, rec["inp"], rec["par"], rec["r64"], rec["delta"], MEM.get(name, "device"), [] if keep is None else keep, name)


@pytest.mark.parametrize("name", list(solo_cases.BUILDERS))
def test_constructed_case_equals_the_reference(gpu_ctx_factory, name):
    """one frame of every constructed case.  The tie cases compare against the reference with both sorts stable: equal scores in candidate order, then in first-sort order"""
    rec = solo_cases.get(name)
    planes, st, labels, _ = run_case(gpu_ctx_factory, name)
    assert len(planes) == rec["r64"]["n"] and st.n_planes == min(len(labels), 64)          # (all n planes lie in memory behind the 64 the stack names: planes_of read them)


def test_over_capacity_at_scale_then_the_next_frame(gpu_ctx_factory):
    """4097 candidates against max_candidates 4096, then every class of every cell of five 64 x 64 grids (2 621 440: the scan's carry over 20 iterations): both are refused
    at collect with the reference's count in the message, and the ctx goes on with the next frame"""
    import torch
    from dynamic_vins_amd._abi import DvinsError
    from tests import solo_ref
    ctx, keep = stage_ctx(gpu_ctx_factory, 67, 5), []
    inp, par = solo_cases.over_capacity_by_one()
    n_pass = solo_ref.head(inp["kernels"], inp["cates"], inp["feature"], dict(par, lean=True, nms_pre=1), torch.float32)["n_pass"]
    assert n_pass == 4097
    with pytest.raises(DvinsError, match=rf"\b{n_pass} cells pass score_thr, more than max_candidates"):
        ctx.solo_head(device_outputs(inp, "device", keep), to_params(par))
    inp, par, n_pass = solo_cases.every_cell_passes()
    with pytest.raises(DvinsError, match=rf"\b{n_pass} cells pass score_thr, more than max_candidates"):
        ctx.solo_head(device_outputs(inp, "host", keep), to_params(par))
    run_case(gpu_ctx_factory, "cells_g64", ctx, keep)


def test_small_frame_after_the_largest_equals_a_fresh_ctx(gpu_ctx_factory):
    """work memory is carved per size: after the 4096-candidate / 512 / 128 frame a small frame gives, bit for bit, the labels, scores and planes it gives on a ctx that
    has seen nothing else"""
    from dynamic_vins_amd.frontend import make_cam
    used, keep = stage_ctx(gpu_ctx_factory, 67, 5), []
    run_case(gpu_ctx_factory, "cap4096", used, keep)
    a = run_case(gpu_ctx_factory, "tie_three", used, keep)
    fresh = gpu_ctx_factory(width=67, height=5, max_cnt=50, min_dist=10, cam0=make_cam(100, 100, 33.5, 2.5), cam1=make_cam(100, 100, 33.5, 2.5))
    b = run_case(gpu_ctx_factory, "tie_three", fresh, keep)
    assert np.array_equal(a[2], b[2]) and a[3].tobytes() == b[3].tobytes() and np.array_equal(a[0], b[0])
    n = len(a[2])
    assert np.array_equal(planes_of(a[1], n, 67, 5), planes_of(b[1], n, 67, 5))
