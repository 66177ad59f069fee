"""The detector head without a GPU (`-m "not gpu"`): the float32 and the float64 reference of tests/solo_ref.py agree on every decision for the cases of the GPU sweep;
dv_solo_rect equals Pipeline::GetXYWHS (det2d/pipeline.cpp:23-48) restated here; bad shapes and parameters are refused by host code; csrc/solo_head_host.h runs as a
stand-alone program under AddressSanitizer + UBSan (nothing loaded into Python runs under a sanitizer)."""
import os
import subprocess

import numpy as np
import pytest

from tests import solo_cases, solo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (5, 4, 3, 2, 2)
# channels, (fh, fw), classes, candidates, survivors asked, NMS kernel, strides: the GPU sweep's shapes without its memory kinds
SWEEP = [(128, (24, 72), 80, 63, 8, "gaussian", (8, 8, 8, 8, 8)), (12, (7, 13), 3, 65, 11, "linear", (4, 8, 16, 32, 32)), (12, (24, 72), 3, 52, 1, "gaussian", (4, 8, 16, 32, 32)),
         (128, (7, 13), 80, 72, 8, "linear", (8, 8, 8, 8, 8)), (12, (7, 13), 3, 1, 1, "gaussian", (8, 8, 8, 8, 8))]


def get_xywhs(model_w, model_h, img_w, img_h):
    f = np.float32
    r_w, r_h = f(model_w) / (f(img_w) * f(1.0)), f(model_h) / (f(img_h) * f(1.0))
    if r_h > r_w:
        w, h = model_w, int(r_w * f(img_h))
        h += h % 2 == 1
        return 0, (model_h - h) // 2, w, h
    w, h = int(r_h * f(img_w)), model_h
    w += w % 2 == 1
    return (model_w - w) // 2, 0, w, h


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: f"c{c[0]}_f{c[1][0]}x{c[1][1]}_k{c[2]}_n{c[3]}_{c[5]}")
def test_float32_and_float64_reference_agree(case):
    import torch
    ch, (fh, fw), ncls, n_cand, n_surv, kern, strides = case
    par = solo_ref.params(strides=strides, nms_kernel=kern, rect=(0, 0, 4 * fw, 4 * fh), origin=(70, 23))
    inp, par, _ = solo_ref.make_case(ch, fh, fw, GRIDS, ncls, n_cand, n_surv, par, seed=SWEEP.index(case) + 11)
    r64, r32 = solo_ref.reference(inp, par, torch.float64), solo_ref.reference(inp, par, torch.float32)
    assert torch.equal(r64["logits"], r32["logits"].double()), "a logit is not exact in float32: the generator is wrong"
    assert r64["n_pass"] == r32["n_pass"] == n_cand and all(np.array_equal(a, b) for a, b in zip(r64["cand"], r32["cand"]))
    assert np.array_equal(r64["sorted"][0], r32["sorted"][0]) and r64["n"] == r32["n"] == min(n_surv, par["max_per_img"])
    assert np.array_equal(r64["survivors"], r32["survivors"]) and np.array_equal(r64["labels"], r32["labels"])
    delta = np.abs(r64["values"] - r32["values"].astype(np.float64)).max()
    differ = r64["planes"] != r32["planes"]
    assert delta < 1e-4 and (np.abs(r64["values"][differ] - par["mask_thr"]) < 1e-5).all()


@pytest.mark.parametrize("name", list(solo_cases.BUILDERS))
def test_constructed_case_stands_on_the_reference_alone(name):
    """every case of tests/test_solo_head_limits.py, before a GPU sees it: the float32 and the float64 reference agree on n_pass, the candidates, the first sort, the
    survivors and the labels; the logits are bit-equal; no plane has more than 1 % of its pixels within 4 delta of mask_thr; and the case's own premise (the cells, counts,
    ranks, NaN, exact tie it exists for) holds — a case that stopped reaching its path fails here.  (The spacing conditions are asserted by solo_cases.tile_case.)"""
    import torch
    rec = solo_cases.get(name)
    r64, r32, par = rec["r64"], rec["r32"], rec["par"]
    assert torch.equal(r64["logits"], r32["logits"].double()) and not (r64["logits"] == 0).any(), "a logit is not exact in float32, or zero: the generator is wrong"
    assert r64["n_pass"] == r32["n_pass"] and all(np.array_equal(a, b) for a, b in zip(r64["cand"], r32["cand"]))
    assert r64["n_floor"] == r32["n_floor"] and r64["n_sorted"] == r32["n_sorted"] and np.array_equal(r64["sorted"][0], r32["sorted"][0])
    assert np.array_equal(np.isnan(r64["updated"]), np.isnan(r32["updated"])) and np.array_equal(r64["updated"] >= par["update_thr"], r32["updated"] >= par["update_thr"])
    assert r64["n"] == r32["n"] and np.array_equal(r64["survivors"], r32["survivors"]) and np.array_equal(r64["labels"], r32["labels"])
    assert (np.abs(r32["scores"] - r64["scores"]) <= 1e-5 * r64["scores"]).all()          # a tenth of what the device is allowed against float64
    band = np.abs(r64["values"] - par["mask_thr"]) < 4 * rec["delta"]
    assert rec["delta"] < 1e-4 and band.reshape(r64["n"], -1).mean(1).max() <= 0.01, "more than 1 % of a plane's pixels lie within 4 delta of mask_thr"
    assert np.array_equal(r64["planes"][~band], r32["planes"][~band])
    rec["premise"](rec)


def test_over_capacity_counts_on_the_reference_alone():
    """the two over-capacity frames of the GPU module: one more candidate than the 4096 of `cap4096`, and every class of every cell of five 64 x 64 grids"""
    import torch
    inp, par = solo_cases.over_capacity_by_one()
    assert solo_ref.head(inp["kernels"], inp["cates"], inp["feature"], dict(par, lean=True, nms_pre=1), torch.float32)["n_pass"] == 4097 == par["max_candidates"] + 1
    inp, par, n_pass = solo_cases.every_cell_passes()
    assert n_pass == 5 * 64 * 64 * 128 == 2621440 and all((c > np.float32(par["score_thr"])).all() for c in inp["cates"])


def test_rect_equals_get_xywhs():
    from dynamic_vins_amd.frontend import solo_rect
    seen = set()
    for args in [(1152, 384, 1242, 375), (288, 96, 70, 23), (288, 90, 70, 23), (288, 96, 64, 4), (52, 28, 67, 5), (50, 14, 70, 23), (288, 10, 64, 4), (640, 480, 333, 500), (97, 211, 50, 41)]:
        r = solo_rect(*args)
        assert r == get_xywhs(*args), args
        f = np.float32
        branch = f(args[1]) / f(args[3]) > f(args[0]) / f(args[2])
        side = int((f(args[0]) / f(args[2]) * f(args[3])) if branch else (f(args[1]) / f(args[3]) * f(args[2])))
        seen.add((bool(branch), side % 2 == 1))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}, "a branch or an odd -> even bump is not covered"


def test_bad_shapes_and_parameters_are_refused_without_a_gpu():
    from dynamic_vins_amd._abi import DvinsError
    from dynamic_vins_amd.frontend import solo_check, solo_outputs, solo_params
    z = lambda *s: np.zeros(s, np.float32)
    good_o = lambda **kw: solo_outputs([z(12, g, g) for g in GRIDS], [z(3, g, g) for g in GRIDS], z(12, 7, 13), **kw)
    good_p = dict(rect=(0, 1, 52, 26), origin=(70, 23), num_grids=(2, 2, 3, 4, 5), nms_pre=48, max_per_img=8, max_candidates=72)
    solo_check(good_o(), solo_params(**good_p))
    for bad in (dict(max_candidates=4097), dict(nms_pre=513), dict(max_per_img=129), dict(rect=(0, 3, 52, 26)), dict(rect=(1, 0, 52, 26)), dict(origin=(0, 23)),
                dict(nms_sigma=0.0), dict(nms_kernel=2), dict(mask_thr=float("nan")), dict(strides=(8, -1, 8, 8, 8)), dict(num_grids=(0, 2, 3, 4, 5))):
        with pytest.raises(DvinsError, match="dv_solo_check"):
            solo_check(good_o(), solo_params(**dict(good_p, **bad)))
    o = good_o()
    o.n_levels = 6
    with pytest.raises(DvinsError, match="levels"):
        solo_check(o, solo_params(**good_p))
    o = good_o()
    o.channels = 257
    with pytest.raises(DvinsError, match="channels"):
        solo_check(o, solo_params(**good_p))
    o = good_o()
    o.mem = 7
    with pytest.raises(DvinsError, match="memory kind"):
        solo_check(o, solo_params(**good_p))


def test_host_rules_under_the_sanitizers():
    """csrc/solo_head_host.h as a stand-alone program (tests/host/solo_head_host.cpp) under -fsanitize=address,undefined"""
    host = os.path.join(ROOT, "tests", "host")
    subprocess.run(["make", "-s", "-C", host, "-f", "solo_head.mk", "solo_head"], check=True, capture_output=True, text=True)
    r = subprocess.run([os.path.join(host, "_build", "solo_head_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "solo_head_host ok" in r.stdout, r.stdout + r.stderr


def test_shim_head_overloads_compile(tmp_path):
    """Solov2::GetSegTensor / Detector2D::ForwardHead of dvins_shim.hpp (tests/host/solo_shim_test.cpp) compile with plain g++ -Wall -Werror against include/dvins.h and
    link against the library, as tests/test_host_shim.py builds its driver; the host part (SetImageInfo = GetXYWHS) runs"""
    exe, lib = str(tmp_path / "solo_shim_test"), os.path.join(ROOT, "dynamic_vins_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
           os.path.join(ROOT, "tests", "host", "solo_shim_test.cpp"), "-o", exe, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe, "rect"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [0, 18, 1152, 348, 1242, 375]
