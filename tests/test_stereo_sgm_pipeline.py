"""The stereo matcher's map where SemanticImage::disp goes (`-m gpu`): the operator entry of the extra-point pipeline reads it in device memory, DynamicPipeline(
stereo_sgm=...) feeds it to the object tracker per frame — also over a ViodeSequence, which carries no disparity — and the shim's MyStereoMatcher::WaitResult hands
over the same map as the ctypes path.  Equality means bit for bit."""
import copy
import os
import subprocess

import numpy as np
import pytest

from dynamic_vins_amd import sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES, D = 320, 180, 8, 64
KW = dict(max_cnt=120, min_dist=15, max_iters=6, use_det3d=0, mask_morphology_size=0, static_inst_threshold=10.0, live_masks=True)
_CACHE = {}


def cam():
    """the rig's cameras without distortion: the pair is rectified as rendered"""
    c = sim.scaled_cam(sim.ZED, W, H, 1280, 720)
    return dict(c, k1=0.0, k2=0.0, p1=0.0, p2=0.0)


def new_ctx():
    from dynamic_vins_amd.frontend import Context, make_cam
    c = make_cam(*sim.cam_tuple(cam()))
    return Context(width=W, height=H, max_cnt=120, min_dist=15, cam0=c, cam1=c)


def sequence():
    if "seq" not in _CACHE:
        from dynamic_vins_amd.viode import ViodeSequence
        masker = new_ctx()
        _CACHE["seq"] = ViodeSequence(W, H, cam(), FRAMES, masker, rate=20.0)
        masker.close()
    return _CACHE["seq"]


def params():
    from dynamic_vins_amd.frontend import sgm_params
    return sgm_params(n_disp=D)


def maps():
    """Context.stereo_sgm of every frame of the sequence, as host arrays"""
    if "maps" not in _CACHE:
        from dynamic_vins_amd.frontend import DV_MEM_DEVICE
        seq, ctx = sequence(), new_ctx()
        _CACHE["maps"] = [ctx.stereo_sgm(l.data_ptr(), r.data_ptr(), params(), mem=DV_MEM_DEVICE, stride=l.stride(0)) for l, r in seq.frames]
        ctx.close()
    return _CACHE["maps"]


def run(seq, **kw):
    from dynamic_vins_amd.pipeline import DynamicPipeline
    p = DynamicPipeline(seq, **dict(KW, **kw))
    frames = []
    for _ in range(FRAMES):
        st = p.step()
        frames.append(dict(rows=p.rows.tobytes(), insts=p.insts.tobytes(), feats=p.ifeats.tobytes(), points=p.ipts.tobytes(), n_points=len(p.ipts),
                           pose=p.est.window()[10, :7].tobytes(), nonlinear=int(st.nonlinear)))
    out = dict(frames=frames, stat=dict(p.stat), traj=np.array(p.poses).tobytes())
    p.ctx.close()
    return out


def with_keyword():
    if "kw" not in _CACHE:
        _CACHE["kw"] = run(sequence(), stereo_sgm=params())
    return _CACHE["kw"]


def test_operator_entry_reads_the_device_map():
    """Context.extra_points from the matcher's map in device memory equals Context.extra_points from the same map downloaded to the host"""
    from dynamic_vins_amd.frontend import DV_MEM_DEVICE
    seq, ctx = sequence(), new_ctx()
    l, r = seq.frames[3]
    ptr, stride = ctx.stereo_sgm(l.data_ptr(), r.data_ptr(), params(), mem=DV_MEM_DEVICE, stride=l.stride(0), host=False)
    host = maps()[3]
    assert stride == 4 * W and (host > 0).mean() > 0.5
    mask = np.full((60, 90), 255, np.uint8)
    mask[:7, :9] = 0
    for stage in (1, 0):
        a = ctx.extra_points(mask, (110, 60), ptr, seq.baseline, stage, mem=DV_MEM_DEVICE, stride_bytes=stride)
        b = ctx.extra_points(mask, (110, 60), host, seq.baseline, stage)
        assert len(b) > 0 and a.tobytes() == b.tobytes(), "stage %d" % stage
    ctx.close()


def test_viode_sequence_gets_extra_points_from_the_matcher():
    """DynamicPipeline(live_masks=True, stereo_sgm=params) over a ViodeSequence — which has no disparity maps — yields objects with extra points, and every result equals
    the same pipeline fed, per frame, the map Context.stereo_sgm computed for that frame through inst_set_disparity"""
    import torch
    seq = sequence()
    assert len(seq.disp_dev) == 0
    got = with_keyword()
    assert any(f["n_points"] > 0 for f in got["frames"]) and got["stat"]["object_detections"] > 0
    fed = copy.copy(seq)
    fed.disp_dev = [torch.from_numpy(m).cuda().contiguous() for m in maps()]
    torch.cuda.synchronize()
    want = run(fed)
    assert want["stat"] == got["stat"] and want["traj"] == got["traj"]
    for k, (a, b) in enumerate(zip(want["frames"], got["frames"])):
        for item in ("rows", "insts", "feats", "points", "pose", "nonlinear"):
            assert a[item] == b[item], "frame %d: %s" % (k, item)


def test_without_the_keyword_nothing_changes():
    """no keyword: a ViodeSequence still yields no extra points, and both trackers' rows are those of the run with the matcher (the points touch neither)"""
    a, b = run(sequence()), with_keyword()
    assert all(f["n_points"] == 0 for f in a["frames"])
    for k, (x, y) in enumerate(zip(a["frames"], b["frames"])):
        assert x["rows"] == y["rows"] and x["feats"] == y["feats"], "frame %d" % k


def test_shim_matcher_equals_the_ctypes_path(tmp_path):
    exe, lib = str(tmp_path / "sgm_shim_test"), os.path.join(ROOT, "dynamic_vins_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
           os.path.join(ROOT, "tests", "host", "sgm_shim_test.cpp"), "-o", exe, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread", "-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and "refused: MyStereoMatcher: a ctx is required" in r.stdout, r.stdout + r.stderr
    seq = sequence()
    pairs = [(seq.frames[k][0].cpu().numpy(), seq.frames[k][1].cpu().numpy()) for k in (0, 1, 2)]
    spath, opath = str(tmp_path / "scene.bin"), str(tmp_path / "maps.bin")
    with open(spath, "wb") as fh:
        fh.write(np.array([W, H, D, len(pairs)], np.int32).tobytes())
        for l, rr in pairs:
            fh.write(np.ascontiguousarray(l).tobytes() + np.ascontiguousarray(rr).tobytes())
    out = subprocess.run([exe, "run", spath, opath], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.fromfile(opath, np.float32).reshape(len(pairs), H, W)
    for k in range(len(pairs)):
        assert np.array_equal(got[k].view(np.uint32), maps()[k].view(np.uint32)), "frame %d" % k
    assert out.stdout.split() == ["alternating", "1", "points", "1"], out.stdout
