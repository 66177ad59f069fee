"""Extra-point parity on hostile clouds (builders, conditions and the sweep emulation: tests/xp_cases.py).

CPU (`-m "not gpu"`): every case passes its own conditions — the counts it is named for and, for the two thresholds, that the numpy restatement with the comparison
flipped answers differently —, the convergence set straddles the 16 label sweeps the host launches (12, 15 | 16, 18, 48 changing sweeps), and the oracle
(oracle/extra_points.cpp) equals the independent numpy restatement of tests/test_extra_points.py bit for bit on every case.
GPU: dv_extra_points, stage 1 and stage 0, against the oracle on every case: values, order and counts, no tolerance; a large cloud and then a small one on one context
against a fresh context; flag 8 refused by name with the context usable afterwards; and one frame of five objects (an empty mask, a tie, a U whose sweeps do not
converge in 16, the capacity band, a cluster of exactly 10) through dv_inst_set_disparity + dv_inst_track_enqueue + dv_inst_track_collect, every object's points against
the operator form and the oracle on that object alone.
Changing sweeps per family (emulated; the friendly scenes of tests/test_extra_points.py need about 5): thresholds, counts, winners <= 3, block and pass edges <= 6
(capacity band 6), U arms 40 / 50 / 52 / 60 / 148 nodes: 12 / 15 / 16 / 18 / 48, serpentine 24.  From 16 on the last kernel finishes the labels itself
(csrc/extra_points.hip); before that change those cases failed with flag 16."""
import numpy as np
import pytest

from tests import inst_hostile as ih
from tests import xp_cases as xc

NAMES = sorted(xc.CASES)
_ORACLE = {}


def oracle_of(oracle, name, s=None):
    """(sampled points, pipeline answer) of the oracle for a case, computed once and shared"""
    if name not in _ORACLE:
        s = s if s is not None else xc.scene(name)
        raw = oracle.detect_extra_points(s.mask, s.xy, s.disp, s.cam, s.baseline)
        _ORACLE[name] = (raw, oracle.process_extra_points(raw))
    return _ORACLE[name]


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# =============================================================== conditions and the oracle (CPU)
@pytest.mark.parametrize("name", sorted(xc.CASES_ALL))
def test_case_conditions(name):
    xc.check(name)
    s = xc.scene(name)
    print(f"\n[xp] {name}: ROI {s.mask.shape[1]} x {s.mask.shape[0]} at {s.xy} in {s.size}, step {xc.step_rule(*s.mask.shape)}, "
          f"sampled / survivors / returned {xc.counts(name) if name in xc.CASES else (len(xc.points(name)), 0, 0)}, changing sweeps {xc.sweeps_of(name) if name in xc.CASES else 0}")


def test_convergence_set_straddles_the_launched_sweeps():
    got = xc.check_convergence_set()
    fam = {}
    for name, (_, chk) in xc.CASES.items():
        fam[chk.__name__[7:]] = max(fam.get(chk.__name__[7:], 0), xc.sweeps_of(name))
    print(f"\n[xp] changing sweeps of the U arms {sorted(xc.U_ARMS)}: {got}; serpentine {xc.sweeps_of('serpentine_4x75')}; worst per family {fam}")
    assert xc.sweeps_of("serpentine_4x75") >= xc.XP_SWEEPS
    assert max(v for k, v in fam.items() if k != "convergence") <= 6


@pytest.mark.parametrize("name", sorted(xc.CASES_ALL))
def test_oracle_matches_restatement(oracle, name):
    raw, seg = oracle_of(oracle, name)
    assert bits_equal(raw, xc.points(name))
    assert bits_equal(seg, xc.result(name) if name in xc.CASES else np.zeros((0, 3), np.float32))


def frame_inputs():
    W, H = xc.FRAME_SIZE
    disp, objs = xc.frame_objects()
    dets = [ih.det(tid, s.xy + s.mask.shape[::-1], s.mask) for tid, _, s in objs]
    return ih.stereo_frames(W, H, 1, seed=131)[0], disp, objs, dets, xc.CAM + (0.0, 0.0, 0.0, 0.0)


def frame_oracle(oracle):
    """the oracle's two trackers on the frame (computed once) -> (rows, insts, feats, points)"""
    if "frame" not in _ORACLE:
        (l, r), disp, objs, dets, cam = frame_inputs()
        W, H = xc.FRAME_SIZE
        trk = oracle.tracker(W, H, 30, 10, 1, 1, cam, cam)
        oin = oracle.insts(trk, 50, 5, 0)
        rows = trk.track_image(l, r, 0.0)
        oin.set_disparity(disp, xc.BASELINE)
        _ORACLE["frame"] = (rows,) + tuple(oin.track(l, r, 0.0, dets, None, ih.INSTOBS_DTYPE, ih.BOX3D_DTYPE))
    return _ORACLE["frame"]


def object_points(insts, pts, tid):
    o = insts[insts["id"] == tid]
    assert len(o) == 1, f"object {tid} is not in the frame's table"
    return pts[int(o["first_point"][0]): int(o["first_point"][0]) + int(o["n_points"][0])]


def test_frame_objects_on_the_oracle(oracle):
    """every object of the frame is in the oracle's table, and its points are the oracle's pipeline on that object alone: nothing for the empty mask, the right-hand
    cluster of the tie, every survivor of the U and of the band"""
    _, io, _, po = frame_oracle(oracle)
    _, _, objs, _, _ = frame_inputs()
    n = {}
    for tid, name, s in objs:
        seg = oracle_of(oracle, f"frame:{name}", s)[1]
        got = object_points(io, po, tid)
        assert np.array_equal(got, seg.astype(np.float64))
        n[name] = len(got)
    print(f"\n[xp] frame objects -> points: {n}")
    assert n == {"empty": 0, "tie_right_first": 24, "u_arm_60": 374, "capacity_band": 1869, "count_4x7": 10}


# =============================================================== the device against the oracle
_CTX = {}


def ctx_of(factory, size):
    """one operator context per image size"""
    from dynamic_vins_amd.frontend import make_cam
    if size not in _CTX:
        cam = make_cam(*xc.CAM, 0, 0, 0, 0)
        _CTX[size] = factory(width=size[0], height=size[1], max_cnt=50, min_dist=10, cam0=cam, cam1=cam)
    return _CTX[size]


def device_equals_oracle(ctx, s, raw_o, seg_o):
    raw_d = ctx.extra_points(s.mask, s.xy, s.disp, s.baseline, stage=1)
    assert raw_d.shape == raw_o.shape
    assert np.array_equal(raw_d.astype(np.float32).view(np.uint32), raw_o.view(np.uint32)) and np.array_equal(raw_d, raw_o.astype(np.float64))      # floats widened, nothing else
    seg_d = ctx.extra_points(s.mask, s.xy, s.disp, s.baseline, stage=0)
    assert seg_d.shape == seg_o.shape and np.array_equal(seg_d, seg_o.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_hostile_bit_exact(gpu_ctx_factory, oracle, name):
    s = xc.scene(name)
    device_equals_oracle(ctx_of(gpu_ctx_factory, s.size), s, *oracle_of(oracle, name))


def moved(name, size):
    """a constant-disparity case in a larger image"""
    s = xc.scene(name)
    assert (s.disp == s.disp[0, 0]).all() and s.mask.shape[1] <= size[0] and s.mask.shape[0] <= size[1]
    return s._replace(disp=np.full(size[::-1], s.disp[0, 0], np.float32), size=size)


@pytest.mark.gpu
@pytest.mark.parametrize("large,small", [("capacity_band", "count_4x7"), ("u_arm_148", "tie_right_first")])
def test_hip_scratch_pool_leaves_no_trace(gpu_ctx_factory, oracle, large, small):
    """a large cloud (the second one through the last kernel's own sweeps) and then a small one on one context: the second answer is a fresh context's and the oracle's"""
    from dynamic_vins_amd.frontend import make_cam
    big = xc.scene(large)
    s = moved(small, big.size)
    cam = make_cam(*xc.CAM, 0, 0, 0, 0)
    used, fresh = (gpu_ctx_factory(width=big.size[0], height=big.size[1], max_cnt=50, min_dist=10, cam0=cam, cam1=cam) for _ in range(2))
    device_equals_oracle(used, big, *oracle_of(oracle, large))
    raw_o, seg_o = oracle_of(oracle, f"{small}@{large}", s)
    assert len(seg_o) >= 10
    outs = [[c.extra_points(s.mask, s.xy, s.disp, s.baseline, stage=st) for st in (1, 0)] for c in (used, fresh)]
    for raw_d, seg_d in outs:
        assert np.array_equal(raw_d, raw_o.astype(np.float64)) and np.array_equal(seg_d, seg_o.astype(np.float64))


@pytest.mark.gpu
def test_hip_flag8_refused_by_name_and_context_usable(gpu_ctx_factory, oracle):
    """4000 sampled points on one object: both stages are refused with the flag in the message, and the next call on the same context is the oracle's"""
    from dynamic_vins_amd import DvinsError
    s = xc.scene("overflow_1x8000")
    ctx = ctx_of(gpu_ctx_factory, s.size)
    for stage in (0, 1):
        with pytest.raises(DvinsError, match=r"more than DV_XP_CAP sampled points.*device error flags=8\b"):
            ctx.extra_points(s.mask, s.xy, s.disp, s.baseline, stage=stage)
    nxt = s._replace(mask=s.mask[:, :200].copy(), xy=(33, 0))
    raw_o, seg_o = oracle_of(oracle, "overflow_next", nxt)
    assert len(raw_o) == 100 and len(seg_o) == 0
    device_equals_oracle(ctx, nxt, raw_o, seg_o)


@pytest.mark.gpu
def test_hip_frame_of_hostile_objects_through_the_tracker(gpu_ctx_factory, oracle):
    """five objects in one launch of each extra-point kernel (blockIdx.y, the per-object scratch slices): the frame is not refused, the whole output is the oracle's, and
    every object's points are the operator form's and the oracle's on that object alone"""
    from dynamic_vins_amd.frontend import make_cam
    (l, r), disp, objs, dets, cam = frame_inputs()
    W, H = xc.FRAME_SIZE
    ctx = gpu_ctx_factory(width=W, height=H, max_cnt=30, min_dist=10, flow_back=1, stereo=1, cam0=make_cam(*cam), cam1=make_cam(*cam))
    ctx.inst_config(50, 5, 0)
    ctx.track_stereo_enqueue(l, r, 0.0)
    ctx.inst_set_disparity(disp, xc.BASELINE)
    ctx.inst_track_enqueue(0.0, dets)
    rows = ctx.track_stereo_collect()
    insts, feats, pts = ctx.inst_track_collect()          # a raised flag would refuse the frame here
    ih.frame_equal((rows, insts, feats, pts), frame_oracle(oracle), "hostile objects")
    op = ctx_of(gpu_ctx_factory, xc.FRAME_SIZE)
    for tid, name, s in objs:
        got = object_points(insts, pts, tid)
        seg_o = oracle_of(oracle, f"frame:{name}", s)[1]
        assert np.array_equal(got, seg_o.astype(np.float64)), name
        assert np.array_equal(got, op.extra_points(s.mask, s.xy, s.disp, s.baseline, stage=0)), name
