"""dv_batch_track_enqueue with members whose pyramid level 0 is not a copy of the frame (`-m gpu`): installed undistortion maps (cfg::is_undistort_input), BGR frames,
or both.  One more shared launch (level0_multi_kernel) fills level 0 of all of them, each through its own maps; everything behind it is the group's ordinary launches.
The yardstick throughout is the member's own dv_track_stereo on a twin context fed the same frames: rows compared as bytes, frame after frame."""
import numpy as np
import pytest

from dynamic_vins_amd import sim

pytestmark = pytest.mark.gpu

EUROC0 = sim.EUROC
EUROC1 = dict(fx=457.587, fy=456.134, cx=379.999, cy=255.238, k1=-0.28368365, k2=0.07451284, p1=-0.00010473, p2=-3.555907e-05)
STRONG = dict(fx=611.3, fy=598.7, cx=371.9, cy=236.2, k1=-0.39, k2=0.09, p1=1.7e-3, p2=-1.9e-3)      # 752x480 scale: strong barrel distortion with tangential terms


def _cam(c, w, h):
    from dynamic_vins_amd.frontend import make_cam
    return make_cam(*sim.cam_tuple(sim.scaled_cam(c, w, h, 752, 480)))


def _bgr(g):
    """gray -> three unequal channels (a swap of any two changes the 14-bit weighted sum): B = g, G = 3 g / 4 + 20, R = 255 - g / 4"""
    g = g.astype(np.uint16)
    return np.ascontiguousarray(np.stack([g, (3 * g) // 4 + 20, 255 - g // 4], -1).astype(np.uint8))


def _padded(g, stride):
    """the frame inside rows of `stride` bytes; the padding holds a value no frame pixel may be mistaken for"""
    out = np.full((g.shape[0], stride), 0xA5, np.uint8)
    out[:, : g.shape[1]] = g
    return out


class Member:
    """a batched context and its twin, set up alike; kind: 'gray' | 'bgr'; maps: None | alpha of undistort_setup | (maps0, maps1) for set_undistort_maps;
    host: pageable host numpy frames instead of device frames, with host_stride (gray only) in rows of that many bytes"""

    def __init__(self, factory, w, h, seed, kind="gray", maps=None, cams=(EUROC0, EUROC1), host=False, host_stride=0, max_cnt=100, min_dist=15):
        from dynamic_vins_amd import synth
        from dynamic_vins_amd.frontend import DV_FMT_BGR, DV_MEM_DEVICE, DV_MEM_HOST
        self.w, self.h, self.kind, self.host, self.host_stride = w, h, kind, host or host_stride > 0, host_stride
        kw = dict(width=w, height=h, max_cnt=max_cnt, min_dist=min_dist, cam0=_cam(cams[0], w, h), cam1=_cam(cams[1], w, h))
        self.batched, self.twin = factory(**kw), factory(**kw)
        for c in (self.batched, self.twin):
            if isinstance(maps, float):
                c.undistort_setup(maps)
            elif maps is not None:
                c.set_undistort_maps(0, *maps[0]); c.set_undistort_maps(1, *maps[1])
        self.seq = synth.PlaneSequence(w, h, seed=seed, disparity=4.0 + 0.5 * (seed % 5))
        self.fmt = DV_FMT_BGR if kind == "bgr" else 0
        self.mem_twin, self.mem_job = DV_MEM_HOST | self.fmt, (DV_MEM_HOST if self.host else DV_MEM_DEVICE) | self.fmt
        self.keep = []

    def frame(self, f):
        l, r = self.seq.frame(f)
        if self.kind == "bgr":
            return _bgr(l), _bgr(r)
        if self.host_stride:
            return _padded(l, self.host_stride), _padded(r, self.host_stride)
        return l, r

    def step(self, index, f, t):
        """the twin tracks frame f; -> (its rows, the job of the batched context for the same frame)"""
        import torch
        l, r = self.frame(f)
        stride = l.strides[0]
        want = self.twin.track_stereo(l, r, t, mem=self.mem_twin, stride=stride)
        job = dict(member=index, t=t, mem=self.mem_job)
        if self.host_stride:
            job.update(gray0=l, gray1=r, stride=stride)
        elif self.host:      # (h, w) or (h, w, 3) arrays, the row stride left to the call's default
            job.update(gray0=l, gray1=r)
        else:      # device frames; the row stride is left to the call's default (width, or 3 * width for BGR)
            dl, dr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
            self.keep = [dl, dr]
            job.update(gray0=dl.data_ptr(), gray1=dr.data_ptr())
        return want, job


def _run(members, frames, sits_out=None, min_rows=20):
    """-> (track_info, jobs handed in) after `frames` rounds in which every member's rows were compared with its twin's"""
    import torch
    from dynamic_vins_amd.backend import Batch
    batch = Batch([m.batched for m in members])
    handed = 0
    for f in range(frames):
        t = 0.05 * f
        jobs, want = [], {}
        for i, m in enumerate(members):
            if sits_out == (i, f):
                continue
            want[i], job = m.step(i, f, t)
            jobs.append(job)
        torch.cuda.synchronize()
        batch.track_enqueue(jobs)
        handed += len(jobs)
        for i in want:
            got = members[i].batched.track_stereo_collect()
            assert len(got) == len(want[i]) and len(got) > min_rows, f"frame {f}, member {i}: {len(got)} vs {len(want[i])} rows"
            assert got.tobytes() == want[i].tobytes(), f"frame {f}, member {i}"
    info = batch.track_info()
    batch.close()
    return info, handed


def test_mixed_group_shares_launches_and_equals_the_single_trackers(gpu_ctx_factory):
    """320 x 240 stereo, 8 frames, six members in one group: plain gray | gray + undistort_setup | gray + undistort_setup on another camera pair (other maps; it sits
    round 4 out) | BGR + undistort_setup | BGR without maps | gray + maps from pageable host arrays in rows of 352 bytes.  Every member's rows equal its twin's
    dv_track_stereo, and every job went through the shared launches (no round degenerates to a single job)."""
    w, h = 320, 240
    members = [Member(gpu_ctx_factory, w, h, 11),
               Member(gpu_ctx_factory, w, h, 12, maps=0.0),
               Member(gpu_ctx_factory, w, h, 13, maps=0.0, cams=(STRONG, EUROC0)),
               Member(gpu_ctx_factory, w, h, 14, kind="bgr", maps=0.0),
               Member(gpu_ctx_factory, w, h, 15, kind="bgr"),
               Member(gpu_ctx_factory, w, h, 16, maps=0.0, host_stride=352)]
    a, b = members[1].batched.undistort_maps(0), members[2].batched.undistort_maps(0)
    assert not np.array_equal(a[0], b[0])                      # members 1 and 2 do carry different maps
    info, handed = _run(members, 8, sits_out=(2, 4))
    assert handed == 6 * 8 - 1
    assert info["members_single"] == 0 and info["members_batched"] == handed and info["rounds"] == 8, info


def _alpha1_maps(oracle, w, h):
    """the maps dv_undistort_setup(alpha = 1) installs for the EuRoC pair scaled to w x h, from the oracle; checked on the CPU to take both guarded paths of the remap
    body: the border path (a neighbour outside the source reads 0) and the last-row rule of the paired 8-byte load of the three-channel case (in-bounds entries with
    sy == h - 2 and sx in {w - 3, w - 2}).  The guard only keeps the load from reading 2 bytes past the last source row; both forms of the load give the same pixels, so no
    comparison of rows can tell whether it is there: the test makes sure the guarded path is run, not that the guard works.  -> (hand_made, maps)"""
    from dynamic_vins_amd.frontend import optimal_new_camera
    maps = []
    for c in (EUROC0, EUROC1):
        cam = sim.cam_tuple(sim.scaled_cam(c, w, h, 752, 480))
        m1, m2 = oracle.init_undistort_map(cam, optimal_new_camera(cam, w, h, 1.0), w, h)
        maps.append((m1.copy(), m2.copy()))
    sx, sy = maps[0][0][..., 0].astype(int), maps[0][0][..., 1].astype(int)
    border = (sx < 0) | (sx >= w - 1) | (sy < 0) | (sy >= h - 1)
    guard = lambda sx, sy: (sy == h - 2) & (sx >= w - 3) & (sx <= w - 2)      # (sx >= w - 1 is the border path, not the guard)
    last = guard(sx, sy)
    assert border.any()
    hand_made = not last.any()
    if hand_made:      # this camera does not reach the last source row's end: three entries of the first row are pointed there by hand
        for k, x in enumerate((w - 3, w - 2, w - 1)):
            maps[0][0][0, k] = (x, h - 2)
        sx, sy = maps[0][0][..., 0].astype(int), maps[0][0][..., 1].astype(int)
        assert guard(sx, sy).any()
    return hand_made, maps


@pytest.mark.parametrize("w,h", [(322, 242), (1030, 64)])
def test_tail_and_border_shapes(gpu_ctx_factory, oracle, w, h):
    """gray + maps | BGR + maps | BGR as (h, w, 3) host arrays, 4 frames.  322 x 242: w % 4 == 2 — the tail store and the clamped map read.  1030 x 64: one x-block of 1024 pixels and a second
    one that holds 6.  Maps of alpha = 1: destination pixels outside the source (border path) and at the end of the last but one source row (the paired load's guard)."""
    hand_made, maps = _alpha1_maps(oracle, w, h)
    setup = maps if hand_made else 1.0
    kw = dict(max_cnt=100, min_dist=8)
    members = [Member(gpu_ctx_factory, w, h, 21, maps=setup, **kw),
               Member(gpu_ctx_factory, w, h, 22, kind="bgr", maps=setup, **kw),
               Member(gpu_ctx_factory, w, h, 23, kind="bgr", host=True, **kw)]
    if not hand_made:      # what the test reasoned about on the CPU is what the device installed
        for c in (0, 1):
            got = members[1].batched.undistort_maps(c)
            assert np.array_equal(got[0], maps[c][0]) and np.array_equal(got[1], maps[c][1])
    info, handed = _run(members, 4)
    assert info["members_single"] == 0 and info["members_batched"] == handed == 12, info


def test_all_plain_group_is_unchanged(gpu_ctx_factory):
    """three plain members: rows and counters as before.  (That the level-0 launch is not issued cannot be recorded without a new ABI symbol — a member with
    dv_timing on keeps its own launches — so the launch count of this case rests on tests/test_batch.py and on the code: the launch sits behind `if (n_l0)`.)"""
    members = [Member(gpu_ctx_factory, 320, 240, 31 + i) for i in range(3)]
    info, handed = _run(members, 4)
    assert info["members_single"] == 0 and info["members_batched"] == handed == 12 and info["rounds"] == 4, info


def test_failed_round_leaves_no_wreckage(gpu_ctx_factory):
    """a stereo member with maps for camera 0 only makes the round fail with the single path's message; no member keeps a flipped current pyramid or a pending frame:
    after the maps are completed, the following rounds give the rows of twins that never saw the bad round"""
    import torch
    from dynamic_vins_amd.backend import Batch
    from dynamic_vins_amd.frontend import DvinsError
    w, h = 320, 240
    members = [Member(gpu_ctx_factory, w, h, 41), Member(gpu_ctx_factory, w, h, 42, maps=0.0), Member(gpu_ctx_factory, w, h, 43, kind="bgr", maps=0.0)]
    bad = members[1].batched
    maps1 = bad.undistort_maps(1)
    maps0 = bad.undistort_maps(0)
    for c in (bad, members[1].twin):      # own maps (same values) on both: the cameras the rows are lifted with stay alike
        c.set_undistort_maps(0, *maps0); c.set_undistort_maps(1, *maps1)
    # the single path's message, from a context of its own
    lone = gpu_ctx_factory(width=w, height=h, max_cnt=100, min_dist=15, cam0=_cam(EUROC0, w, h), cam1=_cam(EUROC1, w, h))
    lone.set_undistort_maps(0, *maps0)
    l, r = members[1].seq.frame(0)
    with pytest.raises(DvinsError) as single_err:
        lone.track_stereo(l, r, 0.0)
    assert "camera 1" in str(single_err.value)
    batch = Batch([m.batched for m in members])

    def good_round(f):
        want, jobs = {}, []
        for i, m in enumerate(members):
            want[i], job = m.step(i, f, 0.05 * f)
            jobs.append(job)
        torch.cuda.synchronize()
        batch.track_enqueue(jobs)
        for i in want:
            got = members[i].batched.track_stereo_collect()
            assert len(got) > 20 and got.tobytes() == want[i].tobytes(), f"frame {f}, member {i}"

    good_round(0)
    good_round(1)
    # the bad round: frame 2 for everybody, but member 1 has lost its camera 1 maps.  The twins do not see it.
    bad.set_undistort_maps(1)
    jobs, keep = [], []
    for i, m in enumerate(members):
        fl, fr = m.frame(2)
        dl, dr = torch.from_numpy(fl).cuda(), torch.from_numpy(fr).cuda()
        keep += [dl, dr]
        jobs.append(dict(member=i, gray0=dl.data_ptr(), gray1=dr.data_ptr(), t=0.1, mem=m.mem_job))
    torch.cuda.synchronize()
    with pytest.raises(DvinsError) as batch_err:
        batch.track_enqueue(jobs)
    assert str(batch_err.value) == str(single_err.value)
    for m in members:      # nothing is pending on any member
        with pytest.raises(DvinsError):
            m.batched.track_stereo_collect()
    bad.set_undistort_maps(1, *maps1)
    for f in (2, 3, 4):
        good_round(f)
    info = batch.track_info()
    assert info["members_batched"] == 15 and info["members_single"] == 0, info
    batch.close()


def test_unknown_memory_kind_fails_the_round_and_leaves_no_wreckage(gpu_ctx_factory):
    """160 x 120 stereo, two members: a job with memory kind 7 makes the round fail with exactly the text a lone context gives for track_stereo(..., mem=7); nothing
    is pending on either member, and the following rounds give the rows of twins that never saw the bad round"""
    import torch
    from dynamic_vins_amd.backend import Batch
    from dynamic_vins_amd.frontend import DvinsError
    w, h = 160, 120
    kw = dict(max_cnt=40, min_dist=10)
    members = [Member(gpu_ctx_factory, w, h, 51, **kw), Member(gpu_ctx_factory, w, h, 52, **kw)]
    lone = gpu_ctx_factory(width=w, height=h, cam0=_cam(EUROC0, w, h), cam1=_cam(EUROC1, w, h), **kw)
    l, r = members[1].seq.frame(0)
    with pytest.raises(DvinsError) as single_err:
        lone.track_stereo(l, r, 0.0, mem=7)
    assert "memory kind" in str(single_err.value)
    batch = Batch([m.batched for m in members])

    def good_round(f):
        want, jobs = {}, []
        for i, m in enumerate(members):
            want[i], job = m.step(i, f, 0.05 * f)
            jobs.append(job)
        torch.cuda.synchronize()
        batch.track_enqueue(jobs)
        for i in want:
            got = members[i].batched.track_stereo_collect()
            assert len(got) > 20 and got.tobytes() == want[i].tobytes(), f"frame {f}, member {i}"

    good_round(0)
    good_round(1)
    # the bad round: frame 2 for both, member 1's job with a memory kind that does not exist.  The twins do not see it.
    jobs, keep = [], []
    for i, m in enumerate(members):
        fl, fr = m.frame(2)
        dl, dr = torch.from_numpy(fl).cuda(), torch.from_numpy(fr).cuda()
        keep += [dl, dr]
        jobs.append(dict(member=i, gray0=dl.data_ptr(), gray1=dr.data_ptr(), t=0.1, mem=7 if i == 1 else m.mem_job))
    torch.cuda.synchronize()
    with pytest.raises(DvinsError) as batch_err:
        batch.track_enqueue(jobs)
    assert str(batch_err.value) == str(single_err.value)
    for m in members:      # nothing is pending on either member
        with pytest.raises(DvinsError):
            m.batched.track_stereo_collect()
    for f in (2, 3):
        good_round(f)
    info = batch.track_info()
    assert info["members_batched"] == 8 and info["members_single"] == 0, info
    batch.close()


def test_refused_single_enqueue_leaves_the_context_as_it_was(gpu_ctx_factory):
    """160 x 120 stereo, one context and its twin, both with the same maps for both cameras.  After two frames the context loses its camera 1 maps and has
    track_stereo refused; with the maps back, its next frames' rows equal the twin's, which never saw the refused call: the refusal did not turn the context to the
    other pyramid (the temporal LK of the next frame would start from the frame before last)"""
    from dynamic_vins_amd.frontend import DvinsError
    w, h = 160, 120
    m = Member(gpu_ctx_factory, w, h, 61, maps=0.0, max_cnt=40, min_dist=10)
    ctx, twin = m.batched, m.twin
    maps0, maps1 = ctx.undistort_maps(0), ctx.undistort_maps(1)
    for c in (ctx, twin):      # own maps (same values) on both: the cameras the rows are lifted with stay alike when camera 1's maps go and come back
        c.set_undistort_maps(0, *maps0); c.set_undistort_maps(1, *maps1)

    def good_frame(f):
        l, r = m.frame(f)
        got, want = ctx.track_stereo(l, r, 0.05 * f), twin.track_stereo(l, r, 0.05 * f)
        assert len(got) > 20 and got.tobytes() == want.tobytes(), f"frame {f}"

    good_frame(0)
    good_frame(1)
    ctx.set_undistort_maps(1)
    l, r = m.frame(2)
    with pytest.raises(DvinsError) as err:
        ctx.track_stereo(l, r, 0.1)
    assert "camera 1" in str(err.value)
    with pytest.raises(DvinsError):      # nothing is pending
        ctx.track_stereo_collect()
    ctx.set_undistort_maps(1, *maps1)
    good_frame(2)
    good_frame(3)


def test_runner_group_of_undistorted_members_shares_the_front_end():
    """Runner over three Pipeline(undistort_input=True) members in one group: the shared front end (default) against `batch_front` 0 — states, trajectories and row
    counts bit for bit, and the members are counted as batched"""
    from dynamic_vins_amd.backend import Runner
    from dynamic_vins_amd.pipeline import Pipeline, SyntheticSequence
    w, h, S, frames = 320, 240, 3, 20
    cam0, cam1 = sim.scaled_cam(EUROC0, w, h, 752, 480), sim.scaled_cam(EUROC1, w, h, 752, 480)
    seqs = [SyntheticSequence(w, h, cam0, frames, rate=20.0, phase=0.9 * i, cam1=cam1) for i in range(S)]
    a = [Pipeline(q, max_cnt=100, min_dist=15, max_iters=8, use_imu=1, undistort_input=True) for q in seqs]
    b = [Pipeline(q, max_cnt=100, min_dist=15, max_iters=8, use_imu=1, undistort_input=True) for q in seqs]
    ra, rb = Runner(a, group_size=S, threads=1), Runner(b, group_size=S, threads=1)
    rb.set("batch_front", 0)
    ra.run(frames - 1); rb.run(frames - 1)
    ia, ib = ra.track_info(), rb.track_info()
    assert ia["members_batched"] > 0 and ia["members_single"] == 0, ia
    assert ib["members_batched"] == 0, ib
    for i in range(S):
        sa, pa, _, fa = ra.get(i); rows_a = ra.last_rows
        sb, pb, _, fb = rb.get(i); rows_b = rb.last_rows
        assert fa == fb == frames - 1 and rows_a == rows_b and rows_a > 0 and len(pa) == len(pb) >= 1
        assert np.array_equal(pa, pb) and np.array_equal(np.ctypeslib.as_array(sa.window), np.ctypeslib.as_array(sb.window)), i
        assert np.array_equal(ra.frames(i), rb.frames(i)), i
    ra.close(); rb.close()
    for p in a + b:
        p.ctx.close()
