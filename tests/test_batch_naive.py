"""dv_batch_track_enqueue with DV_MODE_NAIVE members that carry instance masks (`-m gpu`): TrackImageNaive of several sequences in the group's shared launches —
the GPU tracker over a job table (lk_cuda_track_multi_kernel), its cuda::pyrDown-rule pyramid levels and the masks' erosion in one launch each — beside raw members.
The yardstick throughout is the member's own dv_track_stereo on a twin context fed the same frames and masks: rows compared as bytes, frame after frame, and
dv_batch_track_info asserted exactly.  The masks differ per member and move from frame to frame: a stale or swapped mask changes rows."""
import numpy as np
import pytest

from dynamic_vins_amd import sim

pytestmark = pytest.mark.gpu

RAW, NAIVE = 0, 1      # DV_MODE_RAW, DV_MODE_NAIVE


def _cam(w, h):
    from dynamic_vins_amd.frontend import make_cam
    return make_cam(*sim.cam_tuple(sim.scaled_cam(sim.EUROC, w, h, 752, 480)))


def _bgr(g):
    """gray -> three unequal channels: B = g, G = 3 g / 4 + 20, R = 255 - g / 4"""
    g = g.astype(np.uint16)
    return np.ascontiguousarray(np.stack([g, (3 * g) // 4 + 20, 255 - g // 4], -1).astype(np.uint8))


def _padded(g, stride):
    """the image inside rows of `stride` bytes; the padding holds a value that is neither 0 nor 255"""
    out = np.full((g.shape[0], stride), 0xA5, np.uint8)
    out[:, : g.shape[1]] = g
    return out


def band_mask(w, h, f, seed, border=False):
    """the inverse instance mask of frame f (0 = object, excluded): one object a third of the image wide that moves 14 px per frame, placed by the member's seed.
    border: the object starts at the left image border over the full height and grows to the right"""
    m = np.full((h, w), 255, np.uint8)
    bw = w // 3
    if border:
        m[:, : bw // 2 + 14 * f] = 0
    else:
        x0 = (17 * seed + 14 * f) % (w - bw)
        m[h // 8 + seed % 7: h - h // 8, x0: x0 + bw] = 0
    return m


class Member:
    """a batched context and its twin, set up alike.  mode(f) -> RAW | NAIVE per frame (an int: every frame); kind 'gray' | 'bgr'; host: pageable host frames and masks,
    with host_stride in rows of that many bytes; the twin is always fed host arrays"""

    def __init__(self, factory, w, h, seed, mode=NAIVE, kind="gray", host=False, host_stride=0, max_cnt=100, min_dist=15, morph=0, border=False, mask_of=None):
        from dynamic_vins_amd import synth
        from dynamic_vins_amd.frontend import DV_FMT_BGR, DV_MEM_DEVICE, DV_MEM_HOST
        self.w, self.h, self.seed, self.kind, self.host, self.host_stride, self.border = w, h, seed, kind, host or host_stride > 0, host_stride, border
        self.mode = mode if callable(mode) else (lambda f, m=mode: m)
        self.mask_of = mask_of or (lambda f: band_mask(w, h, f, seed, border))
        self.kw = dict(width=w, height=h, max_cnt=max_cnt, min_dist=min_dist, cam0=_cam(w, h), cam1=_cam(w, h), mask_morphology_size=morph)
        self.factory = factory
        self.batched, self.twin = factory(**self.kw), factory(**self.kw)
        self.seq = synth.PlaneSequence(w, h, seed=seed, disparity=4.0 + 0.5 * (seed % 5))
        self.fmt = DV_FMT_BGR if kind == "bgr" else 0
        self.mem_twin, self.mem_job = DV_MEM_HOST | self.fmt, (DV_MEM_HOST if self.host else DV_MEM_DEVICE) | self.fmt
        self.keep = []

    def inputs(self, f):
        """-> (left, right, mask or None, mode) of frame f as host arrays, in the row layout both contexts are given"""
        l, r = self.seq.frame(f)
        mode = self.mode(f)
        mask = self.mask_of(f) if mode == NAIVE else None
        if self.kind == "bgr":
            l, r = _bgr(l), _bgr(r)
        elif self.host_stride:
            l, r = _padded(l, self.host_stride), _padded(r, self.host_stride)
            mask = _padded(mask, self.host_stride) if mask is not None else None
        return l, r, mask, mode

    def job(self, index, f, t):
        """the job of the batched context for frame f"""
        import torch
        l, r, mask, mode = self.inputs(f)
        job = dict(member=index, t=t, mem=self.mem_job, mode=mode)
        if self.host:      # host arrays (the mask too); a padded layout names its stride
            job.update(gray0=l, gray1=r, mask=mask)
            if self.host_stride:
                job.update(stride=self.host_stride)
        else:      # device frames and a device mask; the row stride is left to the call's default (width, or 3 * width for BGR; the mask: width)
            dl, dr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
            dm = torch.from_numpy(mask).cuda() if mask is not None else None
            self.keep = [dl, dr, dm]
            job.update(gray0=dl.data_ptr(), gray1=dr.data_ptr(), mask=dm.data_ptr() if dm is not None else None)
        return job

    def step(self, index, f, t, twin=None):
        """the twin tracks frame f; -> (its rows, the job of the batched context for the same frame)"""
        l, r, mask, mode = self.inputs(f)
        want = (twin or self.twin).track_stereo(l, r, t, mask, mode, mem=self.mem_twin, stride=l.strides[0])
        return want, self.job(index, f, t)


def _round(batch, members, f, present=None, min_rows=20, no_min=()):
    """one round: the twins track frame f, the batch enqueues the same jobs, every member's rows are compared.  -> jobs handed in"""
    import torch
    t = 0.05 * f
    jobs, want = [], {}
    for i, m in enumerate(members):
        if present is not None and i not in present:
            continue
        want[i], job = m.step(i, f, t)
        jobs.append(job)
    torch.cuda.synchronize()
    batch.track_enqueue(jobs)
    for i in want:
        got = members[i].batched.track_stereo_collect()
        assert len(got) == len(want[i]), f"frame {f}, member {i}: {len(got)} vs {len(want[i])} rows"
        if i not in no_min:
            assert len(got) > min_rows, f"frame {f}, member {i}: {len(got)} rows"
        assert got.tobytes() == want[i].tobytes(), f"frame {f}, member {i}"
    return len(jobs), want


def test_mixed_group_of_raw_and_naive_members_shares_launches(gpu_ctx_factory):
    """330 x 250 stereo (levels 165 x 125, 83 x 63, 42 x 32: the cuda-rule levels have odd sizes), 7 frames, seven members in one group: two raw gray | naive with device
    frames and a device mask | naive with mask_morphology_size 5 and an object that touches the image border | naive from pageable host arrays, frames and mask in rows
    of 352 bytes | naive BGR with a single-channel mask | naive with max_cnt 60, which sits round 3 out.  Every member's rows equal its twin's dv_track_stereo, and
    every job went through the shared launches."""
    from dynamic_vins_amd.backend import Batch
    w, h, frames = 330, 250, 7
    members = [Member(gpu_ctx_factory, w, h, 11, mode=RAW),
               Member(gpu_ctx_factory, w, h, 12, mode=RAW),
               Member(gpu_ctx_factory, w, h, 13),
               Member(gpu_ctx_factory, w, h, 14, morph=5, border=True),
               Member(gpu_ctx_factory, w, h, 15, host_stride=352),
               Member(gpu_ctx_factory, w, h, 16, kind="bgr"),
               Member(gpu_ctx_factory, w, h, 17, max_cnt=60)]
    assert not np.array_equal(members[2].mask_of(1), members[4].mask_of(1)) and not np.array_equal(members[2].mask_of(1), members[2].mask_of(2))
    # the test's own inputs, on twins alone: the mask of member 2 does remove tracked points — a second twin tracks the same frames in naive mode without a mask
    masked, free = gpu_ctx_factory(**members[2].kw), gpu_ctx_factory(**members[2].kw)
    bites = 0
    for f in range(frames):
        l, r, mask, _ = members[2].inputs(f)
        a, b = masked.track_stereo(l, r, 0.05 * f, mask, NAIVE), free.track_stereo(l, r, 0.05 * f, None, NAIVE)
        ta, tb = int((a["track_cnt"] > 1).sum()), int((b["track_cnt"] > 1).sum())
        print(f"frame {f}: {len(a)} rows ({ta} tracked) with the mask, {len(b)} ({tb} tracked) without")
        bites += len(a) < len(b) or ta < tb
    assert bites >= 1, "the mask never removed a tracked point: the comparison below would test nothing"
    batch = Batch([m.batched for m in members])
    handed = 0
    for f in range(frames):
        n, _ = _round(batch, members, f, present=[i for i in range(7) if not (i == 6 and f == 3)])
        handed += n
    info = batch.track_info()
    batch.close()
    assert handed == 7 * frames - 1
    assert info["members_single"] == 0 and info["members_batched"] == handed and info["rounds"] == frames, info


def test_class_rules_round_by_round(gpu_ctx_factory):
    """320 x 240 stereo, 7 rounds, members A, B raw | C naive, raw in round 4 | D naive from round 1 on (it has no frame in round 0) | E raw, naive from round 2 on.
    (single, batched) per round: 0: C is the only naive job (1, 3) | 1: C and D (0, 5) | 2: E changes to naive, its previous frame has no pyramid of the GPU
    tracker's flavour (1, 4) | 3: (0, 5) | 4: C tracks raw (0, 5) | 5: C is naive again, its previous frame was raw: its own launches, which rebuild that pyramid —
    a pyramid left marked valid from round 3 would give other rows — (1, 4) | 6: C shares again, D has dv_track_unmask_static staged (1, 4)."""
    from dynamic_vins_amd.backend import Batch
    w, h = 320, 240
    members = [Member(gpu_ctx_factory, w, h, 21, mode=RAW),
               Member(gpu_ctx_factory, w, h, 22, mode=RAW),
               Member(gpu_ctx_factory, w, h, 23, mode=lambda f: RAW if f == 4 else NAIVE),
               Member(gpu_ctx_factory, w, h, 24),
               Member(gpu_ctx_factory, w, h, 25, mode=lambda f: RAW if f < 2 else NAIVE)]
    expect = [(1, 3), (0, 5), (1, 4), (0, 5), (0, 5), (1, 4), (1, 4)]
    batch = Batch([m.batched for m in members])
    single = batched = 0
    for f, (ds, db) in enumerate(expect):
        if f == 6:      # a static instance's pixels leave D's mask: a rectangle inside the object of frame 6, on both contexts
            d = members[3]
            ys, xs = np.nonzero(d.mask_of(6) == 0)
            x0, y0 = int(xs.min()) + 8, int(ys.min()) + 8
            roi = np.zeros((60, 50), np.uint8); roi[5:55, 5:45] = 1
            det = dict(track_id=7, rect=(x0, y0, 50, 60), mask=roi)
            for c in (d.batched, d.twin):
                c.track_unmask_static([det], [7])
        _round(batch, members, f, present=[1, 2, 4, 0] if f == 0 else None)
        info = batch.track_info()
        assert (info["members_single"] - single, info["members_batched"] - batched) == (ds, db), (f, info)
        single, batched = info["members_single"], info["members_batched"]
    assert batch.track_info()["rounds"] == len(expect)
    batch.close()


def test_first_frames_and_an_empty_mask(gpu_ctx_factory):
    """320 x 240 stereo, 6 frames, three naive members and a raw one.  Round 0 has no previous frame: the temporal stage has nothing to do.  In frame 3 member 1's mask is 0
    everywhere: both sides give the same rows there (possibly none), and frame 4 recovers identically."""
    from dynamic_vins_amd.backend import Batch
    w, h = 320, 240
    empty = lambda f: np.zeros((h, w), np.uint8) if f == 3 else band_mask(w, h, f, 32)
    members = [Member(gpu_ctx_factory, w, h, 31), Member(gpu_ctx_factory, w, h, 32, mask_of=empty), Member(gpu_ctx_factory, w, h, 33, morph=3), Member(gpu_ctx_factory, w, h, 34, mode=RAW)]
    batch = Batch([m.batched for m in members])
    for f in range(6):
        _, want = _round(batch, members, f, no_min=(1,) if f == 3 else ())
        if f == 3:
            print(f"frame 3, member 1: {len(want[1])} rows under the empty mask")
    info = batch.track_info()
    batch.close()
    assert info["members_single"] == 0 and info["members_batched"] == 24 and info["rounds"] == 6, info


def test_refused_round_leaves_no_wreckage(gpu_ctx_factory):
    """320 x 240 stereo, two naive members and a raw one.  After round 2 member 1 is not collected, so the next call fails with the text a lone context gives for a second
    dv_track_stereo_enqueue; nothing is pending on the other members, member 1 still holds its rows of round 2, and rounds 3 to 5 give the rows of twins that never saw
    the refused call: no member was turned to the other pyramid"""
    import torch
    from dynamic_vins_amd.backend import Batch
    from dynamic_vins_amd.frontend import DvinsError
    w, h = 320, 240
    members = [Member(gpu_ctx_factory, w, h, 41), Member(gpu_ctx_factory, w, h, 42), Member(gpu_ctx_factory, w, h, 43, mode=RAW)]
    lone = gpu_ctx_factory(**members[1].kw)
    l, r, mask, _ = members[1].inputs(0)
    lone.track_stereo_enqueue(l, r, 0.0, mask, NAIVE)
    with pytest.raises(DvinsError) as single_err:
        lone.track_stereo_enqueue(l, r, 0.05, mask, NAIVE)
    lone.track_stereo_collect()
    assert "not collected" in str(single_err.value)
    batch = Batch([m.batched for m in members])
    _round(batch, members, 0)
    _round(batch, members, 1)
    # round 2, member 1 left uncollected
    jobs, want = [], {}
    for i, m in enumerate(members):
        want[i], job = m.step(i, 2, 0.1)
        jobs.append(job)
    torch.cuda.synchronize()
    batch.track_enqueue(jobs)
    for i in (0, 2):
        got = members[i].batched.track_stereo_collect()
        assert len(got) > 20 and got.tobytes() == want[i].tobytes(), i
    held = [m.keep for m in members]
    # the refused round: frame 3 for everybody.  The twins do not see it.
    jobs = [m.job(i, 3, 0.15) for i, m in enumerate(members)]
    torch.cuda.synchronize()
    with pytest.raises(DvinsError) as batch_err:
        batch.track_enqueue(jobs)
    assert str(batch_err.value) == str(single_err.value)
    for i in (0, 2):      # nothing is pending on the others
        with pytest.raises(DvinsError):
            members[i].batched.track_stereo_collect()
    got = members[1].batched.track_stereo_collect()      # round 2's rows are still there
    assert len(got) > 20 and got.tobytes() == want[1].tobytes()
    del held
    for f in (3, 4, 5):
        _round(batch, members, f)
    info = batch.track_info()
    batch.close()
    assert info["members_batched"] == 18 and info["members_single"] == 0 and info["rounds"] == 6, info
