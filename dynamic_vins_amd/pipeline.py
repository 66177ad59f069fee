"""Track + BA pipeline on one GPU (what the reference runs as threads T2 + T3, system/main.cpp:178,394-404):
the front end of frame k+1 is enqueued on the ctx's tracking stream before the back end of frame k is solved on
the BA stream, so the two overlap on the device like the reference's two threads overlap on the CPU."""
import numpy as np

from . import sim
from .backend import Estimator
from .frontend import Context, DV_MEM_DEVICE, DV_MEM_HOST, DV_MODE_RAW, make_cam


class SyntheticSequence:
    """rendered stereo frames resident in HBM + IMU stream for one trajectory (SURVEY 8(d) primary input)"""

    def __init__(self, w, h, cam, n_frames, rate=20.0, t0=1.0, phase=0.0, noise=None, device=None, seed=sim.TEX_SEED, baseline=0.12, body_is_camera=False, cam1=None, traj=None):
        import torch
        from .render import RoomRenderer
        self.w, self.h, self.cam, self.dt, self.t0 = w, h, cam, 1.0 / rate, t0 + phase
        self.cam1 = cam1 if cam1 is not None else cam
        self.noise = noise or dict(acc_n=0.02, gyr_n=0.002, acc_w=2e-4, gyr_w=2e-5)
        self.rig = sim.rig(baseline, body_is_camera)
        self.traj = traj if traj is not None else sim.Trajectory()
        rr = RoomRenderer(cam, w, h, device=device, seed=seed, cam1=cam1)
        self.frames = [rr.stereo(self.traj, self.t0 + k * self.dt, self.rig["t_ic1"]) for k in range(n_frames)]
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.times = [self.t0 + k * self.dt for k in range(n_frames)]
        self.imu_t, self.imu_a, self.imu_g = sim.imu_stream(self.traj, self.t0 - 0.05, self.times[-1] + 0.1, 200.0, seed=0xBEEF, **self.noise)

    def host_frame(self, k):
        return self.frames[k][0].cpu().numpy(), self.frames[k][1].cpu().numpy()


class Pipeline:
    def __init__(self, seq: SyntheticSequence, max_cnt=250, min_dist=25, max_iters=10, device=0, use_imu=1, host_frames=False, ba_stride=1, est_kw=None, undistort_input=False,
                 undistort_alpha=0.0):
        self.seq = seq
        self.host = [seq.host_frame(k) for k in range(len(seq.frames))] if host_frames else None
        c = make_cam(*sim.cam_tuple(seq.cam))
        self.ctx = Context(width=seq.w, height=seq.h, max_cnt=max_cnt, min_dist=min_dist, cam0=c, cam1=make_cam(*sim.cam_tuple(seq.cam1)), device=device)
        # undistort_input (cfg::is_undistort_input, utils/camera_model.cpp:479-504): the sequence's frames are the DISTORTED ones; the tracker remaps them on the way into
        # pyramid level 0 and every camera behind it — the estimator's included — is (newK, 0)
        self.undistort_input = bool(undistort_input)
        self.cam0, self.cam1 = self.ctx.undistort_setup(undistort_alpha) if self.undistort_input else self.ctx.cameras()
        self.est_kw = dict(use_imu=use_imu, stereo=1, max_iters=max_iters, ric=seq.rig["est_ric"], tic=seq.rig["est_tic"], **seq.noise)
        self.est_kw.update(est_kw or {})          # keyframe_parallax, g_norm, ... of a shipped YAML (ref_configs.py)
        self.est = Estimator(self.ctx, **self.est_kw)
        self.k_imu = 0
        self.next = 0
        self.enqueued = False
        self._prefetched = None
        self.poses, self.pose_times = [], []
        self.ba_stride = ba_stride          # 2: only every 2nd tracked frame is forwarded to the back end (system/main.cpp:300-307)
        self.last_state = None

    def _enqueue(self, k):
        if self.host is not None:                      # host buffers: the upload rides on the tracking stream
            l, r = self.host[k]
            self.ctx.track_stereo_enqueue(l, r, self.seq.times[k], None, DV_MODE_RAW, DV_MEM_HOST)
        else:
            l, r = self.seq.frames[k]
            self.ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), self.seq.times[k], None, DV_MODE_RAW, DV_MEM_DEVICE)
        self.enqueued = True

    def _feed_imu(self, t):
        s = self.seq
        hi = self.k_imu
        while hi < len(s.imu_t) and s.imu_t[hi] <= t + 0.006:
            hi += 1
        for j in range(self.k_imu, hi):
            self.est.InputIMU(s.imu_t[j], s.imu_a[j], s.imu_g[j])
        self.k_imu = hi

    def step(self, defer_end=False):
        """processes frame self.next through track + BA; returns the estimator state.
        Order (the reference's T2 / T3 overlap on one host thread): collect tracking of k -> begin BA of k (host prep +
        enqueue on the BA stream) -> enqueue tracking of k+1 and feed k+1's IMU samples while the GPU solves -> end BA of k."""
        k = self.next
        s = self.seq
        rows, self._prefetched = self._prefetched, None
        if rows is None:
            if not self.enqueued:
                self._enqueue(k)
            rows = self.ctx.track_stereo_collect()
        self.enqueued = False
        t = s.times[k]
        if self.ba_stride > 1 and (k % self.ba_stride) != 0:      # tracked only: the reference pushes frames 0, 2, 4, ... (cnt % 2 == 0, cnt from 0: system/main.cpp:181,300-312)
            if k + 1 < len(s.frames):
                self._enqueue(k + 1)
            self.next += 1
            self.rows = rows
            return self.last_state if self.last_state is not None else self.est.state
        self._feed_imu(t)
        rc = self.est.ProcessMeasurementsBegin(rows, t)
        if rc != 0:
            raise RuntimeError("IMU stream does not cover the frame")
        if k + 1 < len(s.frames):
            self._enqueue(k + 1)                     # overlaps with the BA of frame k
            self._feed_imu(s.times[k + 1])
            if not defer_end:
                # the tracker finishes frame k+1 long before the BA of frame k does: its rows are collected NOW, not between the end of this frame's BA and the
                # begin of the next (where the collect sat on the critical path of the BA stream: ~11 us per frame)
                self._prefetched = self.ctx.track_stereo_collect()
        self.rows = rows
        if defer_end:
            self._pending_t = t
            return None
        return self._finish(t)

    def _finish(self, t):
        st = self.est.ProcessMeasurementsEnd()
        if getattr(self, "keep_frame_rows", False):          # every frame handed to the back end, as the runner's dv_runner_get_frames keeps them (what SaveBodyTrajectory writes)
            self.frame_rows.append((t, self.est.window()[10, :7].copy(), int(st.nonlinear)))
        if st.nonlinear:
            self.poses.append(self.est.window()[10, :7])
            self.pose_times.append(t)
        self.next += 1
        self.last_state = st
        return st

    def step_begin(self):
        """first half of step(): everything up to and including the enqueue of frame k's BA and of frame k+1's tracking.  With step_end() it lets ONE host
        thread interleave several independent sequences on one GPU (each Pipeline owns its streams): while the BA of sequence A runs, the host prepares B."""
        self._pending_t = None
        st = self.step(defer_end=True)
        self._early = st                              # tracked-only frame (ba_stride): already complete
        return st

    def step_end(self):
        if self._pending_t is None:
            return self._early
        t, self._pending_t = self._pending_t, None
        return self._finish(t)

    def ate(self):
        """ATE RMSE against the synthetic ground truth, computed the way the reference's scripts do: associate.py's nearest-stamp pairing (0.02 s) of the two
        stamped trajectories, then evaluate_ate.py's alignment (io_formats.evaluate_ate)"""
        from . import io_formats
        gt = [self.seq.traj.p(t) for t in self.pose_times]
        return io_formats.evaluate_ate(self.pose_times, gt, self.pose_times, np.array(self.poses)[:, :3])[0]


class DynamicSequence(SyntheticSequence):
    """SyntheticSequence with moving boxes (dynsim.default_boxes): per frame the stereo pair (resident in HBM), and — as host arrays — what the perception
    front end of the reference delivers: the inverse merged instance mask, one detection per visible object (track id, rectangle, ROI mask, 3-D box,
    extra 3-D points sampled from the depth map like InstFeat::DetectExtraPoints, front_end/instance_feature.cpp:413-461) (dynamic variant)."""

    def __init__(self, w, h, cam, n_frames, rate=20.0, t0=1.0, noise=None, device=None, boxes=None, min_pixels=400, seed=sim.TEX_SEED, baseline=0.12, body_is_camera=False, cam1=None, traj=None):
        import torch
        from . import dynsim
        from .render import DynRoomRenderer
        self.w, self.h, self.cam, self.dt, self.t0 = w, h, cam, 1.0 / rate, t0
        self.cam1 = cam1 if cam1 is not None else cam
        self.noise = noise or dict(acc_n=0.02, gyr_n=0.002, acc_w=2e-4, gyr_w=2e-5)
        self.rig = sim.rig(baseline, body_is_camera)
        self.traj = traj if traj is not None else sim.Trajectory()
        if boxes == "escort" or (isinstance(boxes, tuple) and boxes[0] == "escort"):      # boxes travelling with the camera: objects in every frame
            boxes = dynsim.escort_boxes(self.traj, boxes[1] if isinstance(boxes, tuple) else 4)
        self.boxes = boxes if boxes is not None else dynsim.default_boxes()
        rr = DynRoomRenderer(cam, w, h, device=device, seed=seed, cam1=cam1)
        self.times = [self.t0 + k * self.dt for k in range(n_frames)]
        self.frames, self.inv_mask, self.inv_mask_dev, self.dets, self.boxes3d = [], [], [], [], []
        self.disp_dev, self.baseline = [], float(baseline)      # SemanticImage::disp per frame (CV_32F, resident): what the stereo network of the reference delivers
        rays = rr.rays.cpu().numpy().reshape(h, w, 3)
        for t in self.times:
            left, right, ident, depth = rr.stereo_dynamic(self.traj, t, self.boxes, self.rig["t_ic1"])
            self.frames.append((left, right))
            idm, dep = ident.cpu().numpy(), depth.cpu().numpy()
            self.inv_mask.append(np.ascontiguousarray(np.where(idm == 0, 255, 0).astype(np.uint8)))
            self.inv_mask_dev.append(torch.where(ident == 0, 255, 0).to(torch.uint8).contiguous())      # resident next to the frames
            # disparity of the left image: fx0 * baseline / depth in float (0 where the ray hits nothing), the map InstFeat::DetectExtraPoints samples
            fxb = torch.tensor(np.float32(np.float32(cam["fx"]) * np.float32(baseline)), dtype=torch.float32, device=depth.device)
            d32 = depth.to(torch.float32)
            self.disp_dev.append(torch.where(torch.isfinite(d32) & (d32 > 0), fxb / d32, torch.zeros_like(d32)).contiguous())
            dets, b3 = [], np.zeros(0, dynsim.BOX3D_DTYPE)
            Rwc, pwc = self.traj.R(t) @ sim.R_IC, self.traj.p(t) + self.traj.R(t) @ sim.T_IC0
            for b in self.boxes:
                ys, xs = np.nonzero(idm == b.id)
                if len(ys) < min_pixels:
                    continue
                x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())      # VIODE::SetViodeMaskAndRoi: rect = (min_pt, max_pt), i.e. max EXCLUSIVE (cv::Rect(pt1, pt2))
                rw, rh = x1 - x0, y1 - y0
                if rw < 24 or rh < 24:
                    continue
                mask = np.ascontiguousarray(np.where(idm[y0:y0 + rh, x0:x0 + rw] == b.id, 255, 0).astype(np.uint8))
                step = int(max(np.sqrt(0.8 * rh * rw / 1000.0), 2.0))                              # DetectExtraPoints: N_max 1000, step >= 2
                ii, jj = np.mgrid[0:rh:step, 0:rw:step]
                sel = mask[ii, jj] > 0
                r, c = ii[sel] + y0, jj[sel] + x0
                z = dep[r, c]
                ok = (z > 0.1) & (z <= 100)
                pts = rays[r[ok], c[ok]] * z[ok, None]
                Rco = Rwc.T @ b.R(t)
                bx = np.zeros(1, dynsim.BOX3D_DTYPE)
                bx["class_id"], bx["score"], bx["center"], bx["dims"] = b.class_id, 0.9, Rwc.T @ (b.p(t) - pwc), b.dims
                bx["yaw"] = np.arctan2(-Rco[2, 0], Rco[0, 0])
                bx["rect_min"], bx["rect_max"] = [x0, y0], [x1, y1]
                b3 = np.concatenate([b3, bx])
                dets.append(dict(track_id=b.id, class_id=b.class_id, rect=(x0, y0, rw, rh), mask=mask, points=np.ascontiguousarray(pts)))
            self.dets.append(dets); self.boxes3d.append(b3)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.imu_t, self.imu_a, self.imu_g = sim.imu_stream(self.traj, self.t0 - 0.05, self.times[-1] + 0.1, 200.0, seed=0xBEEF, **self.noise)


    def disp_host(self, k):
        """the frame's disparity map as a host float32 array (for the CPU oracle)"""
        return self.disp_dev[k].cpu().numpy()


class DynamicPipeline(Pipeline):
    """Pipeline in dynamic mode (cfg::slam == kDynamic): TrackSemanticImage for the background + InstsFeatManager::InstsTrack for the objects on the tracking
    stream, Estimator::ProcessImage with the object branch (window solve on the BA stream, object solve on a third one).  `segments` (a sim.SegmentSim):
    use_line — the detector's matched segments of every frame go through FrameLines::UndistortedLineEndPoints (dv_undistort_lines) into frame.features.lines,
    as TrackSemanticImage's line thread delivers them (background_tracker.cpp:774-780, 809-817)."""

    def __init__(self, seq: DynamicSequence, max_cnt=250, min_dist=25, max_iters=10, device=0, use_imu=1, max_dynamic_cnt=50, min_dynamic_dist=5, use_det3d=1,
                 static_inst_threshold=1.0, mask_morphology_size=0, segments=None, est_kw=None, extra_from_disparity=True, ba_stride=1,
                 static_as_background=False, live_masks=False, mask_stack=False, solo_head=None, mot=None, solo_input=None, stereo_sgm=None):
        from .frontend import DV_MODE_SEMANTIC
        # live_masks: `seq` carries label images (a viode.ViodeSequence: seg0, seg1, dyn_keys) and thread T1's stage runs per frame on the device (viode_frame_enqueue /
        # _collect + the key-image entries) instead of reading the sequence's pre-computed masks, detections and key images; same results, bit for bit
        self.live_masks, self._live_enq = bool(live_masks), None
        # mask_stack: the detector branch of the same stage — per frame an N x H x W instance-mask stack on the device (stack_input(): seq.mask_stacks, or one plane per
        # dynamic key cut from a label-image sequence) through inst_stack_frame_enqueue / _collect and the plane entries; bit for bit the pre-computed path's results
        self.mask_stack, self._stack_in = bool(mask_stack), None
        assert not (live_masks and mask_stack)
        # solo_head: the detector's head in front of that stack — a callable k -> (dv_solo_outputs, dv_solo_params, ids) supplies the network's eleven output tensors of
        # frame k (frontend.solo_outputs / solo_params) and ids(labels, scores, stack) -> (track ids, class ids) per plane, the upstream multi-object tracker's answer
        # (-1 drops a plane).  Context.solo_head_enqueue / _collect fill the stack, which goes down the mask-stack path unchanged; the head of frame k + 1 is enqueued
        # behind the tracking of frame k.  Refused together with live_masks (and with mask_stack: the head IS the source of the stack).  With solo_input (below) the
        # callable is called as (k, input) -> the same triple
        if solo_head is not None and (live_masks or mask_stack):
            raise ValueError("DynamicPipeline: solo_head cannot be combined with live_masks or mask_stack")
        if solo_head is not None and not callable(solo_head):
            raise ValueError("DynamicPipeline: solo_head must be a callable k -> (outputs, params, ids), or (k, input) -> the same with solo_input")
        self.solo_head, self._solo_enq, self._solo_ids, self._solo_blank = solo_head, None, None, None
        # solo_input: the detector's input in front of the caller's network — (model_w, model_h[, mean, std]), the keywords of Context.solo_input_enqueue.  The callable
        # is then called as solo_head(k, input): input = the [3, model_h, model_w] float32 device tensor built from reid_image(k) by Pipeline::ImageToTensor + ProcessInput's
        # rule (det2d/pipeline.cpp:370-387,204-232), in the library's memory (the two alternating buffers: frame k's stays intact while frame k + 1's is built).  Only
        # together with solo_head
        if solo_input is not None:
            if solo_head is None:
                raise ValueError("DynamicPipeline: solo_input needs solo_head, the callable that takes the input")
            if not (isinstance(solo_input, (tuple, list)) and len(solo_input) in (2, 4)):
                raise ValueError("DynamicPipeline: solo_input must be (model_w, model_h) or (model_w, model_h, mean, std)")
        self.solo_input = None if solo_input is None else tuple(solo_input)
        # mot: the multi-object tracker on the device (DeepSORT::update, mot/deep_sort.cpp:72-139) behind the stack stage — (feats, params): feats(k, dets, stack) ->
        # the caller's ReID network on the frame's crops, an [n, feat_dim] float32 device tensor (or a device pointer) with L2-normalised rows, one per detection the
        # stack stage reports after the class filter, in that order; params = the keywords of frontend.mot_params.  Track ids then come from Context.mot_update_* in place
        # of the sequence's / of ids(), which may return class ids alone; a detection without a Confirmed track (-1) is dropped, as AddInstancesByTracking leaves it out.
        # Only where detections come from a stack: refused with pre-computed masks and with live_masks
        if mot is not None:
            if live_masks or not (mask_stack or solo_head is not None):
                raise ValueError("DynamicPipeline: mot needs mask_stack=True or solo_head; it cannot be combined with pre-computed masks or live_masks")
            if not (isinstance(mot, (tuple, list)) and len(mot) == 2 and (callable(mot[0]) or mot[0] == "device") and isinstance(mot[1], dict)):
                raise ValueError("DynamicPipeline: mot must be (callable (k, dets, stack) -> feats, dict of mot_params keywords)")
            # mot = ("device", params): the embeddings come from the device extractor (Context.reid_*; Extractor::extract, mot/extractor.cpp:31-52) instead of a callable.
            # params then also carries reid_weights (an array or the path of ReIdNetImpl::load_form's flat file) and optionally reid_input = (width, height); the rest are
            # mot_params keywords as before (feat_dim must stay 512).  The extractor reads reid_image(k): the sequence's left colour image where it has one (seq.color0[k],
            # an (h, w, 3) uint8 BGR device tensor), else the left GRAY image replicated to three channels (the rendered sequences of this package carry no colour)
            if mot[0] == "device":
                par = dict(mot[1])
                if "reid_weights" not in par:
                    raise ValueError("DynamicPipeline: mot must be (\"device\", params) with params['reid_weights']")
                self._reid_load = (par.pop("reid_weights"), tuple(par.pop("reid_input", (64, 128))))
                if int(par.get("feat_dim", 512)) != 512:
                    raise ValueError("DynamicPipeline: mot must be (\"device\", params) with feat_dim 512, the extractor's width")
                mot = ("device", par)
        self.mot, self._mot_keep, self._reid_img = mot, None, (None, None)
        # stereo_sgm: the stereo matcher on the device in MyStereoMatcher's place (stereo/stereo.cpp) — a frontend.sgm_params(...) or a dict of its keywords.  Per frame
        # Context.stereo_sgm_enqueue / _collect turn the frame's gray pair into SemanticImage::disp in the library's memory, and that map goes to inst_set_disparity in
        # place of seq.disp_dev[k] — also for a sequence that carries none (a ViodeSequence).  The matcher of frame k + 1 is enqueued where that frame's other T1 stages
        # are, behind the tracking of frame k.  The images are rectified as they are (no undistortion in front of it)
        if stereo_sgm is not None:
            from .frontend import dv_sgm_params, sgm_params, sgm_check
            if isinstance(stereo_sgm, dict):
                stereo_sgm = sgm_params(**stereo_sgm)
            if not isinstance(stereo_sgm, dv_sgm_params):
                raise ValueError("DynamicPipeline: stereo_sgm must be frontend.sgm_params(...) or a dict of its keywords")
            if not extra_from_disparity:
                raise ValueError("DynamicPipeline: stereo_sgm needs extra_from_disparity: its map is the extra points' source")
            sgm_check(seq.w, seq.h, stereo_sgm)
        self.stereo_sgm, self._sgm_enq = stereo_sgm, None
        self.extra_from_disparity = extra_from_disparity      # False: the detections' own `points` are handed through (the caller ran the extra-point pipeline)
        self.seq, self.host = seq, None
        c = make_cam(*sim.cam_tuple(seq.cam))
        self.cam_c, self.cam1_c = c, make_cam(*sim.cam_tuple(seq.cam1))
        self.ctx = Context(width=seq.w, height=seq.h, max_cnt=max_cnt, min_dist=min_dist, cam0=c, cam1=self.cam1_c, device=device, mask_morphology_size=mask_morphology_size)
        self.ctx.inst_config(max_dynamic_cnt, min_dynamic_dist, use_det3d)
        if self.mot is not None:
            self.ctx.mot_config(**self.mot[1])
            if self.mot[0] == "device":
                self.ctx.reid_load(self._reid_load[0], *self._reid_load[1])
        self.est_kw = dict(use_imu=use_imu, stereo=1, max_iters=max_iters, ric=seq.rig["est_ric"], tic=seq.rig["est_tic"], dynamic=1, use_det3d=use_det3d,
                           static_inst_threshold=static_inst_threshold, use_line=int(segments is not None), **seq.noise)
        self.est_kw.update(est_kw or {})
        self.est = Estimator(self.ctx, **self.est_kw)
        self.mode, self.use_det3d, self.segments = DV_MODE_SEMANTIC, use_det3d, segments
        self.k_imu = self.next = 0
        self.enqueued = False
        self._prefetched = None
        self.ba_stride = ba_stride          # 2: every tracked frame goes through both trackers, every 2nd one to the back end (system/main.cpp:300-307: every data set but KITTI)
        self.last_state = None
        self.poses, self.pose_times = [], []
        # para::is_static_inst_as_background (reference default: true): before tracking frame f the pixels of the instances the estimator reported static leave the merged mask
        # (system/main.cpp:194,217-245).  The reference reads that report across threads without an order; here: the snapshot of the newest back-end frame <= f - 2 (runner.hip)
        self.static_as_background, self.static_snaps = static_as_background, []
        self.frame_rows, self.keep_frame_rows = [], False      # (t, [px py pz qx qy qz qw], nonlinear) of every frame handed to the back end when keep_frame_rows is set
        self.stat = dict(frames=0, frames_with_objects=0, object_detections=0, object_features=0, min_detections=10 ** 9)      # what the object branch was fed over the run

    def static_ids_for(self, k):
        from ._abi import DV_STATIC_REPORT_LAG
        best = [s for s in self.static_snaps if s[0] <= k - DV_STATIC_REPORT_LAG]
        return best[-1][1] if best else np.zeros(0, np.uint32)

    def stack_input(self):
        """-> dict(stacks: per frame a uint8 [n, h, w] device tensor, track_ids / class_ids: per frame one int per plane, min_inst_size).  A sequence that carries
        mask_stacks / stack_track_ids / stack_class_ids hands them over; a label-image sequence (seg0, dyn_keys) is turned into one plane per dynamic key, track id = key"""
        if self._stack_in is None:
            import torch
            from . import viode
            s = self.seq
            if hasattr(s, "mask_stacks"):
                self._stack_in = dict(stacks=s.mask_stacks, track_ids=s.stack_track_ids, class_ids=s.stack_class_ids, min_inst_size=getattr(s, "min_inst_size", viode.MIN_INST_SIZE))
            else:
                keys = [int(v) for v in s.dyn_keys]
                dev = s.frames[0][0].device
                stacks = []
                for g in s.seg0:
                    kimg = viode.pixel_to_key(g[..., 2], g[..., 1], g[..., 0])
                    stacks.append(torch.from_numpy(np.stack([kimg == key for key in keys]).astype(np.uint8)).to(dev))
                torch.cuda.synchronize()
                self._stack_in = dict(stacks=stacks, track_ids=[np.array(keys, np.int32)] * len(stacks), class_ids=[np.zeros(len(keys), np.int32)] * len(stacks), min_inst_size=viode.MIN_INST_SIZE)
        return self._stack_in

    def _mot_ids(self, k, dets, stack):
        """dets (class filter applied) -> the same with track_id from the device tracker, those without a Confirmed track dropped.  A frame without detections does not
        reach the tracker (front_end/dynamic_tracker.cpp:795-796)"""
        from .frontend import DV_MEM_DEVICE as DEV
        if not len(dets):
            return dets
        rects = np.array([d["rect"] for d in dets], np.float32)
        if self.mot[0] == "device":          # image and embeddings stay on the device: the collect's pointer goes straight into the tracker
            import torch
            img = self.reid_image(k)
            torch.cuda.current_stream().synchronize()
            self.ctx.reid_extract_enqueue(img.data_ptr(), rects, n=len(dets), mem=DEV, stride=img.stride(0))
            feats, _ = self.ctx.reid_extract_collect()
            ids, _, _ = self.ctx.mot_update(rects, feats, n=len(dets), mem=DEV)
            return [dict(d, track_id=int(i)) for d, i in zip(dets, ids) if i >= 0]
        feats = self.mot[0](k, dets, stack)
        if hasattr(feats, "data_ptr"):
            import torch
            if feats.dtype != torch.float32 or tuple(feats.shape) != (len(dets), int(self.mot[1].get("feat_dim", 512))) or not feats.is_contiguous():
                raise ValueError("DynamicPipeline: mot feats must be a contiguous float32 [n, feat_dim] tensor")
            torch.cuda.current_stream().synchronize()      # the caller's network ran on the tensor library's stream
            self._mot_keep, feats = feats, feats.data_ptr()
        ids, _, _ = self.ctx.mot_update(rects, int(feats), n=len(dets), mem=DEV)
        return [dict(d, track_id=int(i)) for d, i in zip(dets, ids) if i >= 0]

    def reid_image(self, k):
        """the image the device extractor crops for frame k, an (h, w, 3) uint8 BGR device tensor: seq.color0[k] where the sequence has colour, else the left gray image
        replicated to three channels"""
        if self._reid_img[0] != k:
            c = getattr(self.seq, "color0", None)
            img = c[k] if c is not None else self.seq.frames[k][0].unsqueeze(-1).expand(-1, -1, 3).contiguous()
            self._reid_img = (k, img)
        return self._reid_img[1]

    def _sgm_enqueue(self, k):
        l, r = self.seq.frames[k]
        self.ctx.stereo_sgm_enqueue(l.data_ptr(), r.data_ptr(), self.stereo_sgm, mem=DV_MEM_DEVICE, stride=l.stride(0))
        self._sgm_enq = k

    def _set_disparity(self, k):
        """SemanticImage::disp of frame k for the object tracker: the matcher's map (stereo_sgm), else the sequence's own where it has one"""
        if not self.extra_from_disparity:
            return
        if self.stereo_sgm is not None:
            if self._sgm_enq != k:
                self._sgm_enqueue(k)
            self._sgm_enq = None
            ptr, stride = self.ctx.stereo_sgm_collect()
            self.ctx.inst_set_disparity(ptr, self.seq.baseline, DV_MEM_DEVICE, stride)
        elif len(getattr(self.seq, "disp_dev", [])):
            self.ctx.inst_set_disparity(self.seq.disp_dev[k].data_ptr(), self.seq.baseline, DV_MEM_DEVICE)

    def _sgm_next(self, k):
        """the matcher of frame k + 1 behind the tracking of frame k, beside that frame's other T1 stages"""
        if self.stereo_sgm is not None and k + 1 < len(self.seq.frames):
            self._sgm_enqueue(k + 1)

    def _enqueue_stack(self, k):
        from .frontend import DV_MEM_DEVICE as DEV
        s, ctx, q = self.seq, self.ctx, self.stack_input()
        l, r = s.frames[k]
        kw = lambda j: dict(mem=DEV, n_planes=q["stacks"][j].shape[0])
        if self._live_enq != k:
            ctx.inst_stack_frame_enqueue(q["stacks"][k].data_ptr(), **kw(k))
        self._live_enq = None
        dets, inv, _ = ctx.inst_stack_frame_collect(q["min_inst_size"])
        dets = [dict(d, track_id=int(q["track_ids"][k][d["plane"]]), class_id=int(q["class_ids"][k][d["plane"]])) for d in dets]
        if self.mot is not None:          # the class filter first (image_process.cpp:217-232), then the device tracker's ids
            dets = self._mot_ids(k, [d for d in dets if d["class_id"] >= 0], q["stacks"][k])
        dets = [d for d in dets if d["track_id"] >= 0 and d["class_id"] >= 0]          # the upstream tracker's answer; -1 drops the plane
        if self.static_as_background and len(dets):
            ctx.track_unmask_static_planes(dets, self.static_ids_for(k), q["stacks"][k].data_ptr(), **kw(k))
        ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), s.times[k], inv, self.mode, DEV)
        self._set_disparity(k)
        ctx.inst_track_enqueue_planes(s.times[k], dets, q["stacks"][k].data_ptr(), **kw(k))
        self.enqueued = True
        if k + 1 < len(s.frames):          # T1's stage of the next frame behind this frame's tracking
            ctx.inst_stack_frame_enqueue(q["stacks"][k + 1].data_ptr(), **kw(k + 1))
            self._live_enq = k + 1
        self._sgm_next(k)

    def _solo_enqueue_head(self, k):
        if self.solo_input is not None:          # the network's input of frame k from the resident colour frame, then the caller's network on it
            import torch
            from .frontend import DV_MEM_DEVICE as DEV
            img = self.reid_image(k)
            torch.cuda.current_stream().synchronize()
            inp, _ = self.ctx.solo_input(img.data_ptr(), *self.solo_input, mem=DEV, stride=img.stride(0))
            o, p, ids = self.solo_head(k, inp)
        else:
            o, p, ids = self.solo_head(k)
        self.ctx.solo_head_enqueue(o, p)
        self._solo_enq, self._solo_ids = k, ids

    def _enqueue_solo(self, k):
        """the mask-stack path on the head's own stack (Detector2D::ForwardTensor behind the network, det2d/detector2d.cpp:273-278, then ImageProcessor::Run's detector branch)"""
        from .frontend import DV_MEM_DEVICE as DEV
        from . import viode
        s, ctx = self.seq, self.ctx
        l, r = s.frames[k]
        if self._solo_enq != k:
            self._solo_enqueue_head(k)
        ids, self._solo_enq = self._solo_ids, None
        labels, scores, st, _ = ctx.solo_head_collect()
        dets = []
        if st.n_planes:
            ctx.inst_stack_frame_enqueue(st)
            dets, inv, _ = ctx.inst_stack_frame_collect(getattr(s, "min_inst_size", viode.MIN_INST_SIZE))
            if self.mot is not None:          # ids() may return the class ids alone
                res = ids(labels, scores, st)
                cid = res[1] if isinstance(res, tuple) else res
                dets = self._mot_ids(k, [d for d in (dict(d, class_id=int(cid[d["plane"]])) for d in dets) if d["class_id"] >= 0], st)
            else:
                tid, cid = ids(labels, scores, st)
                dets = [dict(d, track_id=int(tid[d["plane"]]), class_id=int(cid[d["plane"]])) for d in dets]
            dets = [d for d in dets if d["track_id"] >= 0 and d["class_id"] >= 0]
            if self.static_as_background and len(dets):
                ctx.track_unmask_static_planes(dets, self.static_ids_for(k), st)
        else:          # a frame without instances: nothing is masked, no object is tracked
            if self._solo_blank is None:
                import torch
                self._solo_blank = torch.full((s.h, s.w), 255, dtype=torch.uint8, device=l.device)
                torch.cuda.synchronize()
            inv = self._solo_blank.data_ptr()
        ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), s.times[k], inv, self.mode, DEV)
        self._set_disparity(k)
        if st.n_planes:
            ctx.inst_track_enqueue_planes(s.times[k], dets, st)
        else:
            ctx.inst_track_enqueue(s.times[k], [], None)
        self.enqueued = True
        if k + 1 < len(s.frames):          # the head of the next frame behind this frame's tracking: its planes go to the other of the two sets
            self._solo_enqueue_head(k + 1)
        self._sgm_next(k)

    def _enqueue_live(self, k):
        from . import viode
        s, ctx = self.seq, self.ctx
        l, r = s.frames[k]
        if self._live_enq != k:
            ctx.viode_frame_enqueue(s.seg0[k], s.seg1[k], s.dyn_keys)
        self._live_enq = None
        dets, inv, k0, k1 = ctx.viode_frame_collect(viode.MIN_INST_SIZE)
        if self.static_as_background and len(dets):
            ctx.track_unmask_static_keys(dets, self.static_ids_for(k), k0, DV_MEM_DEVICE)
        ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), s.times[k], inv, self.mode, DV_MEM_DEVICE)
        self._set_disparity(k)
        if k1:
            ctx.inst_set_right_keys(k1, DV_MEM_DEVICE)
        ctx.inst_track_enqueue_keys(s.times[k], dets, k0, DV_MEM_DEVICE)
        self.enqueued = True
        if k + 1 < len(s.frames):          # T1's stage of the next frame behind this frame's tracking: its boxes are there when the host turns to it
            ctx.viode_frame_enqueue(s.seg0[k + 1], s.seg1[k + 1], s.dyn_keys)
            self._live_enq = k + 1
        self._sgm_next(k)

    def _enqueue(self, k):
        if self.mask_stack:
            return self._enqueue_stack(k)
        if self.solo_head is not None:
            return self._enqueue_solo(k)
        if self.live_masks:
            return self._enqueue_live(k)
        l, r = self.seq.frames[k]
        if self.static_as_background and len(self.seq.dets[k]):
            self.ctx.track_unmask_static(self.seq.dets[k], self.static_ids_for(k))
        self.ctx.track_stereo_enqueue(l.data_ptr(), r.data_ptr(), self.seq.times[k], self.seq.inv_mask_dev[k].data_ptr(), self.mode, DV_MEM_DEVICE)
        if self.stereo_sgm is not None:
            self._set_disparity(k)
        elif self.extra_from_disparity:      # the extra points of the objects: DetectExtraPoints + ProcessExtraPoints on the device from the frame's disparity map
            self.ctx.inst_set_disparity(self.seq.disp_dev[k].data_ptr(), self.seq.baseline, DV_MEM_DEVICE)
        if getattr(self.seq, "right_keys", None) is not None:      # VIODE: seg1's key image -> TrackRightByPad's segmentation-key test
            self.ctx.inst_set_right_keys(self.seq.right_keys[k])
        self.ctx.inst_track_enqueue(self.seq.times[k], self.seq.dets[k], self.seq.boxes3d[k] if self.use_det3d else None)
        self.enqueued = True
        self._sgm_next(k)

    def _collect(self):
        return (self.ctx.track_stereo_collect(),) + tuple(self.ctx.inst_track_collect())

    def line_rows(self, t):
        """frame.features.lines of the frame at time t: the detector's pixel segments through UndistortedLineEndPoints (cam0 / cam1)"""
        il, sl, ir, sr = self.segments.frame(t)
        self.seg_px = (il, sl, ir, sr)
        return sim.line_rows(il, self.ctx.undistort_lines(self.cam_c, sl), ir, self.ctx.undistort_lines(self.cam1_c, sr))

    def step(self, defer_end=False):
        k, s = self.next, self.seq
        pre, self._prefetched = self._prefetched, None
        if pre is None:
            if not self.enqueued:
                self._enqueue(k)
            pre = self._collect()
        rows, insts, ifeats, pts = pre
        self.enqueued = False
        t = s.times[k]
        if self.ba_stride > 1 and (k % self.ba_stride) != 0:      # tracked only (both trackers keep their state up to date; system/main.cpp:300-312)
            if k + 1 < len(s.frames):
                self._enqueue(k + 1)
                self._prefetched = self._collect()
            self.next += 1
            self.rows, self.insts, self.ifeats, self.ipts = rows, insts, ifeats, pts
            return self.last_state if self.last_state is not None else self.est.state
        self._feed_imu(t)
        if self.segments is not None:
            self.lrows = self.line_rows(t)
            self.est.SetLines(self.lrows)
        # Three-phase back end (dv_est_process_dynamic_begin_ego / _attach): the window solve of frame k goes to the GPU first, with the background rows alone (~0.17 ms
        # of host work in front of it); then the tracking of frame k+1 (background + objects: ~60 launches, 0.25 ms of host time) is enqueued — thread T2 of the
        # reference, independent of T3 —; then the object branch of ProcessImage (~0.4 ms of host work + the object solve on the third stream).  All of it runs
        # beside the window solve (the chain of ~30 dependent launches that IS the frame) instead of in front of it.
        if self.est.ProcessMeasurementsDynamicBeginEgo(rows, t) != 0:
            raise RuntimeError("IMU stream does not cover the frame")
        if k + 1 < len(s.frames):
            self._enqueue(k + 1)
        self.est.AttachInstances(insts, ifeats, pts)
        if self.static_as_background:
            self.static_snaps = (self.static_snaps + [(k, self.est.static_instances())])[-4:]
        if k + 1 < len(s.frames):
            self._feed_imu(s.times[k + 1])
            if not defer_end:
                self._prefetched = self._collect()      # while the BA of frame k runs (see Pipeline.step)
        self.rows, self.insts, self.ifeats, self.ipts = rows, insts, ifeats, pts
        self.stat["frames"] += 1; self.stat["frames_with_objects"] += int(len(insts) > 0); self.stat["object_detections"] += len(insts); self.stat["object_features"] += len(ifeats)
        self.stat["min_detections"] = min(self.stat["min_detections"], len(insts))
        if defer_end:
            self._pending_t = t
            return None
        return self._finish(t)
