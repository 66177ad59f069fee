"""Python mirror of the reference's front-end interface, on top of the C ABI (for tests and bench.py;
the C++ drop-in shim with the reference's class signatures is dynamic_vins_amd/host/feature_tracker.h).

Names follow dynamic_vins/src/front_end/background_tracker.h:41-88 and feature_utils.h.
"""
import ctypes as C
import numpy as np

from . import _abi
from ._abi import DvinsError, dv_cam, dv_config, dv_feat, DV_MEM_HOST, DV_MEM_DEVICE, DV_MEM_PINNED, DV_FMT_BGR, DV_MODE_RAW, DV_MODE_NAIVE, DV_MODE_SEMANTIC

class dv_inst_det(C.Structure):
    _fields_ = [("track_id", C.c_uint32), ("class_id", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("mask", C.c_void_p), ("points", C.c_void_p), ("n_points", C.c_int32), ("pad_", C.c_int32)]


class dv_mask_stack(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n_planes", C.c_int32), ("kind", C.c_int32), ("mem", C.c_int32), ("row_stride", C.c_int32), ("plane_stride", C.c_int64),
                ("threshold", C.c_float), ("reserved", C.c_int32)]


DV_STACK_U8, DV_STACK_F32, DV_STACK_REMAP_MERGED = 0, 1, 1


def mask_stack(stack, mem=DV_MEM_HOST, n_planes=0, kind=DV_STACK_U8, row_stride=0, plane_stride=0, threshold=0.0):
    """dv_mask_stack of a detector's instance masks: a [n, h, w] numpy array (uint8 / bool -> DV_STACK_U8, float32 -> DV_STACK_F32; any strides with unit element stride;
    host memory, kept alive by the caller) or a raw device / pinned pointer (int) with mem, n_planes, kind and the strides in bytes (0 = tight)"""
    if isinstance(stack, dv_mask_stack):
        return stack
    if isinstance(stack, np.ndarray):
        assert stack.ndim == 3 and stack.dtype in (np.uint8, np.bool_, np.float32) and stack.strides[2] == stack.itemsize
        kind = DV_STACK_F32 if stack.dtype == np.float32 else DV_STACK_U8
        return dv_mask_stack(stack.ctypes.data, stack.shape[0], kind, DV_MEM_HOST, stack.strides[1], stack.strides[0], float(threshold), 0)
    return dv_mask_stack(int(stack), int(n_planes), int(kind), int(mem), int(row_stride), int(plane_stride), float(threshold), 0)


class dv_solo_outputs(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("channels", C.c_int32), ("n_classes", C.c_int32), ("mem", C.c_int32), ("kernel", C.c_void_p * 5), ("cate", C.c_void_p * 5),
                ("grid", C.c_int32 * 5), ("fh", C.c_int32), ("fw", C.c_int32), ("reserved", C.c_int32), ("feature", C.c_void_p)]


class dv_solo_params(C.Structure):
    _fields_ = [("score_thr", C.c_float), ("mask_thr", C.c_float), ("update_thr", C.c_float), ("nms_sigma", C.c_float), ("nms_pre", C.c_int32), ("max_per_img", C.c_int32),
                ("nms_kernel", C.c_int32), ("max_candidates", C.c_int32), ("num_grids", C.c_int32 * 5), ("strides", C.c_float * 5),
                ("rect_x", C.c_int32), ("rect_y", C.c_int32), ("rect_w", C.c_int32), ("rect_h", C.c_int32), ("origin_w", C.c_int32), ("origin_h", C.c_int32)]


DV_SOLO_NMS_GAUSSIAN, DV_SOLO_NMS_LINEAR = 0, 1


def solo_rect(model_w, model_h, img_w, img_h):
    """Pipeline::GetXYWHS (det2d/pipeline.cpp:23-48): the image's rectangle (x, y, w, h) inside the network input.  Host code: needs no GPU."""
    lib = _abi.load()
    v = [C.c_int(0) for _ in range(4)]
    if lib.dv_solo_rect(int(model_w), int(model_h), int(img_w), int(img_h), *[C.byref(a) for a in v]) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())
    return tuple(a.value for a in v)


def solo_outputs(kernels, cates, feature, mem=DV_MEM_HOST, shapes=None):
    """dv_solo_outputs of a SOLOv2 network's outputs.  Host: float32 C-contiguous numpy arrays, kernels[l] [channels, g, g], cates[l] [n_classes, g, g], feature
    [channels, fh, fw] (kept alive by the caller).  Device / pinned: raw pointers (int) with shapes = (channels, n_classes, [g per level], fh, fw)."""
    o = dv_solo_outputs()
    if shapes is None:
        for a in list(kernels) + list(cates) + [feature]:
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.ndim == 3
        shapes = (feature.shape[0], cates[0].shape[0], [k.shape[1] for k in kernels], feature.shape[1], feature.shape[2])
        ptr = lambda a: a.ctypes.data
    else:
        ptr = int
    channels, n_classes, grids, fh, fw = shapes
    o.n_levels, o.channels, o.n_classes, o.mem, o.fh, o.fw = len(kernels), int(channels), int(n_classes), int(mem), int(fh), int(fw)
    for l in range(min(len(kernels), 5)):
        o.kernel[l], o.cate[l], o.grid[l] = ptr(kernels[l]), ptr(cates[l]), int(grids[l])
    o.feature = ptr(feature)
    return o


def solo_params(score_thr=0.1, mask_thr=0.5, update_thr=0.05, nms_pre=500, max_per_img=100, nms_kernel="gaussian", nms_sigma=2.0, num_grids=(40, 36, 24, 16, 12),
                strides=(8, 8, 16, 32, 32), max_candidates=2048, rect=(0, 0, 0, 0), origin=(0, 0)):
    """dv_solo_params; the defaults are the reference's tables (det2d/det2d_parameter.h:30-31) and its KITTI YAML"""
    p = dv_solo_params()
    p.score_thr, p.mask_thr, p.update_thr, p.nms_sigma = float(score_thr), float(mask_thr), float(update_thr), float(nms_sigma)
    p.nms_pre, p.max_per_img, p.max_candidates = int(nms_pre), int(max_per_img), int(max_candidates)
    p.nms_kernel = {"gaussian": DV_SOLO_NMS_GAUSSIAN, "linear": DV_SOLO_NMS_LINEAR}.get(nms_kernel, nms_kernel)
    for l in range(min(len(num_grids), 5)):
        p.num_grids[l], p.strides[l] = int(num_grids[l]), float(strides[l])
    (p.rect_x, p.rect_y, p.rect_w, p.rect_h), (p.origin_w, p.origin_h) = [int(v) for v in rect], [int(v) for v in origin]
    return p


class dv_solo_input_params(C.Structure):
    _fields_ = [("model_w", C.c_int32), ("model_h", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3)]


SOLO_IMG_MEAN, SOLO_IMG_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)      # kSoloImgMean / kSoloImgStd, RGB order (det2d/det2d_parameter.h:24-25)


def solo_input_params(model_w, model_h, mean=SOLO_IMG_MEAN, std=SOLO_IMG_STD):
    """dv_solo_input_params: the network's input size and the normalisation in RGB order; the defaults are the reference's (det2d/det2d_parameter.h:24-25)"""
    p = dv_solo_input_params()
    p.model_w, p.model_h = int(model_w), int(model_h)
    for c in range(3):
        p.mean[c], p.std[c] = float(mean[c]), float(std[c])
    return p


def solo_input_check(img_w, img_h, model_w, model_h, mean=SOLO_IMG_MEAN, std=SOLO_IMG_STD, stride=None):
    """the refusals of Context.solo_input_enqueue for an img_w x img_h frame (stride: bytes per row, default 3 * img_w), without a device: raises DvinsError with the reason"""
    lib = _abi.load()
    p = solo_input_params(model_w, model_h, mean, std)
    if lib.dv_solo_input_check(int(img_w), int(img_h), int(3 * img_w if stride is None else stride), C.addressof(p)) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())


class dv_sgm_params(C.Structure):
    _fields_ = [("n_disp", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("uniqueness", C.c_int32), ("lr_max_diff", C.c_int32), ("reserved", C.c_int32 * 3)]


DV_SGM_DEBUG_CENSUS_L, DV_SGM_DEBUG_CENSUS_R, DV_SGM_DEBUG_S, DV_SGM_DEBUG_DSTAR, DV_SGM_DEBUG_DR = 0, 1, 2, 3, 4


def sgm_params(n_disp=128, p1=10, p2=120, uniqueness=5, lr_max_diff=1, reserved=(0, 0, 0)):
    """dv_sgm_params of the stereo matcher (MyStereoMatcher's place, stereo/stereo.cpp): n_disp 64 / 128 / 256, the two path penalties, OpenCV's uniqueness margin in
    per cent, the left-right tolerance (< 0: no test)"""
    p = dv_sgm_params()
    p.n_disp, p.p1, p.p2, p.uniqueness, p.lr_max_diff = int(n_disp), int(p1), int(p2), int(uniqueness), int(lr_max_diff)
    for i in range(3):
        p.reserved[i] = int(reserved[i])
    return p


def sgm_check(w, h, params=None, stride=None, **kw):
    """the refusals of Context.stereo_sgm_enqueue for a w x h pair (stride: bytes per row, default w), without a device: raises DvinsError with the reason"""
    lib = _abi.load()
    p = params if params is not None else sgm_params(**kw)
    if lib.dv_stereo_sgm_check(int(w), int(h), int(w if stride is None else stride), C.addressof(p)) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())


class _DeviceArray:
    """a device pointer and a shape behind __cuda_array_interface__: what torch.as_tensor wraps without a copy"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(int(v) for v in shape), typestr=typestr, data=(int(ptr), False), strides=None, version=2)


def device_tensor(ptr, shape, typestr="<f4", device=0):
    """a contiguous torch tensor on `device` over the library's (or the caller's) device memory at ptr: no copy, no ownership — valid as long as the memory is"""
    import torch
    return torch.as_tensor(_DeviceArray(ptr, shape, typestr), device="cuda:%d" % device)


class dv_mot_params(C.Structure):
    _fields_ = [("n_init", C.c_int32), ("max_age", C.c_int32), ("budget", C.c_int32), ("feat_dim", C.c_int32), ("max_tracks", C.c_int32), ("reserved", C.c_int32 * 3)]


# dv_mot_track: a row of Context.mot_tracks()
MOT_TRACK_DTYPE = np.dtype([("x", np.float32, 7), ("p_diag", np.float32, 7), ("rect", np.float32, 4), ("state", np.int32), ("id", np.int32), ("hits", np.int32),
                            ("time_since_update", np.int32), ("n_feats", np.int32), ("reserved", np.int32)])
assert MOT_TRACK_DTYPE.itemsize == 96
DV_MOT_MAX_TRACKS, DV_MOT_MAX_DETS = 128, 64


def mot_params(n_init=3, max_age=5, budget=100, feat_dim=512, max_tracks=128):
    """dv_mot_params; the defaults are the reference's tracking YAML (mot/mot_parameter.cpp)"""
    p = dv_mot_params()
    p.n_init, p.max_age, p.budget, p.feat_dim, p.max_tracks = int(n_init), int(max_age), int(budget), int(feat_dim), int(max_tracks)
    return p


def mot_check(params):
    """the refusals of mot_config, without a device: raises DvinsError with the reason"""
    lib = _abi.load()
    if lib.dv_mot_check(C.addressof(params) if params is not None else None) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())


DV_REID_N_FLOATS, DV_REID_FEAT_DIM, DV_REID_MAX_CROPS = 11178496, 512, 64

# dv_key_line: what LineDetector::Detect leaves of a cv::line_descriptor::KeyLine (line_detector/line_detector.cpp:82-96)
KEYLINE_DTYPE = np.dtype([("sx", np.float32), ("sy", np.float32), ("ex", np.float32), ("ey", np.float32), ("angle", np.float32), ("length", np.float32)])
assert KEYLINE_DTYPE.itemsize == 24
DV_LINE_MAX, DV_LINE_DESC_BYTES = 512, 32


def _key_lines(lines, desc):
    """host key lines ([n, 6] float32 or KEYLINE_DTYPE records) and descriptors ([n, 32] uint8), contiguous -> (lines, desc, n)"""
    lines = np.asarray(lines)
    lines = np.ascontiguousarray(lines.view(np.float32) if lines.dtype == KEYLINE_DTYPE else lines, np.float32).reshape(-1, 6)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, DV_LINE_DESC_BYTES)
    if len(lines) != len(desc):
        raise ValueError("one descriptor row per key line")
    return lines, desc, len(lines)


def line_track_check(left_lines, left_desc, n_left, right_lines=None, right_desc=None, n_right=0, mem=DV_MEM_HOST):
    """the refusals of Context.line_track_enqueue, without a device (pointers as int or host arrays): raises DvinsError with the reason"""
    lib = _abi.load()
    if lib.dv_line_track_check(_ptr(left_lines), _ptr(left_desc), int(n_left), _ptr(right_lines), _ptr(right_desc), int(n_right), int(mem)) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())


def _host_lines(lines, num_pixels=None):
    """host key lines ([n, 6] float32 or KEYLINE_DTYPE records) and optional num_pixels ([n] int32), contiguous -> (lines, num_pixels, n)"""
    lines = np.asarray(lines)
    lines = np.ascontiguousarray(lines.view(np.float32) if lines.dtype == KEYLINE_DTYPE else lines, np.float32).reshape(-1, 6)
    if num_pixels is not None:
        num_pixels = np.ascontiguousarray(num_pixels, np.int32).reshape(-1)
        if len(num_pixels) != len(lines):
            raise ValueError("one num_pixels per key line")
    return lines, num_pixels, len(lines)


def lbd_check(w, h, stride, lines, num_pixels=None, n=None, mem=DV_MEM_HOST, mask=None, mask_stride=0):
    """the refusals of Context.lbd_describe_enqueue, without a device (host arrays, or pointers as int with n): raises DvinsError with the reason"""
    lib = _abi.load()
    if n is None:
        lines, num_pixels, n = _host_lines(lines, num_pixels)
    if isinstance(mask, np.ndarray) and not mask_stride:
        mask_stride = mask.strides[0]
    if lib.dv_lbd_check(int(w), int(h), int(stride), _ptr(lines), _ptr(num_pixels), int(n), int(mem), _ptr(mask), int(mask_stride)) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())


def lbd_num_pixels(lines):
    """KeyLine::numOfPixels by the library's rule, max(|rint(ex) - rint(sx)|, |rint(ey) - rint(sy)|) + 1, for host key lines -> [n] int32.  Host code: needs no GPU."""
    lib = _abi.load()
    lines, _, n = _host_lines(lines)
    out = np.zeros(max(n, 1), np.int32)
    if lib.dv_lbd_num_pixels(lines.ctypes.data if n else None, n, out.ctypes.data) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())
    return out[:n].copy()


def reid_check(n_floats, in_w=64, in_h=128):
    """the refusals of Context.reid_load, without a device: raises DvinsError with the reason"""
    lib = _abi.load()
    if lib.dv_reid_check(int(n_floats), int(in_w), int(in_h)) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())


def solo_check(outputs, params):
    """the refusals of solo_head_enqueue, without a device: raises DvinsError with the reason"""
    lib = _abi.load()
    if lib.dv_solo_check(C.addressof(outputs), C.addressof(params)) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())


FEAT_DTYPE = np.dtype([("id", np.uint32), ("track_cnt", np.int32), ("has_right", np.int32), ("pad_", np.int32),
                       ("left", np.float64, 7), ("right", np.float64, 7)])
assert FEAT_DTYPE.itemsize == C.sizeof(dv_feat) == 128


def make_cam(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
    return dv_cam(fx, fy, cx, cy, k1, k2, p1, p2)


def _ptr(a):
    """pointer of a host ndarray, or pass through a raw device pointer (int)."""
    if a is None:
        return None
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a))
    return C.c_void_p(a.ctypes.data)


def optimal_new_camera(cam, w, h, alpha=0.0):
    """cv::getOptimalNewCameraMatrix(K, D, (w, h), alpha, (w, h)) for a pinhole + radtan dv_cam (or its 8-tuple) -> (fx, fy, cx, cy).  Host code: needs no GPU."""
    lib = _abi.load()
    c = cam if isinstance(cam, dv_cam) else make_cam(*cam)
    nk = (C.c_double * 4)()
    if lib.dv_optimal_new_camera(C.byref(c), int(w), int(h), float(alpha), nk) != 0:
        raise DvinsError(lib.dv_last_error(None).decode())
    return tuple(nk)


def cam_tuple(c):
    return (c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2)


class Context:
    """Owns a dv_ctx (device memory + stream).  One per thread, like the reference's FeatureTracker."""

    def __init__(self, width, height, max_cnt=150, min_dist=30, flow_back=1, stereo=1, cam0=None, cam1=None, device=0, mask_morphology_size=0):
        self.lib = _abi.load()
        cfg = dv_config()
        cfg.width, cfg.height, cfg.max_cnt, cfg.min_dist = width, height, max_cnt, min_dist
        cfg.flow_back, cfg.stereo, cfg.device = flow_back, stereo, device
        cfg.mask_morphology_size = mask_morphology_size
        cfg.cam0 = cam0 if cam0 is not None else make_cam(1, 1, 0, 0)
        cfg.cam1 = cam1 if cam1 is not None else cfg.cam0
        self.cfg = cfg
        self.h = self.lib.dv_create(C.byref(cfg))
        if not self.h:
            raise DvinsError(self.lib.dv_last_error(None).decode())
        self._out = np.zeros(_abi.DV_MAX_FEATS, FEAT_DTYPE)
        self._mot_par, self._mot_n, self._mot_keep, self._mot_pin = None, 0, None, None
        self._reid_size, self._reid_n, self._reid_keep, self._reid_pin = None, 0, None, None
        self._solo_in_keep, self._solo_in_shape = None, None

    def close(self):
        if getattr(self, "h", None):
            self.lib.dv_destroy(self.h)
            self.h = None
            if getattr(self, "_mot_pin", None):
                self.lib.dv_pinned_free(self._mot_pin)
                self._mot_pin = None
            if getattr(self, "_reid_pin", None):
                self.lib.dv_pinned_free(self._reid_pin)
                self._reid_pin = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise DvinsError(self.lib.dv_last_error(self.h).decode())

    # ---- whole-frame entries ----
    def track_stereo(self, gray0, gray1, t, mask=None, mode=DV_MODE_RAW, mem=DV_MEM_HOST, w=None, h=None, stride=None):
        w = w or self.cfg.width
        h = h or self.cfg.height
        stride = stride or w
        n = C.c_int(0)
        self._check(self.lib.dv_track_stereo(self.h, _ptr(gray0), _ptr(gray1), w, h, stride, float(t), _ptr(mask), mode, mem,
                                             self._out.ctypes.data_as(C.POINTER(dv_feat)), C.byref(n)))
        return self._out[: n.value].copy()

    def track_stereo_enqueue(self, gray0, gray1, t, mask=None, mode=DV_MODE_RAW, mem=DV_MEM_HOST, stride=None):
        w, h = self.cfg.width, self.cfg.height
        self._check(self.lib.dv_track_stereo_enqueue(self.h, _ptr(gray0), _ptr(gray1), w, h, stride or w, float(t), _ptr(mask), mode, mem))

    # ---- dynamic mode: the per-object tracker (InstsFeatManager) ----
    def inst_config(self, max_dynamic_cnt=50, min_dynamic_dist=5, use_det3d=0):
        self._check(self.lib.dv_inst_config(self.h, int(max_dynamic_cnt), int(min_dynamic_dist), int(use_det3d)))
        from .dynsim import INSTOBS_DTYPE
        self._inst_out = (np.zeros(64, INSTOBS_DTYPE), np.zeros(64 * 256, FEAT_DTYPE), np.zeros((1 << 16, 3), np.float64))

    def inst_reset(self):
        """drops every object (dv_inst_reset); the background tracker and the shared id counter go on"""
        self._check(self.lib.dv_inst_reset(self.h))

    def inst_track_enqueue(self, t, dets, boxes3d=None):
        """dets: list of dict(track_id, class_id, rect=(x, y, w, h), mask=uint8[h, w], points=float64[n, 3] or None); boxes3d: BOX3D_DTYPE array or None.
        Call right after track_stereo_enqueue of the same frame."""
        from .dynsim import BOX3D_DTYPE
        arr = (dv_inst_det * max(len(dets), 1))()
        self._inst_keep = []
        for k, d in enumerate(dets):
            m = np.ascontiguousarray(d["mask"], np.uint8)
            x, y, w, h = [int(v) for v in d["rect"]]
            assert m.shape == (h, w)
            pts = None if d.get("points") is None else np.ascontiguousarray(d["points"], np.float64)
            self._inst_keep += [m, pts]
            arr[k].track_id, arr[k].class_id, arr[k].x, arr[k].y, arr[k].w, arr[k].h = int(d["track_id"]), int(d.get("class_id", 0)), x, y, w, h
            arr[k].mask = m.ctypes.data
            arr[k].points = pts.ctypes.data if pts is not None and len(pts) else None
            arr[k].n_points = 0 if pts is None else len(pts)
        b3 = np.ascontiguousarray(boxes3d, BOX3D_DTYPE) if boxes3d is not None else np.zeros(0, BOX3D_DTYPE)
        self._inst_keep.append(b3)
        self._check(self.lib.dv_inst_track_enqueue(self.h, float(t), C.addressof(arr) if len(dets) else None, len(dets), b3.ctypes.data if len(b3) else None, len(b3)))

    def inst_set_disparity(self, disp, baseline, mem=DV_MEM_HOST, stride_bytes=0):
        """SemanticImage::disp of the frame the next inst_track_enqueue processes: float32 [h, w] numpy array (host) or a device pointer (int, mem=DV_MEM_DEVICE, kept alive
        by the caller until inst_track_collect).  The extra points of every visible object are then computed on the device (DetectExtraPoints + ProcessExtraPoints)."""
        if disp is None:
            self._check(self.lib.dv_inst_set_disparity(self.h, None, 0, 0, 0.0))
            return
        if isinstance(disp, np.ndarray):
            self._disp_keep = np.ascontiguousarray(disp, np.float32)
            ptr, mem, stride_bytes = self._disp_keep.ctypes.data, DV_MEM_HOST, self._disp_keep.strides[0]
        else:
            ptr = int(disp)
        self._check(self.lib.dv_inst_set_disparity(self.h, ptr, int(stride_bytes), int(mem), float(baseline)))

    def track_unmask_static(self, dets, static_ids):
        """FeatureTrack, system/main.cpp:217-245 (para::is_static_inst_as_background): for the NEXT track_stereo_enqueue (which must carry a mask) the pixels of the frame's
        detections whose track_id the estimator reported static leave the merged instance mask.  dets: the frame's detection dicts (rect, mask)."""
        ids = np.ascontiguousarray(static_ids, np.uint32)
        if not len(ids) or not len(dets):
            self._check(self.lib.dv_track_unmask_static(self.h, None, 0, None, 0))
            return
        arr = (dv_inst_det * len(dets))()
        keep = []
        for k, d in enumerate(dets):
            m = np.ascontiguousarray(d["mask"], np.uint8); keep.append(m)
            x, y, w, h = [int(v) for v in d["rect"]]
            arr[k].track_id, arr[k].x, arr[k].y, arr[k].w, arr[k].h, arr[k].mask = int(d["track_id"]), x, y, w, h, m.ctypes.data
        self._check(self.lib.dv_track_unmask_static(self.h, C.addressof(arr), len(dets), ids.ctypes.data, len(ids)))

    @staticmethod
    def _det_array(dets):
        """dv_inst_det[len(dets)] with the rectangles and track ids alone (the key-image entries ignore mask and points)"""
        arr = (dv_inst_det * max(len(dets), 1))()
        for k, d in enumerate(dets):
            x, y, w, h = [int(v) for v in d["rect"]]
            arr[k].track_id, arr[k].class_id, arr[k].x, arr[k].y, arr[k].w, arr[k].h = int(d["track_id"]), int(d.get("class_id", 0)), x, y, w, h
        return arr

    def _key_image(self, key_img, mem, stride_bytes):
        """(pointer, stride in bytes, mem) of a key image: a uint32 [h, w] numpy array (host, kept alive on self) or a raw pointer (int) with the caller's mem / stride"""
        if isinstance(key_img, np.ndarray):
            assert key_img.dtype == np.uint32 and key_img.strides[1] == 4
            self._keyimg_keep = key_img
            return key_img.ctypes.data, key_img.strides[0], DV_MEM_HOST
        return (None if key_img is None else int(key_img)), int(stride_bytes), int(mem)

    def inst_track_enqueue_keys(self, t, dets, key_img, mem=DV_MEM_HOST, stride_bytes=0, boxes3d=None):
        """inst_track_enqueue with the objects' masks cut on the device from the frame's key image: mask of a detection = key_img[rect] == track_id.  dets: dicts with track_id
        and rect (mask / points are ignored); key_img: uint32 [h, w] numpy array or a device / pinned pointer (int) with mem and stride_bytes."""
        from .dynsim import BOX3D_DTYPE
        arr = self._det_array(dets)
        ptr, stride_bytes, mem = self._key_image(key_img, mem, stride_bytes)
        b3 = np.ascontiguousarray(boxes3d, BOX3D_DTYPE) if boxes3d is not None else np.zeros(0, BOX3D_DTYPE)
        self._inst_keep = [arr, b3]
        self._check(self.lib.dv_inst_track_enqueue_keys(self.h, float(t), C.addressof(arr) if len(dets) else None, len(dets), ptr, stride_bytes, mem, b3.ctypes.data if len(b3) else None, len(b3)))

    def track_unmask_static_keys(self, dets, static_ids, key_img, mem=DV_MEM_HOST, stride_bytes=0):
        """track_unmask_static from the frame's key image: the pixels with key == track_id inside the rectangles of the static detections leave the merged mask"""
        ids = np.ascontiguousarray(static_ids, np.uint32)
        arr = self._det_array(dets)
        ptr, stride_bytes, mem = self._key_image(key_img, mem, stride_bytes)
        self._check(self.lib.dv_track_unmask_static_keys(self.h, C.addressof(arr) if len(dets) else None, len(dets), ids.ctypes.data if len(ids) else None, len(ids), ptr, stride_bytes, mem))

    def viode_frame_enqueue(self, seg0, seg1, dyn_keys, mem=DV_MEM_HOST, stride=0):
        """thread T1's stage of one frame: label images (uint8 [h, w, 3] B G R numpy arrays, or device / pinned pointers with mem and stride) -> library-owned device buffers"""
        keys = np.ascontiguousarray(dyn_keys, np.uint32)
        ptrs = []
        for sg in (seg0, seg1):
            if isinstance(sg, np.ndarray):
                assert sg.dtype == np.uint8 and sg.ndim == 3 and sg.strides[1] == 3 and sg.strides[2] == 1
                ptrs.append(sg.ctypes.data); mem, stride = DV_MEM_HOST, sg.strides[0]
            else:
                ptrs.append(None if sg is None else int(sg))
        self._viode_keep = (seg0, seg1, keys)
        self._check(self.lib.dv_viode_frame_enqueue(self.h, ptrs[0], ptrs[1], self.cfg.width, self.cfg.height, int(stride), int(mem), keys.ctypes.data, len(keys)))

    def viode_frame_collect(self, min_inst_size=8, cap=64):
        """-> (dets [dict(track_id, class_id, rect, mask=None, points=None)], inverse merged mask, key image left, key image right or None) — the three as DEVICE POINTERS
        (int) into the library's buffers of that frame"""
        arr = (dv_inst_det * max(cap, 1))()
        n, inv, k0, k1 = C.c_int(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        self._check(self.lib.dv_viode_frame_collect(self.h, int(min_inst_size), C.addressof(arr), int(cap), C.byref(n), C.byref(inv), C.byref(k0), C.byref(k1)))
        dets = [dict(track_id=int(a.track_id), class_id=int(a.class_id), rect=(int(a.x), int(a.y), int(a.w), int(a.h)), mask=None, points=None) for a in arr[: n.value]]
        return dets, inv.value, k0.value, k1.value

    def inst_stack_frame_enqueue(self, stack, remap_merged=False, **kw):
        """thread T1's stage of one frame from a detector's mask stack (see mask_stack() for `stack` and the keywords) -> library-owned device buffers.
        remap_merged: SemanticImage::SetBackgroundMask's remap of the merged mask (needs installed undistortion maps)"""
        st = mask_stack(stack, **kw)
        self._stack_keep = (stack, st)
        self._check(self.lib.dv_inst_stack_frame_enqueue(self.h, C.addressof(st), self.cfg.width, self.cfg.height, DV_STACK_REMAP_MERGED if remap_merged else 0))

    def inst_stack_frame_collect(self, min_inst_size=8, cap=64):
        """-> (dets [dict(track_id = plane, class_id, rect, plane, mask=None, points=None)], inverse merged mask, merged mask) — the two masks as DEVICE POINTERS (int)
        into the library's buffers of that frame.  The caller's multi-object tracker overwrites track_id / class_id; `plane` stays."""
        arr = (dv_inst_det * max(cap, 1))()
        planes = (C.c_int32 * max(cap, 1))()
        n, inv, mrg = C.c_int(0), C.c_void_p(0), C.c_void_p(0)
        self._check(self.lib.dv_inst_stack_frame_collect(self.h, int(min_inst_size), C.addressof(arr), C.addressof(planes), int(cap), C.byref(n), C.byref(inv), C.byref(mrg)))
        dets = [dict(track_id=int(a.track_id), class_id=int(a.class_id), rect=(int(a.x), int(a.y), int(a.w), int(a.h)), plane=int(planes[i]), mask=None, points=None)
                for i, a in enumerate(arr[: n.value])]
        return dets, inv.value, mrg.value

    def solo_head_enqueue(self, outputs, params):
        """the detector's head of one frame (Solov2::GetSegTensor, det2d/solo_head.cpp:410-559) on the ctx's stream: outputs = solo_outputs(...), params = solo_params(...)"""
        self._solo_keep = (outputs, params)
        self._check(self.lib.dv_solo_head_enqueue(self.h, C.addressof(outputs), C.addressof(params)))

    def solo_head_collect(self):
        """-> (labels int32 [n], scores float32 [n], dv_mask_stack of the first min(n, 64) planes — DV_STACK_U8 in the library's device memory —, cells over score_thr)"""
        labels, scores = np.zeros(128, np.int32), np.zeros(128, np.float32)
        n, nc, st = C.c_int(0), C.c_int(0), dv_mask_stack()
        self._check(self.lib.dv_solo_head_collect(self.h, labels.ctypes.data, scores.ctypes.data, 128, C.byref(n), C.byref(nc), C.addressof(st)))
        return labels[: n.value].copy(), scores[: n.value].copy(), st, nc.value

    # ---- the detector's input (Pipeline::ImageToTensor + ProcessInput, det2d/pipeline.cpp:370-387,204-232): colour frame -> the network's [3, model_h, model_w] tensor ----
    def solo_input_enqueue(self, bgr, model_w, model_h, mean=SOLO_IMG_MEAN, std=SOLO_IMG_STD, mem=DV_MEM_HOST, stride=None, dst=None):
        """one frame on the ctx's stream.  mem = DV_MEM_HOST: bgr an (height, width, 3) uint8 array of the ctx's size (any row stride), staged.  DV_MEM_DEVICE /
        DV_MEM_PINNED: bgr is a pointer (int) read in place until the collect, with the row stride in bytes — the caller keeps that memory alive; only a host array
        is held here until the collect.  dst: None — the library's two alternating buffers — or a
        device pointer (int) to 3 * model_h * model_w floats of the caller's, 4-byte aligned"""
        if mem == DV_MEM_HOST:
            if not (isinstance(bgr, np.ndarray) and bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3 and bgr.strides[2] == 1 and bgr.strides[1] == 3):
                raise ValueError("solo_input_enqueue: bgr must be (height, width, 3) uint8 with packed pixels")
            if bgr.shape[:2] != (self.cfg.height, self.cfg.width):
                raise ValueError("solo_input_enqueue: the image must have the ctx's size")
            stride = bgr.strides[0]
        else:
            if stride is None:
                raise ValueError("solo_input_enqueue: stride is required with device or pinned pointers")
            if not isinstance(bgr, (int, np.integer)):
                raise ValueError("solo_input_enqueue: bgr must be a pointer (int) with device or pinned memory")
        par = solo_input_params(model_w, model_h, mean, std)
        self._solo_in_keep, self._solo_in_shape = (bgr if mem == DV_MEM_HOST else None), (3, int(model_h), int(model_w))
        self._check(self.lib.dv_solo_input_enqueue(self.h, _ptr(bgr), int(stride), int(mem), C.addressof(par), _ptr(None if dst is None else int(dst))))

    def solo_input_collect(self):
        """waits for the stage -> (device pointer of the [3, model_h, model_w] float32 tensor, its shape, the image's rectangle (x, y, w, h) inside it).  A library-owned
        tensor stays valid until the second enqueue after this collect; frontend.device_tensor(ptr, shape) wraps it for torch without a copy"""
        p, r = C.c_void_p(0), [C.c_int(0) for _ in range(4)]
        self._solo_in_keep = None
        self._check(self.lib.dv_solo_input_collect(self.h, C.byref(p), *[C.byref(v) for v in r]))
        return p.value, self._solo_in_shape, tuple(v.value for v in r)

    def solo_input(self, bgr, model_w, model_h, mean=SOLO_IMG_MEAN, std=SOLO_IMG_STD, mem=DV_MEM_HOST, stride=None, dst=None):
        """solo_input_enqueue + solo_input_collect -> (torch device tensor [3, model_h, model_w] over the stage's memory, no copy; rectangle)"""
        self.solo_input_enqueue(bgr, model_w, model_h, mean, std, mem, stride, dst)
        ptr, shape, rect = self.solo_input_collect()
        return device_tensor(ptr, shape, device=self.cfg.device), rect

    # ---- the stereo matcher (MyStereoMatcher::Launch / WaitResult, stereo/stereo.cpp): rectified gray pair -> SemanticImage::disp on the device ----
    def stereo_sgm_enqueue(self, gray0, gray1, params=None, mem=DV_MEM_HOST, stride=None, **kw):
        """one frame on the ctx's stream; params = sgm_params(...) or its keywords.  mem = DV_MEM_HOST: two (height, width) uint8 arrays of the ctx's size with ONE row
        stride, staged.  DV_MEM_DEVICE / DV_MEM_PINNED: pointers (int) read in place until the collect, with the row stride in bytes"""
        par = params if params is not None else sgm_params(**kw)
        if mem == DV_MEM_HOST:
            for g in (gray0, gray1):
                if not (isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.ndim == 2 and g.strides[1] == 1 and g.shape == (self.cfg.height, self.cfg.width)):
                    raise ValueError("stereo_sgm_enqueue: images must be (height, width) uint8 arrays of the ctx's size")
            if gray0.strides[0] != gray1.strides[0]:
                raise ValueError("stereo_sgm_enqueue: the two images must share one row stride")
            stride = gray0.strides[0]
        else:
            if stride is None:
                raise ValueError("stereo_sgm_enqueue: stride is required with device or pinned pointers")
            if not (isinstance(gray0, (int, np.integer)) and isinstance(gray1, (int, np.integer))):
                raise ValueError("stereo_sgm_enqueue: images must be pointers (int) with device or pinned memory")
        self._sgm_keep, self._sgm_par = ((gray0, gray1) if mem == DV_MEM_HOST else None), par
        self._check(self.lib.dv_stereo_sgm_enqueue(self.h, _ptr(gray0), _ptr(gray1), int(stride), int(mem), C.addressof(par)))

    def stereo_sgm_collect(self):
        """waits for the stage -> (device pointer of the float32 [height, width] disparity map, its row stride in bytes).  The map is the library's and stays valid until
        the second enqueue after this collect; it goes straight into inst_set_disparity(ptr, baseline, DV_MEM_DEVICE, stride)"""
        p, st = C.c_void_p(0), C.c_int(0)
        self._sgm_keep = None
        self._check(self.lib.dv_stereo_sgm_collect(self.h, C.byref(p), C.byref(st)))
        return p.value, st.value

    def stereo_sgm(self, gray0, gray1, params=None, mem=DV_MEM_HOST, stride=None, host=True, **kw):
        """stereo_sgm_enqueue + stereo_sgm_collect -> the disparity map as a float32 [height, width] host array (host=True) or (device pointer, stride in bytes)"""
        self.stereo_sgm_enqueue(gray0, gray1, params, mem, stride, **kw)
        ptr, st = self.stereo_sgm_collect()
        if not host:
            return ptr, st
        return device_tensor(ptr, (self.cfg.height, self.cfg.width), device=self.cfg.device).cpu().numpy()

    def stereo_sgm_debug(self, what):
        """the last collected frame, for tests: what = DV_SGM_DEBUG_CENSUS_L / _R -> uint64 [h, w]; _S -> uint16 [h, w, n_disp]; _DSTAR / _DR -> int16 [h, w]"""
        h, w = self.cfg.height, self.cfg.width
        if what in (DV_SGM_DEBUG_CENSUS_L, DV_SGM_DEBUG_CENSUS_R):
            out = np.zeros((h, w), np.uint64)
        elif what == DV_SGM_DEBUG_S:
            out = np.zeros((h, w, int(self._sgm_par.n_disp)), np.uint16)
        else:
            out = np.zeros((h, w), np.int16)
        self._check(self.lib.dv_stereo_sgm_debug(self.h, int(what), out.ctypes.data, out.nbytes))
        return out

    # ---- the multi-object tracker (DeepSORT::update, mot/deep_sort.cpp:72-139): detections + embeddings -> track ids, table and galleries resident ----
    def mot_config(self, params=None, **kw):
        """allocates and resets the tracker; params = mot_params(...) or its keywords"""
        self._mot_par = params if params is not None else mot_params(**kw)
        self._check(self.lib.dv_mot_config(self.h, C.addressof(self._mot_par)))

    def mot_reset(self):
        self._check(self.lib.dv_mot_reset(self.h))

    def mot_update_enqueue(self, rects, feats, n=None, mem=DV_MEM_HOST):
        """one frame on the ctx's stream.  rects [n, 4] x, y, w, h and feats [n, feat_dim] (L2-normalised rows), float32.  mem = DV_MEM_HOST: host arrays, staged.
        DV_MEM_DEVICE / DV_MEM_PINNED: feats is a pointer (int) read in place and n is required; rects is a pointer of either in-place kind, or a host array, which goes
        through a small pinned buffer of the ctx (the rectangles come from inst_stack_frame_collect on the host, the embeddings from the ReID network on the device).
        n = 0 is the reference's "tracker not called": nothing predicts or ages"""
        if mem == DV_MEM_HOST:
            rects = np.ascontiguousarray(rects, np.float32).reshape(-1, 4)
            n = len(rects) if n is None else int(n)
            if n:
                if self._mot_par is None:
                    raise DvinsError("mot_update_enqueue: mot_config first")
                feats = np.ascontiguousarray(feats, np.float32)
                if feats.shape != (n, self._mot_par.feat_dim):
                    raise ValueError(f"feats must be [{n}, {self._mot_par.feat_dim}]")
        else:
            if n is None:
                raise ValueError("mot_update_enqueue: n is required with device or pinned pointers")
            n = int(n)
            if n and not isinstance(feats, (int, np.integer)):
                raise ValueError("mot_update_enqueue: feats must be a pointer (int) with device or pinned memory")
            if n and not isinstance(rects, (int, np.integer)):
                r = np.ascontiguousarray(rects, np.float32).reshape(-1, 4)
                if len(r) != n or n > DV_MOT_MAX_DETS:
                    raise ValueError(f"rects must be [{n}, 4], n <= {DV_MOT_MAX_DETS}")
                if self._mot_pin is None:
                    self._mot_pin = self.lib.dv_pinned_alloc(DV_MOT_MAX_DETS * 16)
                    if not self._mot_pin:
                        raise DvinsError("mot_update_enqueue: no pinned memory")
                C.memmove(self._mot_pin, r.ctypes.data, n * 16)
                rects = int(self._mot_pin)
        self._mot_keep = (rects, feats)
        self._check(self.lib.dv_mot_update_enqueue(self.h, _ptr(rects) if n else None, _ptr(feats) if n else None, n, mem))
        self._mot_n = n

    def mot_update_collect(self):
        """-> (track_id int32 [n]: the Confirmed track updated with each detection, else -1; tracks in the table; Confirmed ones)"""
        ids, nt, nc = np.full(max(self._mot_n, 1), -1, np.int32), C.c_int(0), C.c_int(0)
        n, self._mot_n, self._mot_keep = self._mot_n, 0, None
        self._check(self.lib.dv_mot_update_collect(self.h, ids.ctypes.data, C.byref(nt), C.byref(nc)))
        return ids[:n].copy(), nt.value, nc.value

    def mot_update(self, rects, feats, n=None, mem=DV_MEM_HOST):
        """mot_update_enqueue + mot_update_collect"""
        self.mot_update_enqueue(rects, feats, n, mem)
        return self.mot_update_collect()

    def mot_tracks(self):
        """the track table in order (MOT_TRACK_DTYPE rows): for tests and the shim"""
        out, n = np.zeros(DV_MOT_MAX_TRACKS, MOT_TRACK_DTYPE), C.c_int(0)
        self._check(self.lib.dv_mot_get_tracks(self.h, out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def mot_assign(self, cost):
        """the device Munkres alone (HungarianAlgorithm::Solve, mot/hungarian.cpp) on a [rows <= 128, cols <= 64] cost matrix -> column per row, or -1"""
        cost = np.ascontiguousarray(cost, np.float32)
        rows, cols = cost.shape
        out = np.full(max(rows, 1), -1, np.int32)
        self._check(self.lib.dv_mot_assign(self.h, cost.ctypes.data if cost.size else None, rows, cols, out.ctypes.data))
        return out[:rows].copy()

    # ---- the line tracker (LineDetector::TrackLeftLine / TrackRightLine, line_detector/line_detector.cpp:101-297): key lines + LBD descriptors -> ids, counts, rows ----
    def line_track_reset(self):
        """no previous frame, id counter back to 0"""
        self._check(self.lib.dv_line_track_reset(self.h))

    def line_track_enqueue(self, left_lines, left_desc, right_lines=None, right_desc=None, n_left=None, n_right=0, mem=DV_MEM_HOST):
        """Host: left_lines [n, 6] float32 (KEYLINE_DTYPE order), left_desc [n, 32] uint8; right_* the same or None (no right image).  Device / pinned: raw pointers
        (int) with n_left / n_right, valid until line_track_collect."""
        if mem == DV_MEM_HOST:
            left_lines, left_desc, n_left = _key_lines(left_lines, left_desc)
            if right_lines is not None:
                right_lines, right_desc, n_right = _key_lines(right_lines, right_desc)
        elif n_left is None:
            raise ValueError("line_track_enqueue: n_left is required with device or pinned pointers")
        self._line_keep = (left_lines, left_desc, right_lines, right_desc)
        has_r = right_lines is not None
        self._check(self.lib.dv_line_track_enqueue(self.h, _ptr(left_lines) if n_left else None, _ptr(left_desc) if n_left else None, int(n_left),
                                                   _ptr(right_lines) if has_r and n_right else None, _ptr(right_desc) if has_r and n_right else None, int(n_right) if has_r else 0, int(mem)))

    def line_track_collect(self):
        """-> dict: rows (LINEROW_DTYPE, ascending id: what Estimator.set_lines takes), left_ids / left_src / left_cnt and right_ids / right_src per surviving line in
        output order (*_src = the line's index in the enqueued array)"""
        from .backend import LINEROW_DTYPE
        rows = np.zeros(DV_LINE_MAX, LINEROW_DTYPE)
        lid, lsrc, lcnt = np.zeros(DV_LINE_MAX, np.uint32), np.zeros(DV_LINE_MAX, np.int32), np.zeros(DV_LINE_MAX, np.int32)
        rid, rsrc = np.zeros(DV_LINE_MAX, np.uint32), np.zeros(DV_LINE_MAX, np.int32)
        nr, nl, nrt = C.c_int(0), C.c_int(0), C.c_int(0)
        self._line_keep = None
        self._check(self.lib.dv_line_track_collect(self.h, rows.ctypes.data, len(rows), C.byref(nr), lid.ctypes.data, lsrc.ctypes.data, lcnt.ctypes.data, C.byref(nl),
                                                   rid.ctypes.data, rsrc.ctypes.data, C.byref(nrt)))
        return {"rows": rows[: nr.value].copy(), "left_ids": lid[: nl.value].copy(), "left_src": lsrc[: nl.value].copy(), "left_cnt": lcnt[: nl.value].copy(),
                "right_ids": rid[: nrt.value].copy(), "right_src": rsrc[: nrt.value].copy()}

    def line_track(self, left_lines, left_desc, right_lines=None, right_desc=None, **kw):
        """line_track_enqueue + line_track_collect"""
        self.line_track_enqueue(left_lines, left_desc, right_lines, right_desc, **kw)
        return self.line_track_collect()

    def line_match(self, query_desc, train_desc):
        """BinaryDescriptorMatcher::match(query, train) alone on [n, 32] uint8 rows -> (train_idx, distance) int32; -1 / 0 where the minimum distance is >= 30"""
        q = np.ascontiguousarray(query_desc, np.uint8).reshape(-1, DV_LINE_DESC_BYTES)
        t = np.ascontiguousarray(train_desc, np.uint8).reshape(-1, DV_LINE_DESC_BYTES)
        idx, dist = np.full(max(len(q), 1), -1, np.int32), np.zeros(max(len(q), 1), np.int32)
        self._check(self.lib.dv_line_match(self.h, q.ctypes.data if len(q) else None, len(q), t.ctypes.data if len(t) else None, len(t), idx.ctypes.data, dist.ctypes.data))
        return idx[: len(q)].copy(), dist[: len(q)].copy()

    # ---- the LBD descriptor (LineDetector::Detect behind LSD, line_detector/line_detector.cpp:78-97): gray image + key lines -> selected lines and 32-byte rows on the device ----
    def lbd_describe_enqueue(self, cam, image, lines, num_pixels=None, mask=None, min_length=60.0, n=None, mem=DV_MEM_HOST, lines_mem=DV_MEM_HOST, size=None, stride=None,
                             mask_stride=None):
        """cam: 0 / 1, one buffer set each.  image / mask: [h, w] uint8 arrays (any row stride), or raw pointers (int) with mem, size = (w, h), stride and mask_stride.
        lines ([n, 6] float32) / num_pixels ([n] int32 or None: the library's rule): host arrays, or raw pointers (int) with lines_mem and n."""
        if isinstance(image, np.ndarray):
            assert image.ndim == 2 and image.dtype == np.uint8 and image.strides[1] == 1
            (h, w), stride = image.shape, image.strides[0]
        else:
            (w, h) = size
        if isinstance(mask, np.ndarray):
            assert mask.shape == (h, w) and mask.dtype == np.uint8 and mask.strides[1] == 1
            mask_stride = mask.strides[0]
        if lines_mem == DV_MEM_HOST and n is None:
            lines, num_pixels, n = _host_lines(lines, num_pixels)
        elif n is None:
            raise ValueError("lbd_describe_enqueue: n is required with device or pinned lines")
        self._lbd_keep = getattr(self, "_lbd_keep", {})
        self._lbd_keep[cam] = (image, mask, lines, num_pixels)
        self._check(self.lib.dv_lbd_describe_enqueue(self.h, int(cam), _ptr(image), int(stride), int(w), int(h), int(mem), _ptr(lines) if n else None,
                                                     _ptr(num_pixels) if n else None, int(n), int(lines_mem), _ptr(mask), int(mask_stride or 0), float(min_length)))

    def lbd_describe_collect(self, cam, host=True):
        """-> dict: n, src (each survivor's index in the enqueued array), dev_lines / dev_desc (device pointers, valid until the next enqueue on cam: what
        line_track_enqueue(..., mem=DV_MEM_DEVICE) takes) and, with host=True, lines [n, 6] float32 and desc [n, 32] uint8"""
        nk, src = C.c_int(0), np.zeros(DV_LINE_MAX, np.int32)
        dl, dd = C.c_void_p(0), C.c_void_p(0)
        hl, hd = (np.zeros((DV_LINE_MAX, 6), np.float32), np.zeros((DV_LINE_MAX, DV_LINE_DESC_BYTES), np.uint8)) if host else (None, None)
        if getattr(self, "_lbd_keep", None):
            self._lbd_keep.pop(cam, None)
        self._check(self.lib.dv_lbd_describe_collect(self.h, int(cam), C.byref(nk), src.ctypes.data, C.byref(dl), C.byref(dd), _ptr(hl), _ptr(hd)))
        out = {"n": nk.value, "src": src[: nk.value].copy(), "dev_lines": dl.value or 0, "dev_desc": dd.value or 0}
        if host:
            out["lines"], out["desc"] = hl[: nk.value].copy(), hd[: nk.value].copy()
        return out

    def lbd_describe(self, image, lines, num_pixels=None, mask=None, cam=0, host=True, **kw):
        """lbd_describe_enqueue + lbd_describe_collect"""
        self.lbd_describe_enqueue(cam, image, lines, num_pixels, mask, **kw)
        return self.lbd_describe_collect(cam, host=host)

    def lbd_debug(self, cam, w, h, n):
        """the last frame of cam, for tests: (dx [h, w] int16, dy [h, w] int16, the 72 floats of every enqueued line [n, 72] float32, before selection)"""
        dx, dy, fd = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16), np.zeros((max(n, 1), 72), np.float32)
        self._check(self.lib.dv_lbd_debug(self.h, int(cam), dx.ctypes.data, dy.ctypes.data, fd.ctypes.data))
        return dx, dy, fd[:n].copy()

    def lbd_track(self, left, left_lines, right=None, right_lines=None, left_num_pixels=None, right_num_pixels=None, mask=None, min_length=60.0):
        """Detect's second half and the tracker back to back, with no descriptor on the host: both images are described (cam 0 / 1 in flight together) and the device
        buffers go to line_track_enqueue(..., mem=DV_MEM_DEVICE).  -> line_track_collect's dict plus left_kept / right_kept (the describe stage's src)"""
        self.lbd_describe_enqueue(0, left, left_lines, left_num_pixels, mask, min_length)
        if right is not None:
            self.lbd_describe_enqueue(1, right, right_lines, right_num_pixels, None, min_length)
        a = self.lbd_describe_collect(0, host=False)
        b = self.lbd_describe_collect(1, host=False) if right is not None else None
        self.line_track_enqueue(a["dev_lines"], a["dev_desc"], b["dev_lines"] if b else None, b["dev_desc"] if b else None, n_left=a["n"], n_right=b["n"] if b else 0,
                                mem=DV_MEM_DEVICE)
        out = self.line_track_collect()
        out["left_kept"], out["right_kept"] = a["src"], (b["src"] if b else np.zeros(0, np.int32))
        return out

    # ---- the ReID extractor (Extractor::extract, mot/extractor.cpp:31-52; ReIdNetImpl, mot/reid_net.cpp): colour image + rectangles -> [n, 512] embeddings on the device ----
    def reid_load(self, weights, in_w=64, in_h=128):
        """weights: a float32 array or the path of the flat file ReIdNetImpl::load_form reads (11 178 496 floats); in_w x in_h = reid_input_width x reid_input_height.
        A second load replaces the weights; a refused one leaves the ctx as it was"""
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            weights = np.fromfile(weights, np.float32)
        weights = np.ascontiguousarray(weights, np.float32).reshape(-1)
        self._check(self.lib.dv_reid_load(self.h, weights.ctypes.data, weights.size, int(in_w), int(in_h)))
        self._reid_size = (int(in_w), int(in_h))

    def reid_extract_enqueue(self, bgr, rects, n=None, mem=DV_MEM_HOST, stride=None):
        """one frame on the ctx's stream.  mem = DV_MEM_HOST: bgr an (height, width, 3) uint8 array of the ctx's size (any row stride), rects [n, 4] x, y, w, h float32;
        both staged.  DV_MEM_DEVICE / DV_MEM_PINNED: bgr is a pointer (int) read in place until the collect, with n and the row stride in bytes; rects is a pointer of either
        in-place kind, or a host array, which goes through a small pinned buffer of the ctx"""
        if mem == DV_MEM_HOST:
            rects = np.ascontiguousarray(rects, np.float32).reshape(-1, 4)
            n = len(rects) if n is None else int(n)
            if n:
                if bgr.dtype != np.uint8 or bgr.ndim != 3 or bgr.shape[2] != 3 or bgr.strides[2] != 1 or bgr.strides[1] != 3:
                    raise ValueError("reid_extract_enqueue: bgr must be (height, width, 3) uint8 with packed pixels")
                if bgr.shape[:2] != (self.cfg.height, self.cfg.width):
                    raise ValueError("reid_extract_enqueue: the image must have the ctx's size")
                stride = bgr.strides[0]
        else:
            if n is None or (int(n) and stride is None):
                raise ValueError("reid_extract_enqueue: n and stride are required with device or pinned pointers")
            n = int(n)
            if n and not isinstance(bgr, (int, np.integer)):
                raise ValueError("reid_extract_enqueue: bgr must be a pointer (int) with device or pinned memory")
            if n and not isinstance(rects, (int, np.integer)):      # a host array of rectangles beside an in-place image: through a small pinned buffer of the ctx
                r = np.ascontiguousarray(rects, np.float32).reshape(-1, 4)
                if len(r) != n or n > DV_REID_MAX_CROPS:
                    raise ValueError(f"rects must be [{n}, 4], n <= {DV_REID_MAX_CROPS}")
                if self._reid_pin is None:
                    self._reid_pin = self.lib.dv_pinned_alloc(DV_REID_MAX_CROPS * 16)
                    if not self._reid_pin:
                        raise DvinsError("reid_extract_enqueue: no pinned memory")
                C.memmove(self._reid_pin, r.ctypes.data, n * 16)
                rects = int(self._reid_pin)
        self._reid_keep = (bgr, rects)
        self._check(self.lib.dv_reid_extract_enqueue(self.h, _ptr(bgr) if n else None, int(stride or 0), _ptr(rects) if n else None, n, mem))
        self._reid_n = n

    def reid_extract_collect(self):
        """-> (device pointer of the [n, 512] float32 embeddings, valid until the next enqueue; n).  mot_update_enqueue(rects, ptr, n, DV_MEM_DEVICE) reads it in place"""
        p = C.c_void_p(0)
        n, self._reid_n, self._reid_keep = self._reid_n, 0, None
        self._check(self.lib.dv_reid_extract_collect(self.h, C.byref(p)))
        return int(p.value or 0), n

    def reid_feats(self, n):
        """the first n embeddings of the last collected frame, downloaded"""
        out = np.zeros((int(n), DV_REID_FEAT_DIM), np.float32)
        self._check(self.lib.dv_reid_get_feats(self.h, out.ctypes.data if n else None, int(n)))
        return out

    def reid_extract(self, bgr, rects, n=None, mem=DV_MEM_HOST, stride=None):
        """reid_extract_enqueue + reid_extract_collect + the download -> [n, 512] float32"""
        self.reid_extract_enqueue(bgr, rects, n, mem, stride)
        _, n = self.reid_extract_collect()
        return self.reid_feats(n)

    def reid_input(self, n):
        """the prepared [n, 3, in_h, in_w] tensor of the last collected frame of n crops (for tests)"""
        if self._reid_size is None:
            raise DvinsError("reid_input: reid_load first")
        w, h = self._reid_size
        out = np.zeros((max(int(n), 1), 3, h, w), np.float32)
        self._check(self.lib.dv_reid_input(self.h, out.ctypes.data))
        return out[: int(n)]

    def reid_layer(self, x, weight, scale, shift, residual=None, stride=1, relu=True):
        """the extractor's convolution kernel alone: relu?(conv2d(x, weight, stride, padding 1 for a 3 x 3, 0 for a 1 x 1) * scale + shift + residual), NCHW float32"""
        x, weight = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(weight, np.float32)
        scale, shift = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(shift, np.float32)
        n, ci, h, w = x.shape
        co, ci2, k, k2 = weight.shape
        if ci2 != ci or k2 != k or scale.shape != (co,) or shift.shape != (co,):
            raise ValueError("reid_layer: shapes do not agree")
        ho, wo = (h + (2 if k == 3 else 0) - k) // stride + 1, (w + (2 if k == 3 else 0) - k) // stride + 1
        out = np.zeros((n, co, max(ho, 1), max(wo, 1)), np.float32)
        if residual is not None:
            residual = np.ascontiguousarray(residual, np.float32)
            if residual.shape != out.shape:
                raise ValueError("reid_layer: residual must have the output's shape")
        self._check(self.lib.dv_reid_layer(self.h, x.ctypes.data, n, ci, h, w, weight.ctypes.data, co, k, int(stride), scale.ctypes.data, shift.ctypes.data,
                                           residual.ctypes.data if residual is not None else None, int(bool(relu)), out.ctypes.data))
        return out

    def reid_stem(self, x, weight, scale, shift):
        """the extractor's fused stem kernel alone: max_pool2d(relu(conv2d(x, weight, padding 1) * scale + shift), 3, 2, 1), x [n, 3, h, w] -> [n, 64, ceil(h / 2),
        ceil(w / 2)], NCHW float32"""
        x, weight = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(weight, np.float32)
        scale, shift = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(shift, np.float32)
        if x.ndim != 4 or x.shape[1] != 3 or weight.shape != (64, 3, 3, 3) or scale.shape != (64,) or shift.shape != (64,):
            raise ValueError("reid_stem: x [n, 3, h, w], weight [64, 3, 3, 3], scale and shift [64]")
        n, _, h, w = x.shape
        out = np.zeros((n, 64, max((h + 1) // 2, 1), max((w + 1) // 2, 1)), np.float32)
        self._check(self.lib.dv_reid_stem(self.h, x.ctypes.data, n, h, w, weight.ctypes.data, scale.ctypes.data, shift.ctypes.data, out.ctypes.data))
        return out

    def solo_head(self, outputs, params):
        """solo_head_enqueue + solo_head_collect"""
        self.solo_head_enqueue(outputs, params)
        return self.solo_head_collect()

    @staticmethod
    def _plane_array(dets):
        planes = (C.c_int32 * max(len(dets), 1))()
        for k, d in enumerate(dets):
            planes[k] = int(d["plane"])
        return planes

    def inst_track_enqueue_planes(self, t, dets, stack, boxes3d=None, **kw):
        """inst_track_enqueue with the objects' masks cut on the device from the detector's mask stack: mask of a detection = "plane d['plane'] has the pixel" over its
        rectangle.  dets: dicts with track_id, rect and plane (mask / points are ignored)"""
        from .dynsim import BOX3D_DTYPE
        arr, planes, st = self._det_array(dets), self._plane_array(dets), mask_stack(stack, **kw)
        b3 = np.ascontiguousarray(boxes3d, BOX3D_DTYPE) if boxes3d is not None else np.zeros(0, BOX3D_DTYPE)
        self._inst_keep = [arr, planes, b3, stack, st]
        self._check(self.lib.dv_inst_track_enqueue_planes(self.h, float(t), C.addressof(arr) if len(dets) else None, C.addressof(planes) if len(dets) else None, len(dets),
                                                          C.addressof(st), b3.ctypes.data if len(b3) else None, len(b3)))

    def track_unmask_static_planes(self, dets, static_ids, stack, **kw):
        """track_unmask_static from the detector's mask stack: the pixels of plane d['plane'] inside the rectangles of the static detections leave the merged mask"""
        ids = np.ascontiguousarray(static_ids, np.uint32)
        arr, planes, st = self._det_array(dets), self._plane_array(dets), mask_stack(stack, **kw)
        self._unmask_keep = [stack, st]
        self._check(self.lib.dv_track_unmask_static_planes(self.h, C.addressof(arr) if len(dets) else None, C.addressof(planes) if len(dets) else None, len(dets),
                                                           ids.ctypes.data if len(ids) else None, len(ids), C.addressof(st)))

    def inst_set_right_keys(self, key_img, mem=DV_MEM_HOST):
        """VIODE: the key image of seg1 (viode_mask(...)[2]: uint32 [h, w] numpy array, or a device pointer with mem=DV_MEM_DEVICE) of the frame the next inst_track_enqueue
        processes: TrackRightByPad's segmentation-key test (front_end/instance_feature.cpp:263-268)"""
        if key_img is None:
            self._check(self.lib.dv_inst_set_right_keys(self.h, None, 0, 0))
            return
        if isinstance(key_img, np.ndarray):
            self._keys_keep = np.ascontiguousarray(key_img, np.uint32)
            self._check(self.lib.dv_inst_set_right_keys(self.h, self._keys_keep.ctypes.data, self._keys_keep.strides[0], DV_MEM_HOST))
        else:
            self._check(self.lib.dv_inst_set_right_keys(self.h, int(key_img), 0, int(mem)))

    def extra_points(self, mask, box_xy, disp, baseline, stage=0, mem=DV_MEM_HOST, stride_bytes=0):
        """operator form: one object through InstFeat::DetectExtraPoints (stage 1) or the whole extra-point pipeline (stage 0) -> float64 [n, 3].  disp: a float32 [h, w]
        host array, or a device pointer (int) with mem=DV_MEM_DEVICE (stereo_sgm_collect's map), read in place"""
        mask = np.ascontiguousarray(mask, np.uint8)
        if isinstance(disp, (int, np.integer)):
            dptr, dstride, dmem = int(disp), int(stride_bytes), int(mem)
        else:
            disp = np.ascontiguousarray(disp, np.float32)
            dptr, dstride, dmem = disp.ctypes.data, disp.strides[0], DV_MEM_HOST
        h, w = mask.shape
        out = np.zeros((4096, 3), np.float64)
        n = C.c_int(0)
        self._check(self.lib.dv_extra_points(self.h, mask.ctypes.data, int(box_xy[0]), int(box_xy[1]), w, h, dptr, dstride, dmem, float(baseline), int(stage),
                                             out.ctypes.data, len(out), C.byref(n)))
        return out[: n.value].copy()

    def inst_track_collect(self):
        """-> (insts [INSTOBS_DTYPE], feats [FEAT_DTYPE], points [n, 3]) laid out as Estimator.ProcessMeasurementsDynamic takes them"""
        oi, of, op = self._inst_out
        ni, nf, npt = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.dv_inst_track_collect(self.h, oi.ctypes.data, len(oi), C.byref(ni), of.ctypes.data, len(of), C.byref(nf), op.ctypes.data, len(op), C.byref(npt)))
        return oi[: ni.value].copy(), of[: nf.value].copy(), op[: npt.value].copy()

    def front_debug_mask(self, which, track_id=0):
        """for tests, after the frame was collected: which = 0 the background tracker's working mask, which = 1 the ROI mask of object track_id -> (uint8 [h, pitch], w)"""
        cap = (self.cfg.width + 15) // 16 * 16 * self.cfg.height
        out = np.zeros(cap, np.uint8)
        w, h, p = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.lib.dv_front_debug_mask(self.h, int(which), int(track_id), out.ctypes.data, cap, C.byref(w), C.byref(h), C.byref(p)))
        return out[: p.value * h.value].reshape(h.value, p.value).copy(), w.value

    def track_stereo_collect(self):
        n = C.c_int(0)
        self._check(self.lib.dv_track_stereo_collect(self.h, self._out.ctypes.data_as(C.POINTER(dv_feat)), C.byref(n)))
        return self._out[: n.value].copy()

    def reset(self):
        self._check(self.lib.dv_reset(self.h))

    def sync(self):
        self._check(self.lib.dv_sync(self.h))

    # ---- operator-level entries (host numpy in / out) ----
    def lk(self, img_a, img_b, pts_a, max_level=3, iters=30, eps=0.01, initial=None):
        h, w = img_a.shape
        pts_a = np.ascontiguousarray(pts_a, np.float32)
        n = len(pts_a)
        pts_b = np.ascontiguousarray(initial, np.float32).copy() if initial is not None else np.zeros((n, 2), np.float32)
        st = np.zeros(n, np.uint8)
        self._check(self.lib.dv_lk(self.h, _ptr(img_a), _ptr(img_b), w, h, img_a.strides[0], _ptr(pts_a), n, max_level, iters, float(eps),
                                   1 if initial is not None else 0, _ptr(pts_b), _ptr(st), DV_MEM_HOST))
        return pts_b, st

    def track_by_lk(self, img1, img2, pts1, flow_back=True, dist_thresh=0.5):
        """FeatureTrackByLK (front_end/feature_utils.cpp:35-69)."""
        h, w = img1.shape
        pts1 = np.ascontiguousarray(pts1, np.float32)
        n = len(pts1)
        pts2 = np.zeros((n, 2), np.float32)
        st = np.zeros(n, np.uint8)
        self._check(self.lib.dv_track_by_lk(self.h, _ptr(img1), _ptr(img2), w, h, img1.strides[0], _ptr(pts1), n, int(flow_back),
                                            float(dist_thresh), _ptr(pts2), _ptr(st), DV_MEM_HOST))
        return pts2, st

    def lk_cuda(self, img_a, img_b, pts_a, max_level=3, iters=30, initial=None):
        """cv::cuda::SparsePyrLKOpticalFlow(Size(21, 21), max_level, iters, useInitialFlow)->calc"""
        h, w = img_a.shape
        pts_a = np.ascontiguousarray(pts_a, np.float32); n = len(pts_a)
        pts_b = np.ascontiguousarray(initial, np.float32).copy() if initial is not None else np.zeros((n, 2), np.float32)
        st = np.zeros(n, np.uint8)
        self._check(self.lib.dv_lk_cuda(self.h, _ptr(img_a), _ptr(img_b), w, h, img_a.strides[0], _ptr(pts_a), n, int(max_level), int(iters), 1 if initial is not None else 0,
                                        _ptr(pts_b), _ptr(st), DV_MEM_HOST))
        return pts_b, st

    def track_by_lk_gpu(self, img1, img2, pts1, flow_back=True):
        """FeatureTrackByLKGpu (front_end/feature_utils.cpp:83-163)"""
        h, w = img1.shape
        pts1 = np.ascontiguousarray(pts1, np.float32); n = len(pts1)
        pts2 = np.zeros((n, 2), np.float32); st = np.zeros(n, np.uint8)
        self._check(self.lib.dv_track_by_lk_gpu(self.h, _ptr(img1), _ptr(img2), w, h, img1.strides[0], _ptr(pts1), n, int(flow_back), _ptr(pts2), _ptr(st), DV_MEM_HOST))
        return pts2, st

    def pyr_down_cuda(self, img):
        h, w = img.shape
        dst = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
        self._check(self.lib.dv_pyr_down_cuda(self.h, _ptr(img), w, h, img.strides[0], _ptr(dst), DV_MEM_HOST))
        return dst

    def gftt(self, img, max_n, quality, min_dist, mask=None, rule="cpu"):
        """rule "cpu": cv::goodFeaturesToTrack (dv_gftt); "cuda": cv::cuda::GoodFeaturesToTrackDetector, TrackImageNaive's detector (dv_gftt_cuda)"""
        h, w = img.shape
        out = np.zeros((_abi.DV_MAX_FEATS, 2), np.float32)
        n = C.c_int(0)
        self._check((self.lib.dv_gftt_cuda if rule == "cuda" else self.lib.dv_gftt)(self.h, _ptr(img), _ptr(mask), w, h, img.strides[0], int(max_n), float(quality), float(min_dist),
                                     _ptr(out), C.byref(n), DV_MEM_HOST))
        return out[: n.value].copy()

    def min_eigen(self, img, rule="cpu"):
        h, w = img.shape
        eig = np.zeros((h, w), np.float32)
        self._check((self.lib.dv_min_eigen_cuda if rule == "cuda" else self.lib.dv_min_eigen)(self.h, _ptr(img), w, h, img.strides[0], _ptr(eig), DV_MEM_HOST))
        return eig

    def viode_mask(self, seg_bgr, dyn_keys, want_keys=True):
        """VIODE::SetViodeMaskSimple / BuildViodeMask -> (merge_mask, inv_merge_mask, key_image or None, boxes[nkeys, 4])"""
        seg = np.ascontiguousarray(seg_bgr)
        h, w, _ = seg.shape
        keys = np.ascontiguousarray(dyn_keys, np.uint32)
        merge, inv = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        kimg = np.zeros((h, w), np.uint32) if want_keys else None
        boxes = np.zeros((len(keys), 4), np.int32)
        self._check(self.lib.dv_viode_mask(self.h, _ptr(seg), w, h, seg.strides[0], _ptr(keys), len(keys), _ptr(merge), _ptr(inv), _ptr(kimg), _ptr(boxes)))
        return merge, inv, kimg, boxes

    def bgr2gray(self, bgr):
        """cv::cvtColor(BGR2GRAY) of an (h, w, 3) uint8 image"""
        bgr = np.ascontiguousarray(bgr)
        h, w, _ = bgr.shape
        out = np.zeros((h, w), np.uint8)
        self._check(self.lib.dv_bgr2gray(self.h, _ptr(bgr), w, h, bgr.strides[0], _ptr(out), DV_MEM_HOST))
        return out

    def remap(self, src, map1, map2):
        """cv::remap(src, map1 (h, w, 2) int16, map2 (h, w) uint16, INTER_LINEAR) of an (h, w) or (h, w, 3) uint8 image"""
        src = np.ascontiguousarray(src)
        h, w = src.shape[:2]
        cn = 1 if src.ndim == 2 else src.shape[2]
        m1, m2 = np.ascontiguousarray(map1, np.int16), np.ascontiguousarray(map2, np.uint16)
        assert m1.shape == (h, w, 2) and m2.shape == (h, w)
        out = np.zeros_like(src)
        self._check(self.lib.dv_remap(self.h, _ptr(src), w, h, src.strides[0], cn, m1.ctypes.data, m2.ctypes.data, _ptr(out), DV_MEM_HOST))
        return out

    def set_undistort_maps(self, cam, map1=None, map2=None):
        """cfg::is_undistort_input: install (or, with map1=None, remove) the fixed-point undistortion maps of camera 0 / 1"""
        if map1 is None:
            self._check(self.lib.dv_set_undistort_maps(self.h, int(cam), None, None, 0, 0))
            self.cfg.cam0, self.cfg.cam1 = self.cameras()      # the original cameras again, had undistort_setup switched them
            return
        m1, m2 = np.ascontiguousarray(map1, np.int16), np.ascontiguousarray(map2, np.uint16)
        h, w = m2.shape
        assert m1.shape == (h, w, 2)
        self._check(self.lib.dv_set_undistort_maps(self.h, int(cam), m1.ctypes.data, m2.ctypes.data, w, h))
        self.cfg.cam0, self.cfg.cam1 = self.cameras()      # own maps after undistort_setup: that camera's original intrinsics hold again

    def init_undistort_map(self, cam, new_k, w, h, map1=None, map2=None):
        """cv::initUndistortRectifyMap(K, D, I, newK, (w, h), CV_16SC2) on the device -> (map1 (h, w, 2) int16, map2 (h, w) uint16) as host arrays, or — map1 / map2 given
        as device pointers (int) — written there (DV_MEM_DEVICE)"""
        c = cam if isinstance(cam, dv_cam) else make_cam(*cam)
        nk = (C.c_double * 4)(*[float(v) for v in new_k])
        if map1 is not None:
            self._check(self.lib.dv_init_undistort_map(self.h, C.byref(c), nk, int(w), int(h), _ptr(int(map1)), _ptr(int(map2)), DV_MEM_DEVICE))
            return None
        m1, m2 = np.zeros((h, w, 2), np.int16), np.zeros((h, w), np.uint16)
        self._check(self.lib.dv_init_undistort_map(self.h, C.byref(c), nk, int(w), int(h), m1.ctypes.data, m2.ctypes.data, DV_MEM_HOST))
        return m1, m2

    def undistort_setup(self, alpha=0.0):
        """cfg::is_undistort_input as InitOneCamera sets it up (utils/camera_model.cpp:479-504): new camera matrices, both map pairs built and installed on the device, the
        ctx's cameras switched to (newK, 0).  From then on the tracker takes DISTORTED frames.  -> (new_cam0, new_cam1); set_undistort_maps(0) undoes it."""
        c0, c1 = dv_cam(), dv_cam()
        self._check(self.lib.dv_undistort_setup(self.h, float(alpha), C.byref(c0), C.byref(c1)))
        self.cfg.cam0, self.cfg.cam1 = c0, c1
        return c0, c1

    def undistort_maps(self, cam):
        """the installed maps of camera 0 / 1 -> (map1 (h, w, 2) int16, map2 (h, w) uint16)"""
        w, h = self.cfg.width, self.cfg.height
        m1, m2 = np.zeros((h, w, 2), np.int16), np.zeros((h, w), np.uint16)
        self._check(self.lib.dv_get_undistort_maps(self.h, int(cam), m1.ctypes.data, m2.ctypes.data, DV_MEM_HOST))
        return m1, m2

    def cameras(self):
        """the cameras the ctx lifts with at the moment"""
        c0, c1 = dv_cam(), dv_cam()
        self._check(self.lib.dv_get_cameras(self.h, C.byref(c0), C.byref(c1)))
        return c0, c1

    def pyr_down(self, img):
        h, w = img.shape
        dst = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
        self._check(self.lib.dv_pyr_down(self.h, _ptr(img), w, h, img.strides[0], _ptr(dst), DV_MEM_HOST))
        return dst

    def circle_mask(self, mask, pts, radius):
        h, w = mask.shape
        pts = np.ascontiguousarray(pts, np.float32)
        out = np.ascontiguousarray(mask).copy()
        self._check(self.lib.dv_circle_mask(self.h, _ptr(out), w, h, out.strides[0], _ptr(pts), len(pts), int(radius), DV_MEM_HOST))
        return out

    def erode(self, mask, k):
        h, w = mask.shape
        out = np.zeros_like(mask)
        self._check(self.lib.dv_erode(self.h, _ptr(mask), w, h, mask.strides[0], int(k), _ptr(out), DV_MEM_HOST))
        return out

    def lift_projective(self, cam, pts, offset=(0.0, 0.0)):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        out = np.zeros_like(pts)
        if len(pts):
            self._check(self.lib.dv_lift_projective_offset(self.h, C.byref(cam), _ptr(pts), len(pts), float(offset[0]), float(offset[1]), _ptr(out), DV_MEM_HOST))
        return out

    # ---- measurement ----
    def undistort_lines(self, cam, segs_px):
        """FrameLines::UndistortedLineEndPoints: [n, 4] pixel end points (x1 y1 x2 y2, float32) -> [n, 4] normalised undistorted, float64"""
        segs = np.ascontiguousarray(segs_px, np.float32).reshape(-1, 4)
        out = np.zeros((len(segs), 4), np.float64)
        if len(segs):
            self._check(self.lib.dv_undistort_lines(self.h, C.byref(cam), segs.ctypes.data, len(segs), out.ctypes.data))
        return out

    def timing_enable(self, on=1):
        self._check(self.lib.dv_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._check(self.lib.dv_timing_reset(self.h))

    def timing_get(self, name):
        ms, cnt = C.c_double(0), C.c_longlong(0)
        self._check(self.lib.dv_timing_get(self.h, name.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value


class FeatureTracker:
    """Mirror of dynamic_vins::FeatureTracker (front_end/background_tracker.h:41-88).

    TrackImage / TrackImageNaive return the FeatureBackground.points map:
        {id: [(0, [x,y,1,u,v,vx,vy]), (1, [...right...])]}
    camelCase aliases (VINS-Fusion spelling used by BASELINE.json) are provided.
    """

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.cur_time = 0.0

    @staticmethod
    def _to_map(rows):
        pts = {}
        for r in rows:
            obs = [(0, np.array(r["left"]))]
            if r["has_right"]:
                obs.append((1, np.array(r["right"])))
            pts[int(r["id"])] = obs
        return pts

    def TrackImage(self, gray0, gray1, time0):
        self.cur_time = time0
        self.rows = self.ctx.track_stereo(gray0, gray1, time0, None, DV_MODE_RAW)
        return self._to_map(self.rows)

    def TrackImageNaive(self, gray0, gray1, time0, inv_merge_mask=None):
        self.cur_time = time0
        self.rows = self.ctx.track_stereo(gray0, gray1, time0, inv_merge_mask, DV_MODE_NAIVE)
        return self._to_map(self.rows)

    def TrackSemanticImage(self, gray0, gray1, time0, inv_merge_mask=None):
        """background half of dynamic mode (background_tracker.cpp:757-837)"""
        self.cur_time = time0
        self.rows = self.ctx.track_stereo(gray0, gray1, time0, inv_merge_mask, DV_MODE_SEMANTIC)
        return self._to_map(self.rows)

    trackImage = TrackImage
    trackImageNaive = TrackImageNaive


class InstFeat:
    """Mirror of dynamic_vins::InstFeat for ONE object instance as InstsFeatManager::InstsTrack drives it
    (front_end/dynamic_tracker.cpp:348-470, front_end/instance_feature.cpp): ROI-local LK on zero-padded crops,
    Shi-Tomasi top-up inside the eroded instance mask, undistortion with the 2-D box offset, right-image LK on the
    full frames.  Host composition of the C-ABI operators (dv_track_by_lk, dv_erode, dv_circle_mask, dv_gftt,
    dv_lift_projective_offset); every pixel / index result is bit-exact against the oracle's dvo_inst_track.
    The VIODE segmentation-key test of TrackRightByPad is applied when the key image of the right frame (Context.viode_mask) is given."""

    global_id_count = 1        # InstFeat::global_id_count (static, shared with the background tracker in the reference)

    def __init__(self, ctx: Context, cam0, cam1, max_cnt=50, min_dist=4, flow_back=True):
        self.ctx, self.cam0, self.cam1 = ctx, cam0, cam1
        self.max_cnt, self.min_dist, self.flow_back = max_cnt, min_dist, flow_back      # max_dynamic_cnt, min_dynamic_dist, flow_back
        self.last_points = np.zeros((0, 2), np.float32)
        self.ids = np.zeros(0, np.uint32)
        self.track_cnt = np.zeros(0, np.int32)
        self.prev_roi_gray = None

    def Track(self, roi_gray, roi_mask, box_tl, gray0, gray1=None, seg1_keys=None, key=None):
        """one frame; returns dict(curr_points, ids, track_cnt, curr_un_points, right_points, right_ids, right_un_points)"""
        ctx = self.ctx
        roi_gray = np.ascontiguousarray(roi_gray)
        curr, ids, cnt = np.zeros((0, 2), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.int32)
        if self.prev_roi_gray is not None and len(self.last_points):
            h = max(self.prev_roi_gray.shape[0], roi_gray.shape[0]); w = max(self.prev_roi_gray.shape[1], roi_gray.shape[1])
            a = np.zeros((h, w), np.uint8); b = np.zeros((h, w), np.uint8)          # InstanceImagePadding (feature_utils.cpp:406-413)
            a[: self.prev_roi_gray.shape[0], : self.prev_roi_gray.shape[1]] = self.prev_roi_gray
            b[: roi_gray.shape[0], : roi_gray.shape[1]] = roi_gray
            pts, st = ctx.track_by_lk(a, b, self.last_points, self.flow_back, 0.5)   # InstFeat::TrackLeft, no mask
            keep = st > 0
            curr, ids, cnt = pts[keep], self.ids[keep], self.track_cnt[keep] + 1
        if len(curr) < self.max_cnt:
            m = ctx.erode(np.ascontiguousarray(roi_mask), 5) if roi_mask is not None else np.full(roi_gray.shape, 255, np.uint8)
            if len(curr):
                m = ctx.circle_mask(m, curr, self.min_dist)
            new = ctx.gftt(roi_gray, self.max_cnt - len(curr), 0.01, self.min_dist, m)
            if len(new):
                nid = np.arange(InstFeat.global_id_count, InstFeat.global_id_count + len(new), dtype=np.uint32)
                InstFeat.global_id_count += len(new)
                curr = np.concatenate([curr, new]); ids = np.concatenate([ids, nid]); cnt = np.concatenate([cnt, np.ones(len(new), np.int32)])
        un = ctx.lift_projective(self.cam0, curr, offset=box_tl)                   # UndistortedPointsWithAddOffset
        out = dict(curr_points=curr, ids=ids, track_cnt=cnt, curr_un_points=un, right_points=np.zeros((0, 2), np.float32),
                   right_ids=np.zeros(0, np.uint32), right_un_points=np.zeros((0, 2), np.float32))
        if gray1 is not None and len(curr):                                         # TrackRightByPad
            padded = (curr + np.array(box_tl, np.float32)).astype(np.float32)
            rp, st = ctx.track_by_lk(gray0, gray1, padded, self.flow_back, 0.5)
            if seg1_keys is not None:                                              # VIODE::PixelToKey(right_points[i], img.seg1) != id -> lost
                xi = np.rint(rp[:, 0]).astype(int).clip(0, seg1_keys.shape[1] - 1); yi = np.rint(rp[:, 1]).astype(int).clip(0, seg1_keys.shape[0] - 1)
                st = np.where((st > 0) & (seg1_keys[yi, xi] == key), 1, 0).astype(np.uint8)
            keep = st > 0
            out["right_points"], out["right_ids"] = rp[keep], ids[keep]
            out["right_un_points"] = ctx.lift_projective(self.cam1, rp[keep])
        self.last_points, self.ids, self.track_cnt, self.prev_roi_gray = curr, ids, cnt, roi_gray      # PostProcess
        return out
