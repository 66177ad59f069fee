/*
 * dvins.h — C ABI of libdvins_hip.so: the MI355X (gfx950) implementation of dynamic_vins'
 * hot path (front-end feature tracking + sliding-window bundle adjustment).
 *
 * The reference has no plugin/FFI layer: its seam is the two C++ classes FeatureTracker
 * (dynamic_vins/src/front_end/background_tracker.h:41-88) and Estimator
 * (dynamic_vins/src/estimator/estimator.h:55-164).  The header-only C++ shims in
 * dynamic_vins_amd/host/ keep those class signatures and call the entry points below; a
 * reference maintainer swaps the bodies of the cited functions for these calls
 * (INTEGRATION.md shows the binding).
 *
 * Conventions: every function returns 0 on success, <0 on error (message via
 * dv_last_error); no exceptions cross the ABI; the caller owns every buffer it passes;
 * the ctx owns device memory and streams; one ctx per thread.  Image/point buffers are host
 * memory when mem == DV_MEM_HOST and device (HBM) memory when mem == DV_MEM_DEVICE.
 */
#ifndef DVINS_H
#define DVINS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DV_MEM_HOST   0
#define DV_MEM_DEVICE 1
/* dv_track_stereo* / dv_batch_track_enqueue / dv_seq_input::mem / dv_seq_dynamic::mask_mem: host memory the CALLER has pinned and mapped for the device
 * (hipHostMalloc, or hipHostRegister with hipHostRegisterMapped).  The kernels read it over PCIe directly — no staging copy, no copy engine in the per-frame
 * path; the buffers must stay unchanged until the frame is collected, as device buffers must. */
#define DV_MEM_PINNED 2
/* pinned + device-mapped host memory for DV_MEM_PINNED buffers, for hosts that do not link the HIP runtime themselves (hipHostMalloc / hipHostFree); NULL on failure */
void* dv_pinned_alloc(size_t bytes);
void dv_pinned_free(void* p);
/* OR into `mem` of dv_track_stereo*: gray0 / gray1 point to 8-bit BGR frames (stride in bytes, >= 3 w); they are converted with
 * cv::cvtColor's fixed-point weights straight into pyramid level 0 (SemanticImage::SetGrayImageGpu, basic/semantic_image.cpp:103-118).
 * A mask, if given, is single-channel with stride w. */
#define DV_FMT_BGR    0x100

#define DV_MODE_RAW   0   /* FeatureTracker::TrackImage      (background_tracker.cpp:52-158)  */
#define DV_MODE_NAIVE 1   /* FeatureTracker::TrackImageNaive (background_tracker.cpp:400-516): both trackings by FeatureTrackByLKGpu */
#define DV_MODE_SEMANTIC 2 /* FeatureTracker::TrackSemanticImage (background_tracker.cpp:757-837): the background half of dynamic mode —
                             temporal tracking by FeatureTrackByLK (dist <= 0.5), right image by FeatureTrackByLKGpu (the GPU tracker, dist <= 1.0) */

#define DV_MAX_FEATS 1024 /* device capacity for tracked points per tracker */

typedef struct dv_ctx dv_ctx;

/* camodocal::PinholeCamera parameters (camera_models/src/camera_models/PinholeCamera.cc:292-295) */
typedef struct dv_cam { double fx, fy, cx, cy, k1, k2, p1, p2; } dv_cam;

/* fe_para (front_end/front_end_parameters.cpp:18-40) + cfg::is_stereo (utils/parameters.cpp) */
typedef struct dv_config {
    int width, height;      /* image_width / image_height */
    int max_cnt;            /* max_cnt   -> fe_para::kMaxCnt  */
    int min_dist;           /* min_dist  -> fe_para::kMinDist */
    int flow_back;          /* flow_back -> fe_para::is_flow_back */
    int stereo;             /* num_of_cam == 2 */
    dv_cam cam0, cam1;
    int device;             /* HIP device ordinal (LOCAL_RANK for one-process-per-GPU) */
    int mask_morphology_size; /* > 0: the inverse instance mask is eroded by a k x k rectangle first (use_mask_morphology /
                                 mask_morphology_size, background_tracker.cpp:408-416,764-768); naive / semantic modes only */
    int reserved[6];
} dv_config;

/* One tracked feature = one entry of FeatureBackground::points
 * (basic/frontend_feature.h:34-44): id -> [(0, left Vec7d), (1, right Vec7d)] */
typedef struct dv_feat {
    uint32_t id;
    int32_t  track_cnt;
    int32_t  has_right;
    int32_t  pad_;
    double   left[7];       /* x_n, y_n, 1, u, v, vx, vy (background_tracker.cpp:347-355) */
    double   right[7];
} dv_feat;

/* ---- lifetime ---- */
dv_ctx*     dv_create(const dv_config* cfg);      /* NULL on failure; dv_last_error(NULL) */
void        dv_destroy(dv_ctx* ctx);
const char* dv_last_error(dv_ctx* ctx);
/* resets tracker state (ids, previous frame); Estimator::ClearState analogue for the front end */
int         dv_reset(dv_ctx* ctx);
int         dv_sync(dv_ctx* ctx);                 /* block until all work queued on the ctx is done */

/* ---- front end: whole-frame entry (replaces the body of FeatureTracker::TrackImage /
 * TrackImageNaive, background_tracker.cpp:52-158 / 400-516).  gray0/gray1: CV_8UC1 rows of
 * `stride` bytes.  mask_or_null: inv_merge_mask (0 = object) for DV_MODE_NAIVE, already eroded.
 * out: >= max_cnt rows (host memory always); *n_out = rows written. */
int dv_track_stereo(dv_ctx* ctx, const uint8_t* gray0, const uint8_t* gray1, int w, int h, int stride,
                    double t, const uint8_t* mask_or_null, int mode, int mem, dv_feat* out, int* n_out);
/* asynchronous split of the same call: enqueue the frame, later collect its output.  Lets the
 * caller overlap frame k+1's tracking with frame k's bundle adjustment (the reference does this
 * with two threads, system/main.cpp:178,394-404). */
int dv_track_stereo_enqueue(dv_ctx* ctx, const uint8_t* gray0, const uint8_t* gray1, int w, int h, int stride,
                            double t, const uint8_t* mask_or_null, int mode, int mem);
int dv_track_stereo_collect(dv_ctx* ctx, dv_feat* out, int* n_out);
struct dv_inst_det;
/* para::is_static_inst_as_background (default true, estimator/vio_parameters.h:86) — FeatureTrack, system/main.cpp:217-245: before TrackSemanticImage the pixels of
 * every visible instance the estimator reported static (dv_est_get_static_instances) are taken OUT of the merged instance mask, so the background tracker may pick
 * features on parked objects: merge_mask(row + rect.y, col + rect.x) = 0 where the instance's ROI mask is set, inv_merge_mask = ~merge_mask.
 * For the NEXT dv_track_stereo_enqueue (which must carry a mask): dets = the frame's detections (rect + ROI mask, host memory, valid until that call), static_ids =
 * the estimator's list.  Detections whose track_id is not in the list are left alone; n_static 0 cancels.  The caller's mask is not written to. */
int dv_track_unmask_static(dv_ctx* ctx, const struct dv_inst_det* dets, int n_dets, const uint32_t* static_ids, int n_static);
/* The same step of FeatureTrack (system/main.cpp:217-245) from the frame's KEY IMAGE instead of host ROI masks: the ROI mask of detection d is, by definition,
 * key_image[y + d.y][x + d.x] == d.track_id over its rectangle (what VIODE::SetViodeMaskAndRoi cuts, utils/dataset/viode_utils.cpp:177-218), compared on the device;
 * dv_inst_det::mask is ignored.  key_image: w x h uint32 (dv_viode_mask's / dv_viode_frame_collect's), rows of stride_bytes (0 = 4 w), mem = DV_MEM_HOST (staged once by
 * the enqueue; valid until that call returns), DV_MEM_DEVICE or DV_MEM_PINNED (read in place; valid until the frame is collected).  Every rectangle is checked against the
 * image before a job is staged.  Applies to the NEXT dv_track_stereo_enqueue, as dv_track_unmask_static does, and EVERY return of that call, 0 or -1, drops the staged
 * jobs (so does dv_batch_track_enqueue for the members handed in: such a member keeps its own launches in that round). */
int dv_track_unmask_static_keys(dv_ctx* ctx, const struct dv_inst_det* dets, int n_dets, const uint32_t* static_ids, int n_static, const uint32_t* key_image, int stride_bytes, int mem);

/* ---- front end: operator-level entries ---- */
/* cv::calcOpticalFlowPyrLK(img_a,img_b,pts_a,pts_b,status,err,Size(21,21),max_level,
 *   TermCriteria(COUNT+EPS,iters,eps), use_initial ? OPTFLOW_USE_INITIAL_FLOW : 0)
 * call sites: front_end/feature_utils.cpp:43,50.  pts: interleaved float (x,y). */
int dv_lk(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride,
          const float* pts_a, int n, int max_level, int iters, double eps, int use_initial,
          float* pts_b, uint8_t* status, int mem);
/* FeatureTrackByLK (front_end/feature_utils.cpp:35-69): fwd LK + bwd LK + distance + InBorder */
int dv_track_by_lk(dv_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride,
                   const float* pts1, int n, int flow_back, float dist_thresh,
                   float* pts2, uint8_t* status, int mem);
/* The reference's GPU tracker, used by dv_track_stereo* where the reference uses it (DV_MODE_NAIVE: temporal + right image; DV_MODE_SEMANTIC: right image):
 * cv::cuda::SparsePyrLKOpticalFlow::create(Size(21, 21), 3, 30[, useInitialFlow])->calc (front_end/background_tracker.cpp:34-36) — float patches sampled bilinearly,
 * Scharr derivatives on the fly, no minimum-eigenvalue test, its own pyramid (cuda::pyrDown) — and FeatureTrackByLKGpu (front_end/feature_utils.cpp:83-163: forward,
 * backward from the previous points, |p - p_rev| <= 1.0, InBorder).  Operator forms; the ctx must not be tracking a sequence. */
int dv_lk_cuda(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride, const float* pts_a, int n, int max_level, int iters, int use_initial,
               float* pts_b, uint8_t* status, int mem);
int dv_track_by_lk_gpu(dv_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride, const float* pts1, int n, int flow_back,
                       float* pts2, uint8_t* status, int mem);
int dv_pyr_down_cuda(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, int mem);      /* cuda::pyrDown, 8-bit: the same sums as cv::pyrDown, rounded half to even */
/* cv::goodFeaturesToTrack(img, out, max_n, quality, min_dist, mask) call sites:
 * background_tracker.cpp:85,238; instance_feature.cpp:381; dynamic_tracker.cpp:435
 * Limits (dv_gftt, dv_gftt_cuda and the detector inside dv_track_stereo*): an input beyond one of them is refused with an error that names the flag
 * ("device error flags=N", N the sum of the flags raised), nothing is returned for it, and the context stays usable.
 *   flag 1  more candidates (interior, unmasked pixels with a non-zero response that is >= its eight neighbours) than the context's candidate buffer holds:
 *           max(4096, w * h / 4) of the largest image the context has processed so far (the buffer only grows);
 *   flag 2  min_dist >= 1 and ceil(w / c) * ceil(h / c) > 32768 grid cells, c = min_dist rounded half to even (320 x 240 at min_dist 1 has 76800);
 *           min_dist < 1 uses no grid and has no such limit;
 *   flag 4  the selection, taking the 2048 equal bins between the quality threshold and the maximum from the top, reaches a bin with more than 8192
 *           candidates before max_n corners are accepted (many exactly equal responses: a 4 px checkerboard over 320 x 240); a request that is
 *           met from the bins above such a bin is served.  Inside dv_track_stereo* the refused frame keeps the corners the bins above gave and takes none from
 *           that bin on: the tracker's state behind a refused frame is the same in every run.
 * At most 1024 corners are returned (max_n <= 0: 1024). */
int dv_gftt(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride,
            int max_n, double quality, double min_dist, float* out_xy, int* n_out, int mem);
/* cv::cornerMinEigenVal(img, eig, 3, 3) (inside goodFeaturesToTrack) */
int dv_min_eigen(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem);
/* The reference's GPU corner detector, used by dv_track_stereo* where the reference uses it (DV_MODE_NAIVE only: DetectNewFeature(img, use_gpu = true, ...),
 * front_end/background_tracker.cpp:445 -> front_end/instance_feature.cpp:372-379 -> DetectShiTomasiCornersGpu, front_end/feature_utils.cpp:339-348):
 * cv::cuda::createGoodFeaturesToTrackDetector(CV_8UC1, max_n, quality, min_dist)->detect(img, out, mask).  Against dv_gftt: the response map is the GPU module's
 * (float multiply-add chains, block sums inside the eigenvalue kernel), the quality threshold comes from the maximum over the WHOLE image (the CPU detector takes
 * it under the mask), candidates are eig > threshold && eig == max of the raw 3 x 3 neighbourhood; the ordering and the minimum-distance grid are the same.
 * dv_min_eigen_cuda: cv::cuda::createMinEigenValCorner(CV_8UC1, 3, 3)->compute.  Operator forms. */
int dv_gftt_cuda(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride,
                 int max_n, double quality, double min_dist, float* out_xy, int* n_out, int mem);
int dv_min_eigen_cuda(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem);
/* cv::pyrDown (inside buildOpticalFlowPyramid); dst is ((w+1)/2) x ((h+1)/2), tightly packed */
int dv_pyr_down(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, int mem);
/* VIODE segmentation image -> instance masks (VIODE::SetViodeMaskSimple / BuildViodeMask, utils/dataset/viode_utils.cpp:21-170).
 * key(pixel) = r*1000000 + g*1000*b (viode_utils.h:23-26, sic); a pixel is an object pixel if its key is in dyn_keys[nkeys <= 64].
 * merge_mask: 255 = object; inv_merge_mask: its complement (what TrackImageNaive / TrackSemanticImage take); key_image (optional,
 * w*h uint32): the key of every pixel (PixelToKey lookups of TrackRightByPad); boxes[nkeys][4] = row_min,row_max,col_min,col_max of
 * each key's pixels, -1 if absent (InstanceSimple).  Host buffers, tightly packed outputs. */
int dv_viode_mask(dv_ctx* ctx, const uint8_t* seg_bgr, int w, int h, int stride, const uint32_t* dyn_keys, int nkeys,
                  uint8_t* merge_mask, uint8_t* inv_merge_mask, uint32_t* key_image, int32_t* boxes);
/* Thread T1's stage of ONE frame of a VIODE-style stream (label image in, instances out) without a host round trip of pixels: ImageProcessor::Run
 * (image_process/image_process.cpp:161-178) -> VIODE::SetViodeMaskAndRoi (utils/dataset/viode_utils.cpp:21-218), as FeatureTrack consumes it (system/main.cpp:196-250).
 * _enqueue runs dv_viode_mask's kernel on the LEFT label image and, if given, on the RIGHT one (whose key image TrackRightByPad tests, front_end/instance_feature.cpp:263-268)
 * on the ctx's stream, into device buffers the LIBRARY owns, and records an event.  seg*_bgr: 8-bit B G R, size of the config, rows of `stride` bytes (0 = 3 w), mem =
 * DV_MEM_HOST (staged; valid until the frame is collected), DV_MEM_DEVICE or DV_MEM_PINNED (read in place).  dyn_keys[nkeys], 1 <= nkeys <= 64, host memory.
 * _collect waits for that event and builds the frame's detections by the rule dvins_node and dynamic_vins_amd/viode.py detections() share: one per key present, ASCENDING
 * key, rect = cv::Rect(min_pt, max_pt) (max row / column excluded), rectangles under min_inst_size pixels on a side dropped, track_id = key, class 0, mask = points = NULL.
 * It hands back the device pointers of that frame's inverse merged mask (w x h bytes, tightly packed: give it to dv_track_stereo_enqueue with DV_MEM_DEVICE beside frames
 * of row stride w) and of its two key images (w x h uint32, tightly packed; keys1 NULL without a right image): for dv_inst_track_enqueue_keys,
 * dv_track_unmask_static_keys and dv_inst_set_right_keys.  The buffers exist twice and alternate: those of frame k stay intact while frame k + 1 is enqueued and until
 * frame k + 2 is; the caller never frees them.  One frame may be in flight: _enqueue twice without _collect is refused.
 * The ONLY device -> host traffic per frame is nkeys x 16 bytes of boxes (into pinned memory): the host needs them because the object tracker's job tables are sized
 * from the rectangles.  dv_viode_mask itself is unchanged. */
struct dv_inst_det;
int dv_viode_frame_enqueue(dv_ctx* ctx, const uint8_t* seg0_bgr, const uint8_t* seg1_bgr_or_null, int w, int h, int stride, int mem, const uint32_t* dyn_keys, int nkeys);
int dv_viode_frame_collect(dv_ctx* ctx, int min_inst_size, struct dv_inst_det* dets, int cap, int* n_dets, const uint8_t** inv_mask_dev, const uint32_t** keys0_dev, const uint32_t** keys1_dev);
/* Thread T1's stage of ONE frame whose instances arrive as a detector's MASK STACK (ImageProcessor::Run's detector branch, image_process/image_process.cpp:160-170):
 * N planes of the configured image size, one per instance, as the segmentation network leaves them on the device.  It covers Detector2D::Launch's
 * `seg_label > kSoloMaskThr` (det2d/detector2d.cpp:441; DV_STACK_F32 only), BuildBoxes2D (det2d/detector2d.cpp:58-97) and the mask half of SemanticImage::SetMaskAndRoi /
 * SetBackgroundMask (basic/semantic_image.cpp:20-93).
 * A pixel BELONGS to a plane by the reference's rule mask_tensor.to(kInt8).abs().clamp(0, 1):
 *   DV_STACK_U8   the thresholded bool / uint8 tensor.  Established with the CPU build, 2.10, of the reference's tensor library (csrc/inst_stack_host.h; scalar and vectorised paths agree over all 256 values): bytes 1..127 -> int8
 *                 1..127 -> 1; bytes 129..255 -> int8 -127..-1 -> abs 127..1 -> 1; byte 128 -> int8 -128, whose abs WRAPS to -128, clamp(0, 1) -> 0.  So 1, 127, 129 and
 *                 255 are object pixels and 128 is NOT: belongs = (byte != 0 && byte != 128).  Implemented bug for bug.
 *   DV_STACK_F32  the detector's soft masks: element > threshold (strict, float compare: NaN is not an object pixel), then the same rule on the resulting 0 / 1.
 * row_stride / plane_stride in BYTES (0 = tight: width * element size, row_stride * height); DV_STACK_F32 wants data and both strides multiples of 4.  mem = DV_MEM_HOST
 * (staged by dv_inst_stack_frame_enqueue; valid until the frame is collected), DV_MEM_DEVICE or DV_MEM_PINNED (read in place; must stay valid until the frame's TRACKING is
 * collected when the stack also goes to dv_inst_track_enqueue_planes / dv_track_unmask_static_planes). */
#define DV_STACK_U8  0
#define DV_STACK_F32 1
#define DV_STACK_MAX_PLANES 64
typedef struct dv_mask_stack {
    const void* data; int32_t n_planes /* 1..64 */, kind /* DV_STACK_* */, mem /* DV_MEM_* */, row_stride; int64_t plane_stride; float threshold /* DV_STACK_F32 */; int32_t reserved;
} dv_mask_stack;
/* _enqueue: ONE kernel pass over the stack on the ctx's stream (every lane reads 4 consecutive pixels of every plane — a dword, or 16 bytes of floats — keeps the OR in
 * registers and writes the two masks once) into device buffers the LIBRARY owns: the merged mask (255 where any plane has the pixel: sum(0).clamp(0, 1) * 255), its inverse,
 * and per plane the box row_min, row_max, col_min, col_max of its pixels (BuildBoxes2D's min / max of nonzero()).  The buffers exist twice and alternate exactly as
 * dv_viode_frame_*'s do: those of frame k stay intact while frame k + 1 is enqueued and until frame k + 2 is.  The ONLY device -> host traffic is n_planes x 16 bytes of
 * boxes into pinned memory.  flags: DV_STACK_REMAP_MERGED = SemanticImage::SetBackgroundMask's extra step (slam_type naive, basic/semantic_image.cpp:85-92): the merged mask
 * goes through cv::remap(left maps, INTER_LINEAR), BORDER_CONSTANT 0 — dv_remap's rule — before it is inverted, inv = ~remap(merged); it needs installed undistortion maps
 * (dv_undistort_setup / dv_set_undistort_maps) and is refused without them.  SetMaskAndRoi (slam_type dynamic) does not remap, and neither does flags = 0.
 * One frame may be in flight: _enqueue twice without _collect is refused.
 * _collect waits for the stage and returns, per NON-EMPTY plane in ASCENDING plane order, a dv_inst_det: rect = cv::Rect(min_pt, max_pt) — max row / column excluded, as
 * Box2D::rect is built at det2d/detector2d.cpp:89 —, rectangles under min_inst_size pixels on a side dropped, track_id = the plane index (Box2D::id = i), class 0,
 * mask = points = NULL; planes[i] = the plane of dets[i].  The caller (its multi-object tracker stays upstream) overwrites track_id / class_id before the next step.  An EMPTY
 * plane is where the reference would throw (the tensor library's max of an empty tensor, det2d/detector2d.cpp:64-66); here it yields no detection.  inv_mask_dev / merge_mask_dev (either may
 * be NULL): the frame's inverse merged mask and merged mask, w x h bytes, tightly packed, device memory (with DV_STACK_REMAP_MERGED the merged mask is the remapped one). */
#define DV_STACK_REMAP_MERGED 1
int dv_inst_stack_frame_enqueue(dv_ctx* ctx, const dv_mask_stack* stack, int w, int h, int flags);
int dv_inst_stack_frame_collect(dv_ctx* ctx, int min_inst_size, struct dv_inst_det* dets, int32_t* planes, int cap, int* n_dets, const uint8_t** inv_mask_dev, const uint8_t** merge_mask_dev);
/* The detector's HEAD for ONE frame: the SOLOv2 network's output tensors -> the instance-mask stack above, on the device.  It restates Solov2::GetSegTensor
 * (det2d/solo_head.cpp:410-559) with Solov2::MatrixNMS (det2d/solo_head.cpp:31-71), the step Detector2D::ForwardTensor runs behind the network
 * (det2d/detector2d.cpp:245-280), AS THE REFERENCE EVALUATES IT; the network itself (TensorRT) stays with the caller, and so does BuildBoxes2D's COCO -> KITTI naming.
 * dv_solo_outputs: per level, in the order the reference concatenates them (outputs[0 .. n_levels - 1], then the category maps), the kernel map [channels, g, g], the
 * category map [n_classes, g, g] and g; then the mask feature [channels, fh, fw].  float32, tightly packed, one memory kind (DV_MEM_DEVICE / DV_MEM_PINNED read in
 * place and valid until the frame is collected; DV_MEM_HOST staged by the enqueue).  channels 1..256, n_classes 1..128, g 1..64, fh * fw <= 2^20.
 * The rule, step by step:
 *   candidates   the cells with cate > score_thr (strict) in nonzero() order: row-major over [cell, class], cells concatenated level by level (an ordered scan).
 *                More than max_candidates of them: the frame FAILS (collect returns < 0 with a message, no planes) — never a silent truncation.
 *   pixel floor  stride(cell) = strides[i] for the first i with cell < num_grids[0]^2 + .. + num_grids[i]^2, else 1, where `cell` is the index into the CONCATENATED
 *                cells and i runs over n_levels entries.  The boundaries depend only on num_grids[], never on the levels' own g: the reference concatenates in the order
 *                of kTensorQueueShapes (grids 12, 16, 24, 36, 40) and builds the boundaries from kSoloNumGrids (40, 36, 24, 16, 12), so with its own tables the first
 *                1600 cells get stride 8 whatever level they came from (solo_head.cpp:24-28,454-465).  Kept as it is.
 *   masks        seg = sigmoid(kernel . feature) (float32 in, float32 accumulate), mask = seg > mask_thr, sum_mask = the mask's pixels as float; kept when
 *                sum_mask > stride; score = cate * (sum(seg * mask) / sum_mask).
 *   sort         descending, the first nms_pre; equal scores in candidate order (the reference's argsort leaves ties open).
 *   Matrix NMS   iou = inter / (sum_i + sum_j - inter) from the masks' inner products, upper triangle, same-label pairs only; compensation = the column maximum; decay =
 *                the minimum over ALL rows i (not only i < j) of exp(-sigma iou^2) / exp(-sigma comp_i^2) (DV_SOLO_NMS_GAUSSIAN) or (1 - iou) / (1 - comp_i)
 *                (DV_SOLO_NMS_LINEAR), NaN carried as the tensor library's min carries it.
 *   second sort  kept when score * decay >= update_thr; descending, the first max_per_img; ties in the order of the first sort.
 *   resampling   bilinear align_corners = true to (4 fh, 4 fw), crop [rect_y : rect_y + rect_h, rect_x : rect_x + rect_w], bilinear align_corners = true to
 *                (origin_h, origin_w), plane = value > mask_thr.  Source coordinates and weights in float32 as upsample_bilinear2d forms them (scale = (in - 1) / (out - 1),
 *                src = scale * dst, weights from the fractional part); the 4 x intermediate is never stored.
 * No candidate, none over the pixel floor, none over update_thr: ZERO planes, not an error (the reference's three early returns).
 * Limits: max_candidates <= 4096, nms_pre <= 512, max_per_img <= 128.  DV_STACK_MAX_PLANES is 64 while the reference's YAML asks for max_per_img 100: collect reports all
 * n survivors (labels, scores, planes in memory) but the dv_mask_stack it fills names the first min(n, 64) planes — the highest scores.
 * dv_solo_rect: Pipeline::GetXYWHS (det2d/pipeline.cpp:23-48), the image's rectangle inside the network input, with its round-up to even.  Host code, no ctx.
 * dv_solo_check: the refusals of dv_solo_head_enqueue without a device (0, or < 0 with dv_last_error(NULL)).
 * _enqueue: everything on the ctx's stream into buffers the LIBRARY owns; the output planes exist twice and alternate as dv_inst_stack_frame_*'s buffers do, so frame
 * k + 1's head may be enqueued behind frame k's tracking.  One frame may be in flight.  Counts stay on the device between the kernels.
 * _collect: waits, returns n (all survivors), *n_candidates, labels[min(n, cap)] / scores[min(n, cap)] (the frame's only device -> host traffic, through pinned memory) and
 * fills *stack: DV_STACK_U8 (0 / 1), DV_MEM_DEVICE, rows of origin_w bytes padded to a multiple of 4 (padding zero), n_planes = min(n, 64) — 0 for a frame without
 * instances, which dv_inst_stack_frame_enqueue refuses: skip the stage for such a frame. */
#define DV_SOLO_MAX_LEVELS 5
#define DV_SOLO_NMS_GAUSSIAN 0
#define DV_SOLO_NMS_LINEAR 1
#define DV_SOLO_MAX_CANDIDATES 4096
#define DV_SOLO_MAX_NMS_PRE 512
#define DV_SOLO_MAX_PER_IMG 128
typedef struct dv_solo_outputs {
    int32_t n_levels /* 1..5 */, channels, n_classes, mem /* DV_MEM_* */;
    const float* kernel[DV_SOLO_MAX_LEVELS]; const float* cate[DV_SOLO_MAX_LEVELS]; int32_t grid[DV_SOLO_MAX_LEVELS];
    int32_t fh, fw, reserved; const float* feature;
} dv_solo_outputs;
typedef struct dv_solo_params {
    float score_thr, mask_thr, update_thr, nms_sigma;
    int32_t nms_pre, max_per_img, nms_kernel /* DV_SOLO_NMS_* */, max_candidates;
    int32_t num_grids[DV_SOLO_MAX_LEVELS]; float strides[DV_SOLO_MAX_LEVELS];
    int32_t rect_x, rect_y, rect_w, rect_h, origin_w, origin_h;
} dv_solo_params;
int dv_solo_rect(int model_w, int model_h, int img_w, int img_h, int* rect_x, int* rect_y, int* rect_w, int* rect_h);
int dv_solo_check(const dv_solo_outputs* out, const dv_solo_params* par);
int dv_solo_head_enqueue(dv_ctx* ctx, const dv_solo_outputs* out, const dv_solo_params* par);
int dv_solo_head_collect(dv_ctx* ctx, int32_t* labels, float* scores, int cap, int* n, int* n_candidates, dv_mask_stack* stack);
/* The detector's INPUT for ONE frame: the colour frame -> the network's normalised, resized, zero-padded [3, model_h, model_w] float32 tensor, on the device.  It restates
 * Pipeline::ImageToTensor (det2d/pipeline.cpp:370-387, called at image_process/image_process.cpp:138) followed by Pipeline::ProcessInput (det2d/pipeline.cpp:204-232,
 * called at det2d/detector2d.cpp:249), the step in front of the network; the network itself stays with the caller.  The frame is the ctx's width x height, 8-bit BGR with
 * `stride` bytes per row, as ImageToTensor receives it (where the reference undistorts, the frame after its remap: dv_remap).  In this order:
 *   swap         plane c of the tensor reads byte 2 - c of a pixel (BGR -> RGB), as float.
 *   normalise    (v - mean[c]) / std[c] in float32, IEEE division; mean / std in RGB order (det2d/det2d_parameter.h:24-25: 123.675, 116.28, 103.53 / 58.395, 57.12, 57.375).
 *   resample     bilinear, align_corners = true, to rect_h x rect_w of dv_solo_rect, by upsample_bilinear2d's float32 rule: per axis scale = float(in - 1) / float(out - 1),
 *                r = scale * dst, i0 = int(r), i1 = i0 + (i0 < in - 1), l1 = r - i0, l0 = 1 - l1; value = lh0 (lw0 p00 + lw1 p01) + lh1 (lw0 p10 + lw1 p11).  A declared
 *                choice of evaluation: float32 nested differences, top = p00 + lw1 (p01 - p00), bot likewise, top + lh1 (bot - top) — the same value within 1.6e-6 of
 *                its exact evaluation (derivation: csrc/solo_input_host.h), and the form in which an upper weight of 0 returns the sample's bits and an image of
 *                constant colour returns the constant's bits (the sum of products with a rounded 1 - l1 leaves such an image up to one ulp off, as the tensor
 *                library's own kernels do).
 *   pad          +0.0 everywhere outside the rectangle (the reference pads with zeros, not with the mean colour).
 * Refused, each with its own dv_last_error text: non-positive sizes (sides above 16384 too); an image or rectangle side under 2; a zero std, a non-finite mean or std; a
 * stride under 3 * width; a rectangle with model_h - rect_h or model_w - rect_w odd — there the reference concatenates two pads of (model - rect) / 2 and hands the network
 * a tensor one row or column short (the rectangle's side is even, so that is every odd model side in the padded direction); an unknown memory kind.
 * dv_solo_input_check: those refusals without a device (0, or < 0 with dv_last_error(NULL)).
 * _enqueue: ONE kernel on the ctx's stream writes EVERY element of the tensor (nothing relies on an earlier clear).  mem = DV_MEM_HOST (the frame is staged) or
 * DV_MEM_DEVICE / DV_MEM_PINNED (read in place, any base alignment, valid until the collect).  dst_dev = NULL: one of two library-owned buffers used alternately — the
 * pointer _collect returns stays valid until the SECOND enqueue after it (as long as the model size does not grow), so frame k + 1's input is built while the caller's
 * network still reads frame k's.  dst_dev != NULL: a caller-owned device buffer of 3 * model_h * model_w floats (the network's own binding), 4-byte aligned, no more.
 * One frame may be in flight.  _collect waits for the stage and returns the tensor's device pointer and the rectangle (any of the five may be NULL). */
typedef struct dv_solo_input_params { int32_t model_w, model_h; float mean[3], std[3]; } dv_solo_input_params;
int dv_solo_input_check(int img_w, int img_h, int stride, const dv_solo_input_params* par);
int dv_solo_input_enqueue(dv_ctx* ctx, const uint8_t* bgr, int stride, int mem, const dv_solo_input_params* par, float* dst_dev);
int dv_solo_input_collect(dv_ctx* ctx, const float** input_dev, int* rect_x, int* rect_y, int* rect_w, int* rect_h);
/* The STEREO MATCHER for ONE frame: the rectified gray pair -> the float disparity map of the left image, on the device: what MyStereoMatcher::Launch (stereo/stereo.cpp,
 * an empty StereoMatch()) leaves to an offline network and MyStereoMatcher::WaitResult reads back from a PNG into SemanticImage::disp.  The reference has no matcher to
 * restate; this one is a semi-global matcher specified in integers, so a numpy restatement matches it bit for bit.  w x h are the ctx's; a left
 * pixel (x, y) with disparity d matches the right pixel (x - d, y), d in [0, n_disp).
 *   census       9 wide x 7 high, source coordinates clamped to the image; one bit per non-centre position, set where neighbour < centre: 62 bits in a uint64.
 *   cost         C(x, y, d) = popcount(cL(x, y) ^ cR(x - d, y)) for x - d >= 0, and 64 for x - d < 0.
 *   paths        eight directions r; L_r(p, d) = C(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + p1, L_r(p-r, d+1) + p1, m + p2) - m with m = min_k L_r(p-r, k); terms with
 *                d +- 1 outside [0, n_disp) are left out; L_r(p, d) = C(p, d) where p - r lies outside the image.  S = the sum over the eight directions (16 bits).
 *   winner       d* = argmin_d S(p, d), ties to the lowest d.
 *   uniqueness   OpenCV's integer rule: invalid if some d with |d - d*| > 1 has S(p, d) (100 - uniqueness) < S(p, d*) 100.
 *   left-right   dR(x, y) = argmin_d S((x + d, y), d) over x + d < w, ties to the lowest d; invalid if |dR(x - d*, y) - d*| > lr_max_diff (lr_max_diff < 0: no test);
 *                d* > x is invalid.
 *   subpixel     for 0 < d* < n_disp - 1: den = max(S(d*-1) + S(d*+1) - 2 S(d*), 1), d16 = 16 d* + floor((16 (S(d*-1) - S(d*+1)) + den) / (2 den)), a mathematical
 *                floor; d16 = 16 d* at the two ends.
 *   output       float(d16) / 16, +0.0f where invalid (DetectExtraPoints reads disparity > 0 as "has a disparity").  Every element is written every frame.
 * Refused, each with its own dv_last_error text: n_disp other than 64, 128, 256; p1 < 0; p2 < p1; p2 > 255; uniqueness outside [0, 100); a non-zero reserved word;
 * stride < w; non-positive sizes; an unknown memory kind.  dv_stereo_sgm_check: those refusals without a device (0, or < 0 with dv_last_error(NULL)).
 * _enqueue: on the ctx's stream.  mem = DV_MEM_HOST (both images staged) or DV_MEM_DEVICE / DV_MEM_PINNED (read in place, any base alignment, valid until the collect).
 * One frame may be in flight.  _collect waits and returns one of two library-owned maps used alternately (rows of *stride_bytes = 4 w): the pointer stays valid until
 * the SECOND enqueue after it and goes straight into dv_inst_set_disparity(ctx, p, stride, DV_MEM_DEVICE, baseline) — SemanticImage::disp without a host round trip.
 * dv_stereo_sgm_debug: for tests — of the last COLLECTED frame, what = DV_SGM_DEBUG_CENSUS_L / _R (w x h uint64), _S (h x w x n_disp uint16), _DSTAR / _DR (w x h int16:
 * the winner and the right image's winner, before any validity test); cap_bytes must cover it. */
typedef struct dv_sgm_params { int32_t n_disp /* 64, 128, 256 */, p1 /* 10 */, p2 /* 120 */, uniqueness /* 5 */, lr_max_diff /* 1 */, reserved[3] /* zero */; } dv_sgm_params;
#define DV_SGM_DEBUG_CENSUS_L 0
#define DV_SGM_DEBUG_CENSUS_R 1
#define DV_SGM_DEBUG_S        2
#define DV_SGM_DEBUG_DSTAR    3
#define DV_SGM_DEBUG_DR       4
int dv_stereo_sgm_check(int w, int h, int stride, const dv_sgm_params* par);
int dv_stereo_sgm_enqueue(dv_ctx* ctx, const uint8_t* gray0, const uint8_t* gray1, int stride, int mem, const dv_sgm_params* par);
int dv_stereo_sgm_collect(dv_ctx* ctx, const float** disp_dev, int* stride_bytes);
int dv_stereo_sgm_debug(dv_ctx* ctx, int what, void* host, long long cap_bytes);
/* The MULTI-OBJECT TRACKER between the detector and the object tracker: a frame's detection rectangles and appearance embeddings -> a track id per detection, as
 * InstsFeatManager::AddInstancesByTracking (front_end/dynamic_tracker.cpp:791-828) gets them from DeepSORT::update (mot/deep_sort.cpp:72-139).  Track table and appearance
 * galleries stay in HBM between frames.  The ReID network (mot/reid_net.cpp, mot/extractor.cpp) stays with the caller: feats is its output, [n, feat_dim] float32 rows
 * already L2-normalised as ReIdNetImpl::forward leaves them (never renormalised here).  rects_xywh: [n, 4] float32 x, y, width, height (Box2D::rect).
 * The filter is cv::KalmanFilter(7, 4, 0), CV_32F (mot/kalman_tracker.cpp:31-51): state [cx, cy, s = area, r = w / h, vcx, vcy, vs], constant-velocity transition,
 * H = the 4 x 7 identity, Q = 1e-2 I, R = 1e-1 I, P0 = I; rect(): w = sqrt(s r), h = s / w, x = cx - w / 2, y = cy - h / 2 (:20-28).  predict / correct are restated from
 * OpenCV 3.4 video/src/kalman.cpp (unpinned): x' = A x, P' = A P A^T + Q; S = H P' H^T + R, K = (S^-1 H P')^T, x = x' + K (z - H x'), P = P' - K H P'.  Evaluated in
 * float32; the 4 x 4 solve is Gaussian elimination with partial pivoting where OpenCV takes DECOMP_SVD (DESIGN.md has the measured distance to a float64 evaluation).
 * A frame with n = 0 does not reach the reference's tracker at all (dynamic_tracker.cpp:795-796): accepted, it predicts and ages NOTHING.  Otherwise, step by step:
 *   predict      every track: ++time_since_update, the filter's predict (kalman_tracker.cpp:63-67, tracker_manager.h:40-44).
 *   remove_nan   tracks whose rect() has a NaN component are erased, order kept (tracker_manager.h:46-52).
 *   stage 1      rows = the Confirmed tracks in table order, columns = all detections.  iou_dist = 1 - RectIou (deep_sort.cpp:27-35: cv::Rect2f arithmetic, the overlap
 *                empty when its width or height is <= 0, 0 when the union is < DBL_EPSILON); feat = min over the track's stored embeddings g of 1 - g . f
 *                (feature_metric.h:59-61); cost = feat, INVALID_DIST = 1000 where iou_dist > 0.8f or feat > 0.2f (deep_sort.cpp:99).  HungarianAlgorithm::Solve on the costs
 *                widened to double (tracker_manager.cpp:20-50); an assigned pair with cost > 100 is dropped.
 *   stage 2      rows = the tracks stage 1 left unmatched, in their order, then the Tentative tracks in table order (tracker_manager.h:89-97); columns = the detections
 *                still unmatched, ascending.  cost = iou_dist, 1000 where > 0.7f (deep_sort.cpp:105-119).  Same solve, same drop.  A Confirmed track whose appearance gate
 *                failed can be matched here.
 *   miss         every track still unmatched: Tentative -> Deleted, else Deleted when time_since_update > max_age (kalman_tracker.cpp:90-96).
 *   update       every matched track, stage-1 pairs by row, then stage-2 pairs by row: time_since_update = 0, ++hits, Tentative with hits > n_init -> Confirmed with the next
 *                id of a counter that starts at 1 (ONE PER TRACKER here; one process-wide static in the reference), then correct with z = [x + w/2, y + h/2, w h, w / h].
 *   birth        a new Tentative track (hits 0, id -1) per detection the reference leaves in unmatched_dets, ascending (tracker_manager.h:110-117).  That list is KEPT AS THE
 *                REFERENCE COMPUTES IT: tracker_manager.cpp:62-68 subtracts the assigned COLUMN INDICES from the detection ids, which are the same numbers in stage 1 and
 *                not in stage 2 once stage 1 has matched something.  So after stage 2 a detection d of its columns is born unless some pair was assigned column INDEX d: a
 *                detection matched in stage 2 may ALSO start a track, and an unmatched one may start none.
 *   gallery      for every matched pair, births included, the embedding goes into the track's ring of `budget` rows by FeatureBundle::add (feature_bundle.h:40-46): if
 *                next == budget then full = true, next = 0; stored at next++.  A distance reads `next` rows, all `budget` once full.  Rows past that count are excluded BY
 *                INDEX, never multiplied in: they are uninitialised (dv_mot_config fills the allocation with NaN so that a slip shows).
 *   remove_deleted, order kept; removal never moves gallery rows (a track owns a gallery slot; freed slots are taken lowest first).
 *   answer       visible_tracks_info (tracker_manager.h:136-156): track_id[j] = the id of the Confirmed track updated with detection j in this frame, else -1 — the value
 *                the plane entries drop a detection by.
 * The assignment is the one the reference's Munkres (mot/hungarian.cpp, Buehren's steps) returns, ties included: same scan orders, same fabs(x) < DBL_EPSILON zero test.
 * A NaN appearance or IoU distance counts as gated (1000) in both stages: Munkres on a NaN need not end.
 * A frame after which the table would hold more than max_tracks tracks FAILS in _collect with a message and leaves the tracker as it was before the frame.
 * dv_mot_check: the refusals of dv_mot_config without a device.  dv_mot_config: allocates (galleries max_tracks x budget x feat_dim float32, once) and resets; a second
 * call reconfigures.  dv_mot_reset: no tracks, id counter back to 1.
 * _enqueue: on the ctx's stream — behind dv_inst_stack_frame_collect, in front of dv_inst_track_enqueue_planes.  mem = DV_MEM_HOST (both staged) or DV_MEM_DEVICE /
 * DV_MEM_PINNED (both read in place until the collect; each pointer may be of either in-place kind: rectangles in pinned memory beside embeddings in device memory).  One frame may be in flight; n > 64 is refused.  No host round trip between _enqueue and _collect: counts stay on the
 * device; the frame's only device -> host traffic is n ids and a few counters through pinned memory.
 * dv_mot_get_tracks: the table in order (for tests and the shim).  dv_mot_assign: the operator form of the device Munkres alone on a row-major float cost matrix (host
 * memory, finite, >= 0, rows <= 128, cols <= 64): assignment[row] = column or -1, nothing dropped. */
#define DV_MOT_MAX_TRACKS 128
#define DV_MOT_MAX_BUDGET 100
#define DV_MOT_MAX_FEAT_DIM 512
typedef struct dv_mot_params { int32_t n_init, max_age, budget, feat_dim, max_tracks, reserved[3]; } dv_mot_params;
typedef struct dv_mot_track {
    float x[7], p_diag[7], rect[4];      /* state, diagonal of the covariance, rect() = x, y, w, h */
    int32_t state /* 0 Tentative, 1 Confirmed */, id, hits, time_since_update, n_feats /* stored embeddings */, reserved;
} dv_mot_track;
int dv_mot_check(const dv_mot_params* par);
int dv_mot_config(dv_ctx* ctx, const dv_mot_params* par);
int dv_mot_reset(dv_ctx* ctx);
int dv_mot_update_enqueue(dv_ctx* ctx, const float* rects_xywh, const float* feats, int n, int mem);
int dv_mot_update_collect(dv_ctx* ctx, int32_t* track_id, int* n_tracks, int* n_confirmed);
int dv_mot_get_tracks(dv_ctx* ctx, dv_mot_track* out, int cap, int* n);
int dv_mot_assign(dv_ctx* ctx, const float* cost, int rows, int cols, int32_t* assignment);
/* The ReID EXTRACTOR in front of the multi-object tracker: the frame's colour image and the detections' rectangles -> one L2-normalised 512-float embedding per detection,
 * as DeepSORT::update gets them from Extractor::extract (mot/extractor.cpp:31-52) and ReIdNetImpl::forward (mot/reid_net.cpp:113-121).  float32 throughout.
 * Weights (dv_reid_load): host memory in the order ReIdNetImpl::load_form reads its flat file (mot/reid_net.cpp:123-135, the modules of :17-44 and :98-110):
 *   conv1     weight [64, 3, 3, 3], bias [64], then its BatchNorm2d: weight, bias, running_mean, running_var (64 each);
 *   8 blocks  (c_in, c_out, down) = (64,64,0) (64,64,0) (64,128,1) (128,128,0) (128,256,1) (256,256,0) (256,512,1) (512,512,0), each: conv.0 weight [c_out, c_in, 3, 3]
 *             (stride 2 when down) and its batch-norm (4 x c_out), conv.3 weight [c_out, c_out, 3, 3] and its batch-norm, and for a down block the 1 x 1 stride-2
 *             weight [c_out, c_in, 1, 1] and its batch-norm.  No num_batches_tracked.
 * That is 2 048 + 2 x 74 240 + 230 912 + 295 936 + 920 576 + 1 181 696 + 3 676 160 + 4 722 688 = DV_REID_N_FLOATS; any other length is refused (the reference reads short
 * without a word).  Batch-norm is the eval-mode form with eps 1e-5, folded on the host in float64 into one scale and one shift per channel, conv1's bias inside the shift
 * (declared: the reference evaluates it unfolded in float32).  in_w x in_h = reid_input_width x reid_input_height (mot/mot_parameter.h:29-30, 64 x 128): accepted are the
 * sizes whose last map is 8 x 4 after four stride-2 stages n -> ceil(n / 2), so that avg_pool2d({8, 4}, 1) leaves 512 values: widths 49..64, heights 113..128.
 * A second load replaces the weights; a refused one leaves the ctx as it was.  Activations for DV_REID_MAX_CROPS crops are allocated at the load.
 * Crops (one launch, no host image work), per rectangle x, y, w, h (float32; Rect2f -> Rect is cvRound per field, half to even): ori_img(rect), cv::resize(.., {in_w,
 * in_h}), cvtColor(RGB2BGR) = a channel swap, convertTo(CV_32F, 1 / 255), (v - mean[c]) / std[c] with mot/mot_parameter.h:26-27 on the SWAPPED order, NCHW.  The resize
 * is OpenCV's 8-bit INTER_LINEAR restated (unpinned): scale = src / (double) dst; f = (float)((d + 0.5) scale - 0.5); s = floor(f); f -= s;
 * horizontally s < 0 -> s = 0, f = 0 and s >= src - 1 -> s = src - 1, f = 0; vertically f is kept and the two row indices are clamped to [0, src - 1] (the CROP's
 * edges); coefficients cvRound((1 - f) 2048) and cvRound(f 2048); S = s0 a0 + s1 a1; the byte is (((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2.  A crop of
 * exactly 2 in_w x 2 in_h takes the fast area path (a + b + c + d + 2) >> 2.  The float is (u * (1 / 255.f) - mean) / std in that order, float32, IEEE division.
 * A rounded rectangle that is empty or leaves the image makes the reference throw: here the frame FAILS at _collect with a message and the stage stays usable.
 * Network: conv1 + batch-norm + ReLU + max_pool2d(3, 2, 1) (padding -inf) in one kernel; every other convolution is one implicit-GEMM kernel on the f32 matrix cores
 * whose epilogue applies scale and shift, the residual (the block's input, or the 1 x 1 branch's output) and the ReLU; the tail (average over the 8 x 4 map in a fixed
 * order, row 2-norm, division) is one kernel.
 * dv_reid_check: the refusals of dv_reid_load without a device.
 * _enqueue: on the ctx's stream, the image being the ctx's width x height, 8-bit BGR with `stride` bytes per row.  mem = DV_MEM_HOST (image and rectangles staged) or
 * DV_MEM_DEVICE / DV_MEM_PINNED (both read in place until the collect).  One frame may be in flight; n > 64 is refused; n = 0 returns at once as extract does on an empty
 * list.  _collect: *feats_dev = the library's [n, 512] float32 device buffer, valid until the next enqueue; dv_mot_update_enqueue(.., DV_MEM_DEVICE) reads it in place.
 * dv_reid_get_feats: the first n rows of the last collected frame, downloaded (tests, the shim).  dv_reid_input: the prepared [n, 3, in_h, in_w] tensor of the last frame.
 * dv_reid_layer: the operator form of the convolution kernel alone on host tensors: x [n, c_in, h, w], weight [c_out, c_in, k, k], scale and shift [c_out], residual
 * [n, c_out, h_out, w_out] or null -> out [n, c_out, h_out, w_out] = relu?(conv(x) * scale + shift + residual), h_out = (h + 2 pad - k) / stride + 1 with pad 1 for
 * k = 3 and 0 for k = 1.  (k, stride) in {(3, 1), (3, 2), (1, 2)}, c_in a multiple of 32, c_out of 64, both <= 512, h and w <= 128, n <= 64, n h w max(c_in, c_out) <= 2^24.
 * dv_reid_stem: the operator form of the fused stem kernel alone on host tensors: x [n, 3, h, w], weight [64, 3, 3, 3], scale and shift [64] -> out [n, 64, ceil(h / 2),
 * ceil(w / 2)] = max_pool2d(relu(conv(x, padding 1) * scale + shift), 3, 2, 1).  n in 1..64, h and w in 1..128.  Both operators are refused while a frame is in flight. */
#define DV_REID_N_FLOATS 11178496
#define DV_REID_FEAT_DIM 512
#define DV_REID_MAX_CROPS 64
int dv_reid_check(size_t n_floats, int in_w, int in_h);
int dv_reid_load(dv_ctx* ctx, const float* weights, size_t n_floats, int in_w, int in_h);
int dv_reid_extract_enqueue(dv_ctx* ctx, const uint8_t* bgr, int stride, const float* rects_xywh, int n, int mem);
int dv_reid_extract_collect(dv_ctx* ctx, const float** feats_dev);
int dv_reid_get_feats(dv_ctx* ctx, float* out, int n);
int dv_reid_input(dv_ctx* ctx, float* out);
int dv_reid_layer(dv_ctx* ctx, const float* x, int n, int c_in, int h, int w, const float* weight, int c_out, int k, int stride, const float* scale, const float* shift,
                  const float* residual_or_null, int relu, float* out);
int dv_reid_stem(dv_ctx* ctx, const float* x, int n, int h, int w, const float* weight, const float* scale, const float* shift, float* out);
/* cv::cvtColor(BGR2GRAY) on 8-bit images: (B 1868 + G 9617 + R 4899 + 8192) >> 14; gray is w x h, tightly packed */
int dv_bgr2gray(dv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* gray, int mem);
/* cv::remap(src, dst, map1, map2, INTER_LINEAR) — BORDER_CONSTANT 0 — with the fixed-point maps cv::initUndistortRectifyMap(..., CV_16SC2, ...)
 * returns (utils/camera_model.cpp:481-499): map1_xy = w*h (x, y) int16 pairs, map2 = w*h uint16 (fy << 5 | fx).  8-bit source with
 * channels 1 or 3 (stride in bytes); dst is w x h x channels, tightly packed.  The calls of ImageProcessor::Run on the colour frames
 * (image_process/image_process.cpp:109-121) and of SemanticImage::SetMask on the merged mask (basic/semantic_image.cpp:86-89).
 * The maps are host memory; src / dst follow `mem`. */
int dv_remap(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, int channels, const int16_t* map1_xy, const uint16_t* map2, uint8_t* dst, int mem);
/* cfg::is_undistort_input (utils/camera_model.cpp:481-499): installs (map1_xy != NULL) or removes (NULL) the undistortion maps of camera
 * `cam` (0 left, 1 right) in HBM.  While installed, dv_track_stereo* take DISTORTED frames and undistort them on the way into pyramid
 * level 0: with DV_FMT_BGR the remap of the three channels and cvtColor are fused (the remapped colour image never exists); gray frames
 * are remapped as one channel, which is what the reference's mono -> BGR -> remap -> gray chain yields.  w, h must equal the config's.
 * dv_config.cam0 / cam1 should then be the NEW intrinsics without distortion, as the reference resets them (camera_model.cpp:486-503).
 * A mask passed to the tracker is used as given (the reference remaps it before inverting it: use dv_remap with channels = 1). */
int dv_set_undistort_maps(dv_ctx* ctx, int cam, const int16_t* map1_xy, const uint16_t* map2, int w, int h);
/* cv::getOptimalNewCameraMatrix(K, D, Size(w, h), alpha, Size(w, h)) without principal-point centring (utils/camera_model.cpp:483,493), for the pinhole + radtan
 * camera of dv_cam (k3 = 0): newK4 = fx, fy, cx, cy.  Host code, no ctx.  Restated from OpenCV 3.4 calib3d (un-vendored: from memory, like SURVEY App. A):
 * cvGetOptimalNewCameraMatrix -> icvGetRectangles (a 9 x 9 grid over the image, pixel (x w / 8, y h / 8)) -> cvUndistortPoints with R = P = I (5 fixed-point
 * iterations from the normalised point) -> inner rectangle (largest of the left / top edge points, smallest of the right / bottom ones) and outer rectangle (bounding
 * box of all 81), each mapped onto [0, w - 1] x [0, h - 1]; the two projections are blended by alpha (0: no black border, 1: every source pixel kept).  All in double
 * (the library keeps the grid as float points: declared choice U1).  <0: bad argument or a degenerate rectangle. */
int dv_optimal_new_camera(const dv_cam* cam, int w, int h, double alpha, double newK4[4]);
/* cv::initUndistortRectifyMap(K, D, Mat(), newK, Size(w, h), CV_16SC2, map1, map2) (utils/camera_model.cpp:484,494; OpenCV 3.4 imgproc undistort.cpp) on the device:
 * the map pair dv_remap / dv_set_undistort_maps read, map1_xy = w*h (x, y) int16 pairs, map2 = w*h uint16 (fy << 5 | fx).  The library walks a row by _x += 1 / fx',
 * one rounded addition per pixel: the column values are produced by that same chain once (they are the same in every row for R = I) and the distortion polynomial of
 * all pixels is evaluated in parallel (undistort_map.hip).  The maps follow `mem` (DV_MEM_HOST / DV_MEM_DEVICE); w, h <= 32767. */
int dv_init_undistort_map(dv_ctx* ctx, const dv_cam* cam, const double newK4[4], int w, int h, int16_t* map1_xy, uint16_t* map2, int mem);
/* The whole of cfg::is_undistort_input in InitOneCamera (utils/camera_model.cpp:479-504) for the cameras the ctx was created with: newK of camera 0 (and of camera 1 on
 * a stereo ctx) by dv_optimal_new_camera(alpha) (the reference: alpha = 0), both map pairs built in HBM and installed as dv_set_undistort_maps would install them (no
 * host round trip), and the ctx's cameras switched to (newK, 0, 0, 0, 0): the rows of dv_track_stereo* and the object tracker then lift with the undistorted intrinsics,
 * as the reference's re-parameterised cam0 / cam1 do (:501-511); give them (dv_get_cameras) to dv_lift_projective* / dv_undistort_lines.  new_cam0 / new_cam1 (may be NULL) receive
 * them (new_cam1 = the unchanged camera 1 on a mono ctx).  Refused, with nothing changed, while a frame is pending.  A second call starts from the original cameras
 * again; if it fails after that refusal point (allocation, launch), no maps are installed and the original cameras hold.  dv_set_undistort_maps(ctx, 0, NULL, ...)
 * removes the maps AND restores the original cameras ((ctx, 1, NULL, ...): camera 1's).  Installing the caller's OWN maps for a camera afterwards also restores that camera's
 * original intrinsics: (newK, 0) belongs to the maps built here. */
int dv_undistort_setup(dv_ctx* ctx, double alpha, dv_cam* new_cam0, dv_cam* new_cam1);
/* copies the installed maps of camera `cam` out of HBM (w*h*2 int16, w*h uint16; host or device memory by `mem`), e.g. to dv_remap the merged mask with them as the
 * reference does (basic/semantic_image.cpp:86-89); <0 if none are installed */
int dv_get_undistort_maps(dv_ctx* ctx, int cam, int16_t* map1_xy, uint16_t* map2, int mem);
/* the cameras the ctx lifts with at the moment (dv_config's, or those of dv_undistort_setup); either pointer may be NULL */
int dv_get_cameras(dv_ctx* ctx, dv_cam* cam0, dv_cam* cam1);
/* cv::circle(mask, pt, radius, 0, -1) per point (background_tracker.cpp:79-80) */
int dv_circle_mask(dv_ctx* ctx, uint8_t* mask, int w, int h, int stride, const float* pts_xy, int n,
                   int radius, int mem);
/* ErodeMask / ErodeMaskGpu (front_end/feature_utils.h:130-146) */
int dv_erode(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, int k, uint8_t* dst, int mem);
/* InstFeat::UndistortedPts -> PinholeCamera::liftProjective (instance_feature.cpp:94-103) */
int dv_lift_projective(dv_ctx* ctx, const dv_cam* cam, const float* pts_xy, int n, float* out_xy, int mem);
/* InstFeat::UndistortedPointsWithAddOffset (front_end/instance_feature.cpp:123-133): points in ROI coordinates, the 2-D box's
 * top-left corner added in double before lifting */
int dv_lift_projective_offset(dv_ctx* ctx, const dv_cam* cam, const float* pts_xy, int n, double off_x, double off_y, float* out_xy, int mem);

/* ======================= back end: sliding-window bundle adjustment ======================= */

/* One reprojection residual block = the constructor arguments of ProjectionTwoFrameOneCamFactor (kind 0),
 * ProjectionTwoFrameTwoCamFactor (kind 1) or ProjectionOneFrameTwoCamFactor (kind 2)
 * (estimator/factor/projection_*_factor.h; built at estimator/estimator.cpp:134-178).  112 bytes. */
typedef struct dv_ba_factor {
    double pix, piy, pjx, pjy;      /* pts_i, pts_j on the normalised plane */
    double vix, viy, vjx, vjy;      /* velocity_i, velocity_j */
    double td_i, td_j;
    int32_t kind, lm, fi, fj;       /* landmark index, anchor frame (start_frame), observing frame */
    double pad_[2];
} dv_ba_factor;

/* per landmark (>= 4 observations, estimator.cpp:134-136): its factors are contiguous */
typedef struct dv_ba_lm { int32_t first, count, anchor, mask; } dv_ba_lm;

/* IMUFactor between frames fi and fj = fi+1: the IntegrationBase results (imu/integration_base.h) */
typedef struct dv_ba_imu {
    double sum_dt, dp[3], dq[4] /* w x y z */, dv[3], lin_ba[3], lin_bg[3];
    double jacobian[225], covariance[225];     /* 15x15 row-major, order P R V BA BG */
    int32_t fi, fj, pad0, pad1;
} dv_ba_imu;

/* marginalization prior in information form: cost(dx) = c0/2 + b.dx + dx.A dx/2, dx w.r.t. the linearisation
 * point x0 of the kept blocks (equivalent to MarginalizationFactor's r0 + J0 dx with A = J0^T J0, b = J0^T r0,
 * c0 = r0^T r0; factor/marginalization_factor.cpp:283-309,350-396) */
typedef struct dv_ba_prior_block { int32_t type /* 0 pose, 1 speed-bias, 2 ex_pose, 3 td */, idx, off, size_local; } dv_ba_prior_block;
typedef struct dv_ba_prior {
    int32_t valid, n, nblocks, pad;
    double c0;
    dv_ba_prior_block blocks[16];
    double x0[16][9];
} dv_ba_prior;

typedef struct dv_ba_problem {
    int32_t nframes, nlm, nfac, nimu;     /* frames in the window (frame+1), landmarks, residual blocks, IMU factors */
    int32_t use_imu, plane_kind /* 0 none, 1 PoseConstraint with IMU (dz=0), 2 vision-only (dy=0) */, max_iters;
    int32_t free_blocks; /* bit 0: para_ex_pose[0..1] are NOT SetParameterBlockConstant (estimate_extrinsic 1 once openExEstimation is set), bit 1: para_td is not
                            (estimate_td 1 while |Vs[0]| >= 0.2) — Estimator::AddBodyParameterBlock, estimator/estimator.cpp:87-100.  0 in every shipped configuration.
                            Their columns follow the frames' in the reduced system (6 + 6 + 1); such a solve takes the generic factorisation and two more launches
                            per linearisation (csrc/be_ext.hip); not available on a landmark-sharded window */
    double g_norm;
    double* pose;        /* [nframes][7] x y z qx qy qz qw   (para_pose, in/out) */
    double* speed_bias;  /* [nframes][9]                      (para_speed_bias, in/out; ignored if !use_imu) */
    double* ex_pose;     /* [2][7]                            (para_ex_pose; in/out when free_blocks bit 0 is set, else constant) */
    double* td;          /* [1]                               (para_td; in/out when free_blocks bit 1 is set, else constant) */
    double* inv_depth;   /* [nlm]                             (para_point_features, in/out) */
    const dv_ba_factor* factors; const dv_ba_lm* landmarks; const dv_ba_imu* imu;
    const dv_ba_prior* prior; const double* prior_A; const double* prior_b;     /* prior may be NULL */
    double x_norm2_extra;   /* squared norm of further free parameter blocks that count in ceres' parameter-tolerance test |step| <= 1e-8 (|x| + 1e-8) without moving:
                               the lineProjectionFactor blocks of AddLineResidualBlock under the reference's zero sqrt_info; 0 otherwise */
} dv_ba_problem;

typedef struct dv_ba_summary {
    int32_t iterations, successful, termination /* 0 max iterations, 1 converged, 2 failure */, slots;
    double initial_cost, final_cost;
} dv_ba_summary;

/* Replaces ceres::Solve in Estimator::Optimization (estimator/estimator.cpp:261-326): DENSE_SCHUR + DOGLEG,
 * HuberLoss(1.0) on reprojection blocks, max_num_iterations = max_iters, wall-clock budget disabled.
 * The whole trust-region loop runs on the device; states are updated in place. */
int dv_ba_solve(dv_ctx* ctx, dv_ba_problem* problem, dv_ba_summary* summary);

/* One evaluation at the given states (what one ceres Evaluate() pass + the Schur elimination produce): total cost, the reduced
 * camera system S = H_pp - sum_l w_l w_l^T / h_l (n x n, row-major, symmetric) and its right-hand side g = g_p - sum_l w_l g_l / h_l.
 * Column order: per frame, 6 pose columns (if the pose is free) then 9 speed-bias columns (if use_imu); then, if free (free_blocks), 6 + 6 extrinsic columns and the td
 * column; *n = their count (<= 178).
 * The sum over landmarks, IMU factors and the prior is linear, so a window sharded BY LANDMARK over several GPUs (IMU factors
 * and prior on one rank) is assembled by adding the per-rank [S | g | cost] — the all-reduce of SURVEY 8(e)
 * (dynamic_vins_amd/dist.py:allreduce_reduced_system). cost, S, g may be NULL. */
int dv_ba_eval(dv_ctx* ctx, const dv_ba_problem* problem, int* n, double* cost, double* S, double* g);

/* ---- one window sharded BY LANDMARK over several GPUs (BASELINE north_star: "RCCL all-reduce of the reduced camera-pose Hessian") ----
 * The reference has no multi-GPU path; this is the exchange step its Schur elimination (ceres DENSE_SCHUR inside Estimator::Optimization,
 * estimator.cpp:296-326) admits: rank r owns a contiguous range of landmarks, evaluates and eliminates only those, and the per-rank partial reduced
 * systems are summed IN RANK ORDER on every rank (identical bits everywhere).  After dv_dist_init_*, dv_ba_solve / dv_ba_eval / dv_est_process on this
 * ctx run sharded: every rank must be given the SAME problem and makes the same calls; every rank returns the same result.
 * A binding in the reference would sit in Estimator::SetParameter (one ctx per rank, rank / world from the launcher). */
typedef int (*dv_allgather_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);      /* recv: world x bytes_per_rank, rank-major; 0 = ok */
int dv_dist_unique_id(uint8_t id[128]);                                                  /* ncclGetUniqueId: rank 0 creates it, the launcher broadcasts it */
int dv_dist_init_rccl(dv_ctx* ctx, int rank, int world, const uint8_t id[128]);          /* RCCL all-gather on the BA stream (xGMI); no host round trip per iteration */
int dv_dist_init_host(dv_ctx* ctx, int rank, int world, dv_allgather_fn fn, void* user); /* exchange staged through pinned host memory and the caller's all-gather */
/* one-shot exchange: every rank writes its vector into a window each peer exposes through hipIpc (direct xGMI link), then a sequence flag; no
 * library call per exchange.  prepare -> all-gather the 64-byte handles with the launcher's own means -> init. */
int dv_dist_peer_prepare(dv_ctx* ctx, int rank, int world, uint8_t handle[64]);
int dv_dist_init_peer(dv_ctx* ctx, const uint8_t* handles /* [world][64], rank order */);
int dv_dist_rccl_ranks(dv_ctx* ctx, int* n);                                             /* ncclCommCount of the communicator behind dv_dist_init_rccl (0: other transport) */
int dv_dist_shutdown(dv_ctx* ctx);
/* what one rank contributes to the exchanges of a sharded window solve (bytes): `system` once per linearisation — the partial reduced camera system and the coefficients of the
 * quadratic forms the trust-region step needs of the landmarks it does not own: 12 424 doubles whatever the window holds —, `cost` once per cost-only slot, `depth` once per solve */
int dv_dist_exchange_bytes(dv_ctx* ctx, int n_landmarks, long long* system_bytes, long long* cost_bytes, long long* depth_bytes);
int dv_dist_info(dv_ctx* ctx, int* rank, int* world, int* transport, long long* exchanges);
/* operator form of the exchange: S_g (host, n doubles — this rank's partial [S | g | cost], e.g. of dv_ba_eval on the rank's share of the landmarks)
 * is replaced by the rank-ordered sum over all ranks */
int dv_allreduce_reduced_system(dv_ctx* ctx, double* S_g, int n);

/* ---- several independent sequences on ONE GPU whose window solves share every launch ("batched") ----
 * No counterpart in the reference (one process per sequence).  The members are ordinary contexts with their own estimators; after
 * dv_est_process_begin (or _dynamic_begin) has been called on every member that has a frame, dv_batch_enqueue launches the iteration slots of all
 * pending window solves as one launch per stage (argument tables in HBM, window index in the grid); dv_est_process_end then collects each member
 * as usual.  A member collected without dv_batch_enqueue is solved on its own stream.  Results are bit-identical to the unbatched path.
 * DYNAMIC members (dv_est_config::dynamic = 1, entered through dv_est_process_dynamic_begin / _begin_ego + _attach): the object solve of a member's object branch
 * (InstanceManager::Optimization, estimator_insts.cpp:772-807) is packed and uploaded by the member's call and launched by dv_batch_enqueue too — the object solves of
 * all members of the round as ONE grid of independent workgroups on the group's object stream, beside the window solves (dv_batch_obj_info counts them).  A round
 * with a single object solve, a member with dv_timing_enable, and a member collected without dv_batch_enqueue use the single-workgroup launch.  dv_destroy of a
 * member and dv_batch_destroy drain the group's streams first: an uploaded or running object solve never outlives its buffers, and a member that leaves with a solve
 * not yet launched launches it alone when it is collected. */
typedef struct dv_batch dv_batch;
dv_batch* dv_batch_create(dv_ctx* const* ctxs, int n);      /* idle contexts of one device; NULL + dv_last_error(NULL) on failure */
void dv_batch_destroy(dv_batch* batch);                      /* the members stay valid; dv_destroy of a member before the batch detaches it from the batch */
int dv_batch_enqueue(dv_batch* batch);
int dv_batch_arrive(dv_batch* batch);                        /* one host thread per member: blocks until every member's thread has arrived; the last one enqueues */
int dv_batch_abort(dv_batch* batch);                         /* a member thread failed before arriving: every waiting and later dv_batch_arrive returns -1 */
int dv_batch_info(dv_batch* batch, long long* batched_rounds, long long* single_rounds);
/* The FRONT ENDS of the members in shared launches: dv_track_stereo_enqueue for several members at once — FeatureTracker::TrackImage (front_end/background_tracker.cpp:52-158)
 * of S sequences as one launch per stage (pyramid levels, aprons, temporal LK, compaction, Shi-Tomasi tile, corner selection, stereo LK, rows: 10 launches per group and
 * frame instead of 10 per sequence; the reference runs one process per sequence, system/main.cpp:178-330).  member = index into the array dv_batch_create was given.
 * BGR frames (mem = DV_MEM_* | DV_FMT_BGR) and members with installed undistortion maps (dv_undistort_setup / dv_set_undistort_maps; the maps are per member, so
 * the members' cameras may differ) share the launches too: one more launch fills pyramid level 0 of all such members of the round (remap, remap + BGR -> gray, or
 * BGR -> gray), their DV_MEM_HOST frames are staged on the group's stream first, DV_MEM_DEVICE / DV_MEM_PINNED frames are read in place.  A round of gray members
 * without maps enqueues exactly the ten launches above.
 * DV_MODE_NAIVE jobs with a mask (TrackImageNaive, what dv_runner_set_mask feeds) share the launches as a second class when the round holds at least two of them:
 * the GPU tracker runs over their slice of the job tables, one launch per level builds its cuda::pyrDown-rule pyramids and one erodes the masks of the members with
 * mask_morphology_size > 0; compaction, detection and rows are the group's launches, each job under its own mask and rules.  A DV_MEM_HOST job's mask is staged into
 * the member's own buffer on the group's stream, a DV_MEM_DEVICE / DV_MEM_PINNED job's mask is read in place (rows of `stride` bytes, of width bytes for a BGR job).
 * A round without such jobs enqueues nothing for them.
 * DV_MODE_SEMANTIC jobs with a mask (TrackSemanticImage: the background tracking of a dynamic sequence, what dv_runner_set_dynamic feeds) are the third class, and the
 * only one whose member may own an object tracker (dv_inst_config): TrackLeft runs with the raw jobs' slice, TrackRightGPU with the naive jobs' slice, the GPU
 * tracker's pyramid levels and the erosion are those of the naive class, and semantic and naive jobs are counted together for the "at least two" rule.  Whatever
 * dv_track_unmask_static staged on such a member is applied by ONE launch for all members of the round, in the member's own copy of the mask (made by the same launch
 * for a DV_MEM_DEVICE / DV_MEM_PINNED mask: the caller's buffer is never written).  The group's stream keeps the hand-shake with the member's object tracker — it
 * waits for the objects of the previous frame, and dv_inst_track_enqueue of this frame (call it per member after this call, as after dv_track_stereo_enqueue; it
 * stays one set of launches per member) starts behind the round's pyramids and draws its ids behind the round's corner selection.
 * On EVERY return of this call, 0 or -1, the dv_track_unmask_static jobs of the members handed in are gone: none survives into a later frame.
 * Jobs that cannot share launches (a semantic or naive job without a mask, a raw job with one, a lone semantic / naive job, a naive job with dv_track_unmask_static
 * jobs staged or whose previous frame was tracked in raw mode, a raw or naive job of a member with an object tracker, dv_timing_enable on the ctx, another image
 * size than the first shareable job's) run through their member's own dv_track_stereo_enqueue inside this call, in this round only.  Every member is collected with
 * dv_track_stereo_collect as usual; its rows are bit-identical to the unbatched path's.  A member whose maps do not fit (another size, camera 1 missing on a stereo
 * member) or whose previous frame was not collected fails the call with dv_track_stereo's message; no member of the shared part has a frame pending then.
 * Between this call and a member's dv_track_stereo_collect, call no image operator (dv_remap, dv_bgr2gray, dv_pyr_down_cuda, ...) on that member: its staging buffers
 * are in use on the group's stream, which the operators' own stream is not ordered against. */
typedef struct dv_track_job { int32_t member, mem /* DV_MEM_* [| DV_FMT_BGR] */; const uint8_t* gray0; const uint8_t* gray1; int32_t stride /* bytes, 0 = width (3 * width for DV_FMT_BGR) */, mode; double t; const uint8_t* mask; } dv_track_job;
int dv_batch_track_enqueue(dv_batch* batch, const dv_track_job* jobs, int n);
int dv_batch_track_info(dv_batch* batch, long long* rounds, long long* members_batched, long long* members_single);
/* measurement: HIP events on the batch stream around the solve / evaluation / reduce launches of one steady-state iteration slot per round; out3 = average ms per launch so far */
int dv_batch_timing(dv_batch* batch, int on, double* out3, long long* rounds, int* windows);

/* Replaces MarginalizationInfo::{preMarginalize,marginalize,getParameterBlocks} as driven by
 * Estimator::SetMarginalizationInfo (estimator/estimator.cpp:403-619).
 *   mode 0 = kMarginOld: P holds the linearisation point (all 11 window states), the residual blocks of the landmarks
 *            anchored in frame 0 (>= 4 observations), imu[0] = the IMUFactor (0,1) (nimu 0 if sum_dt >= 10) and the
 *            current prior; pose 0 / speed-bias 0 / those landmarks are marginalized.
 *   mode 1 = kMarginSecondNew: only the prior is used; pose[kWinSize-1] is marginalized.
 * out_A: n x n (n <= 192), out_b: n.  Block indices of out_prior are already shifted (addr_shift).
 * out_prior->valid = 0 when nothing can be marginalized.  diag4 (may be NULL): c0, smallest pivot of A_mm, failure
 * flag, numerical rank of A' (under DV_MARG_EIGEN: the count of kept eigenvalues, the rank of J0). */
int dv_marginalize(dv_ctx* ctx, const dv_ba_problem* P, int mode, dv_ba_prior* out_prior, double* out_A, double* out_b, double* diag4);

/* The form of the prior a marginalization leaves (MarginalizationInfo::marginalize, estimator/factor/marginalization_factor.cpp:283-308).  Both are handed
 * on in information form (A', b', c0 = J0^T J0, J0^T r0, r0^T r0); they differ in how A' = Arr - Arm Amm^-1 Amr is treated:
 *   DV_MARG_INFO   A', b' as the Schur complement leaves them, c0 from a rank-revealing LDL^T that skips pivots <= 1e-8
 *   DV_MARG_EIGEN  A' eigen-decomposed on the device (be_marg_eig: parallel Jacobi), eigenvalues <= 1e-8 zeroed: A', b' projected onto the kept
 *                  eigenvectors and c0 summed over them in ascending order, as the reference's J0 = S^1/2 Q^T, r0 = S^-1/2 Q^T b' (:297-308).
 *                  In BOTH forms the system being reduced and A' share the LDS of one workgroup: at most 89 kept dims beside 6 dropped ones, 88 beside 9, 85 beside 15
 *                  (the shipped configurations: <= 82); larger priors are refused before anything is uploaded.  A rank-deficient A_mm is still eliminated by the
 *                  LDL^T of DV_MARG_INFO (its pivots are reported by dv_est_get_marg_health). */
#define DV_MARG_INFO  0
#define DV_MARG_EIGEN 1
/* takes effect at the next marginalization of this ctx (estimator or dv_marginalize).  Refused (form unchanged) for a form other than 0 / 1, while a solve or
 * marginalization is in flight (between _begin and _end), and for a dv_batch member (dv_batch_create refuses a ctx whose form is not DV_MARG_INFO) */
int dv_set_marg_form(dv_ctx* ctx, int form);
int dv_get_marg_form(dv_ctx* ctx, int* form);
/* eigenvalues of A' (ascending, before the clamp; ev[0 .. *n - 1], cap >= *n) and the Jacobi sweep count of the LAST DV_MARG_EIGEN marginalization of this
 * ctx (SelfAdjointEigenSolver::eigenvalues of marginalization_factor.cpp:297); waits for it.  ev may be NULL to ask for n / sweeps only */
int dv_marg_last_spectrum(dv_ctx* ctx, double* ev, int cap, int* n, int* sweeps);

/* operator-level factor evaluation (Evaluate() of the three projection factors / IMUFactor) for parity tests.
 * out: n x 54 doubles = r[2] J_pose_i[2x6] J_pose_j[2x6] J_ex0[2x6] J_ex1[2x6] J_lambda[2] J_td[2] (tangent space) */
int dv_proj_eval(dv_ctx* ctx, const dv_ba_factor* factors, int n, const double* pose_i, const double* pose_j,
                 const double* ex0, const double* ex1, const double* inv_depth, const double* td, double* out);
/* out: 15 whitened residuals followed by the whitened 15 x 30 Jacobian (pose_i 6, sb_i 9, pose_j 6, sb_j 9) */
int dv_imu_eval(dv_ctx* ctx, const dv_ba_imu* imu, double g_norm, const double* pose_i, const double* sb_i,
                const double* pose_j, const double* sb_j, double* out);
/* operator-level entries of the two kernels behind a window solve, for tests against a float64 restatement.
 * dv_ba_gauge: the yaw / position gauge fix of Estimator::Double2vector -> BodyState::GetOptimizationParameters (estimator/estimator.cpp:1110-1154,
 * estimator/body.cpp:61-129) on a caller-given solved window.  pose 11 x 7 (x y z qx qy qz qw), speed_bias 11 x 9, inv_depth[nlm] (nlm <= 1000, may be NULL at 0);
 * R0 (3x3 row-major), ypr0 (degrees, Utility::R2ypr) and P0: frame 0 before the solve.  Frames >= nframes are copied.  Outputs in the same layouts. */
int dv_ba_gauge(dv_ctx* ctx, const double* pose, const double* speed_bias, const double* inv_depth, int nlm, int nframes, int use_imu,
                const double* R0, const double* ypr0, const double* P0, double* out_pose, double* out_speed_bias, double* out_inv_depth);
/* dv_ba_reject: OutliersRejection / ReprojectionError (estimator/vio_util.cpp:381-444): flags[l] = 1 when the mean over landmark l's residual blocks of the
 * normalised reprojection error, times focal, exceeds 3.  pose 11 x 7, ex_pose 2 x 7, inv_depth[nlm]; ric 2 x (3x3 row-major), tic 2 x 3: the extrinsics used
 * unless ex_from_state != 0, which takes them from ex_pose (free extrinsic blocks).  count <= 24 per landmark, frames < nframes. */
int dv_ba_reject(dv_ctx* ctx, const double* pose, const double* ex_pose, const double* inv_depth, const dv_ba_factor* factors, int nfac,
                 const dv_ba_lm* landmarks, int nlm, int nframes, const double* ric, const double* tic, double focal, int ex_from_state, uint8_t* flags);

/* ---- line and dynamic-object factors: residual + Jacobians, one record per residual block.
 * Jacobians are returned in LOCAL sizes, row-major (pose blocks 6 wide: the reference's 7th column is always zero).
 * Bug-for-bug with the reference where its Jacobian is not the derivative of its residual (see be_obj.hip). ---- */
typedef struct dv_line_factor {          /* lineProjectionFactor(obs_i) + its static sqrt_info (line_projection_factor.h) */
    double obs[4];                       /* the two observed endpoints on the normalised plane: x1 y1 x2 y2 */
    double sqrt_info[4];                 /* 2x2 row-major; NOTE the reference never assigns it (zero) — SURVEY 0.6 */
} dv_line_factor;
/* out[n][34] = r[2] | d r / d pose (2x6) | d r / d ex_pose (2x6) | d r / d orth (2x4)
 * (lineProjectionFactor::Evaluate, estimator/factor/line_projection_factor.cpp:24-159) */
int dv_line_eval(dv_ctx* ctx, const dv_line_factor* factors, int n, const double* pose /* n x 7 */, const double* ex_pose /* n x 7 */,
                 const double* orth /* n x 4 */, double* out);
/* LineOrthParameterization::Plus (estimator/factor/line_parameterization.cpp:9-72): out[n][4] = orth (+) delta */
int dv_line_plus(dv_ctx* ctx, const double* orth, const double* delta, int n, double* out);

typedef struct dv_box_point { double pts_w[3]; double dims[3]; } dv_box_point;      /* BoxEncloseStereoPointFactor(point_w, dims) */
/* out[n][21] = r[3] | d r / d pose_obj (3x6)   (estimator/factor/box_factor.cpp:523-565) */
int dv_box_enclose_eval(dv_ctx* ctx, const dv_box_point* points, int n, const double* pose_obj /* n x 7 */, double* out);
/* out[n][4] = r | d r / d box (1x3)            (BoxDimsFactor, box_factor.cpp:728-743) */
int dv_box_dims_eval(dv_ctx* ctx, const double* dims /* n x 3 */, const double* box /* n x 3 */, int n, double* out);
/* out[n][39] = r[3] | d r / d pose_body (3x6, zero) | d r / d pose_obj (3x6)   (BoxOrientationFactor, box_factor.cpp:752-806) */
int dv_box_orientation_eval(dv_ctx* ctx, const double* R_cioi /* n x 9 */, const double* R_bc /* n x 9 */, const double* pose_body /* n x 7 */,
                            const double* pose_obj /* n x 7 */, int n, double* out);

/* ProjectionInstanceFactor(pts_j, pts_i, velocity_j, velocity_i, td_j, td_i, cur_td) (estimator/factor/project_instance_factor.h:30-60): the
 * reprojection factor of a point ON a moving object — observed in frame j with inverse depth inv_dep_j, carried through the object's poses at j
 * and i into camera i.  The reference ships it switched off (every AddResidualBlock in InstanceManager::AddResidualBlockForJointOpt is commented
 * out, estimator_insts.cpp:1258-1419); it is provided as an operator because BASELINE.json's north_star names it.  112 bytes per record. */
typedef struct dv_inst_proj_factor { double pts_j[3], pts_i[3], vel_j[2], vel_i[2], td_j, td_i, cur_td, pad_; } dv_inst_proj_factor;
/* ProjectionInstanceFactor::Evaluate (project_instance_factor.cpp:27-172); parameter blocks per record: body pose j, body pose i, ex_pose[0],
 * object pose j, object pose i (n x 7 each: p, qx qy qz qw), inv_dep_j (n).
 * out[n][64] = r[2] | J_body_j | J_body_i | J_ex | J_obj_j | J_obj_i (2x6 each, tangent space, row-major) | J_inv_dep (2).
 * Bug-for-bug: J_inv_dep has the reference's + sign and un-compensated pts_j (:166). */
int dv_inst_proj_eval(dv_ctx* ctx, const dv_inst_proj_factor* factors, int n, const double* pose_bj, const double* pose_bi, const double* ex_pose,
                      const double* pose_oj, const double* pose_oi, const double* inv_dep_j, double* out);

/* ---- the per-frame object solve (the numeric part): replaces ceres::Solve inside
 * InstanceManager::Optimization (estimator/estimator_insts.cpp:772-807) for the problem that
 * AddInstanceParameterBlock / AddResidualBlockForInstOpt build (estimator_insts.cpp:989-1245):
 *   variables   per object: para_state[0..kWinSize] (pose, PoseLocalParameterization or — plane_constraint —
 *               PoseConstraintLocalParameterization) and para_box[0] (dims)
 *   residuals   per (object, frame) with a 3-D detection: BoxDimsFactor(detection dims) on para_box with HuberLoss(1.0)
 *               and BoxOrientationFactor(R_cioi, ric[0]) on (body pose, para_state[frame]) without a loss;
 *               per triangulated object point: BoxEncloseStereoPointFactor(p_w, inst.box3d->dims) on
 *               para_state[frame] with HuberLoss(1.0); the dims inside this factor are the values para_box holds
 *               when the solve starts (the reference passes them by value)
 *   options     DENSE_SCHUR + DOGLEG, max_num_iterations = max_iters, wall-clock budget disabled (as dv_ba_solve).
 * The body poses enter BoxOrientationFactor with a zero Jacobian (sic), so they never move; they only count in the
 * parameter-tolerance norm, as they do in ceres.  Blocks without a residual are not variables (ceres removes them).
 * The Hessian of this problem is block diagonal (6x6 per object pose, 3x3 per dims block); the trust region is global. ---- */
typedef struct dv_obj_box {              /* Instance::boxes3d[frame]: one per (object, frame) at most */
    int32_t obj, frame;
    double dims[3];                      /* Box3D::dims of the detection */
    double R_cioi[9];                    /* Box3D::R_cioi(), row-major */
} dv_obj_box;
typedef struct dv_obj_point { int32_t obj, frame; double p_w[3]; } dv_obj_point;      /* FeaturePoint::p_w of a triangulated observation */
typedef struct dv_obj_problem {
    int32_t n_obj, n_boxes, n_points, max_iters;
    int32_t plane_kind;                  /* 0 PoseLocalParameterization, 1 plane constraint with IMU (dz = 0), 2 vision only (dy = 0) */
    int32_t reserved;
    double* state;                       /* n_obj x 11 x 7 [p, qx qy qz qw]   in/out: Instance::para_state */
    double* dims;                        /* n_obj x 3                          in/out: Instance::para_box  */
    const double* body_pose;             /* 11 x 7: body.para_pose */
    double R_bc[9];                      /* body.ric[0], row-major */
    const dv_obj_box* boxes; const dv_obj_point* points;
} dv_obj_problem;
int dv_obj_solve(dv_ctx* ctx, dv_obj_problem* problem, dv_ba_summary* summary);
/* InstanceManager::Optimization (estimator/estimator_insts.cpp:772-807) of several dv_batch members in ONE launch: problems[i] is solved on member members[i] (index into
 * the array dv_batch_create was given; every member at most once) by one workgroup of a shared grid on the group's object stream, summaries[i] receives its summary.
 * States, dims and summaries carry the bits dv_obj_solve gives for the same problem on the same member.  Argument checks and messages are dv_obj_solve's, reported on
 * the problem's member and on the group's first member; all problems are checked before anything is launched, so one bad problem among good ones leaves every problem
 * untouched.  n = 1 uses dv_obj_solve's own kernel.  This is what dv_batch_enqueue does for the object branches of the group's dynamic members (below). */
int dv_batch_obj_solve(dv_batch* batch, const int* members, dv_obj_problem* const* problems, int n, dv_ba_summary* summaries);
/* object solves of the group so far, from dv_batch_enqueue rounds and dv_batch_obj_solve calls alike: shared launches, the jobs in them (jobs / launches = solves per
 * launch), and solves that were launched alone (a round with one object solve, a member collected without dv_batch_enqueue counts where it is launched: not here) */
int dv_batch_obj_info(dv_batch* batch, long long* launches, long long* jobs, long long* single);

/* ---- the line-only refinement: replaces ceres::Solve inside Estimator::OptimizationWithOnlyLine
 * (estimator/estimator.cpp:345-395) for the problem AddLineResidualBlock builds (:222-253): one LineOrthParameterization block
 * (body.para_line_features[k], 4 parameters) per triangulated line landmark, one lineProjectionFactor per observation with
 * CauchyLoss(1.0), every pose / extrinsic block constant; DENSE_SCHUR + DOGLEG, max_num_iterations = max_iters.
 * sqrt_info is lineProjectionFactor::sqrt_info (the reference leaves it zero: the solve then returns at once). ---- */
typedef struct dv_line_obs { int32_t line, frame; double obs[4]; } dv_line_obs;      /* LineFeature::line_obs of landmark `line` in window frame `frame` */
typedef struct dv_line_problem {
    int32_t n_lines, n_obs, max_iters, reserved;
    double* orth;                        /* n_lines x 4   in/out: body.para_line_features */
    const double* pose;                  /* 11 x 7: body.para_pose */
    const double* ex_pose;               /* 7: body.para_ex_pose[0] */
    double sqrt_info[4];                 /* 2x2 row-major */
    const dv_line_obs* obs;
} dv_line_problem;
int dv_line_solve(dv_ctx* ctx, dv_line_problem* problem, dv_ba_summary* summary);

/* ---- Estimator (estimator/estimator.h:55-164): IMU buffer + one ProcessMeasurements iteration per call ---- */
typedef struct dv_est_config {          /* para (estimator/vio_parameters.cpp:19-83), cfg flags, extrinsics (utils/parameters.cpp) */
    int32_t use_imu, stereo, plane_constraint, max_iters;      /* imu, num_of_cam==2, plane_constraint, max_num_iterations */
    double keyframe_parallax;           /* pixels; kMinParallax = keyframe_parallax / 460 */
    double init_depth, g_norm, td;      /* INIT_DEPTH, g_norm, td */
    double acc_n, gyr_n, acc_w, gyr_w;
    double ric[2][9], tic[2][3];        /* body_T_cam0 / body_T_cam1: rotation (row-major) and translation */
    /* dynamic mode (cfg::slam == SLAM::kDynamic): the object branch of ProcessImage (estimator.cpp:1562-1622,1653-1676) */
    int32_t dynamic;                    /* 1: dv_est_process_dynamic* run the InstanceManager */
    int32_t use_det3d;                  /* use_det3d: objects are initialised from 3-D detections */
    int32_t instance_init_min_num;      /* instance_init_min_num (viode.yaml:135: 4) */
    int32_t estimate;                   /* bit 0: cfg::is_estimate_ex == 1 (estimate_extrinsic 1: the extrinsics are optimised around the configured ones from the first full window with
                                           |Vs[0]| > 0.2 on — openExEstimation, estimator.cpp:87-95,632), bit 1: cfg::is_estimate_td (estimate_td 1, :98-100).  estimate_extrinsic 2
                                           (no initial guess: CalibrationExRotation, estimator.cpp:1426-1445) is not built.  0 in every shipped YAML.  Refused together with dynamic = 1
                                           (dv_est_create fails): the object branch's factors carry no extrinsic / td Jacobians (the reference's do, estimator.cpp:205) */
    double static_inst_threshold;       /* static_inst_threshold: scene-flow norm above which an object counts as moving (default 10) */
    /* line mode (cfg::use_line): line landmarks in FeatureManager, TriangulateLineMono, OptimizationWithOnlyLine, AddLineResidualBlock (estimator.cpp:224-253,345-395) */
    int32_t use_line, line_min_obs;     /* use_line ; line_min_obs (default 5, vio_parameters.cpp:47-54) */
    double line_sqrt_info[4];           /* lineProjectionFactor::sqrt_info, 2x2 row-major.  The reference never assigns it (zero: SURVEY 0.6) — then the line blocks are
                                           inert and only enter the window solve's parameter-tolerance norm.  Non-zero weights are honoured by the line-only solve;
                                           the window solve refuses them (line e-blocks inside the Schur elimination are not built). */
} dv_est_config;

typedef struct dv_est_state {
    int32_t frame, nonlinear /* solver_flag == kNonLinear */, margin_old /* margin_flag == kMarginOld */, n_landmarks, n_long, iterations;
    double initial_cost, final_cost;
    double window[11][16];              /* body.Ps / Rs (as qx qy qz qw) / Vs / Bas / Bgs per window slot */
} dv_est_state;

int dv_est_create(dv_ctx* ctx, const dv_est_config* cfg);       /* Estimator::Estimator + SetParameter */
/* diagnostics, after dv_debug_set(ctx, "hash_log", 1): per window solve [counter, hash of the states uploaded, hash of the tables uploaded, hash of the states downloaded,
 * hash of the outlier flags consumed, iterations]; two runs of the same sequence must agree row by row */
int dv_est_debug_hash_log(dv_ctx* ctx, unsigned long long* rows6, int cap, int* n_rows);
/* the same on the device side: per fused window solve [counter, hash of the uploaded block as it arrived, of the prior A and b the round reads, of x after the round, of the
 * candidate buffer (gauge-fixed copy), of the control block] */
int dv_ba_debug_dev_log(dv_ctx* ctx, unsigned long long* rows7, int cap, int* n_rows);
/* and per LAUNCH of the round: for every fused solve 16 slots x 5 launch kinds (head evaluation, head reduce, solve, candidate evaluation, candidate reduce) x 16 hashed buffers */
int dv_ba_debug_slot_log(dv_ctx* ctx, unsigned long long* vals, long long cap_vals, long long* n_vals, int* row_len);
/* the linearisation buffers of the window solve as the device holds them (bit comparisons of the evaluation across library versions): which = 0 packets
 * [928][1024] doubles, 1 imu_out [10][936], 2 prior_out [193], 3 cand_cost [1011], 4 lm_obs [1000] int32, 5 Hd [178][178], 6 Sc [178 * 178], 7 gvec [356], 8 scale_l [1000] (the
 * landmarks' Jacobi scales, written by the reduce of a first iteration); set = 0 / 1 (ignored for 3, 4, 8).  host != NULL: the first `bytes` bytes of the buffer, after the BA stream has drained; host == NULL: the whole buffer is filled with 0xFF bytes, so
 * that what a later launch does not write shows.  -1: bad argument or `bytes` beyond the buffer */
int dv_ba_debug_buffer(dv_ctx* ctx, int which, int set, void* host, long long bytes);
/* the mask bytes the dynamic front end's kernels wrote, for tests, after the frame was collected: which = 0 the background tracker's working mask of the last frame that
 * was staged or unmasked into the library's own buffer (w x h = the configured size), which = 1 the ROI mask of object track_id of the last dv_inst_track_enqueue*
 * (w x h = its rectangle).  Rows of *pitch = w rounded up to 16 bytes, padding columns included; host takes *pitch * *h bytes (cap_bytes: its size).  -1: bad argument,
 * a frame in flight, no such mask / object, or cap_bytes too small */
int dv_front_debug_mask(dv_ctx* ctx, int which, uint32_t track_id, void* host, long long cap_bytes, int* w, int* h, int* pitch);
int dv_est_reset(dv_ctx* ctx);                                   /* Estimator::ClearState + SetParameter */
int dv_est_input_imu(dv_ctx* ctx, double t, const double* acc, const double* gyr);      /* Estimator::InputIMU */
/* one iteration of Estimator::ProcessMeasurements (estimator.cpp:1786-1863): IMU interval, pre-integration,
 * ProcessImage (keyframe test, triangulation, Optimization on the GPU, marginalization on the GPU, outlier rejection,
 * sliding window).  returns 0 = processed, 1 = IMU data does not cover t yet (feed more, call again), <0 error.
 * The frame's pose is out->window[10] once nonlinear (what SaveBodyTrajectory writes, utils/io/output.cpp:199-227). */
int dv_est_process(dv_ctx* ctx, const dv_feat* feats, int n, double t, dv_est_state* out);
/* the same in two phases, like dv_track_stereo_enqueue/_collect: _begin does the host bookkeeping and ENQUEUES the window
 * solve + marginalization on the ctx's BA stream (returns 0, or 1 = IMU data missing: nothing was started); _end waits,
 * applies the result (outlier rejection, window slide) and fills `out`.  Between the two the caller may enqueue the next
 * frame's tracking and feed IMU samples — thread T2's work overlapping T3's, as in the reference (system/main.cpp:394-404). */
int dv_est_process_begin(dv_ctx* ctx, const dv_feat* feats, int n, double t);
int dv_est_process_end(dv_ctx* ctx, dv_est_state* out);
/* Estimator::IMUAvailable(t + td) (estimator/estimator.h:128-133): 1 = the IMU buffer reaches the frame time, 0 = not yet (the "wait for imu" test of
 * ProcessMeasurements BEFORE it pops the frame from feature_queue, estimator.cpp:1800-1805), <0 error.  Always 1 without an IMU. */
int dv_est_imu_available(dv_ctx* ctx, double t);

/* one entry of FeatureBackground::lines (basic/frontend_feature.h:41-44): the matched line `id` of this frame with the undistorted normalised end points
 * (Line::StartPt / EndPt of FrameLines::un_lines) in the left image and, if matched, in the right one.  The LSD / LBD detector that produces them is upstream. */
typedef struct dv_line_row { uint32_t id; int32_t has_right; double left[4], right[4]; } dv_line_row;      /* x1 y1 x2 y2 */
/* frame.features.lines of the NEXT dv_est_process* call (use_line) */
int dv_est_set_lines(dv_ctx* ctx, const dv_line_row* lines, int n);
/* FeatureManager::line_landmarks after the last frame: per landmark id, start_frame, observation count, is_triangulation, line_plucker (n, v; camera frame of
 * start_frame), ptw1 / ptw2 (the `lines` marker publisher) */
typedef struct dv_line_landmark { int32_t id, start_frame, n_obs, is_triangulation; double plucker[6], ptw1[3], ptw2[3]; } dv_line_landmark;
int dv_est_get_lines(dv_ctx* ctx, dv_line_landmark* out, int cap, int* n_out);
/* FrameLines::UndistortedLineEndPoints (front_end side of TrackImageLine, line_detector): end points (x1 y1 x2 y2 pixels) -> normalised, undistorted */
int dv_undistort_lines(dv_ctx* ctx, const dv_cam* cam, const float* lines_xyxy, int n, double* out_xyxy);

/* The LINE TRACKER on the device: a frame's detected key lines and their 32-byte LBD descriptors -> the frame's dv_line_rows, ready for dv_est_set_lines.  Reference:
 * LineDetector::TrackLeftLine / TrackLine / TrackRightLine (line_detector/line_detector.cpp:101-297) behind LineDetector::Detect (:60-98) and in front of
 * FrameLines::SetLines / UndistortedLineEndPoints (basic/frame_lines.cpp:15-45) and SetOutputFeats' `lines` map (front_end/background_tracker.cpp:167-189,373-389).
 * LSD and the LBD descriptor themselves stay upstream.  The previous left frame's lines, ids, descriptors and track counts are resident; so is the id counter.
 *   input        per line what Detect leaves (:82-96): KeyLine::startPointX/Y, endPointX/Y, angle, lineLength (dv_key_line, float32) and one descriptor row.
 *   match        BinaryDescriptorMatcher::match(query, train) (thirdparty/line_descriptor/src/binary_descriptor_matcher.cpp:197-254) with Mihasher(256, 32), K = 1: a
 *                multi-index hash search (:635-753) over 32 one-byte substrings (bitops_custom.hpp:99-123) whose buckets keep ascending train order (:926-947).  Below
 *                distance 32 it never leaves search radius s = 0 and stops at substring k = the minimum distance, so it returns, among the train rows at the minimum
 *                distance, the one least by (index of its first byte equal to the query's, train index).  Only distance < 30 is accepted downstream: the kernel
 *                evaluates that closed form and reports "no match" from 30 on (above 128 the reference leaves its result unwritten).  Either side empty: no matches
 *                (:201-205).
 *   gate         distance < 30, serr . serr < 200 * 200, eerr . eerr < 200 * 200, abs(angle1 - angle2) < 0.1 (line_detector.cpp:116-124): serr = query start - train END,
 *                eerr = query end - train END (sic), cv::Point2f arithmetic: float32 products and one float32 add, never fused; abs taken as the float overload.
 *                A matched line takes the train line's id; several query lines may take one train line and so one id.  The "-1" id is 0xFFFFFFFF.
 *   new ids      every unmatched line takes the next id of the counter in line order, the lines the quota then drops included (:146-158).
 *   quota        unmatched lines are "h" when angle is in [3.14/4, 3*3.14/4] or [-3*3.14/4, -3.14/4] (double literals), else "v" (:164-176).  Output order: tracked lines
 *                in their order, then the first 35 - h_tracked new h lines, then the first 35 - v_tracked new v lines (:190-223).
 *   first frame  (no previous frame, :229-234) every line a fresh id, no quota, no counts.  A previous frame WITHOUT lines is not a first frame.
 *   counts       curr[id] = prev[id] + 1 for matched ids (missing: 0); a v top-up gets 1, an h top-up NO entry (:128-139,218).  Reported: the map's value, 0 for none.
 *   right        matched against the left set after the quota, same gate; only matched right lines are kept, in right order (:246-297).
 *   rows         one per left id in ascending id (the std::map's order): the first left line of the id (map::insert, background_tracker.cpp:376-380) and, if any, the
 *                FIRST right line of the id — vec_feat[1] is the only right entry FeatureManager::AddFeatureCheckParallax reads (estimator/feature_manager.cpp:127-128).
 *                End points lifted with the ctx's cam0 / cam1 exactly as dv_undistort_lines lifts them.
 * Differences, declared: one id counter per tracker, starting at 0 (the reference's global_line_id is a member of its one LineDetector); no match from distance 30 on.
 * A ctx has ONE tracker: the resident previous frame and the id counter belong to the dv_ctx, so every caller of dv_line_track_* on a ctx (two LineDetector objects of
 * the shim, say) feeds the same sequence of frames.  Two independent line streams take two ctxs.
 * dv_line_track_check: the refusals of _enqueue without a device (more than DV_LINE_MAX lines in an image, null or misaligned pointers, unknown memory kind).
 * dv_line_track_reset: no previous frame, counter back to 0.
 * _enqueue: on the ctx's stream.  mem = DV_MEM_HOST (all four arrays staged; valid until the call returns) or DV_MEM_DEVICE / DV_MEM_PINNED (read in place until the
 * collect; each pointer may be of either in-place kind).  right_lines = right_desc = NULL, n_right = 0: no right image.  n_left = 0, n_right = 0 are ordinary frames.  One
 * frame may be in flight.  ONE launch; no host round trip between _enqueue and _collect: the frame's only device -> host traffic is the rows, the per-line words and a
 * few counters through pinned memory.
 * _collect: rows[min(cap, *n_rows)]; per surviving left line, in output order, its id, the index of the line in the enqueued array (*_src) and its track count; per
 * surviving right line its id and index.  The per-line arrays hold DV_LINE_MAX entries or are NULL.
 * dv_line_match: the match step alone, in operator form on host memory (nq, nt <= DV_LINE_MAX): train_idx[i] = the row BinaryDescriptorMatcher::match returns for query
 * i and distance[i] its distance; -1 and 0 where the minimum distance is >= 30. */
#define DV_LINE_MAX 512
#define DV_LINE_DESC_BYTES 32
typedef struct dv_key_line { float sx, sy, ex, ey, angle, length; } dv_key_line;
int dv_line_track_check(const dv_key_line* left_lines, const uint8_t* left_desc, int n_left, const dv_key_line* right_lines, const uint8_t* right_desc, int n_right, int mem);
int dv_line_track_reset(dv_ctx* ctx);
int dv_line_track_enqueue(dv_ctx* ctx, const dv_key_line* left_lines, const uint8_t* left_desc, int n_left, const dv_key_line* right_lines, const uint8_t* right_desc, int n_right, int mem);
int dv_line_track_collect(dv_ctx* ctx, dv_line_row* rows, int cap, int* n_rows, uint32_t* left_ids, int32_t* left_src, int32_t* left_cnt, int* n_left_out,
                          uint32_t* right_ids, int32_t* right_src, int* n_right_out);
int dv_line_match(dv_ctx* ctx, const uint8_t* query_desc, int nq, const uint8_t* train_desc, int nt, int32_t* train_idx, int32_t* distance);

/* The LBD DESCRIPTOR on the device: a gray image and the key lines LSD left -> the selected key lines and their 32-byte rows, in device buffers of the layout
 * dv_line_track_enqueue(..., DV_MEM_DEVICE) takes: the second half of LineDetector::Detect (line_detector/line_detector.cpp:78-97).  LSD itself stays upstream.  Reference:
 * BinaryDescriptor::compute -> computeImpl / computeSobel / computeLBD (thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:350-398,539-687,1026-1372).
 *   lines        every line is at octave 0 (Detect keeps no other; a caller drops the rest before the call), where sPointInOctave = startPoint: a dv_key_line plus
 *                KeyLine::numOfPixels.  num_pixels = NULL: max(|rint(ex) - rint(sx)|, |rint(ey) - rint(sy)|) + 1, cv::LineIterator's count for a segment inside the image.
 *   gradients    cv::GaussianBlur(img, Size(5, 5), 1) then cv::Sobel(CV_16SC1, 1, 0, 3) and (0, 1, 3), BORDER_REFLECT_101 both.  The blur is separable 8-bit fixed point,
 *                weights 14 62 104 62 14 / 256, exact sums, one rounding at the end — a DECLARED CHOICE, not pinned against OpenCV.  The Sobel half is exact.
 *   descriptor   computeLBD's float32 evaluation order, operation by operation, as an x86-64 build without FMA runs it: row starts and samples stepped by repeated
 *                addition, (short) round() half away from zero, clamped; row sums in pixel order; band sums in row order; the tail (:1246-1340) as written; sqrt and
 *                1 / sqrt correctly rounded.  dL = ((float)cos((double)angle), (float)sin((double)angle)), computed on the host per line — a DECLARED CHOICE of the overload.
 *                NaN travels: a flat image gives 32 zero bytes.  Bit i of byte k is f1[i] > f2[i] over combinations[k].
 *   selection    line i is kept iff length >= min_length (the reference: 60) and, with a mask (w x h bytes, the image's memory kind), the mask is non-zero at both end
 *                points rounded like cv::Point(Point2f) (ties to even).  DEVIATION, declared: an end point that rounds outside the mask drops the line (the reference
 *                reads outside the matrix).  Survivors keep the input order.
 * dv_lbd_check: the refusals of _enqueue without a device: more than DV_LINE_MAX lines, null or misaligned pointers, unknown memory kind, stride < w, w or h above 32767
 * (the descriptor's 16-bit coordinates), and — for lines the host can read — a non-finite coordinate or angle, num_pixels < 1 or > w + h.  Lines in device
 * memory get the value checks at the enqueue.  dv_lbd_num_pixels: the library's rule for n host lines.
 * _enqueue: on the ctx's stream.  cam = 0 / 1 selects one of two buffer sets, so both images of a stereo frame are in flight together; one frame per cam may be in
 * flight.  image / mask: DV_MEM_HOST (staged), DV_MEM_DEVICE or DV_MEM_PINNED (read in place until the collect).  lines / num_pixels: any kind, valid until the call
 * returns.  The directions are host work, so lines in DV_MEM_DEVICE are FETCHED first: that enqueue BLOCKS until the ctx's stream is idle — the other cam's frame in flight
 * and whatever else is queued on the stream included — before it queues its own work; host and pinned lines do not block.  The mask has no memory kind of its own: it
 * is read as the image's kind (a device image with a host mask takes a copy by the caller).  n = 0 is an ordinary empty frame.
 * _collect: *n_kept and src[n_kept] (each survivor's index in the enqueued array; DV_LINE_MAX entries or NULL); *dev_lines / *dev_desc = the device buffers, valid
 * until the next enqueue on that cam; host_lines / host_desc (DV_LINE_MAX entries, or NULL) ask for host copies.  Without them the frame's only device -> host
 * traffic is the count and src.
 * dv_lbd_debug: for tests — the gradient images (w x h int16 each) and the 72 floats of every ENQUEUED line, before selection, of the last frame of that cam. */
int dv_lbd_check(int w, int h, int stride, const dv_key_line* lines, const int32_t* num_pixels, int n, int lines_mem, const uint8_t* mask, int mask_stride);
int dv_lbd_num_pixels(const dv_key_line* lines, int n, int32_t* out);
int dv_lbd_describe_enqueue(dv_ctx* ctx, int cam, const uint8_t* image, int stride, int w, int h, int image_mem, const dv_key_line* lines, const int32_t* num_pixels, int n,
                            int lines_mem, const uint8_t* mask, int mask_stride, float min_length);
int dv_lbd_describe_collect(dv_ctx* ctx, int cam, int* n_kept, int32_t* src, const dv_key_line** dev_lines, const uint8_t** dev_desc, dv_key_line* host_lines, uint8_t* host_desc);
int dv_lbd_debug(dv_ctx* ctx, int cam, int16_t* dx_out, int16_t* dy_out, float* float_desc_out);

/* ---- the members of Estimator the callbacks and publishers use besides ProcessMeasurements (estimator/estimator.h:55-164) ---- */
/* Estimator::ChangeSensorType (estimator.cpp:697-726; the /vins_imu_switch, /vins_cam_switch callbacks): switching the IMU on restarts the estimator
 * (ClearState + SetParameter), switching it off drops the prior.  use_stereo = 0 is refused (monocular initialisation is out of scope). */
int dv_est_change_sensor_type(dv_ctx* ctx, int use_imu, int use_stereo);
/* latest_time / latest_P / latest_Q (qx qy qz qw) / latest_V: the newest frame's state propagated by every IMU sample fed since — FastPredictIMU inside
 * InputIMU and UpdateLatestStates (estimator.cpp:729-742,1376-1418): what PubLatestOdometry publishes on `imu_propagate`.  Returns 1 while not initialised. */
int dv_est_get_latest(dv_ctx* ctx, double* t, double* P3, double* Q4, double* V3);
/* body.ric / body.tic (row-major rotations, translations of cam0 / cam1) and body.td as the last Double2vector left them: the configured values unless dv_est_config::estimate
 * frees them (what pubOdometry writes out when estimate_extrinsic is on, utils/io/visualization.cpp:94-118).  Any pointer may be NULL. */
int dv_est_get_extrinsics(dv_ctx* ctx, double* ric18, double* tic6, double* td);
/* Health of the marginalization (MarginalizationInfo::marginalize, factor/marginalization_factor.cpp:284-304).  The reference zeroes the eigenvalues
 * <= 1e-8 of A_mm silently; the device skips the LDL^T pivots <= 1e-8 (also negative ones) — the same pseudo-inverse whenever the deficient directions
 * are single columns (a landmark without information), order dependent otherwise.  So the event is counted and readable:
 *   checked   marginalizations whose scalars have come back (the estimator reads them one frame late: they run behind the state download)
 *   clamped   of those, how many skipped at least one pivot
 *   last4     c0, smallest pivot of A_mm, clamp flag (!= 0: skipped), rank of A_mm — of the last one that came back */
int dv_est_get_marg_health(dv_ctx* ctx, long long* checked, long long* clamped, double* last4);

/* ---- the per-frame host loop of the reference's threads T2 (FeatureTrack, system/main.cpp:178-330) + T3 (the estimator thread, :394-404) in C++ inside the library:
 * one call runs n_rounds frames of one or many sequences.  Per sequence the order of pipeline.py: collect tracking(k), IMU up to t_k, dv_est_process_begin(k),
 * enqueue tracking(k+1), IMU up to t_k+1, dv_est_process_end(k) — the front end of frame k+1 overlaps the back end of frame k.  With group_size > 1 the sequences
 * are grouped into dv_batch groups of that size: the begin phases of a group run back to back, ONE dv_batch_enqueue launches the iteration slots of all its window
 * solves, and the host turns to the next group while they run (config 4 of BASELINE.json, "batched").  `threads` host threads each drive their own groups (at most one thread per group; more are not used).
 * Opt-in: dv_runner_set(runner, "teams", 1) before the first run lets threads / groups host threads (a multiple) share the host phases of one group's members between barriers
 * (bit-identical to the single-thread run in tests/test_runner.py; off by default).
 * Round 4 found single members of multi-group runs intermittently leaving their trajectory: a missing workgroup barrier in the accept decision (be_accept_body), exposed when a
 * second group kept the CUs busy; fixed (shared launch: 8 of 30 runs differing before, 0 of 60 after — DESIGN.md 0).  Check every sequence's result when you change this path:
 * bench.py does, and refuses to report a run that fails the check; scripts/dbg/multiseq_first_diff.py compares bit for bit against the single-thread run.
 * The contexts (each with its estimator: dv_est_create) stay the caller's; frames are referenced, not copied (device or host memory: dv_seq_input::mem).
 * dynamic_vins_amd/host/dvins_node.cpp is the ROS-free node built on it (image directory + IMU csv in, `<seq>_<mode>_Odometry.txt` out). */
typedef struct dv_seq_input {
    const uint8_t* const* left; const uint8_t* const* right;      /* [n_frames] gray images of the configured size (DV_FMT_BGR is not taken here: the default row stride is the width).  Contexts with installed undistortion maps take the distorted frames, in a group's shared launches too */
    const double* times; int32_t n_frames, mem /* DV_MEM_HOST / DV_MEM_DEVICE */, stride /* bytes per row, 0 = width */, ba_stride /* 2: only every 2nd tracked frame goes to the back end (system/main.cpp:300-307); 0 / 1: every frame */;
    const double* imu_t; const double* imu_acc; const double* imu_gyr; int32_t n_imu, reserved2;      /* [n_imu], [n_imu][3], [n_imu][3]; n_imu 0 for vision-only */
} dv_seq_input;
/* dynamic mode of a sequence (cfg::slam == kDynamic; the estimator must have been created with dv_est_config::dynamic = 1 and the tracker configured with
 * dv_inst_config): per frame what thread T1 / the perception front end of the reference attaches to the SemanticImage (system/main.cpp:59-171) — the inverse merged
 * instance mask, the detections with their track ids and ROI masks, the 3-D detections (use_det3d) and the disparity map the extra points are sampled from.  The runner
 * then drives the reference's dynamic loop per frame: TrackSemanticImage + InstsTrack (both enqueued together, thread T2), collect, dv_est_process_dynamic_begin_ego,
 * the NEXT frame's tracking, dv_est_process_dynamic_attach (the object branch beside the window solve), dv_est_process_end (estimator.cpp:1562-1676).
 * All arrays have n_frames entries and must outlive the runner; masks of detections are host memory, inv_mask / disp follow their *_mem. */
typedef struct dv_inst_det dv_inst_det; typedef struct dv_box3d dv_box3d;      /* defined with the dynamic-mode entries below */
typedef struct dv_seq_dynamic {
    const uint8_t* const* inv_mask; int32_t mask_mem /* DV_MEM_*: must equal dv_seq_input::mem (frames and mask are handed to dv_track_stereo_enqueue with ONE memory kind; checked) */, mode /* DV_MODE_SEMANTIC (default when 0 is passed is RAW: set it) or DV_MODE_NAIVE */;
    const dv_inst_det* const* dets; const int32_t* n_dets;
    const dv_box3d* const* boxes3d; const int32_t* n_boxes3d;      /* may be NULL (no 3-D detector) */
    const float* const* disp; int32_t disp_mem, disp_stride /* bytes, 0 = 4 * width */; double baseline;      /* disp may be NULL: dv_inst_det::points are handed through */
    const uint32_t* const* right_keys; int32_t right_keys_mem;      /* VIODE: per frame the key image of seg1 (dv_inst_set_right_keys), tightly packed; may be NULL */
    int32_t static_as_background;      /* para::is_static_inst_as_background (vio_parameters.h:86: the reference's default is 1): before tracking frame f the pixels of the instances the
                                          estimator reported static leave the merged mask (dv_est_get_static_instances of the newest back-end frame <= f - 2 -> dv_track_unmask_static;
                                          system/main.cpp:194,217-245).  The reference reads that report across threads without an order; the lag of two frames is this runner's, in every layout */
} dv_seq_dynamic;
/* choice T1: the static-instance report applied to frame f is that of the newest back-end frame <= f - DV_STATIC_REPORT_LAG */
#define DV_STATIC_REPORT_LAG 2
typedef struct dv_runner dv_runner;
/* slam_type naive of a sequence (system/main.cpp:263-265: FeatureTrack -> TrackImageNaive): per frame [n_frames] the inverse merged instance mask (0 = object pixel;
 * VIODE::SetViodeMaskSimple or the detector's SetBackgroundMask) in the frames' memory kind, tracked with `mode` = DV_MODE_NAIVE (GPU tracker's + GPU detector's rules).
 * The back end stays the raw one.  Before the first dv_runner_run; a masked sequence inside a dv_batch group keeps its own tracking launches. */
int dv_runner_set_mask(dv_runner* runner, int seq, const uint8_t* const* inv_mask, int mask_mem, int mode);
/* Before the first dv_runner_run.  A dynamic sequence may be a member of a dv_batch group (group_size > 1), beside raw, naive and other dynamic members: its window
 * solve shares the group's launches, its object solve shares ONE launch with the other dynamic members' (dv_batch_enqueue), its tracking keeps its own launches
 * (TrackSemanticImage + InstsTrack are not shared across members).  Inside a group it always runs the one-thread order whatever "tracker_thread" says — the group's
 * host thread (or its team thread) is its T3, the tracker ring is a feature of group_size 0 — per member: end of frame k-1, dv_est_process_dynamic_begin_ego(k), enqueue
 * tracking(k+1), dv_est_process_dynamic_attach(k), then ONE dv_batch_enqueue for the group, then collect tracking(k+1).  Every member's results are bit-identical to
 * its own run with group_size 0 and "tracker_thread" 0. */
int dv_runner_set_dynamic(dv_runner* runner, int seq, const dv_seq_dynamic* dyn);
/* Dynamic mode of a sequence fed with LABEL IMAGES, one frame at a time: thread T1's stage (ImageProcessor::Run, image_process/image_process.cpp:161-178;
 * VIODE::SetViodeMaskAndRoi, utils/dataset/viode_utils.cpp:21-218) runs per frame inside the loop (dv_viode_frame_enqueue / _collect) instead of as a pre-pass whose
 * masks, detections and key images dv_seq_dynamic carries.  The sequence then runs the dynamic loop of dv_runner_set_dynamic — one-thread order or T2 beside T3
 * ("tracker_thread") — with the key-image entries: dv_track_unmask_static_keys (the static report with the same lag rule, DV_STATIC_REPORT_LAG, choice T1),
 * dv_track_stereo_enqueue with the device-resident inverse mask, dv_inst_set_right_keys, dv_inst_track_enqueue_keys (FeatureTrack, system/main.cpp:196-250).  The stage of
 * frame k + 1 is enqueued right behind the tracking of frame k, so its boxes have arrived when the host turns to frame k + 1.  Results are bit-identical to
 * dv_runner_set_dynamic fed the pre-computed masks, detections (ROI masks cut from the key image) and right key images of the same label images.
 * Before the first dv_runner_run; the frames must be DV_MEM_DEVICE or DV_MEM_PINNED with row stride = width (the inverse mask stays on the device and travels with them).
 * Refused with "dv_runner_set_viode: a sequence of a dv_batch group is not supported ..." for a member of a group (group_size > 1: the group's shared unmask launch reads
 * host masks); the runner stays usable. */
typedef struct dv_seq_viode {
    const uint8_t* const* seg0; const uint8_t* const* seg1;      /* [n_frames] label images of the left / right camera (B G R); seg1 may be NULL (no key test in the right image) */
    int32_t mem /* DV_MEM_* of the label images */, stride /* bytes per row, 0 = 3 * width */;
    const uint32_t* dyn_keys; int32_t nkeys /* 1..64 */, min_inst_size /* rectangles below it are not handed to the object tracker (dvins_node: 8) */;
    int32_t static_as_background, reserved;      /* as dv_seq_dynamic::static_as_background */
    const float* const* disp; int32_t disp_mem, disp_stride; double baseline;      /* as in dv_seq_dynamic; disp may be NULL */
} dv_seq_viode;
int dv_runner_set_viode(dv_runner* runner, int seq, const dv_seq_viode* viode);
/* Dynamic mode of a sequence fed with the detector's INSTANCE-MASK STACKS, one frame at a time (the detector branch of ImageProcessor::Run, image_process/image_process.cpp:160-170;
 * the KITTI-tracking and ZED dynamic configurations): thread T1's stage runs per frame inside the loop (dv_inst_stack_frame_enqueue / _collect), and the sequence runs the
 * dynamic loop of dv_runner_set_dynamic — one-thread order or T2 beside T3 ("tracker_thread") — on the plane entries: dv_track_unmask_static_planes (same lag rule,
 * DV_STATIC_REPORT_LAG), dv_track_stereo_enqueue with the device-resident inverse mask, dv_inst_track_enqueue_planes.  The stage of frame k + 1 is enqueued right behind the
 * tracking of frame k.  Per frame [n_frames]: the stack (layout, kind and mem shared by all frames: dv_mask_stack), its number of planes (1..64; a frame without instances
 * hands one empty plane), and per plane the answer of the upstream multi-object tracker: track_id[k][p] / class_id[k][p] (class_id may be NULL: 0), -1 in either = the plane
 * is dropped (the reference's class filter, image_process/image_process.cpp:217-232; its pixels stay in the merged mask, as there).  Results are bit-identical to
 * dv_runner_set_dynamic fed the masks and detections pre-computed from the same stacks.  Before the first dv_runner_run; frames DV_MEM_DEVICE or DV_MEM_PINNED with row
 * stride = width; device / pinned stacks must outlive the run.  Refused with "dv_runner_set_inst_stack: a sequence of a dv_batch group is not supported ..." for a member
 * of a group; the runner stays usable. */
typedef struct dv_seq_stack {
    const void* const* stack; const int32_t* n_planes;
    int32_t kind /* DV_STACK_* */, mem /* DV_MEM_* of the stacks */, row_stride /* bytes, 0 = tight */, min_inst_size; int64_t plane_stride /* bytes, 0 = tight */; float threshold; int32_t static_as_background;
    const int32_t* const* track_id; const int32_t* const* class_id;
    const dv_box3d* const* boxes3d; const int32_t* n_boxes3d;      /* may be NULL (no 3-D detector) */
    const float* const* disp; int32_t disp_mem, disp_stride; double baseline;      /* as in dv_seq_dynamic; disp may be NULL */
} dv_seq_stack;
int dv_runner_set_inst_stack(dv_runner* runner, int seq, const dv_seq_stack* stack);
/* what the object branch of a dynamic sequence was fed so far: detections, object feature rows, frames with at least one object, fewest detections in a frame */
int dv_runner_dynamic_stats(dv_runner* runner, int seq, long long* detections, long long* object_features, long long* frames_with_objects, int* min_detections);
dv_runner* dv_runner_create(dv_ctx* const* ctxs, const dv_seq_input* seqs, int n_seq, int group_size, int threads);      /* group_size <= 1: no batching */
void dv_runner_destroy(dv_runner* runner);
int dv_runner_run(dv_runner* runner, int n_rounds, double* wall_seconds_or_null);
/* per sequence: the last dv_est_state, the trajectory so far as rows [t, px py pz qx qy qz qw] (one per frame solved in the non-linear phase: what SaveBodyTrajectory
 * writes, utils/io/output.cpp:199-227), the window-solve iterations and frames so far, the number of feature rows of the last tracked frame */
int dv_runner_get(dv_runner* runner, int seq, dv_est_state* last, double* poses8, int cap, int* n_poses, long long* iterations, long long* frames, int* n_rows_last);
/* every frame handed to the back end, initialisation included, as rows [t, px py pz qx qy qz qw, nonlinear]: the lines of `<seq>_<mode>_Odometry.txt` */
int dv_runner_get_frames(dv_runner* runner, int seq, double* rows9, int cap, int* n_rows);
/* diagnostics: per frame handed to the back end [frame index, rows collected from the tracker, FNV-1a hash of those rows' bytes, solver iterations] — two runs of the same
 * sequence must agree entry by entry; where they first differ says whether the tracker's output or only the solve moved (raw mode) */
/* diagnostics: the host's steady clock (seconds) at the end of every frame handed to the back end so far (which = 0), or at which the tracker thread of a dynamic sequence
 * delivered every frame (which = 1): per-frame pacing of a run without cutting it into calls */
int dv_runner_get_frame_clock(dv_runner* runner, int seq, int which, double* seconds, int cap, int* n_out);
int dv_runner_get_row_log(dv_runner* runner, int seq, unsigned long long* rows4, int cap, int* n_rows);
int dv_runner_batch_rounds(dv_runner* runner, long long* batched_rounds, long long* single_rounds);      /* dv_batch_info summed over the groups */
int dv_runner_batch_timing(dv_runner* runner, int on, double* out3, long long* rounds, int* windows);      /* dv_batch_timing of the runner's groups, averaged */
/* the dv_batch objects of the runner's groups (groups of one sequence have none), for the dv_batch_*_info counters the runner does not sum itself (dv_batch_obj_info).
 * They stay the runner's: read counters, enqueue nothing. */
int dv_runner_get_batches(dv_runner* runner, dv_batch** out, int cap, int* n_out);
/* switches: "batch_front" (default 1): the members of a dv_batch group are tracked in shared launches (dv_batch_track_enqueue); 0: one set of launches per sequence.
 * "tracker_thread" (default 1): a dynamic sequence OUTSIDE a dv_batch group runs its tracker on a thread of its own (T2 beside T3); 0: the one-thread loop.  Dynamic members
 * of a dv_batch group always run the one-thread order (dv_runner_set_dynamic).  "teams": see above. */
int dv_runner_set(dv_runner* runner, const char* key, int value);
int dv_runner_track_info(dv_runner* runner, long long* rounds, long long* members_batched, long long* members_single);      /* dv_batch_track_info summed over the groups */
const char* dv_runner_error(dv_runner* runner);

/* FeatureManager::point_landmarks for the point-cloud publishers (utils/io/visualization.cpp:214-249): world point = CamToWorld(point * depth, start_frame);
 * in_point_cloud / in_margin_cloud apply PubPointCloud's two selection rules.  key_poses = window[i][0..2] of dv_est_state. */
typedef struct dv_landmark { int32_t id, start_frame, n_obs, solve_flag; double depth, p_w[3]; int32_t in_point_cloud, in_margin_cloud; } dv_landmark;
int dv_est_get_landmarks(dv_ctx* ctx, dv_landmark* out, int cap, int* n_out);

/* ---- dynamic mode: the object (instance) half of the back end.  Inputs are FrontendFeature::instances (basic/frontend_feature.h:58-75), i.e.
 * what InstsFeatManager::Output() hands over (front_end/dynamic_tracker.cpp:521-577): per object its tracked features, the associated 3-D
 * detection (if any) and the "extra" 3-D points sampled from the disparity map (camera frame).  The association of detections to tracks
 * (DeepSORT / VIODE keys), the detector networks and the PCL clustering of the extra points are upstream of the path. ---- */
typedef struct dv_box3d {               /* Box3D (basic/box3d.h:40-106): the fields the path reads */
    int32_t class_id, pad_; double score;
    double center[3];                   /* center_pt, camera frame */
    double dims[3]; double yaw;         /* R_cioi() is built from yaw (box3d.h:79-83) */
    float rect_min[2], rect_max[2];     /* box2d of the projected corners (BoxAssociate2Dto3D, dynamic_tracker.cpp:61-152) */
} dv_box3d;
typedef struct dv_inst_obs {            /* one FeatureInstance */
    uint32_t id; int32_t has_box3d;     /* map key (Box2D::track_id); box3d valid */
    int32_t first_feat, n_feats;        /* rows of the instance feature array: dv_feat with left = (x_n, y_n, 1, u, v, vx, vy), right likewise if has_right */
    int32_t first_point, n_points;      /* FeatureInstance::points: (x, y, z) triples in the camera frame */
    float rect[4];                      /* Box2D::rect x, y, w, h */
    dv_box3d box3d;
} dv_inst_obs;
typedef struct dv_inst_state {          /* Instance (estimator/instance.h) as the publishers read it + InstEstimatedInfo (basic/inst_estimated_info.h) */
    uint32_t id; int32_t is_initial, is_tracking, is_curr_visible, is_static, is_init_velocity, age, lost_number, static_frame,
             n_landmarks, n_valid, triangle_num;
    double dims[3], vel_v[3], vel_a[3];
    double window[11][7];               /* state[i]: P, then R as qx qy qz qw */
    double time[11];
} dv_inst_state;
/* ---- dynamic mode, front end: InstsFeatManager (front_end/dynamic_tracker.h:42-101).  One detection = one Box2D of SemanticImage::boxes2d AFTER the
 * multi-object tracker assigned its track id (DeepSORT / VIODE keys: upstream).  mask = InstRoi::mask_cv, roi_gray is cropped from the frame by the
 * library.  points (optional) = InstFeat::extra_points3d of this frame computed by the caller, handed through to the output — or give the library the frame's
 * disparity map (dv_inst_set_disparity) and it runs DetectExtraPoints + ProcessExtraPoints itself. */
typedef struct dv_inst_det {
    uint32_t track_id; int32_t class_id;
    int32_t x, y, w, h;                 /* Box2D::rect, inside the image */
    const uint8_t* mask;                /* h rows of w bytes, > 0 = object (host memory) */
    const double* points; int32_t n_points, pad_;      /* ignored for a frame whose disparity map was handed over (dv_inst_set_disparity) */
} dv_inst_det;
/* fe_para::kMaxDynamicCnt / kMinDynamicDist (front_end/front_end_parameters.cpp), cfg::use_det3d; call once before the first frame.
 * max_dynamic_cnt in [1, 248], min_dynamic_dist in [0, 128] (0: no min-distance grid and discs of radius 0).
 * Limits of the per-object detector and of the extra-point kernels: those stated beside dv_gftt, applied to every object's ROI (w x h = its rectangle), plus two.
 * A frame in which ANY object exceeds one makes dv_inst_track_collect fail with "device error flags=N" (N the sum of the flags raised by all objects of the frame);
 * nothing is returned for that frame (the three counts are 0), the flags are cleared and the context stays usable: the next dv_inst_track_enqueue / _collect pair works
 * on the objects' state as the refused frame left it; dv_inst_reset starts over.
 *   flag 1  more candidates in one ROI than the object's candidate buffer holds, max(4096, W * H / 4) of the context's frame size W x H;
 *   flag 2  min_dynamic_dist >= 1 and ceil(w / d) * ceil(h / d) > 32768 grid cells for one ROI, d = min_dynamic_dist (at d = 5 a 1240 x 700 rectangle has
 *           248 * 140 = 34720 cells; at d = 1 every rectangle over 32768 pixels);
 *   flag 4  a value bin of more than 8192 candidates in one ROI, as for dv_gftt;
 *   flag 8  dv_inst_set_disparity frames: more than DV_XP_CAP points sampled on one object;
 *   flag 16 reserved, never raised: it meant "the clustering of one object's points did not converge" while the label sweeps were a fixed number of launches;
 *           the last kernel now goes on to the fixed point, so every cloud of up to DV_XP_CAP points gets its cluster (csrc/extra_points.hip). */
int dv_inst_config(dv_ctx* ctx, int max_dynamic_cnt, int min_dynamic_dist, int use_det3d);
int dv_inst_reset(dv_ctx* ctx);
/* FeatureTrack's object branch for one frame (system/main.cpp:198-250): AddInstancesByTracking + InstsFeatManager::InstsTrack.  Works on the pyramids
 * of the frame last passed to dv_track_stereo_enqueue (call it right after, same frame; `t` = that frame's time).  boxes3d = SemanticImage::boxes3d
 * (only read when use_det3d). */
int dv_inst_track_enqueue(dv_ctx* ctx, double t, const dv_inst_det* dets, int n_dets, const dv_box3d* boxes3d, int n_boxes3d);
/* The same call with the objects' masks cut ON THE DEVICE from the frame's key image (VIODE::SetViodeMaskAndRoi's ROI masks, utils/dataset/viode_utils.cpp:177-218;
 * AddViodeInstances, front_end/dynamic_tracker.cpp:585-605): the mask of detection d is key_image[y + d.y][x + d.x] == d.track_id ? 255 : 0 over its rectangle;
 * dv_inst_det::mask and dv_inst_det::points are ignored.  key_image: w x h uint32, rows of stride_bytes (0 = 4 w), mem = DV_MEM_HOST (staged once per frame, as
 * dv_inst_set_right_keys stages; valid until the frame is collected), DV_MEM_DEVICE or DV_MEM_PINNED (read in place).  One launch for all visible objects writes their
 * masks where dv_inst_track_enqueue uploads them (padding bytes zero); everything behind — ROI crop, erosion, corner detection, LK, extra-point sampling — runs unchanged
 * on those bytes, so the rows equal those of dv_inst_track_enqueue given the masks cut on the host. */
int dv_inst_track_enqueue_keys(dv_ctx* ctx, double t, const dv_inst_det* dets, int n_dets, const uint32_t* key_image, int stride_bytes, int mem, const dv_box3d* boxes3d, int n_boxes3d);
/* The same call with the objects' masks cut ON THE DEVICE from the detector's mask stack (SemanticImage::SetMaskAndRoi's ROI masks, basic/semantic_image.cpp:20-66):
 * the mask of detection i is 255 where plane planes[i] HAS the pixel by dv_mask_stack's rule (for DV_STACK_F32 the threshold is applied here too), over the detection's
 * rectangle; dv_inst_det::mask and ::points are ignored, track_id / class_id are the caller's (its multi-object tracker's answer).  One launch for all visible objects writes
 * their slices of the mask area (padding bytes zero); everything behind runs unchanged on those bytes, so the rows equal those of dv_inst_track_enqueue given the masks cut
 * on the host.  Every rectangle and plane index is checked before anything is staged.  A DV_MEM_HOST stack whose descriptor equals the one the frame's
 * dv_inst_stack_frame_enqueue staged is NOT copied again (one staging per frame, shared by the stage and the two *_planes entries) — from that stage's collect until the
 * frame's dv_track_stereo_collect, which ends the sharing: a buffer refilled for a later frame is never answered from an old copy; any other host stack is staged by this
 * call and must stay valid until the frame is collected.  Device / pinned stacks are read in place and must stay valid until dv_inst_track_collect. */
struct dv_mask_stack;
int dv_inst_track_enqueue_planes(dv_ctx* ctx, double t, const dv_inst_det* dets, const int32_t* planes, int n_dets, const struct dv_mask_stack* stack, const dv_box3d* boxes3d, int n_boxes3d);
/* dv_track_unmask_static (FeatureTrack, system/main.cpp:217-245) with "plane planes[i] has the pixel" as the per-pixel test over the rectangles of the detections whose
 * track_id is in static_ids.  Applied by the NEXT dv_track_stereo_enqueue (which must carry a mask) and dropped on EVERY return of that call, 0 or -1, as the key-image
 * form is.  Every rectangle and plane index is validated before anything is staged.  The stack follows the rule above: a host stack the frame's stage staged is shared, any
 * other is staged by that enqueue (valid until it returns); device / pinned stacks are read in place (valid until the frame is collected). */
int dv_track_unmask_static_planes(dv_ctx* ctx, const dv_inst_det* dets, const int32_t* planes, int n_dets, const uint32_t* static_ids, int n_static, const struct dv_mask_stack* stack);
/* SemanticImage::disp (CV_32F disparity of the left image, basic/semantic_image.h:30-65) of the frame about to be handed to dv_inst_track_enqueue.  With it the library
 * runs the reference's extra-point pipeline for every visible object ON THE DEVICE, one launch for all objects on a side stream (the reference: a second thread):
 * InstFeat::DetectExtraPoints (front_end/instance_feature.cpp:413-461: step = max(sqrt(0.8 rows cols / 1000), 2), mask > 0, disparity > 0 and not NaN,
 * depth = fx0 baseline / disparity in (0.1, 100], x = (c - cx0) depth / fx0 ..., float arithmetic, row-major scan order) and the point-cloud half of
 * InstsFeatManager::ProcessExtraPoints (front_end/dynamic_tracker.cpp:268-338: pcl::RadiusOutlierRemoval(0.5, 10), pcl::EuclideanClusterExtraction(1.0, 10, 25000), first
 * cluster).  dv_inst_det::points is then ignored; dv_inst_track_collect returns the computed points.  disp: rows of `stride_bytes` bytes (0 = 4 * width), config size,
 * host or device memory (a device map must stay valid until dv_inst_track_collect); baseline = cam_s.baseline (utils/camera_model.h:38); fx0, fy0, cx0, cy0 = cam0 of the
 * config as float.  disp == NULL: back to the pass-through form.  Applies to the NEXT dv_inst_track_enqueue only. */
int dv_inst_set_disparity(dv_ctx* ctx, const float* disp, int stride_bytes, int mem, double baseline);
/* cfg::dataset == kViode: the keys (VIODE::PixelToKey; dv_viode_mask's key_image) of SemanticImage::seg1 — the RIGHT camera's segmentation image — of the frame the NEXT
 * dv_inst_track_enqueue processes.  InstFeat::TrackRightByPad then keeps a right-image point only where that image carries the object's key (dv_inst_det::track_id):
 * status[i] && VIODE::PixelToKey(right_points[i], img.seg1) != id -> 0 (front_end/instance_feature.cpp:263-268).  w x h uint32, stride in bytes (0 = 4 w), mem DV_MEM_*;
 * host memory must stay valid until the frame is collected.  NULL: no test (KITTI / custom data sets).  Belongs to one frame, like the disparity map. */
int dv_inst_set_right_keys(dv_ctx* ctx, const uint32_t* key_image, int stride_bytes, int mem);
/* operator form of the same pipeline for one object (parity tests): mask = h rows of w bytes (host), (x, y) = Box2D::rect.tl().  stage 0: the whole pipeline (the segmented
 * cloud); stage 1: InstFeat::DetectExtraPoints alone (the sampled points before any filtering).  out_xyz: cap_out triples at most, the float results widened to double. */
int dv_extra_points(dv_ctx* ctx, const uint8_t* mask, int x, int y, int w, int h, const float* disp, int stride_bytes, int mem, double baseline, int stage,
                    double* out_xyz, int cap_out, int* n_out);
/* InstsFeatManager::Output() (front_end/dynamic_tracker.cpp:521-577): waits for the frame; insts / feats / points are laid out as dv_est_process_dynamic takes them.
 * Once the frame has been waited for, every failure (a device flag, see dv_inst_config; output buffers too small) ends the frame — it cannot be collected again —
 * and leaves *n_insts = *n_feats = *n_points = 0. */
int dv_inst_track_collect(dv_ctx* ctx, dv_inst_obs* insts, int cap_insts, int* n_insts, dv_feat* feats, int cap_feats, int* n_feats,
                          double* points, int cap_points, int* n_points);

/* ProcessMeasurements iteration in dynamic mode: dv_est_process with frame.instances.  insts may be NULL / n_insts 0 (no object in view). */
int dv_est_process_dynamic(dv_ctx* ctx, const dv_feat* feats, int n, double t, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats,
                           const double* points, dv_est_state* out);
/* two-phase form: _begin enqueues the window solve first and runs the object branch (bookkeeping on the host, InstanceManager::Optimization
 * as dv_obj_solve on a third stream) while it is in flight; dv_est_process_end collects both. */
int dv_est_process_dynamic_begin(dv_ctx* ctx, const dv_feat* feats, int n, double t, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats,
                                 const double* points);
/* three-phase form: _begin_ego enqueues the window solve with the background features alone; _attach hands over the frame's instances and runs the object branch
 * while the window solve is in flight (a frame that is never attached is processed as a frame without objects); dv_est_process_end collects both.  Same results
 * as the two-phase form: what the caller does between the calls (enqueueing the next frame's tracking, dv_inst_track_collect) leaves the front of the window solve. */
int dv_est_process_dynamic_begin_ego(dv_ctx* ctx, const dv_feat* feats, int n, double t);
int dv_est_process_dynamic_attach(dv_ctx* ctx, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats, const double* points);
/* Estimator::im.instances after the last processed frame (ascending id); *n_out = number written (<= cap); summary4 (may be NULL): iterations,
 * termination, initial and final cost of the last object solve */
int dv_est_get_instances(dv_ctx* ctx, dv_inst_state* out, int cap, int* n_out, double* summary4);
/* InstanceManager::GetOutputInstInfo as far as the front end reads it (estimator_insts.cpp:967-990; system/main.cpp:194,217-245): the ids of the initialised, tracked
 * instances that were is_static when the LAST dynamic frame took its snapshot — right behind PushBack (estimator.cpp:1579-1586), so with the flags the frame before
 * left.  Ascending.  The tracker side of the feedback is dv_track_unmask_static. */
int dv_est_get_static_instances(dv_ctx* ctx, uint32_t* ids, int cap, int* n_out);

/* ---- measurement hooks (used by bench.py; HIP-event timing on the ctx's own stream) ---- */
/* names: "pyr","lk_temporal","compact","gftt_eig","gftt_select","lk_stereo","frame" */
/* on: 0 off, 1 per-stage events, 2 additionally one event pair around every back-end kernel launch
 * ("k_be_eval_full","k_be_reduce","k_be_solve","k_be_eval_cost","k_be_accept","k_be_marg","k_be_marg_eig"), -1 host wall-clock scopes only
 * ("h_*": no events, no extra synchronisation — the pipeline keeps its overlap) */
int dv_timing_enable(dv_ctx* ctx, int on);
int dv_timing_reset(dv_ctx* ctx);
int dv_timing_get(dv_ctx* ctx, const char* name, double* total_ms, long long* count);

/* debug-only switch for the test-suite (never read from the environment).  key "short_first_pass": the window solve enqueues
 * max_iters - 2 slots first, so the spare-slot continuation (rare in production: only after a failed linear solve) runs every frame. */
int dv_debug_set(dv_ctx* ctx, const char* key, int value);

#ifdef __cplusplus
}
#endif
#endif
