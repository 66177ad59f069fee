// mask_frame.hip — the per-frame mask stages on the ctx's stream, each as enqueue + collect: label images (VIODE) or a detector's mask stack -> merged mask, inverse,
// key images, boxes in library-owned buffers; the resolution of a mask stack for the entries that read one.
#include "dv_ctx.h"
#include "viode_host.h"
#include "inst_stack_host.h"

// dv_viode_frame_enqueue / _collect: thread T1's per-frame stage on the ctx's stream.  Two buffer sets used alternately: set[cur] belongs to the frame enqueued last, the
// inverse mask and key images of the frame before stay intact while that frame is tracked.
struct ViodeFrame {
    struct Set { DevBuf inv, keys0, keys1; } set[2];
    int cur = 1;
    DevBuf seg[2], scratch /* planes nobody reads: the merged mask, the right image's two masks */, small /* keys (256 B) | boxes left (1024 B) | boxes right (1024 B) */;
    PinBuf pinned;      // box initialiser (1024 B) | keys (256 B) | the frame's boxes (1024 B)
    StageSlot slot; bool has_right = false; int nkeys = 0, keys_on_dev = 0; uint32_t keys[64] = { 0 };
};
void dv_stage_delete(ViodeFrame* p) { delete p; }

// dv_inst_stack_frame_enqueue / _collect: the same stage from a detector's mask stack.  Two buffer sets used alternately, as above: set[cur] belongs to the frame enqueued
// last.  A DV_MEM_HOST stack is staged into its set (tightly packed) and `from` remembers its descriptor: the *_planes entries of the frame find the copy there.
struct InstStackFrame {
    struct Set { DevBuf merge, inv, staged; dv_mask_stack from{}; bool has_staged = false; } set[2];
    int cur = 1;
    DevBuf small /* boxes (1024 B) */, scratch /* DV_STACK_REMAP_MERGED: the merged mask before the remap | the remapped one, pitched */;
    PinBuf pinned;      // box initialiser (1024 B) | the frame's boxes (1024 B)
    StageSlot slot; int n_planes = 0;
};
void dv_stage_delete(InstStackFrame* p) { delete p; }
static bool same_stack(const dv_mask_stack& a, const dv_mask_stack& b) {
    return a.data == b.data && a.n_planes == b.n_planes && a.kind == b.kind && a.mem == b.mem && a.row_stride == b.row_stride && a.plane_stride == b.plane_stride;
}
// a host stack -> dst, tightly packed (rows of w * es bytes, planes of w * h * es), on s
static int stage_host_stack(dv_ctx* ctx, const dv_mask_stack& st, int es, DevBuf& dst, hipStream_t s) {
    const int w = ctx->cfg.width, h = ctx->cfg.height;
    const size_t row = (size_t)w * es, plane = row * h;
    DV_CHECK(dst.ensure(plane * st.n_planes));
    if ((size_t)st.row_stride == row) DV_CHECK(hipMemcpy2DAsync(dst.p, plane, st.data, (size_t)st.plane_stride, plane, st.n_planes, hipMemcpyHostToDevice, s));
    else for (int p = 0; p < st.n_planes; ++p)
        DV_CHECK(hipMemcpy2DAsync((uint8_t*)dst.p + p * plane, row, (const uint8_t*)st.data + (size_t)p * st.plane_stride, (size_t)st.row_stride, row, h, hipMemcpyHostToDevice, s));
    return 0;
}
// the frame whose background tracking has just been collected is over: the staged stack of a COLLECTED stage no longer stands in for a host stack of the same descriptor
// (a caller who refills the buffer for the next frame without running the stage gets its new content staged, not the old copy).  A stage in flight belongs to the next frame
void dv_stack_frame_done(dv_ctx* ctx) {
    InstStackFrame* V = ctx->istack;
    if (!V) return;
    if (V->slot.pending) V->set[V->cur ^ 1].has_staged = false;
    else V->set[0].has_staged = V->set[1].has_staged = false;
}
int dv_stack_resolve(dv_ctx* ctx, const dv_mask_stack& st, DevBuf& own_buf, hipStream_t s, DvStackSrc* out) {
    const int es = st.kind == DV_STACK_F32 ? 4 : 1, w = ctx->cfg.width, h = ctx->cfg.height;
    if (st.mem != DV_MEM_HOST) { *out = DvStackSrc{ (const uint8_t*)st.data, (long long)st.plane_stride, st.row_stride, st.n_planes, st.kind, st.threshold }; return 0; }
    const void* dev = nullptr;
    if (ctx->istack && !ctx->istack->slot.pending) {
        const InstStackFrame::Set& Q = ctx->istack->set[ctx->istack->cur];
        if (Q.has_staged && same_stack(Q.from, st)) dev = Q.staged.p;
    }
    if (!dev) { if (stage_host_stack(ctx, st, es, own_buf, s)) return -1; dev = own_buf.p; }
    *out = DvStackSrc{ (const uint8_t*)dev, (long long)w * es * h, w * es, st.n_planes, st.kind, st.threshold };
    return 0;
}

extern "C" {

// ImageProcessor::Run's VIODE branch for ONE frame (image_process/image_process.cpp:161-178 -> VIODE::SetViodeMaskAndRoi, utils/dataset/viode_utils.cpp:21-218) as enqueue +
// collect: viode_mask_kernel on the left label image (and on the right one: its key image is what TrackRightByPad tests) into library-owned device buffers; the boxes of
// the left image — nkeys x 16 bytes — are the frame's ONLY device -> host traffic (the host sizes the job tables of the object tracker from the rectangles).
int dv_viode_frame_enqueue(dv_ctx* ctx, const uint8_t* seg0_bgr, const uint8_t* seg1_bgr_or_null, int w, int h, int stride, int mem, const uint32_t* dyn_keys, int nkeys) {
    if (!ctx) return -1;
    if (!seg0_bgr || !dyn_keys) DV_FAIL("dv_viode_frame_enqueue: null label image / key table");
    if (w != ctx->cfg.width || h != ctx->cfg.height) DV_FAIL("dv_viode_frame_enqueue: image size differs from config");
    if (stride == 0) stride = 3 * w;
    if (stride < 3 * w) DV_FAIL("dv_viode_frame_enqueue: stride below 3 * width");
    if (nkeys < 1 || nkeys > 64) DV_FAIL("dv_viode_frame_enqueue: 1..64 dynamic keys");
    if (!dv_mem_known(mem)) DV_FAIL("dv_viode_frame_enqueue: unknown memory kind");
    if (!ctx->viode) ctx->viode = new ViodeFrame();          // (a half-built one is completed by the next call or deleted by dv_destroy)
    ViodeFrame& V = *ctx->viode;
    if (V.slot.open(ctx, "dv_viode_frame_enqueue: previous frame not collected")) return -1;
    hipStream_t s = ctx->stream;
    if (!V.pinned.p) { DV_CHECK(V.pinned.ensure(1024 + 256 + 1024)); dv_boxes_init((int32_t*)V.pinned.p); }
    const int mp = w;          // the masks are tightly packed: the inverse mask goes to dv_track_stereo_enqueue as a DV_MEM_DEVICE mask beside gray frames of stride w
    const size_t plane = ((size_t)mp * h + 255) / 256 * 256;
    ViodeFrame::Set& Q = V.set[V.cur ^ 1];
    DV_CHECK(Q.inv.ensure(plane)); DV_CHECK(Q.keys0.ensure((size_t)4 * w * h));
    if (seg1_bgr_or_null) DV_CHECK(Q.keys1.ensure((size_t)4 * w * h));
    DV_CHECK(V.scratch.ensure(3 * plane)); DV_CHECK(V.small.ensure(256 + 2048));
    // the set about to be overwritten held the frame before the last: the objects of that frame may still read its key images on the object tracker's stream
    if (dv_inst_wait_before_next_frame(ctx, s, false)) DV_FAIL("dv_viode_frame_enqueue: hipStreamWaitEvent");
    uint32_t* d_keys = (uint32_t*)V.small.p; int32_t* d_box0 = (int32_t*)((uint8_t*)V.small.p + 256); int32_t* d_box1 = d_box0 + 256;
    if (V.keys_on_dev != nkeys || std::memcmp(V.keys, dyn_keys, 4 * (size_t)nkeys) != 0) {      // (no frame is in flight: the pinned copy of the table is not being read)
        std::memcpy(V.keys, dyn_keys, 4 * (size_t)nkeys); std::memcpy(V.pinned.p + 1024, dyn_keys, 4 * (size_t)nkeys);
        DV_CHECK(dv_copy_async(d_keys, V.pinned.p + 1024, 256, s));
        V.keys_on_dev = nkeys;
    }
    V.nkeys = nkeys;
    DV_CHECK(dv_copy_async(d_box0, V.pinned.p, 1024, s));          // the box buffers start every frame at (max, -1, max, -1)
    if (seg1_bgr_or_null) DV_CHECK(dv_copy_async(d_box1, V.pinned.p, 1024, s));
    const uint8_t* src[2] = { seg0_bgr, seg1_bgr_or_null }; int spitch = stride;
    for (int i = 0; i < 2; ++i) if (src[i]) {
        DvRows r;
        if (dv_stage_rows(ctx, V.seg[i], src[i], (size_t)3 * w, h, stride, dv_in_place_device_or_pinned(mem), s, &r)) return -1;
        src[i] = r.p; spitch = r.pitch;
    }
    uint8_t* sc = (uint8_t*)V.scratch.p;
    {
        StageScope sc_t(ctx, "viode_frame");
        dv_launch_viode_mask(src[0], w, h, spitch, d_keys, nkeys, sc, (uint8_t*)Q.inv.p, mp, (uint32_t*)Q.keys0.p, d_box0, s);
        if (src[1]) dv_launch_viode_mask(src[1], w, h, spitch, d_keys, nkeys, sc + plane, sc + 2 * plane, mp, (uint32_t*)Q.keys1.p, d_box1, s);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = dv_copy_async(V.pinned.p + 1280, d_box0, 1024, s);
    if (V.slot.close(ctx, e, s)) return -1;
    V.cur ^= 1; V.has_right = seg1_bgr_or_null != nullptr;
    return 0;
}

int dv_viode_frame_collect(dv_ctx* ctx, int min_inst_size, dv_inst_det* dets, int cap, int* n_dets, const uint8_t** inv_mask_dev, const uint32_t** keys0_dev, const uint32_t** keys1_dev) {
    if (!ctx) return -1;
    if (!ctx->viode || !ctx->viode->slot.pending) DV_FAIL("dv_viode_frame_collect: nothing enqueued");
    if (!n_dets || cap < 0 || (cap > 0 && !dets)) DV_FAIL("dv_viode_frame_collect: bad argument");
    ViodeFrame& V = *ctx->viode;
    if (V.slot.wait(ctx)) return -1;
    const int n = dv_viode_build_dets((const int32_t*)(V.pinned.p + 1280), V.keys, V.nkeys, min_inst_size, dets, cap);
    if (n < 0) DV_FAIL("dv_viode_frame_collect: more detections than `cap`");
    *n_dets = n;
    const ViodeFrame::Set& Q = V.set[V.cur];
    if (inv_mask_dev) *inv_mask_dev = (const uint8_t*)Q.inv.p;
    if (keys0_dev) *keys0_dev = (const uint32_t*)Q.keys0.p;
    if (keys1_dev) *keys1_dev = V.has_right ? (const uint32_t*)Q.keys1.p : nullptr;
    return 0;
}

// ImageProcessor::Run's detector branch for ONE frame (image_process/image_process.cpp:160-170: Detector2D::Launch's threshold + BuildBoxes2D + the mask half of
// SetMaskAndRoi / SetBackgroundMask) as enqueue + collect: inst_stack_kernel over the stack into library-owned buffers; n_planes x 16 bytes of boxes are the frame's ONLY
// device -> host traffic
int dv_inst_stack_frame_enqueue(dv_ctx* ctx, const dv_mask_stack* stack, int w, int h, int flags) {
    if (!ctx) return -1;
    if (w != ctx->cfg.width || h != ctx->cfg.height) DV_FAIL("dv_inst_stack_frame_enqueue: image size differs from config");
    DvStackLayout L;
    if (const char* why = dv_stack_check(stack, w, h, &L)) DV_FAIL(std::string("dv_inst_stack_frame_enqueue: ") + why);
    if (flags & ~DV_STACK_REMAP_MERGED) DV_FAIL("dv_inst_stack_frame_enqueue: unknown flag");
    const bool remap = (flags & DV_STACK_REMAP_MERGED) != 0;
    if (remap && !ctx->undist[0]) DV_FAIL("dv_inst_stack_frame_enqueue: DV_STACK_REMAP_MERGED needs installed undistortion maps (dv_undistort_setup / dv_set_undistort_maps)");
    if (!ctx->istack) ctx->istack = new InstStackFrame();          // (a half-built one is completed by the next call or deleted by dv_destroy)
    InstStackFrame& V = *ctx->istack;
    if (V.slot.open(ctx, "dv_inst_stack_frame_enqueue: previous frame not collected")) return -1;
    hipStream_t s = ctx->stream;
    if (!V.pinned.p) { DV_CHECK(V.pinned.ensure(2048)); dv_boxes_init((int32_t*)V.pinned.p); }
    const size_t plane = ((size_t)w * h + 255) / 256 * 256;          // the masks are tightly packed: the inverse goes to dv_track_stereo_enqueue as a DV_MEM_DEVICE mask beside frames of stride w
    const int rp = align_up(w, 16);
    InstStackFrame::Set& Q = V.set[V.cur ^ 1];
    DV_CHECK(Q.merge.ensure(plane)); DV_CHECK(Q.inv.ensure(plane)); DV_CHECK(V.small.ensure(1024));
    if (remap) DV_CHECK(V.scratch.ensure(plane + (size_t)rp * h));
    // The set about to be overwritten held the frame before the last.  Its masks are read on this stream alone.  Its STAGED host stack may still be read by that frame's
    // objects on the object tracker's stream when the caller enqueues this stage before the dv_track_stereo_enqueue that would wait for them (stage k + 1 in front of
    // tracking k): only then the stream waits for the object tracker.  Device / pinned stacks are never copied, so their stage runs beside the object stream.
    if (Q.has_staged && dv_inst_wait_before_next_frame(ctx, s, false)) DV_FAIL("dv_inst_stack_frame_enqueue: hipStreamWaitEvent");
    dv_mask_stack st = *stack; st.row_stride = L.row_stride; st.plane_stride = L.plane_stride;
    DvStackSrc S{ (const uint8_t*)st.data, L.plane_stride, L.row_stride, st.n_planes, st.kind, st.threshold };
    Q.has_staged = false;
    if (st.mem == DV_MEM_HOST) {
        if (stage_host_stack(ctx, st, L.es, Q.staged, s)) return -1;
        S.base = (const uint8_t*)Q.staged.p; S.row_stride = w * L.es; S.plane_stride = (long long)w * L.es * h;
    }
    int32_t* d_box = (int32_t*)V.small.p;
    DV_CHECK(dv_copy_async(d_box, V.pinned.p, 1024, s));          // the boxes start every frame at (max, -1, max, -1)
    {
        StageScope sc_t(ctx, "inst_stack_frame");
        if (!remap) dv_launch_inst_stack(S, w, h, (uint8_t*)Q.merge.p, (uint8_t*)Q.inv.p, d_box, s);
        else {          // SetBackgroundMask: merged -> cv::remap(left maps, INTER_LINEAR) -> inverted
            uint8_t* raw = (uint8_t*)V.scratch.p; uint8_t* mapped = raw + plane;
            dv_launch_inst_stack(S, w, h, raw, (uint8_t*)Q.inv.p, d_box, s);
            const uint8_t* maps = (const uint8_t*)ctx->undist_buf[0].p;
            dv_launch_remap(raw, nullptr, w, h, w, 1, 0, (const int16_t*)maps, (const uint16_t*)(maps + (size_t)4 * w * h), nullptr, nullptr, mapped, nullptr, rp, s);
            dv_launch_stack_finish_remap(mapped, rp, w, h, (uint8_t*)Q.merge.p, (uint8_t*)Q.inv.p, s);
        }
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = dv_copy_async(V.pinned.p + 1024, d_box, 1024, s);
    if (V.slot.close(ctx, e, s)) return -1;
    if (st.mem == DV_MEM_HOST) { Q.from = st; Q.has_staged = true; }
    V.cur ^= 1; V.n_planes = st.n_planes;
    return 0;
}

int dv_inst_stack_frame_collect(dv_ctx* ctx, int min_inst_size, dv_inst_det* dets, int32_t* planes, int cap, int* n_dets, const uint8_t** inv_mask_dev, const uint8_t** merge_mask_dev) {
    if (!ctx) return -1;
    if (!ctx->istack || !ctx->istack->slot.pending) DV_FAIL("dv_inst_stack_frame_collect: nothing enqueued");
    if (!n_dets || cap < 0 || (cap > 0 && !dets)) DV_FAIL("dv_inst_stack_frame_collect: bad argument");
    InstStackFrame& V = *ctx->istack;
    if (V.slot.wait(ctx)) return -1;
    const int n = dv_stack_build_dets((const int32_t*)(V.pinned.p + 1024), V.n_planes, min_inst_size, dets, planes, cap);
    if (n < 0) DV_FAIL("dv_inst_stack_frame_collect: more detections than `cap`");
    *n_dets = n;
    const InstStackFrame::Set& Q = V.set[V.cur];
    if (inv_mask_dev) *inv_mask_dev = (const uint8_t*)Q.inv.p;
    if (merge_mask_dev) *merge_mask_dev = (const uint8_t*)Q.merge.p;
    return 0;
}

} // extern "C"
