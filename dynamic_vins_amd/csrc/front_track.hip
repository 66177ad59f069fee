// front_track.hip — the tracker's per-frame entries of the C ABI: dv_track_stereo_enqueue / _collect for one sequence, dv_batch_track_enqueue for a dv_batch group.
// One frame = pyrDown x3 (stereo pair per launch) -> LK temporal -> compact/sort -> Shi-Tomasi tile -> select/append -> LK stereo -> finalize (<= max_cnt 128-byte
// rows, written into pinned memory by the kernel); naive and semantic mode add the GPU tracker's own pyramid levels and, with mask_morphology_size, the mask's erosion.
// Both entries take what the stages are given from ONE description of the frame (front_plan), mode and mask included: the single entry launches it by value with the
// single-sequence kernels, the group entry scatters it into the job tables of the _multi kernels — raw, semantic and naive members alike.
#include "dv_ctx.h"
#include "inst_stack_host.h"

// What the stages of one frame of one context are given, in the job types of the table kernels
struct FrontPlan {
    bool dev;                                  // the frames are device-addressable (DV_MEM_DEVICE, or pinned + mapped host memory)
    PyrPlan pyr;                               // level 0, the level steps, the two pyramids of the apron stage, the number of levels
    // FeatureTrackByLKGpu's own pyramids where the reference runs that tracker (naive: TrackLeftGPU + TrackRightGPU; semantic: TrackRightGPU).  cuda_prev: the previous
    // frame was tracked in another mode, its pyramid of this flavour is built now (the single entry only: such a job does not share a round's launches)
    bool cuda, cuda_prev; CudaPyrPlan cpyr, cpyr_prev;
    const uint8_t* mask; int mask_pitch;       // the frame's mask as the device reads it, before the erosion (null: none)
    bool has_erode; DvErodeJob erode;          // ErodeMask of naive / semantic mode with mask_morphology_size > 0
    DvLkJob lk_temporal, lk_stereo;
    bool temporal_gpu_rule, stereo_gpu_rule;   // the stage runs the GPU tracker (lk_cuda.hip) on the cpyr pyramids, not lk.hip's
    float dist_temporal, dist_stereo;
    DvCompactJob compact; GfttTileArgs tile; GfttSelectArgs select; DvFinalizeJob fin;
};

static int job_stride(const dv_track_job& j, int w) { return j.stride > 0 ? j.stride : w * ((j.mem & DV_FMT_BGR) ? 3 : 1); }

// the mask's way into the stages that read it: eroded first in naive / semantic mode (ErodeMask, background_tracker.cpp:408-416,764-768), then the compaction's mask test
// (naive / semantic) and the detector's mask.  Called by front_plan, and again by the single entry after dv_track_unmask_static moved the mask into mask_buf
static int front_plan_mask(dv_ctx* ctx, int mode, const uint8_t* mask, int mask_pitch, FrontPlan& P) {
    const dv_config& c = ctx->cfg;
    const int w = c.width, h = c.height;
    const bool naive = (mode != DV_MODE_RAW);            // naive and semantic share the InstFeat code path (mask test, no sort, >= 10 new)
    P.mask = mask; P.mask_pitch = mask_pitch;
    P.has_erode = naive && mask && c.mask_morphology_size > 0;
    if (P.has_erode) {
        const int ep = align_up(w, 16);
        DV_CHECK(ctx->s3.ensure((size_t)ep * h)); DV_CHECK(ctx->s4.ensure((size_t)ep * h));
        P.erode = DvErodeJob{ mask, (uint8_t*)ctx->s3.p, (uint8_t*)ctx->s4.p, w, h, mask_pitch, ep, ep, c.mask_morphology_size };
        mask = (const uint8_t*)ctx->s4.p; mask_pitch = ep;
    }
    P.compact.mask_pitch = mask_pitch; P.compact.in_mask = naive ? mask : nullptr;
    P.tile.in_mask = mask; P.tile.mask_pitch = mask_pitch;
    return 0;
}

// ---- the static instances' rectangles of a frame (dv_track_unmask_static / _keys / _planes): staged on the ctx, applied by ONE launch of the enqueue that follows ----
// What is staged belongs to one frame: applied by the call this guard lives in, or dropped with whichever return ends it — no rectangle survives into a later frame
struct UnmaskGuard {
    dv_ctx* const* c; int n;
    ~UnmaskGuard() { for (int i = 0; i < n; ++i) { c[i]->unmask.clear(); c[i]->unmask_src = dv_ctx::UnmaskSrc{}; } }
};
static const char* unmask_entry(int form) { return form == dv_ctx::UNMASK_MASKS ? "dv_track_unmask_static" : form == dv_ctx::UNMASK_KEYS ? "dv_track_unmask_static_keys" : "dv_track_unmask_static_planes"; }
static bool unmask_selected(const dv_inst_det& d, const uint32_t* ids, int n) { return std::find(ids, ids + n, d.track_id) != ids + n; }
static bool unmask_rect_ok(const dv_inst_det& d, int W, int H) { return d.w > 0 && d.h > 0 && d.x >= 0 && d.y >= 0 && d.w <= W && d.h <= H && d.x <= W - d.w && d.y <= H - d.h; }
// unmask_pinned = [DvUnmaskJob | n DvUnmaskRect | ROI masks]: where the tables of n rectangles end
size_t dv_unmask_tab_bytes(size_t n) { return (256 + n * sizeof(DvUnmaskRect) + 255) / 256 * 256; }
// room for them and for roi_bytes of ROI masks, at the staging call: the frame before was collected, nothing on the device reads the block.  The tables of up to
// DV_STACK_MAX_PLANES rectangles fit what dv_create allocated: the key and plane forms allocate nothing and wait for nothing here
static int unmask_reserve(dv_ctx* ctx, size_t n, size_t roi_bytes) {
    const size_t need = dv_unmask_tab_bytes(n) + roi_bytes;
    if (ctx->unmask_pinned_bytes < need) {
        DV_CHECK(hipStreamSynchronize(ctx->stream));          // (a previous frame's kernels may still read the old staging area)
        if (ctx->unmask_pinned) (void)hipHostFree(ctx->unmask_pinned);
        ctx->unmask_pinned = nullptr; ctx->unmask_pinned_bytes = 0;
        // (the tables of a full stack's planes and, with ROI masks, a frame's worth from the start: the rectangles grow as objects come closer)
        const size_t want = std::max<size_t>(2 * need, dv_unmask_tab_bytes(DV_STACK_MAX_PLANES) + (roi_bytes ? (size_t)ctx->cfg.width * ctx->cfg.height : 0));
        DV_CHECK(hipHostMalloc(&ctx->unmask_pinned, want, hipHostMallocDefault));
        ctx->unmask_pinned_bytes = want;
    } else if (roi_bytes && ctx->last_done && ctx->last_done == ctx->done) DV_CHECK(hipEventSynchronize(ctx->done));      // the previous frame's unmask kernel has read the block (a no-op wait in the usual case: that frame was collected)
    return 0;
}
// One mask's job and its rectangles, rects[first ...], from what is staged on ctx.  The frame's source is resolved on s: ROI masks lie in unmask_pinned, a device / pinned
// key image or stack is read where it lies, a host one is staged once.  The job works in the ctx's own mask_buf: a host mask is there already, a caller's device mask is
// copied by the launch that applies the rectangles and never written.  mask_buf holds align_up(w, 16) x h bytes (the caller's ensure, under its own error text)
static int front_unmask_tables(dv_ctx* ctx, const FrontPlan& P, hipStream_t s, int first, DvUnmaskJob* job, DvUnmaskRect* rects) {
    const dv_ctx::UnmaskSrc& U = ctx->unmask_src;
    const int w = ctx->cfg.width, h = ctx->cfg.height, mp = align_up(w, 16);
    const uint32_t* kimg = U.key_img; int kstride = U.key_stride;
    DvStackSrc S{};
    if (U.form == dv_ctx::UNMASK_KEYS) {
        DvRows k;
        if (dv_stage_rows(ctx, ctx->unmask_src_buf, kimg, (size_t)4 * w, h, kstride, dv_in_place_device_or_pinned(U.key_mem), s, &k)) return -1;
        kimg = (const uint32_t*)k.p; kstride = k.pitch;
    }
    if (U.form == dv_ctx::UNMASK_PLANES && dv_stack_resolve(ctx, U.stack, ctx->unmask_src_buf, s, &S)) return -1;
    uint8_t* own = (uint8_t*)ctx->mask_buf.p;
    *job = DvUnmaskJob{ own, P.mask == own ? nullptr : P.mask, mp, P.mask_pitch, w, h, first, (int)ctx->unmask.size() };
    for (const dv_ctx::UnmaskRect& r : ctx->unmask) {
        const DvPixSrc src = U.form == dv_ctx::UNMASK_MASKS ? DvPixSrc{ (const uint8_t*)ctx->unmask_pinned + r.off, r.w, DV_PIX_ROI_U8, 0u, 0.f, r.x, r.y }
                           : U.form == dv_ctx::UNMASK_KEYS ? dv_key_src(kimg, kstride, r.id) : dv_plane_src(S, r.plane);
        rects[first++] = DvUnmaskRect{ src, r.x, r.y, r.w, r.h };
    }
    return 0;
}
// the single entry's step (system/main.cpp:217-245, before anything reads the mask): tables in unmask_pinned, read in place, one launch; the stages then read mask_buf
static int front_apply_unmask(dv_ctx* ctx, int mode, hipStream_t s, FrontPlan& P) {
    if (ctx->unmask.empty()) return 0;
    if (!P.mask) DV_FAIL(std::string(unmask_entry(ctx->unmask_src.form)) + ": the frame carries no mask");
    DvUnmaskJob* job = (DvUnmaskJob*)ctx->unmask_pinned; DvUnmaskRect* rects = (DvUnmaskRect*)((uint8_t*)ctx->unmask_pinned + 256);
    DV_CHECK(ctx->mask_buf.ensure((size_t)align_up(ctx->cfg.width, 16) * ctx->cfg.height));
    if (front_unmask_tables(ctx, P, s, 0, job, rects)) return -1;
    dv_launch_unmask(job, 1, rects, job->W, job->H, s);
    return front_plan_mask(ctx, mode, job->dst, job->dpitch, P);
}

// Everything a frame needs before its first launch: the member-level checks, the lazily created resources, the frames' and the mask's way to the device (copies on s)
// and the stages' arguments under the frame's mode.  The frame is built in the pyramid the ctx is NOT looking at (cur ^ 1) and the ctx is not changed: front_commit
// does that, once the whole enqueue has succeeded, so that a refused or failed enqueue of either kind leaves no flipped `cur` and no pending frame behind.
static int front_plan(dv_ctx* ctx, const dv_track_job& j, hipStream_t s, FrontPlan& P) {
    const dv_config& c = ctx->cfg;
    const int w = c.width, h = c.height;
    const bool stereo = c.stereo && j.gray1;
    const int mode = j.mode;
    int mem = j.mem;
    if (!dv_mem_known(mem & 0xff)) DV_FAIL("dv_track_stereo: unknown memory kind");
    if ((mem & 0xff) == DV_MEM_PINNED) mem = (mem & ~0xff) | DV_MEM_DEVICE;      // pinned + mapped host memory is device-addressable: the kernels read it in place ("device or pinned")
    if (ctx->undist[0]) {      // cfg::is_undistort_input.  (The size check cannot fire today — dv_set_undistort_maps / dv_undistort_setup take the config's size only — and is kept, once, because include/dvins.h promises it)
        if (w != ctx->undist_w || h != ctx->undist_h) DV_FAIL("dv_track_stereo: undistortion maps were installed for another image size");
        if (stereo && !ctx->undist[1]) DV_FAIL("dv_track_stereo: undistortion maps installed for camera 0 but not for camera 1");
    }
    P.dev = (mem & ~DV_FMT_BGR) == DV_MEM_DEVICE;
    if (dv_ensure_hw(ctx, c.min_dist) || dv_ensure_cand(ctx, w, h)) return -1;
    if (ctx->last_front && ctx->last_front != s && ctx->last_done) DV_CHECK(hipStreamWaitEvent(s, ctx->last_done, 0));      // the previous frame ran on the other front-end stream (its own / a dv_batch's)
    const int cur = ctx->cur ^ 1;          // the pyramid slot of this frame
    PyrSet& L = ctx->left[cur]; PyrSet& Lp = ctx->left[cur ^ 1];
    DV_CHECK(L.alloc(w, h, 3));
    if (stereo) DV_CHECK(ctx->right.alloc(w, h, 3));
    const DvPyr& a = L.pyr; const DvPyr& b = stereo ? ctx->right.pyr : a;
    if (dv_plan_pyramids(ctx, a, stereo ? &b : nullptr, j.gray0, j.gray1, job_stride(j, w), mem, ctx->undist[0], s, P.pyr)) return -1;
    P.cuda = (mode != DV_MODE_RAW); P.cuda_prev = false;
    if (P.cuda) {
        if (dv_plan_cuda_pyramids(ctx, ctx->leftc[cur], stereo ? &ctx->rightc : nullptr, a, stereo ? &ctx->right.pyr : nullptr, w, h, 3, P.cpyr)) return -1;
        if (mode == DV_MODE_NAIVE && ctx->have_prev && !ctx->leftc_valid[cur ^ 1]) {      // the previous frame was tracked in another mode: its pyramid of this flavour does not exist yet
            if (dv_plan_cuda_pyramids(ctx, ctx->leftc[cur ^ 1], nullptr, Lp.pyr, nullptr, w, h, 3, P.cpyr_prev)) return -1;
            P.cuda_prev = true;
        }
    }
    const DvTrackState& tr = ctx->tr;
    // forward/backward consistency: FeatureTrackByLK keeps <= 0.5 px (feature_utils.cpp:56), FeatureTrackByLKGpu <= 1.0 px (:126) (Q12) — and the two are different
    // trackers (lk.hip / lk_cuda.hip), each used where the reference uses it
    P.temporal_gpu_rule = (mode == DV_MODE_NAIVE); P.stereo_gpu_rule = (mode != DV_MODE_RAW);      // TrackLeftGPU (naive) vs TrackLeft (raw, semantic); TrackRightGPU in naive and semantic
    P.dist_temporal = P.temporal_gpu_rule ? 1.0f : 0.5f; P.dist_stereo = P.stereo_gpu_rule ? 1.0f : 0.5f;
    // temporal LK (a sequence's first frame has no previous pyramid: n_feat is 0, nothing is read), stereo LK
    DvLkJob& t = P.lk_temporal; t = DvLkJob{}; t.pts_a = tr.last_pts; t.n_dev = tr.n_feat; t.pts_b = tr.lk_pts; t.status = tr.lk_status;
    if (P.temporal_gpu_rule) { t.B = ctx->leftc[cur].pyr; t.A = ctx->have_prev ? ctx->leftc[cur ^ 1].pyr : t.B; }      // TrackLeftGPU -> FeatureTrackByLKGpu (instance_feature.cpp:191-216)
    else { t.A = ctx->have_prev ? Lp.pyr : a; t.B = a; }
    DvLkJob& r = P.lk_stereo; r = DvLkJob{}; r.pts_a = tr.curr_pts; r.n_dev = tr.n_feat; r.pts_b = tr.right_pts; r.status = tr.right_status;
    if (P.stereo_gpu_rule) { r.A = ctx->leftc[cur].pyr; r.B = stereo ? ctx->rightc.pyr : r.A; }      // TrackRightGPU -> FeatureTrackByLKGpu (instance_feature.cpp:278-310)
    else { r.A = a; r.B = b; }
    const bool naive = (mode != DV_MODE_RAW);
    const int min_new = naive ? 10 : 1;                   // Q23: instance_feature.cpp:353-356 vs background_tracker.cpp:82-90
    // DetectNewFeature(img, use_gpu, ...): TrackImageNaive passes true (background_tracker.cpp:445) -> DetectShiTomasiCornersGpu (feature_utils.cpp:339-348),
    // TrackSemanticImage passes false (:789) and TrackImage calls cv::goodFeaturesToTrack itself (:85)
    const int gftt_rule = (mode == DV_MODE_NAIVE) ? DV_GFTT_RULE_CUDA : DV_GFTT_RULE_CPU;
    P.compact = DvCompactJob{ tr, nullptr, 0, naive ? 0 : 1, ctx->n_cand, ctx->max_ord };
    GfttTileArgs& g = P.tile; g = GfttTileArgs{};
    g.img = a.L[0].p; g.w = w; g.h = h; g.pitch = a.L[0].pitch; g.in_mask = nullptr; g.mask_pitch = 0;
    g.disc_pts = tr.curr_pts; g.n_disc = tr.n_tracked; g.radius = c.min_dist; g.hw = (const uint8_t*)ctx->hw_buf.p;
    g.n_feat = tr.n_feat; g.max_cnt = c.max_cnt; g.min_new = min_new; g.eig_out = nullptr; g.eig_pitch = 0;
    g.cand = (DvCand*)ctx->cand_buf.p; g.cand_cap = ctx->cand_cap; g.n_cand = ctx->n_cand; g.max_ord = ctx->max_ord; g.rule = gftt_rule;
    GfttSelectArgs& q = P.select; q = GfttSelectArgs{};
    q.cand = (const DvCand*)ctx->cand_buf.p; q.n_cand = ctx->n_cand; q.cand_cap = ctx->cand_cap; q.max_ord = ctx->max_ord;
    q.w = w; q.h = h; q.quality = 0.01; q.min_dist = (double)c.min_dist; q.max_n_host = 0; q.n_feat = tr.n_feat; q.max_cnt = c.max_cnt; q.min_new = min_new;
    q.out_xy = nullptr; q.n_out = nullptr; q.tr = tr; q.has_tr = 1; q.err_flag = ctx->err_flag; q.rule = gftt_rule;
    // the mask: device-addressable jobs are read in place, host jobs staged into the ctx's own mask_buf on s.  The mask of a BGR job has one channel: rows of w bytes
    DvRows mk{};
    if (j.mask && dv_stage_rows(ctx, ctx->mask_buf, j.mask, w, h, (mem & DV_FMT_BGR) ? w : job_stride(j, w), P.dev, s, &mk)) return -1;
    if (front_plan_mask(ctx, mode, mk.p, mk.pitch, P)) return -1;
    // the rows, their count and the device error flags go straight into the pinned buffer (three copy dispatches behind the kernel before: ~20 us of the
    // tracker's latency per frame)
    DvFinalizeJob& f = P.fin; f = DvFinalizeJob{};
    f.tr = tr; f.cam0 = c.cam0; f.cam1 = c.cam1; f.stereo = stereo ? 1 : 0; f.dt = j.t - ctx->prev_time; f.out = ctx->out_pinned; f.n_out = ctx->nout_pinned;
    f.err_in = ctx->err_flag; f.err_out = ctx->err_pinned;
    return 0;
}

// the planned frame is enqueued behind `done` on s: the ctx turns to the pyramid it was built in.  cuda: the frame built the GPU tracker's pyramid levels too (naive, semantic)
static void front_commit(dv_ctx* ctx, double t, hipEvent_t done, hipStream_t s, bool cuda) {
    ctx->cur ^= 1; ctx->last_done = done; ctx->last_front = s;
    ctx->leftc_valid[ctx->cur] = cuda;
    ctx->prev_time = t; ctx->have_prev = true; ctx->pending = true;
}

extern "C" {

int dv_track_stereo_enqueue(dv_ctx* ctx, const uint8_t* gray0, const uint8_t* gray1, int w, int h, int stride, double t,
                            const uint8_t* mask_or_null, int mode, int mem) {
    if (!ctx) return -1;
    HostScope hs(ctx, "h_front_enqueue");
    dv_ctx* const self[1] = { ctx }; UnmaskGuard unmask_guard{ self, 1 };
    if (!gray0) DV_FAIL("dv_track_stereo: gray0 is null");
    if (w != ctx->cfg.width || h != ctx->cfg.height) DV_FAIL("dv_track_stereo: image size differs from config (reference: std::terminate, main.cpp:95-99)");
    if (ctx->pending) DV_FAIL("dv_track_stereo_enqueue: previous frame not collected");
    if (mode != DV_MODE_RAW && mode != DV_MODE_NAIVE && mode != DV_MODE_SEMANTIC) DV_FAIL("dv_track_stereo: unknown mode");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const dv_config& c = ctx->cfg;
    const bool stereo = c.stereo && gray1;
    hipStream_t s = ctx->stream;
    const int cur = ctx->cur ^ 1;          // the pyramid slot of this frame: the ctx turns to it in front_commit
    if (dv_inst_wait_before_next_frame(ctx, s)) DV_FAIL("dv_track_stereo: hipStreamWaitEvent");
    StageScope frame(ctx, "frame");
    FrontPlan P;
    {
        StageScope sc(ctx, "pyr");
        const dv_track_job job{ 0, mem, gray0, gray1, stride, mode, t, mask_or_null };
        if (front_plan(ctx, job, s, P)) return -1;
        dv_launch_pyramids(P.pyr, s);
        DV_CHECK(hipGetLastError());
    }
    // ---- the plan, launched by value; what it does not hold: the object tracker's events and the staged dv_track_unmask_static jobs ----
    if (ctx->inst) DV_CHECK(hipEventRecord(ctx->ev_pyr, s));
    if (P.cuda) {
        StageScope sc(ctx, "pyr_cuda");
        dv_launch_cuda_pyramids(P.cpyr, s);
        if (P.cuda_prev) { dv_launch_cuda_pyramids(P.cpyr_prev, s); ctx->leftc_valid[cur ^ 1] = true; }
        DV_CHECK(hipGetLastError());
    }
    if (front_apply_unmask(ctx, mode, s, P)) return -1;
    if (P.has_erode) { const DvErodeJob& k = P.erode; dv_launch_erode(k.src, k.w, k.h, k.spitch, k.k, k.tmp, k.tpitch, k.dst, k.dpitch, s); }
    if (ctx->have_prev) {
        StageScope sc(ctx, "lk_temporal");
        const DvLkJob& k = P.lk_temporal;
        if (P.temporal_gpu_rule) dv_launch_lk_cuda_track(k.A, k.B, k.pts_a, k.n_dev, c.max_cnt, c.flow_back, P.dist_temporal, k.pts_b, k.status, s);
        else dv_launch_lk_track(k.A, k.B, k.pts_a, k.n_dev, c.max_cnt, c.flow_back, P.dist_temporal, k.pts_b, k.status, s, ctx->tr.lk_order);
    }
    {
        StageScope sc(ctx, "compact");
        const DvCompactJob& k = P.compact;
        dv_launch_compact(k.tr, k.in_mask, k.mask_pitch, k.sort_by_cnt, k.n_cand, k.max_ord, s);
    }
    {
        StageScope sc(ctx, "gftt_eig");
        dv_launch_gftt_tile(P.tile, s);
    }
    {
        StageScope sc(ctx, "gftt_select");
        if (dv_launch_gftt_select(P.select, s)) DV_FAIL("gftt_select: cannot set dynamic LDS size");
    }
    if (ctx->inst) DV_CHECK(hipEventRecord(ctx->ev_bg_select, s));
    if (stereo) {
        StageScope sc(ctx, "lk_stereo");
        const DvLkJob& k = P.lk_stereo;
        if (P.stereo_gpu_rule) dv_launch_lk_cuda_track(k.A, k.B, k.pts_a, k.n_dev, c.max_cnt, c.flow_back, P.dist_stereo, k.pts_b, k.status, s);
        else dv_launch_lk_track(k.A, k.B, k.pts_a, k.n_dev, c.max_cnt, c.flow_back, P.dist_stereo, k.pts_b, k.status, s, ctx->tr.lk_order);
    }
    {
        StageScope sc(ctx, "finalize");
        const DvFinalizeJob& k = P.fin;
        dv_launch_finalize(k.tr, k.cam0, k.cam1, k.stereo, k.dt, c.max_cnt, k.out, k.n_out, s, k.err_in, k.err_out);
    }
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipEventRecord(ctx->done, s));
    front_commit(ctx, t, ctx->done, s, P.cuda);
    return 0;
}

// The three forms stage the same list (dv_ctx::unmask) for the next dv_track_stereo_enqueue / dv_batch_track_enqueue; each call replaces what an earlier one staged.
// Every selected rectangle is checked before anything is sized, allocated or staged: the kernel's reads are bounded by them.
// This one: the ROI mask of detection d is dv_inst_det::mask, copied into unmask_pinned here
int dv_track_unmask_static(dv_ctx* ctx, const dv_inst_det* dets, int n_dets, const uint32_t* static_ids, int n_static) {
    if (!ctx) return -1;
    ctx->unmask.clear(); ctx->unmask_src = dv_ctx::UnmaskSrc{};
    if (n_static <= 0 || n_dets <= 0) return 0;
    if (!dets || !static_ids) DV_FAIL("dv_track_unmask_static: null argument");
    if (ctx->pending) DV_FAIL("dv_track_unmask_static: call it before dv_track_stereo_enqueue of the frame it belongs to");
    size_t n = 0, roi_bytes = 0;
    for (int i = 0; i < n_dets; ++i) {
        const dv_inst_det& d = dets[i];
        if (!unmask_selected(d, static_ids, n_static)) continue;
        if (!d.mask || !unmask_rect_ok(d, ctx->cfg.width, ctx->cfg.height)) DV_FAIL("dv_track_unmask_static: bad detection rectangle / mask");
        ++n; roi_bytes += ((size_t)d.w * d.h + 15) / 16 * 16;
    }
    if (!n) return 0;
    if (unmask_reserve(ctx, n, roi_bytes)) return -1;
    size_t off = dv_unmask_tab_bytes(n);
    for (int i = 0; i < n_dets; ++i) {
        const dv_inst_det& d = dets[i];
        if (!unmask_selected(d, static_ids, n_static)) continue;
        std::memcpy((uint8_t*)ctx->unmask_pinned + off, d.mask, (size_t)d.w * d.h);
        ctx->unmask.push_back({ d.x, d.y, d.w, d.h, off, 0u, 0 });
        off += ((size_t)d.w * d.h + 15) / 16 * 16;
    }
    return 0;
}

// the key-image form: the ROI mask of detection d is key_image(y + d.y, x + d.x) == d.track_id (dv_inst_det::mask is ignored).  The key image is read in place by the
// next dv_track_stereo_enqueue (device / pinned) or staged there once (host): it must stay valid until that call returns — host — or until the frame is collected —
// device / pinned
int dv_track_unmask_static_keys(dv_ctx* ctx, const dv_inst_det* dets, int n_dets, const uint32_t* static_ids, int n_static, const uint32_t* key_image, int stride_bytes, int mem) {
    if (!ctx) return -1;
    ctx->unmask.clear(); ctx->unmask_src = dv_ctx::UnmaskSrc{};
    if (n_static <= 0 || n_dets <= 0) return 0;
    if (!dets || !static_ids) DV_FAIL("dv_track_unmask_static_keys: null argument");
    if (!key_image) DV_FAIL("dv_track_unmask_static_keys: null key image");
    if (!dv_mem_known(mem)) DV_FAIL("dv_track_unmask_static_keys: unknown memory kind");
    if (stride_bytes == 0) stride_bytes = 4 * ctx->cfg.width;
    if (stride_bytes < 4 * ctx->cfg.width || (stride_bytes & 3)) DV_FAIL("dv_track_unmask_static_keys: bad stride");
    if (ctx->pending) DV_FAIL("dv_track_unmask_static_keys: call it before dv_track_stereo_enqueue of the frame it belongs to");
    size_t n = 0;
    for (int i = 0; i < n_dets; ++i) {
        if (!unmask_selected(dets[i], static_ids, n_static)) continue;
        if (!unmask_rect_ok(dets[i], ctx->cfg.width, ctx->cfg.height)) DV_FAIL("dv_track_unmask_static_keys: detection rectangle outside the image");
        ++n;
    }
    if (!n) return 0;
    if (unmask_reserve(ctx, n, 0)) return -1;
    for (int i = 0; i < n_dets; ++i) {
        const dv_inst_det& d = dets[i];
        if (unmask_selected(d, static_ids, n_static)) ctx->unmask.push_back({ d.x, d.y, d.w, d.h, 0, d.track_id, 0 });
    }
    ctx->unmask_src.form = dv_ctx::UNMASK_KEYS; ctx->unmask_src.key_img = key_image; ctx->unmask_src.key_stride = stride_bytes; ctx->unmask_src.key_mem = mem;
    return 0;
}

// the mask-stack form: the ROI mask of detection i is "plane planes[i] has the pixel" (include/dvins.h, dv_mask_stack).  The stack is read in place by the next
// dv_track_stereo_enqueue (device / pinned), taken from the copy the frame's stage staged, or staged there once (any other host stack)
int dv_track_unmask_static_planes(dv_ctx* ctx, const dv_inst_det* dets, const int32_t* planes, int n_dets, const uint32_t* static_ids, int n_static, const dv_mask_stack* stack) {
    if (!ctx) return -1;
    ctx->unmask.clear(); ctx->unmask_src = dv_ctx::UnmaskSrc{};
    if (n_static <= 0 || n_dets <= 0) return 0;
    if (!dets || !planes || !static_ids) DV_FAIL("dv_track_unmask_static_planes: null argument");
    DvStackLayout L;
    if (const char* why = dv_stack_check(stack, ctx->cfg.width, ctx->cfg.height, &L)) DV_FAIL(std::string("dv_track_unmask_static_planes: ") + why);
    if (ctx->pending) DV_FAIL("dv_track_unmask_static_planes: call it before dv_track_stereo_enqueue of the frame it belongs to");
    if (const char* why = dv_stack_check_dets(dets, planes, n_dets, stack->n_planes, ctx->cfg.width, ctx->cfg.height, static_ids, n_static)) DV_FAIL(std::string("dv_track_unmask_static_planes: ") + why);
    size_t n = 0;
    for (int i = 0; i < n_dets; ++i) n += unmask_selected(dets[i], static_ids, n_static);
    if (!n) return 0;
    if (unmask_reserve(ctx, n, 0)) return -1;
    for (int i = 0; i < n_dets; ++i) {
        const dv_inst_det& d = dets[i];
        if (unmask_selected(d, static_ids, n_static)) ctx->unmask.push_back({ d.x, d.y, d.w, d.h, 0, 0u, planes[i] });
    }
    ctx->unmask_src.form = dv_ctx::UNMASK_PLANES; ctx->unmask_src.stack = *stack; ctx->unmask_src.stack.row_stride = L.row_stride; ctx->unmask_src.stack.plane_stride = L.plane_stride;
    return 0;
}

int dv_track_stereo_collect(dv_ctx* ctx, dv_feat* out, int* n_out) {
    if (!ctx) return -1;
    if (!ctx->pending) DV_FAIL("dv_track_stereo_collect: nothing enqueued");
    { HostScope hs(ctx, "h_front_wait"); DV_CHECK(hipEventSynchronize(ctx->last_done ? ctx->last_done : ctx->done)); }
    ctx->pending = false;
    dv_stack_frame_done(ctx);
    if (ctx->timing) dv_harvest_timers(ctx, ctx->stream);
    if (*ctx->err_pinned) {
        int f = *ctx->err_pinned;
        // cleared before this call returns: the next frame may run on another stream than this memset (a group member's frames run on the group's stream, and front_plan
        // orders a frame behind last_done only), where the word could be wiped under that frame's selection, or still be set when its finalize copies it
        DV_CHECK(hipMemsetAsync(ctx->err_flag, 0, 4, ctx->stream));
        DV_CHECK(hipStreamSynchronize(ctx->stream));
        DV_FAIL(std::string("front end device error flags=") + std::to_string(f) +
                " (1: candidate buffer overflow, 2: min-distance grid too large, 4: value bin overflow)");
    }
    const int n = *ctx->nout_pinned;
    if (n_out) *n_out = n;
    if (out && n > 0) std::memcpy(out, ctx->out_pinned, (size_t)n * sizeof(dv_feat));
    return 0;
}

int dv_track_stereo(dv_ctx* ctx, const uint8_t* gray0, const uint8_t* gray1, int w, int h, int stride, double t,
                    const uint8_t* mask_or_null, int mode, int mem, dv_feat* out, int* n_out) {
    if (dv_track_stereo_enqueue(ctx, gray0, gray1, w, h, stride, t, mask_or_null, mode, mem)) return -1;
    return dv_track_stereo_collect(ctx, out, n_out);
}

}  // extern "C"

// ------------------------------- the front ends of a dv_batch group in shared launches -------------------------------
// FeatureTracker::TrackImage (background_tracker.cpp:52-158) of S independent sequences, one launch per STAGE for all of them (the reference runs one process per
// sequence, system/main.cpp:178-330): pyrDown levels 1..3 (level 1 also writes the pitched level-0 copy), aprons, temporal LK, compaction / sort, Shi-Tomasi tile,
// corner selection, stereo LK, rows = 10 launches per group and frame instead of 10 per sequence.  The kernels are the single-sequence kernels' bodies behind a
// job table in HBM (blockIdx.z / .y / .x = member), so every member's rows are bit-identical to what its own dv_track_stereo_enqueue produces.
// Members with undistortion maps (cfg::is_undistort_input) or BGR frames differ in level 0 alone: one more launch (level0_multi_kernel, pyramid.hip) fills it for all
// of them, each through its own maps, and level 1 then reads it; a round without such a member does not launch it.
// TrackImageNaive members (DV_MODE_NAIVE with a mask, background_tracker.cpp:398-470) are a second class of the same round: they share level 0, the pyramid levels,
// aprons, compaction, tile, selection and rows with the raw members — their jobs carry the mask, min_new = 10 and the GPU detector's rule — and have three stages of
// their own: cuda::pyrDown's levels 1..3 (pyr_down_multi_kernel<1>), the masks' erosion (those with mask_morphology_size > 0) and FeatureTrackByLKGpu
// (lk_cuda_track_multi_kernel at 1.0 px) over their slice of the two LK tables, where the raw slice runs lk_track_multi_kernel at 0.5 px.
// TrackSemanticImage members (DV_MODE_SEMANTIC with a mask, background_tracker.cpp:757-834 — the background tracking of a DYNAMIC sequence) are the third class, between
// the two: TrackLeft on the plain pyramids with the raw slice (0.5 px), TrackRightGPU on the GPU tracker's pyramid with the naive slice (1.0 px), the CPU detector's
// rule, the mask test, min_new = 10 and the erosion as in naive mode.  Two things a dynamic sequence adds ride on the group's stream: the staged
// dv_track_unmask_static rectangles of all members (ONE launch, dv_unmask_kernel, which also makes the copy of a caller's device mask) and the hand-shake with the
// member's object tracker (wait for its previous frame, ev_pyr behind the aprons, ev_bg_select behind the selection), so that dv_inst_track_enqueue — still one set of
// launches per member on the tracker's own stream, like the extra-point stages — sees the order the member's own entry gives it.
struct DvFrontBatch {
    hipStream_t stream = nullptr; hipEvent_t done = nullptr, ev_copy[2] = { nullptr, nullptr };
    DevBuf tab[2]; void* tab_pinned[2] = { nullptr, nullptr }; size_t tab_bytes = 0; int parity = 0; bool copy_used[2] = { false, false };
    long long rounds = 0, members_batched = 0, members_single = 0;
};
void dv_front_batch_sync(DvFrontBatch* F) { if (F && F->stream) (void)hipStreamSynchronize(F->stream); }      // be_batch_detach: a member leaves while one of its frames may be in flight on the group's front-end stream
void dv_front_batch_release(DvFrontBatch* F) {
    if (!F) return;
    if (F->stream) { (void)hipStreamSynchronize(F->stream); (void)hipStreamDestroy(F->stream); }
    if (F->done) (void)hipEventDestroy(F->done);
    for (int k = 0; k < 2; ++k) { if (F->ev_copy[k]) (void)hipEventDestroy(F->ev_copy[k]); F->tab[k].release(); if (F->tab_pinned[k]) (void)hipHostFree(F->tab_pinned[k]); }
    delete F;
}

extern "C" int dv_batch_track_enqueue(dv_batch* B, const dv_track_job* jobs, int n) {
    if (!B || (n > 0 && !jobs) || n < 0) { dv_set_error(nullptr, "dv_batch_track_enqueue: bad arguments"); return -1; }
    const std::vector<dv_ctx*>& mem = be_batch_members(B);
    if (n == 0 || mem.empty()) return 0;
    dv_ctx* ctx = mem[0];                                       // errors of the shared part are reported on the first member (and the global slot)
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DvFrontBatch*& Fp = be_batch_front(B);
    if (!Fp) {
        Fp = new DvFrontBatch();
        DV_CHECK(hipStreamCreateWithFlags(&Fp->stream, hipStreamNonBlocking));
        DV_CHECK(hipEventCreateWithFlags(&Fp->done, hipEventDisableTiming));
        for (int k = 0; k < 2; ++k) DV_CHECK(hipEventCreateWithFlags(&Fp->ev_copy[k], hipEventDisableTiming));
    }
    DvFrontBatch& F = *Fp;
    // ---- which jobs can share launches.  Three classes, all without timing on the ctx and of the group's common geometry (gray or BGR frames, with or without the
    //      member's own undistortion maps: those differ in how level 0 is filled and in nothing behind it):
    //        raw       DV_MODE_RAW without a mask (FeatureTracker::TrackImage), no object tracker on the ctx;
    //        semantic  DV_MODE_SEMANTIC with a mask (TrackSemanticImage), with or without an object tracker on the ctx (its hand-shake with dv_inst_track_enqueue is kept on
    //                  the group's stream, below) and with or without dv_track_unmask_static jobs staged (one launch applies those of the whole round);
    //        naive     DV_MODE_NAIVE with a mask (TrackImageNaive), no object tracker, no dv_track_unmask_static jobs staged, and the previous frame — if there is one —
    //                  with a pyramid of the GPU tracker's flavour (a naive or semantic frame).
    //      Semantic and naive jobs share the GPU tracker's stages: at least two of them together in the round, a lone one has nothing to share.
    //      Every other job keeps its member's own launches on its own stream, in this round only. ----
    enum { K_SINGLE = 0, K_RAW = 1, K_SEMANTIC = 2, K_NAIVE = 3 };
    std::vector<int> kind(n, K_SINGLE);
    // whatever dv_track_unmask_static staged on the members handed in belongs to THIS frame: applied by the round's launch or by the member's own entry, or dropped with
    // a refused / failed call — no job survives into a later frame
    std::vector<dv_ctx*> handed;
    for (int i = 0; i < n; ++i) if (jobs[i].member >= 0 && jobs[i].member < (int)mem.size()) handed.push_back(mem[jobs[i].member]);
    UnmaskGuard unmask_guard{ handed.data(), (int)handed.size() };
    for (int i = 0; i < n; ++i) {
        const dv_track_job& j = jobs[i];
        if (j.member < 0 || j.member >= (int)mem.size()) DV_FAIL("dv_batch_track_enqueue: member index out of range");
        for (int q = 0; q < i; ++q) if (jobs[q].member == j.member) DV_FAIL("dv_batch_track_enqueue: a member appears twice");
        const dv_ctx* c = mem[j.member];
        if (c->timing || !j.gray0 || (c->cfg.stereo && !j.gray1)) continue;
        if (!c->unmask.empty() && c->unmask_src.form != dv_ctx::UNMASK_MASKS) continue;     // dv_track_unmask_static_keys / _planes rectangles: the member's own entry applies them
        if (j.mode == DV_MODE_SEMANTIC && j.mask) kind[i] = K_SEMANTIC;
        else if (c->inst) continue;
        else if (j.mode == DV_MODE_RAW && !j.mask) kind[i] = K_RAW;
        else if (j.mode == DV_MODE_NAIVE && j.mask && c->unmask.empty() && !(c->have_prev && !c->leftc_valid[c->cur])) kind[i] = K_NAIVE;
    }
    const dv_config* ref = nullptr;
    int R = 0, N = 0;      // raw jobs; jobs of the GPU tracker's classes (semantic + naive)
    for (int pass = 0; pass < 2; ++pass) {      // (the second pass: fewer than two semantic / naive jobs fit, the geometry is that of the first raw job then)
        ref = nullptr; R = N = 0;
        for (int i = 0; i < n; ++i) {
            if (kind[i] == K_SINGLE) continue;
            const dv_config& g = mem[jobs[i].member]->cfg;
            if (!ref) ref = &g;
            if (g.width != ref->width || g.height != ref->height || g.stereo != ref->stereo || g.flow_back != ref->flow_back) continue;
            (kind[i] == K_RAW ? R : N)++;
        }
        if (N == 0 || N >= 2) break;
        for (int i = 0; i < n; ++i) if (kind[i] != K_RAW) kind[i] = K_SINGLE;
    }
    std::vector<int> M;                                         // job indices that are batched: raw, semantic, naive — both LK stages are two contiguous slices of their table then
    for (int cls = K_RAW; cls <= K_NAIVE; ++cls)
        for (int i = 0; i < n; ++i) {
            if (kind[i] != cls) continue;
            const dv_config& g = mem[jobs[i].member]->cfg;
            if (g.width != ref->width || g.height != ref->height || g.stereo != ref->stereo || g.flow_back != ref->flow_back) kind[i] = K_SINGLE;
            else M.push_back(i);
        }
    if ((int)M.size() == 1) { kind[M[0]] = K_SINGLE; M.clear(); }      // nothing to share
    for (int i : M) {      // (before anything is enqueued, the single jobs included; with dv_track_stereo_enqueue's text, on the member and on the first one)
        dv_ctx* c = mem[jobs[i].member];
        if (c->pending) { dv_set_error(c, "dv_track_stereo_enqueue: previous frame not collected"); dv_set_error(ctx, c->err); return -1; }
    }
    for (int i = 0; i < n; ++i) {
        if (kind[i] != K_SINGLE) continue;      // its own launches on its own stream (ordered behind whatever the batch stream still holds for it: dv_track_stereo_enqueue)
        const dv_track_job& j = jobs[i]; dv_ctx* c = mem[j.member];
        if (dv_track_stereo_enqueue(c, j.gray0, j.gray1, c->cfg.width, c->cfg.height, job_stride(j, c->cfg.width), j.t, j.mask, j.mode, j.mem)) { dv_set_error(ctx, c->err); return -1; }
        F.members_single++;
    }
    const int S = (int)M.size();
    if (S == 0) return 0;
    R = 0; for (int i : M) R += kind[i] == K_RAW;
    int Q = 0; for (int i : M) Q += kind[i] == K_SEMANTIC;      // raw [0, R) | semantic [R, R + Q) | naive [R + Q, S)
    N = S - R;                                                  // the jobs with the GPU tracker's pyramid levels, and maybe an erosion: semantic + naive
    size_t n_rect = 0; int n_umj = 0;                           // staged dv_track_unmask_static rectangles of the round, and the members that have some
    for (int i : M) { const dv_ctx* c = mem[jobs[i].member]; if (kind[i] == K_SEMANTIC && !c->unmask.empty()) { n_rect += c->unmask.size(); ++n_umj; } }
    const int w = ref->width, h = ref->height; const bool stereo = ref->stereo != 0;
    hipStream_t s = F.stream;
    // ---- the job tables of the round: one pinned block, one upload ----
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_pyr = 0, o_apr = o_pyr + (size_t)3 * S * sizeof(DvPyrJob), o_lk = up(o_apr + (size_t)2 * S * sizeof(DvPyr)),
                 o_cmp = up(o_lk + (size_t)2 * S * sizeof(DvLkJob)), o_gt = up(o_cmp + (size_t)S * sizeof(DvCompactJob)),
                 o_gs = up(o_gt + (size_t)S * sizeof(GfttTileArgs)), o_fin = up(o_gs + (size_t)S * sizeof(GfttSelectArgs)),
                 o_l0 = up(o_fin + (size_t)S * sizeof(DvFinalizeJob)), o_cp = up(o_l0 + (size_t)S * sizeof(DvLevel0Job)),
                 o_er = up(o_cp + (size_t)3 * N * sizeof(DvPyrJob)), o_um = up(o_er + (size_t)N * sizeof(DvErodeJob)),
                 o_ur = up(o_um + (size_t)n_umj * sizeof(DvUnmaskJob)), total = up(o_ur + n_rect * sizeof(DvUnmaskRect));
    const int par = F.parity; F.parity ^= 1;
    if (F.copy_used[par]) DV_CHECK(hipEventSynchronize(F.ev_copy[par]));      // the upload that last read this pinned block (two rounds ago) has run
    if (F.tab_bytes < total) {
        DV_CHECK(hipStreamSynchronize(s));
        const size_t cap = total * 2;
        for (int k = 0; k < 2; ++k) {
            DV_CHECK(F.tab[k].ensure(cap));
            if (F.tab_pinned[k]) (void)hipHostFree(F.tab_pinned[k]);
            F.tab_pinned[k] = nullptr;
            DV_CHECK(hipHostMalloc(&F.tab_pinned[k], cap, hipHostMallocDefault));
        }
        F.tab_bytes = cap;
    }
    uint8_t* hp = (uint8_t*)F.tab_pinned[par]; const uint8_t* dp = (const uint8_t*)F.tab[par].p;
    DvPyrJob* h_pyr = (DvPyrJob*)(hp + o_pyr); DvPyr* h_apr = (DvPyr*)(hp + o_apr); DvLkJob* h_lk = (DvLkJob*)(hp + o_lk); DvCompactJob* h_cmp = (DvCompactJob*)(hp + o_cmp);
    GfttTileArgs* h_gt = (GfttTileArgs*)(hp + o_gt); GfttSelectArgs* h_gs = (GfttSelectArgs*)(hp + o_gs); DvFinalizeJob* h_fin = (DvFinalizeJob*)(hp + o_fin);
    DvLevel0Job* h_l0 = (DvLevel0Job*)(hp + o_l0); int n_l0 = 0;      // only the members whose level 0 is not a copy of the frame: none in an all-plain round, and no launch then
    DvPyrJob* h_cp = (DvPyrJob*)(hp + o_cp);                          // the GPU tracker's pyramid levels of the semantic and naive members, level-major like h_pyr
    DvErodeJob* h_er = (DvErodeJob*)(hp + o_er); int n_er = 0;        // only the semantic / naive members with mask_morphology_size > 0
    DvUnmaskJob* h_um = (DvUnmaskJob*)(hp + o_um); int n_um = 0;      // only the semantic members with staged dv_track_unmask_static jobs
    DvUnmaskRect* h_ur = (DvUnmaskRect*)(hp + o_ur); int n_ur = 0;
    // ---- per member: its plan of the frame, scattered into the tables.  (No ctx changes before the commit below: a member's refusal, a failed upload or LDS
    //      attribute leave no member with a flipped current pyramid, a pending frame or a GPU-tracker pyramid marked valid) ----
    int n_max = 0, n_max_cls[3] = { 0, 0, 0 }, levels = 0, lw[DV_MAX_LEVELS] = { 0 }, lh[DV_MAX_LEVELS] = { 0 }, clevels = 0;
    FrontPlan P;
    for (int k = 0; k < S; ++k) {
        const dv_track_job& j = jobs[M[k]]; dv_ctx* c = mem[j.member];
        // a member with an object tracker: the objects of its previous frame (dv_inst_track_enqueue, on the tracker's own stream) still read the pyramids this frame's
        // uploads and levels overwrite
        if (c->inst && dv_inst_wait_before_next_frame(c, s, false)) { dv_set_error(c, "dv_track_stereo: hipStreamWaitEvent"); dv_set_error(ctx, c->err); return -1; }
        if (front_plan(c, j, s, P)) { dv_set_error(ctx, c->err); return -1; }      // (with dv_track_stereo's text, on the member and on the first one)
        if (kind[M[k]] == K_SEMANTIC && !c->unmask.empty()) {      // the static instances' pixels leave the mask in the member's own mask_buf, by the round's one launch
            if (c->mask_buf.ensure((size_t)align_up(w, 16) * h) != hipSuccess) { dv_set_error(c, "dv_track_unmask_static: cannot allocate the mask copy"); dv_set_error(ctx, c->err); return -1; }
            if (front_unmask_tables(c, P, s, n_ur, &h_um[n_um], h_ur)) { dv_set_error(ctx, c->err); return -1; }
            n_ur += h_um[n_um].n;
            if (front_plan_mask(c, j.mode, h_um[n_um].dst, h_um[n_um].dpitch, P)) { dv_set_error(ctx, c->err); return -1; }
            ++n_um;
        }
        if (P.pyr.has_l0) h_l0[n_l0++] = P.pyr.l0;
        levels = P.pyr.levels;
        for (int l = 1; l < levels; ++l) { h_pyr[(size_t)(l - 1) * S + k] = P.pyr.down[l - 1]; lw[l] = P.pyr.down[l - 1].dw; lh[l] = P.pyr.down[l - 1].dh; }
        h_apr[2 * k] = P.pyr.apron[0]; h_apr[2 * k + 1] = P.pyr.apron[1];
        h_lk[k] = P.lk_temporal; h_lk[S + k] = P.lk_stereo;
        h_cmp[k] = P.compact; h_gt[k] = P.tile; h_gs[k] = P.select; h_fin[k] = P.fin;
        n_max = std::max(n_max, c->cfg.max_cnt);
        int& cls_max = n_max_cls[k < R ? 0 : k < R + Q ? 1 : 2]; cls_max = std::max(cls_max, c->cfg.max_cnt);
        if (k >= R) {
            clevels = P.cpyr.levels;      // (every level of the size: the same for all members)
            for (int l = 1; l < clevels; ++l) h_cp[(size_t)(l - 1) * N + (k - R)] = P.cpyr.down[l - 1];
            if (P.has_erode) h_er[n_er++] = P.erode;
        }
    }
    DV_CHECK(dv_copy_async(F.tab[par].p, hp, total, s));
    DV_CHECK(hipEventRecord(F.ev_copy[par], s)); F.copy_used[par] = true;
    // ---- the stages.  A class without a member launches nothing: a round of raw members enqueues the ten launches it always did, no event besides ----
    const DvLkJob* d_lk = (const DvLkJob*)(dp + o_lk);
    if (n_l0) dv_launch_level0_multi((const DvLevel0Job*)(dp + o_l0), n_l0, w, h, s);
    for (int l = 1; l < levels; ++l) dv_launch_pyr_down_multi((const DvPyrJob*)(dp + o_pyr) + (size_t)(l - 1) * S, S, lw[l], lh[l], s);
    dv_launch_pyr_apron_multi((const DvPyr*)(dp + o_apr), 2 * S, levels, s);
    for (int k = R; k < R + Q; ++k) { dv_ctx* c = mem[jobs[M[k]].member]; if (c->inst) DV_CHECK(hipEventRecord(c->ev_pyr, s)); }      // the member's object tracker may start: this frame's pyramids exist
    for (int l = 1; l < clevels; ++l) {      // cuda::pyrDown's levels on top of level 0 (all of them: the level sizes follow from the common geometry)
        const DvPyrJob& j0 = h_cp[(size_t)(l - 1) * N];
        dv_launch_pyr_down_multi((const DvPyrJob*)(dp + o_cp) + (size_t)(l - 1) * N, N, j0.dw, j0.dh, s, 1);
    }
    if (n_um) dv_launch_unmask((const DvUnmaskJob*)(dp + o_um), n_um, (const DvUnmaskRect*)(dp + o_ur), w, h, s);      // system/main.cpp:217-245, before anything reads the masks
    if (n_er) dv_launch_erode_multi((const DvErodeJob*)(dp + o_er), n_er, w, h, s);
    // temporal: FeatureTrackByLK at 0.5 px over raw + semantic (TrackLeft), FeatureTrackByLKGpu at 1.0 px over naive (TrackLeftGPU)
    dv_launch_lk_track_multi(d_lk, R + Q, std::max(n_max_cls[0], n_max_cls[1]), ref->flow_back, 0.5f, s);
    dv_launch_lk_cuda_track_multi(d_lk + R + Q, N - Q, n_max_cls[2], ref->flow_back, 1.0f, s);
    dv_launch_compact_multi((const DvCompactJob*)(dp + o_cmp), S, s);
    dv_launch_gftt_tile_multi((const GfttTileArgs*)(dp + o_gt), S, w, h, s);
    if (dv_launch_gftt_select_multi((const GfttSelectArgs*)(dp + o_gs), S, s)) DV_FAIL("gftt_select: cannot set dynamic LDS size");
    for (int k = R; k < R + Q; ++k) { dv_ctx* c = mem[jobs[M[k]].member]; if (c->inst) DV_CHECK(hipEventRecord(c->ev_bg_select, s)); }      // the shared id counter: background first, then the member's objects
    if (stereo) {      // FeatureTrackByLK over raw (TrackRight), FeatureTrackByLKGpu over semantic + naive (TrackRightGPU)
        dv_launch_lk_track_multi(d_lk + S, R, n_max_cls[0], ref->flow_back, 0.5f, s);
        dv_launch_lk_cuda_track_multi(d_lk + S + R, N, std::max(n_max_cls[1], n_max_cls[2]), ref->flow_back, 1.0f, s);
    }
    dv_launch_finalize_multi((const DvFinalizeJob*)(dp + o_fin), S, n_max, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipEventRecord(F.done, s));
    for (int k = 0; k < S; ++k) front_commit(mem[jobs[M[k]].member], jobs[M[k]].t, F.done, s, k >= R);
    F.rounds++; F.members_batched += S;
    return 0;
}
extern "C" int dv_batch_track_info(dv_batch* B, long long* rounds, long long* members_batched, long long* members_single) {
    if (!B) return -1;
    DvFrontBatch* F = be_batch_front(B);
    if (rounds) *rounds = F ? F->rounds : 0;
    if (members_batched) *members_batched = F ? F->members_batched : 0;
    if (members_single) *members_single = F ? F->members_single : 0;
    return 0;
}
