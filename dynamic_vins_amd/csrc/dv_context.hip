// dv_context.hip — the context of the C ABI (include/dvins.h): lifetime, HBM layout, error strings and the stage timers.
// Everything a frame needs lives in HBM inside the ctx:
//   * three image pyramids (left current, left previous, right), each level pitched to 16 B,
//     level 0 is a pitched copy of the input written by the first pyrDown launch;
//   * the tracker state as a struct of arrays (DvTrackState) with its counters in device memory,
//     so the whole of FeatureTracker::TrackImage is enqueued without a host round trip;
//   * Shi-Tomasi candidate records + the pinned host staging buffer for the frame's output.
// A frame's way into the pyramids is pyr_plan.hip, the per-frame mask stages are mask_frame.hip, the operator-level entries dv_ops.hip; the per-frame orchestration
// of the tracker (one sequence, or a dv_batch group in shared launches) is front_track.hip.
#include "dv_ctx.h"

static std::string g_last_error;
static std::mutex g_err_mutex;

void dv_set_error(dv_ctx* ctx, const std::string& msg) {
    if (ctx) { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->err = msg; }
    std::lock_guard<std::mutex> lk(g_err_mutex);
    g_last_error = msg;
}

// disc half-widths of cv::circle's midpoint rasteriser (drawing.cpp Circle(), fill = true)
void circle_half_widths(int radius, std::vector<uint8_t>& hw) {
    hw.assign(radius + 1, 0);
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        hw[dy] = (uint8_t)std::max<int>(hw[dy], dx);
        hw[dx] = (uint8_t)std::max<int>(hw[dx], dy);
        dy++; err += plus; plus += 2;
        int m = (err <= 0) - 1;
        err -= minus & m; dx += m; minus -= m & 2;
    }
}

int dv_ensure_hw(dv_ctx* ctx, int radius) {
    if (radius < 0 || radius > DV_MAX_RADIUS) DV_FAIL("disc radius (min_dist) out of range [0,128]");
    if (ctx->hw_radius == radius) return 0;
    std::vector<uint8_t> hw; circle_half_widths(radius, hw);
    DV_CHECK(ctx->hw_buf.ensure(DV_MAX_RADIUS + 1));
    DV_CHECK(hipMemcpyAsync(ctx->hw_buf.p, hw.data(), hw.size(), hipMemcpyHostToDevice, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->hw_radius = radius;
    return 0;
}

int dv_ensure_cand(dv_ctx* ctx, int w, int h) {
    int cap = std::max(4096, (w * h) / 4);
    if (cap <= ctx->cand_cap) return 0;
    DV_CHECK(ctx->cand_buf.ensure((size_t)cap * sizeof(DvCand)));
    ctx->cand_cap = cap;
    return 0;
}

StageTimer* dv_timer_for(dv_ctx* ctx, const char* name) {
    std::lock_guard<std::mutex> lk(ctx->timer_mu);
    for (auto& t : ctx->timers) if (t.name == name) return &t;
    ctx->timers.emplace_back();
    StageTimer& t = ctx->timers.back();
    t.name = name;
    return &t;
}
void dv_harvest_timers(dv_ctx* ctx, hipStream_t synced) {
    std::lock_guard<std::mutex> lk(ctx->timer_mu);
    for (auto& t : ctx->timers) {
        if (t.stream != synced) continue;
        for (size_t i = 0; i < t.used; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, t.pool[i].first, t.pool[i].second) == hipSuccess) { t.total_ms += ms; t.count++; }
        }
        t.used = 0;
    }
}

extern "C" {

void* dv_pinned_alloc(size_t bytes) {
    void* p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { dv_set_error(nullptr, "dv_pinned_alloc: hipHostMalloc failed"); return nullptr; }
    return p;
}
void dv_pinned_free(void* p) { if (p) (void)hipHostFree(p); }

const char* dv_last_error(dv_ctx* ctx) {
    if (ctx) {      // a copy per calling thread: another thread of a dynamic sequence may be writing the ctx's string (valid until this thread's next call)
        static thread_local std::string mine;
        std::lock_guard<std::mutex> lk(ctx->err_mu);
        mine = ctx->err;
        return mine.c_str();
    }
    std::lock_guard<std::mutex> lk(g_err_mutex);
    return g_last_error.c_str();
}

dv_ctx* dv_create(const dv_config* cfg) {
    if (!cfg) { dv_set_error(nullptr, "dv_create: null config"); return nullptr; }
    if (cfg->width <= 0 || cfg->height <= 0) { dv_set_error(nullptr, "dv_create: bad image size"); return nullptr; }
    if (cfg->max_cnt <= 0 || cfg->max_cnt > DV_MAX_FEATS) { dv_set_error(nullptr, "dv_create: max_cnt must be in [1,1024]"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { dv_set_error(nullptr, "dv_create: no HIP device (the HIP path has no CPU fallback)"); return nullptr; }
    if (cfg->device < 0 || cfg->device >= ndev) { dv_set_error(nullptr, "dv_create: bad device ordinal"); return nullptr; }
    dv_ctx* ctx = new dv_ctx();
    ctx->cfg = *cfg;
    auto fail = [&](const char* what, hipError_t e) -> dv_ctx* {
        dv_set_error(nullptr, std::string("dv_create: ") + what + ": " + hipGetErrorString(e));
        delete ctx; return nullptr;
    };
    hipError_t e;
    if ((e = hipSetDevice(cfg->device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipStreamCreateWithFlags(&ctx->be_stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipStreamCreateWithFlags(&ctx->obj_stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipEventCreateWithFlags(&ctx->done, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&ctx->ev_pyr, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipEventCreateWithFlags(&ctx->ev_bg_select, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    // tracker state: one block, struct of arrays
    const size_t N = DV_MAX_FEATS;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    size_t o_last = take(N * 8), o_cur = take(N * 8), o_lk = take(N * 8), o_lks = take(N), o_ids = take(N * 4), o_cnt = take(N * 4),
           o_pun = take(N * 8), o_prun = take(N * 8), o_prv = take(N), o_trk = take(N), o_rp = take(N * 8), o_rs = take(N),
           o_scal = take(64), o_ord = take(N * 2);
    if ((e = ctx->state_block.ensure(off)) != hipSuccess) return fail("hipMalloc(state)", e);
    uint8_t* base = (uint8_t*)ctx->state_block.p;
    ctx->tr.last_pts = (float2*)(base + o_last); ctx->tr.curr_pts = (float2*)(base + o_cur); ctx->tr.lk_pts = (float2*)(base + o_lk);
    ctx->tr.lk_status = base + o_lks; ctx->tr.ids = (uint32_t*)(base + o_ids); ctx->tr.track_cnt = (int32_t*)(base + o_cnt);
    ctx->tr.prev_un = (float2*)(base + o_pun); ctx->tr.prev_run = (float2*)(base + o_prun); ctx->tr.prev_rvalid = base + o_prv;
    ctx->tr.tracked = base + o_trk; ctx->tr.right_pts = (float2*)(base + o_rp); ctx->tr.right_status = base + o_rs;
    ctx->tr.n_feat = (int*)(base + o_scal); ctx->tr.n_tracked = ctx->tr.n_feat + 1; ctx->tr.next_id = (uint32_t*)(ctx->tr.n_feat + 2);
    ctx->tr.lk_order = (unsigned short*)(base + o_ord);
    ctx->n_cand = ctx->tr.n_feat + 3; ctx->max_ord = (unsigned*)(ctx->tr.n_feat + 4); ctx->err_flag = ctx->tr.n_feat + 5;
    if ((e = ctx->out_buf.ensure(N * sizeof(dv_feat) + 256)) != hipSuccess) return fail("hipMalloc(out)", e);
    ctx->out_dev = (dv_feat*)ctx->out_buf.p; ctx->nout_dev = (int*)((uint8_t*)ctx->out_buf.p + N * sizeof(dv_feat));
    void* pinned = nullptr;
    if ((e = hipHostMalloc(&pinned, N * sizeof(dv_feat) + 256, hipHostMallocDefault)) != hipSuccess) return fail("hipHostMalloc", e);
    ctx->out_pinned = (dv_feat*)pinned; ctx->nout_pinned = (int*)((uint8_t*)pinned + N * sizeof(dv_feat)); ctx->err_pinned = ctx->nout_pinned + 1;
    // the tables of the static-instance unmask launch (front_track.hip) are read in place from pinned memory: room for a full stack's rectangles from the start
    if ((e = hipHostMalloc(&ctx->unmask_pinned, dv_unmask_tab_bytes(DV_STACK_MAX_PLANES), hipHostMallocDefault)) != hipSuccess) return fail("hipHostMalloc", e);
    ctx->unmask_pinned_bytes = dv_unmask_tab_bytes(DV_STACK_MAX_PLANES);
    if (dv_reset(ctx) != 0) { std::string m = ctx->err; delete ctx; dv_set_error(nullptr, m); return nullptr; }
    return ctx;
}

void dv_destroy(dv_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    be_batch_detach(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    // (a frame tracked on a dv_batch's front-end stream: be_batch_detach above / dv_batch_destroy drain that stream — its event belongs to the batch and may be gone by now,
    //  so it is NOT waited on here: doing so crashed dv_destroy behind dv_runner_destroy, round 5)
    if (ctx->be_stream) (void)hipStreamSynchronize(ctx->be_stream);
    for (auto& t : ctx->timers) for (auto& p : t.pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (DevBuf* b : { &ctx->state_block, &ctx->cand_buf, &ctx->hw_buf, &ctx->mask_buf, &ctx->out_buf, &ctx->s0, &ctx->s1, &ctx->s2, &ctx->s3, &ctx->s4,
                       &ctx->left[0].buf, &ctx->left[1].buf, &ctx->right.buf, &ctx->leftc[0].buf, &ctx->leftc[1].buf, &ctx->rightc.buf, &ctx->opA.buf, &ctx->opB.buf, &ctx->undist_buf[0], &ctx->undist_buf[1] }) b->release();
    if (ctx->inst) dv_inst_destroy_internal(ctx->inst);
    if (ctx->est) dv_est_destroy_internal(ctx->est);
    be_dist_release(ctx);
    ctx->be.block.release(); ctx->be.marg_buf.release(); ctx->be.eig_spec.release();
    if (ctx->be.pinned) (void)hipHostFree(ctx->be.pinned);
    if (ctx->be.rej_pinned) (void)hipHostFree(ctx->be.rej_pinned);
    ctx->obj_buf.release(); ctx->obj_pend.release(); ctx->obj_op_pend.release();
    if (ctx->obj_stream) (void)hipStreamDestroy(ctx->obj_stream);
    if (ctx->be_stream) (void)hipStreamDestroy(ctx->be_stream);
    if (ctx->out_pinned) (void)hipHostFree(ctx->out_pinned);
    if (ctx->unmask_pinned) (void)hipHostFree(ctx->unmask_pinned);
    ctx->unmask_src_buf.release();
    // the nine per-frame stages own their buffers, pinned blocks and events (StageSlot, dv_ctx.h)
    dv_stage_delete(ctx->viode); dv_stage_delete(ctx->istack); dv_stage_delete(ctx->solo); dv_stage_delete(ctx->solo_in);
    dv_stage_delete(ctx->mot); dv_stage_delete(ctx->reid); dv_stage_delete(ctx->line_track); dv_stage_delete(ctx->lbd); dv_stage_delete(ctx->sgm);
    if (ctx->done) (void)hipEventDestroy(ctx->done);
    if (ctx->ev_pyr) (void)hipEventDestroy(ctx->ev_pyr);
    if (ctx->ev_bg_select) (void)hipEventDestroy(ctx->ev_bg_select);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int dv_reset(dv_ctx* ctx) {
    if (!ctx) return -1;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(hipMemsetAsync(ctx->state_block.p, 0, ctx->state_block.bytes, ctx->stream));
    const uint32_t one = 1;    // InstFeat::global_id_count{1} (front_end/instance_feature.h:137)
    DV_CHECK(hipMemcpyAsync(ctx->tr.next_id, &one, 4, hipMemcpyHostToDevice, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->last_front && ctx->last_front != ctx->stream && ctx->last_done) DV_CHECK(hipEventSynchronize(ctx->last_done));
    ctx->have_prev = false; ctx->prev_time = 0.0; ctx->pending = false; ctx->last_done = nullptr; ctx->last_front = nullptr; ctx->leftc_valid[0] = ctx->leftc_valid[1] = false;
    if (ctx->inst && dv_inst_reset(ctx)) return -1;
    return 0;
}

int dv_sync(dv_ctx* ctx) {
    if (!ctx) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_timing_enable(dv_ctx* ctx, int on) { if (!ctx) return -1; ctx->host_timing = on == -1; ctx->timing = on > 0; ctx->kernel_timing = on >= 2; return 0; }      // -1: host wall-clock scopes only (no events, no extra syncs)
int dv_timing_reset(dv_ctx* ctx) { if (!ctx) return -1; std::lock_guard<std::mutex> lk(ctx->timer_mu); for (auto& t : ctx->timers) { t.total_ms = 0; t.count = 0; t.used = 0; } return 0; }
int dv_timing_get(dv_ctx* ctx, const char* name, double* total_ms, long long* count) {
    if (!ctx || !name) return -1;
    std::lock_guard<std::mutex> lk(ctx->timer_mu);
    for (auto& t : ctx->timers) if (t.name == name) { if (total_ms) *total_ms = t.total_ms; if (count) *count = t.count; return 0; }
    if (total_ms) *total_ms = 0; if (count) *count = 0;
    return 0;
}

} // extern "C"
