// dvins_api.hip — C ABI (include/dvins.h) of libdvins_hip.so: context lifetime, HBM layout, timing and the operator-level entries.
// Everything a frame needs lives in HBM inside the ctx:
//   * three image pyramids (left current, left previous, right), each level pitched to 16 B,
//     level 0 is a pitched copy of the input written by the first pyrDown launch;
//   * the tracker state as a struct of arrays (DvTrackState) with its counters in device memory,
//     so the whole of FeatureTracker::TrackImage is enqueued without a host round trip;
//   * Shi-Tomasi candidate records + the pinned host staging buffer for the frame's output.
// The per-frame orchestration of the tracker (one sequence, or a dv_batch group in shared launches) is front_track.hip.
#include "dv_ctx.h"
#include "viode_host.h"
#include "inst_stack_host.h"

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

// How a frame becomes pyramid level 0, decided here and nowhere else.  Maps and / or BGR frames: a level-0 job (cv::remap, with cvtColor for colour frames, or
// cvtColor alone, straight into level 0; host frames are staged in s3 / s4 first, in rows of align_up(channels * w, 16) bytes).  Gray host frames, and pyramids of
// one level: a pitched copy.  Gray device frames: the level-1 step reads the frame itself and writes the pitched level-0 copy beside level 1 (frame read once).
// The copies are enqueued on s, the launches left to dv_launch_pyramids or a dv_batch round's tables.  undistort: the caller has checked the maps.
int dv_plan_pyramids(dv_ctx* ctx, const DvPyr& a, const DvPyr* b, const uint8_t* img0, const uint8_t* img1, int stride, int mem, bool undistort, hipStream_t s, PyrPlan& P) {
    const int w = a.L[0].w, h = a.L[0].h;
    const bool bgr = (mem & DV_FMT_BGR) != 0, dev = (mem & ~DV_FMT_BGR) == DV_MEM_DEVICE;
    if (!b) img1 = nullptr;
    P.has_l0 = undistort || bgr; P.pair = b != nullptr; P.levels = a.levels;
    if (P.has_l0) {
        const int cn = bgr ? 3 : 1;
        DvLevel0Job& z = P.l0; z = DvLevel0Job{};
        z.src0 = img0; z.src1 = img1; z.spitch = stride;
        if (!dev) {
            const int cp = align_up(cn * w, 16);
            DV_CHECK(ctx->s3.ensure((size_t)cp * h)); DV_CHECK(hipMemcpy2DAsync(ctx->s3.p, cp, img0, stride, (size_t)cn * w, h, hipMemcpyHostToDevice, s));
            z.src0 = (const uint8_t*)ctx->s3.p; z.spitch = cp;
            if (b) { DV_CHECK(ctx->s4.ensure((size_t)cp * h)); DV_CHECK(hipMemcpy2DAsync(ctx->s4.p, cp, img1, stride, (size_t)cn * w, h, hipMemcpyHostToDevice, s)); z.src1 = (const uint8_t*)ctx->s4.p; }
        }
        z.map0 = undistort ? (const uint8_t*)ctx->undist_buf[0].p : nullptr; z.map1 = (undistort && b) ? (const uint8_t*)ctx->undist_buf[1].p : nullptr;
        z.dst0 = a.L[0].p; z.dst1 = b ? b->L[0].p : nullptr; z.dpitch = a.L[0].pitch;
        z.kind = undistort ? (bgr ? DV_L0_REMAP_BGR : DV_L0_REMAP_GRAY) : DV_L0_BGR;
    } else if (!dev || a.levels == 1) {
        const hipMemcpyKind k = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        DV_CHECK(hipMemcpy2DAsync(a.L[0].p, a.L[0].pitch, img0, stride, w, h, k, s));
        if (b) DV_CHECK(hipMemcpy2DAsync(b->L[0].p, b->L[0].pitch, img1, stride, w, h, k, s));
    }
    for (int l = 1; l < a.levels; ++l) {
        const bool fuse = dev && l == 1 && !P.has_l0;
        DvPyrJob& pj = P.down[l - 1]; pj = DvPyrJob{};
        pj.src0 = fuse ? img0 : a.L[l - 1].p; pj.src1 = b ? (fuse ? img1 : b->L[l - 1].p) : nullptr;
        pj.dst0 = a.L[l].p; pj.dst1 = b ? b->L[l].p : nullptr;
        pj.sw = a.L[l - 1].w; pj.sh = a.L[l - 1].h; pj.spitch = fuse ? stride : a.L[l - 1].pitch; pj.dw = a.L[l].w; pj.dh = a.L[l].h; pj.dpitch = a.L[l].pitch;
        pj.cpy0 = fuse ? a.L[0].p : nullptr; pj.cpy1 = (fuse && b) ? b->L[0].p : nullptr; pj.cpitch = a.L[0].pitch;
    }
    P.apron[0] = a; P.apron[1] = b ? *b : a;      // (one image: the second entry repeats the first — idempotent in a table, not launched by value)
    return 0;
}

// the plan's launches with the single-sequence kernels, every argument by value
void dv_launch_pyramids(const PyrPlan& P, hipStream_t s) {
    const DvLevel0Job& z = P.l0;
    const int w = P.apron[0].L[0].w, h = P.apron[0].L[0].h;
    if (P.has_l0 && z.kind == DV_L0_BGR) dv_launch_bgr2gray(z.src0, z.src1, w, h, z.spitch, z.dst0, z.dst1, z.dpitch, s);
    else if (P.has_l0) {
        const size_t m2off = (size_t)4 * w * h;      // a camera's map block: w * h short2 of map1, then map2
        const int bgr = z.kind == DV_L0_REMAP_BGR;
        dv_launch_remap(z.src0, z.src1, w, h, z.spitch, bgr ? 3 : 1, bgr, (const int16_t*)z.map0, (const uint16_t*)(z.map0 + m2off),
                        (const int16_t*)z.map1, z.map1 ? (const uint16_t*)(z.map1 + m2off) : nullptr, z.dst0, z.dst1, z.dpitch, s);
    }
    for (int l = 1; l < P.levels; ++l) { const DvPyrJob& j = P.down[l - 1]; dv_launch_pyr_down2(j.src0, j.src1, j.sw, j.sh, j.spitch, j.dst0, j.dst1, j.dpitch, j.cpy0, j.cpy1, j.cpitch, s); }
    dv_launch_pyr_apron(P.apron[0], P.pair ? &P.apron[1] : nullptr, s);
}

// Builds the pyramids of one image (img1 == nullptr) or of a pair with shared launches: the operator-level entries' form (no maps)
static int build_pyramids(dv_ctx* ctx, PyrSet& P0, PyrSet* P1, const uint8_t* img0, const uint8_t* img1, int w, int h, int stride, int mem, int max_level) {
    DV_CHECK(P0.alloc(w, h, max_level));
    if (P1) DV_CHECK(P1->alloc(w, h, max_level));
    PyrPlan P;
    if (dv_plan_pyramids(ctx, P0.pyr, P1 ? &P1->pyr : nullptr, img0, img1, stride, mem, false, ctx->stream, P)) return -1;
    dv_launch_pyramids(P, ctx->stream);
    DV_CHECK(hipGetLastError());
    return 0;
}

// the pyramid cv::cuda::SparsePyrLKOpticalFlow builds (cuda::pyrDown: round half to even) on top of an existing level 0 (a0 / b0: level 0 of the regular pyramids)
int dv_plan_cuda_pyramids(dv_ctx* ctx, PyrSet& C0, PyrSet* C1, const DvPyr& a0, const DvPyr* b0, int w, int h, int max_level, CudaPyrPlan& P) {
    DV_CHECK(C0.alloc(w, h, max_level, true));
    if (C1) DV_CHECK(C1->alloc(w, h, max_level, true));
    C0.pyr.L[0] = a0.L[0];
    if (C1) C1->pyr.L[0] = b0->L[0];
    P.levels = C0.pyr.levels;
    for (int l = 1; l < P.levels; ++l) {
        const DvLevel& f = C0.pyr.L[l - 1]; const DvLevel& t = C0.pyr.L[l];
        DvPyrJob& pj = P.down[l - 1]; pj = DvPyrJob{};
        pj.src0 = f.p; pj.src1 = C1 ? C1->pyr.L[l - 1].p : nullptr; pj.dst0 = t.p; pj.dst1 = C1 ? C1->pyr.L[l].p : nullptr;
        pj.sw = f.w; pj.sh = f.h; pj.spitch = f.pitch; pj.dw = t.w; pj.dh = t.h; pj.dpitch = t.pitch;
    }
    return 0;
}
void dv_launch_cuda_pyramids(const CudaPyrPlan& P, hipStream_t s) {
    for (int l = 1; l < P.levels; ++l) { const DvPyrJob& j = P.down[l - 1]; dv_launch_pyr_down2(j.src0, j.src1, j.sw, j.sh, j.spitch, j.dst0, j.dst1, j.dpitch, nullptr, nullptr, 0, s, 1); }
}
int dv_build_cuda_pyramids(dv_ctx* ctx, PyrSet& C0, PyrSet* C1, const DvPyr& a0, const DvPyr* b0, int w, int h, int max_level) {
    CudaPyrPlan P;
    if (dv_plan_cuda_pyramids(ctx, C0, C1, a0, b0, w, h, max_level, P)) return -1;
    dv_launch_cuda_pyramids(P, ctx->stream);
    DV_CHECK(hipGetLastError());
    return 0;
}

// dv_viode_frame_enqueue / _collect: thread T1's per-frame stage on the ctx's stream.  Two buffer sets used alternately: set[cur] belongs to the frame enqueued last, the
// inverse mask and key images of the frame before stay intact while that frame is tracked.
struct ViodeFrame {
    struct Set { DevBuf inv, keys0, keys1; } set[2];
    int cur = 1;
    DevBuf seg[2], scratch /* planes nobody reads: the merged mask, the right image's two masks */, small /* keys (256 B) | boxes left (1024 B) | boxes right (1024 B) */;
    uint8_t* pinned = nullptr;      // box initialiser (1024 B) | keys (256 B) | the frame's boxes (1024 B)
    hipEvent_t ev = nullptr; bool pending = false, has_right = false; int nkeys = 0, keys_on_dev = 0; uint32_t keys[64] = { 0 };
};
static void dv_viode_frame_release(dv_ctx* ctx) {
    ViodeFrame* V = ctx->viode;
    if (!V) return;
    for (ViodeFrame::Set& q : V->set) { q.inv.release(); q.keys0.release(); q.keys1.release(); }
    V->seg[0].release(); V->seg[1].release(); V->scratch.release(); V->small.release();
    if (V->pinned) (void)hipHostFree(V->pinned);
    if (V->ev) (void)hipEventDestroy(V->ev);
    delete V; ctx->viode = nullptr;
}

// dv_inst_stack_frame_enqueue / _collect: the same stage from a detector's mask stack.  Two buffer sets used alternately, as above: set[cur] belongs to the frame enqueued
// last.  A DV_MEM_HOST stack is staged into its set (tightly packed) and `from` remembers its descriptor: the *_planes entries of the frame find the copy there.
struct InstStackFrame {
    struct Set { DevBuf merge, inv, staged; dv_mask_stack from{}; bool has_staged = false; } set[2];
    int cur = 1;
    DevBuf small /* boxes (1024 B) */, scratch /* DV_STACK_REMAP_MERGED: the merged mask before the remap | the remapped one, pitched */;
    uint8_t* pinned = nullptr;      // box initialiser (1024 B) | the frame's boxes (1024 B)
    hipEvent_t ev = nullptr; bool pending = false; int n_planes = 0;
};
static void dv_inst_stack_frame_release(dv_ctx* ctx) {
    InstStackFrame* V = ctx->istack;
    if (!V) return;
    for (InstStackFrame::Set& q : V->set) { q.merge.release(); q.inv.release(); q.staged.release(); }
    V->small.release(); V->scratch.release();
    if (V->pinned) (void)hipHostFree(V->pinned);
    if (V->ev) (void)hipEventDestroy(V->ev);
    delete V; ctx->istack = nullptr;
}
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
    if (V->pending) V->set[V->cur ^ 1].has_staged = false;
    else V->set[0].has_staged = V->set[1].has_staged = false;
}
int dv_stack_resolve(dv_ctx* ctx, const dv_mask_stack& st, DevBuf& own_buf, hipStream_t s, DvStackSrc* out) {
    const int es = st.kind == DV_STACK_F32 ? 4 : 1, w = ctx->cfg.width, h = ctx->cfg.height;
    if (st.mem != DV_MEM_HOST) { *out = DvStackSrc{ (const uint8_t*)st.data, (long long)st.plane_stride, st.row_stride, st.n_planes, st.kind, st.threshold }; return 0; }
    const void* dev = nullptr;
    if (ctx->istack && !ctx->istack->pending) {
        const InstStackFrame::Set& Q = ctx->istack->set[ctx->istack->cur];
        if (Q.has_staged && same_stack(Q.from, st)) dev = Q.staged.p;
    }
    if (!dev) { if (stage_host_stack(ctx, st, es, own_buf, s)) return -1; dev = own_buf.p; }
    *out = DvStackSrc{ (const uint8_t*)dev, (long long)w * es * h, w * es, st.n_planes, st.kind, st.threshold };
    return 0;
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
    dv_viode_frame_release(ctx);
    dv_inst_stack_frame_release(ctx);
    dv_solo_head_release(ctx);
    dv_solo_input_release(ctx);
    dv_mot_release(ctx);
    dv_reid_release(ctx);
    dv_line_track_release(ctx);
    dv_lbd_release(ctx);
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

// ------------------------------- operator-level entries -------------------------------

// copies `bytes` from user memory (host or device) into a ctx scratch buffer on the device
static int stage_in(dv_ctx* ctx, DevBuf& b, const void* src, size_t bytes, int mem) {
    DV_CHECK(b.ensure(bytes ? bytes : 1));
    if (bytes) DV_CHECK(hipMemcpyAsync(b.p, src, bytes, mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
static int stage_out(dv_ctx* ctx, void* dst, const void* src, size_t bytes, int mem) {
    if (bytes) DV_CHECK(hipMemcpyAsync(dst, src, bytes, mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

int dv_lk(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride, const float* pts_a, int n, int max_level,
          int iters, double eps, int use_initial, float* pts_b, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img_a || !img_b || !pts_a || n <= 0) DV_FAIL("dv_lk: empty input (reference throws std::runtime_error, feature_utils.cpp:39-41)");
    if (max_level < 0 || max_level > 3) DV_FAIL("dv_lk: max_level must be in [0,3]");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (build_pyramids(ctx, ctx->opA, nullptr, img_a, nullptr, w, h, stride, mem, max_level)) return -1;
    if (build_pyramids(ctx, ctx->opB, nullptr, img_b, nullptr, w, h, stride, mem, max_level)) return -1;
    const int ml = std::min(ctx->opA.pyr.levels, ctx->opB.pyr.levels) - 1;
    if (stage_in(ctx, ctx->s0, pts_a, (size_t)n * 8, mem)) return -1;
    if (use_initial) { if (stage_in(ctx, ctx->s1, pts_b, (size_t)n * 8, mem)) return -1; }
    else DV_CHECK(ctx->s1.ensure((size_t)n * 8));
    DV_CHECK(ctx->s2.ensure(n));
    iters = std::min(std::max(iters, 0), 100);
    eps = std::min(std::max(eps, 0.), 10.);
    dv_launch_lk_generic(ctx->opA.pyr, ctx->opB.pyr, (const float2*)ctx->s0.p, n, ml, iters, eps * eps, use_initial, (float2*)ctx->s1.p,
                         (uint8_t*)ctx->s2.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (stage_out(ctx, pts_b, ctx->s1.p, (size_t)n * 8, mem)) return -1;
    if (stage_out(ctx, status, ctx->s2.p, n, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_track_by_lk(dv_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride, const float* pts1, int n,
                   int flow_back, float dist_thresh, float* pts2, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img1 || !img2 || !pts1 || n <= 0) DV_FAIL("dv_track_by_lk: FeatureTrackByLK() input wrong, received at least one of parameter are empty");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (build_pyramids(ctx, ctx->opA, &ctx->opB, img1, img2, w, h, stride, mem, 3)) return -1;
    if (stage_in(ctx, ctx->s0, pts1, (size_t)n * 8, mem)) return -1;
    DV_CHECK(ctx->s1.ensure((size_t)n * 8));
    DV_CHECK(ctx->s2.ensure(n));
    StageScope sc(ctx, "op_lk_track");
    dv_launch_lk_track(ctx->opA.pyr, ctx->opB.pyr, (const float2*)ctx->s0.p, nullptr, n, flow_back, dist_thresh, (float2*)ctx->s1.p,
                       (uint8_t*)ctx->s2.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (stage_out(ctx, pts2, ctx->s1.p, (size_t)n * 8, mem)) return -1;
    if (stage_out(ctx, status, ctx->s2.p, n, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// cv::cuda::SparsePyrLKOpticalFlow::calc (use_initial: pts_b holds the initial flow) and FeatureTrackByLKGpu, operator forms for the parity tests
static int lk_cuda_prepare(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride, int mem, int max_level) {
    if (build_pyramids(ctx, ctx->opA, &ctx->opB, img_a, img_b, w, h, stride, mem, 0)) return -1;          // level 0 only (pitched copies)
    return dv_build_cuda_pyramids(ctx, ctx->leftc[0], &ctx->leftc[1], ctx->opA.pyr, &ctx->opB.pyr, w, h, max_level);
}
int dv_lk_cuda(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride, const float* pts_a, int n, int max_level, int iters, int use_initial,
               float* pts_b, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img_a || !img_b || !pts_a || n <= 0) DV_FAIL("dv_lk_cuda: empty input");
    if (max_level < 0 || max_level > 3 || iters < 0 || iters > 100) DV_FAIL("dv_lk_cuda: max_level must be in [0,3], iters in [0,100]");
    if (ctx->pending || ctx->have_prev) DV_FAIL("dv_lk_cuda: operator calls need a ctx that is not tracking a sequence (its pyramids are used as scratch)");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (lk_cuda_prepare(ctx, img_a, img_b, w, h, stride, mem, max_level)) return -1;
    const int ml = std::min(ctx->leftc[0].pyr.levels, ctx->leftc[1].pyr.levels) - 1;
    if (stage_in(ctx, ctx->s0, pts_a, (size_t)n * 8, mem)) return -1;
    if (use_initial) { if (stage_in(ctx, ctx->s1, pts_b, (size_t)n * 8, mem)) return -1; } else DV_CHECK(ctx->s1.ensure((size_t)n * 8));
    DV_CHECK(ctx->s2.ensure(n));
    dv_launch_lk_cuda_generic(ctx->leftc[0].pyr, ctx->leftc[1].pyr, (const float2*)ctx->s0.p, n, ml, iters, use_initial, (float2*)ctx->s1.p, (uint8_t*)ctx->s2.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (stage_out(ctx, pts_b, ctx->s1.p, (size_t)n * 8, mem)) return -1;
    if (stage_out(ctx, status, ctx->s2.p, n, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int dv_track_by_lk_gpu(dv_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride, const float* pts1, int n, int flow_back, float* pts2, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img1 || !img2 || !pts1 || n <= 0) DV_FAIL("dv_track_by_lk_gpu: flowTrack() input wrong, received at least one of parameter are empty");
    if (ctx->pending || ctx->have_prev) DV_FAIL("dv_track_by_lk_gpu: operator calls need a ctx that is not tracking a sequence (its pyramids are used as scratch)");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (lk_cuda_prepare(ctx, img1, img2, w, h, stride, mem, 3)) return -1;
    if (stage_in(ctx, ctx->s0, pts1, (size_t)n * 8, mem)) return -1;
    DV_CHECK(ctx->s1.ensure((size_t)n * 8)); DV_CHECK(ctx->s2.ensure(n));
    dv_launch_lk_cuda_track(ctx->leftc[0].pyr, ctx->leftc[1].pyr, (const float2*)ctx->s0.p, nullptr, n, flow_back, 1.0f, (float2*)ctx->s1.p, (uint8_t*)ctx->s2.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (stage_out(ctx, pts2, ctx->s1.p, (size_t)n * 8, mem)) return -1;
    if (stage_out(ctx, status, ctx->s2.p, n, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}
// stage an image (host or device) into a pitched device buffer; returns pointer/pitch to use
static int stage_image(dv_ctx* ctx, DevBuf& b, const uint8_t* img, int w, int h, int stride, int mem, const uint8_t** out, int* pitch) {
    if (mem == DV_MEM_DEVICE) { *out = img; *pitch = stride; return 0; }
    const int p = align_up(w, 16);
    DV_CHECK(b.ensure((size_t)p * h + 64));
    DV_CHECK(hipMemcpy2DAsync(b.p, p, img, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    *out = (const uint8_t*)b.p; *pitch = p;
    return 0;
}

// cuda::pyrDown on an 8-bit image (the level step of that tracker's pyramid); dst is ((w+1)/2) x ((h+1)/2), tightly packed
int dv_pyr_down_cuda(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst) DV_FAIL("dv_pyr_down_cuda: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const uint8_t* d_src; int pitch;
    if (stage_image(ctx, ctx->s0, src, w, h, stride, mem, &d_src, &pitch)) return -1;
    const int dw = (w + 1) / 2, dh = (h + 1) / 2, dp = align_up(dw, 16);
    DV_CHECK(ctx->s1.ensure((size_t)dp * dh + 64));
    dv_launch_pyr_down2(d_src, nullptr, w, h, pitch, (uint8_t*)ctx->s1.p, nullptr, dp, nullptr, nullptr, 0, ctx->stream, 1);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpy2DAsync(dst, dw, ctx->s1.p, dp, dw, dh, mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

static int min_eigen_rule(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem, int rule) {
    if (!ctx) return -1;
    if (!img || !eig) DV_FAIL("dv_min_eigen: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const uint8_t* d_img; int pitch;
    if (stage_image(ctx, ctx->s0, img, w, h, stride, mem, &d_img, &pitch)) return -1;
    if (dv_ensure_cand(ctx, w, h)) return -1;
    float* d_eig = eig;
    if (mem != DV_MEM_DEVICE) { DV_CHECK(ctx->s1.ensure((size_t)w * h * 4)); d_eig = (float*)ctx->s1.p; }
    DV_CHECK(hipMemsetAsync(ctx->n_cand, 0, 8, ctx->stream));     // n_cand + max_ord
    GfttTileArgs a{};
    a.img = d_img; a.w = w; a.h = h; a.pitch = pitch; a.eig_out = d_eig; a.eig_pitch = w;
    a.cand = (DvCand*)ctx->cand_buf.p; a.cand_cap = ctx->cand_cap; a.n_cand = ctx->n_cand; a.max_ord = ctx->max_ord; a.rule = rule;
    dv_launch_gftt_tile(a, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (mem != DV_MEM_DEVICE) DV_CHECK(hipMemcpyAsync(eig, d_eig, (size_t)w * h * 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_min_eigen(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem) { return min_eigen_rule(ctx, img, w, h, stride, eig, mem, DV_GFTT_RULE_CPU); }
int dv_min_eigen_cuda(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem) { return min_eigen_rule(ctx, img, w, h, stride, eig, mem, DV_GFTT_RULE_CUDA); }

static int gftt_rule_op(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride, int max_n, double quality,
                        double min_dist, float* out_xy, int* n_out, int mem, int rule) {
    if (!ctx) return -1;
    if (!img || !out_xy || !n_out) DV_FAIL("dv_gftt: null argument");
    if (!(quality > 0)) DV_FAIL("dv_gftt: qualityLevel must be > 0");
    if (min_dist < 0) DV_FAIL("dv_gftt: minDistance must be >= 0");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const uint8_t *d_img, *d_mask = nullptr; int pitch, mpitch = 0;
    if (stage_image(ctx, ctx->s0, img, w, h, stride, mem, &d_img, &pitch)) return -1;
    if (mask_or_null && stage_image(ctx, ctx->s3, mask_or_null, w, h, stride, mem, &d_mask, &mpitch)) return -1;
    if (dv_ensure_cand(ctx, w, h)) return -1;
    DV_CHECK(ctx->s1.ensure((size_t)DV_MAX_FEATS * 8 + 16));
    float2* d_out = (float2*)ctx->s1.p; int* d_n = (int*)((uint8_t*)ctx->s1.p + (size_t)DV_MAX_FEATS * 8);
    DV_CHECK(hipMemsetAsync(ctx->n_cand, 0, 12, ctx->stream));    // n_cand, max_ord, err_flag
    GfttTileArgs a{};
    a.img = d_img; a.w = w; a.h = h; a.pitch = pitch; a.in_mask = d_mask; a.mask_pitch = mpitch;
    a.cand = (DvCand*)ctx->cand_buf.p; a.cand_cap = ctx->cand_cap; a.n_cand = ctx->n_cand; a.max_ord = ctx->max_ord; a.rule = rule;
    dv_launch_gftt_tile(a, ctx->stream);
    GfttSelectArgs sa{};
    sa.cand = (const DvCand*)ctx->cand_buf.p; sa.n_cand = ctx->n_cand; sa.cand_cap = ctx->cand_cap; sa.max_ord = ctx->max_ord;
    sa.w = w; sa.h = h; sa.quality = quality; sa.min_dist = min_dist; sa.max_n_host = max_n; sa.n_feat = nullptr;
    sa.out_xy = d_out; sa.n_out = d_n; sa.has_tr = 0; sa.err_flag = ctx->err_flag; sa.rule = rule;
    if (dv_launch_gftt_select(sa, ctx->stream)) DV_FAIL("gftt_select: cannot set dynamic LDS size");
    DV_CHECK(hipGetLastError());
    int n = 0, ef = 0;
    DV_CHECK(hipMemcpyAsync(&n, d_n, 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipMemcpyAsync(&ef, ctx->err_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    if (ef) { DV_CHECK(hipMemsetAsync(ctx->err_flag, 0, 4, ctx->stream)); DV_FAIL("dv_gftt: device error flags=" + std::to_string(ef)); }
    if (stage_out(ctx, out_xy, d_out, (size_t)n * 8, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    *n_out = n;
    return 0;
}

int dv_gftt(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride, int max_n, double quality,
            double min_dist, float* out_xy, int* n_out, int mem) {
    return gftt_rule_op(ctx, img, mask_or_null, w, h, stride, max_n, quality, min_dist, out_xy, n_out, mem, DV_GFTT_RULE_CPU);
}
int dv_gftt_cuda(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride, int max_n, double quality,
                 double min_dist, float* out_xy, int* n_out, int mem) {
    return gftt_rule_op(ctx, img, mask_or_null, w, h, stride, max_n, quality, min_dist, out_xy, n_out, mem, DV_GFTT_RULE_CUDA);
}

int dv_viode_mask(dv_ctx* ctx, const uint8_t* seg_bgr, int w, int h, int stride, const uint32_t* dyn_keys, int nkeys, uint8_t* merge_mask, uint8_t* inv_merge_mask,
                  uint32_t* key_image, int32_t* boxes) {
    if (!ctx) return -1;
    if (!seg_bgr || !dyn_keys || !merge_mask || !inv_merge_mask || !boxes || w <= 0 || h <= 0 || stride < 3 * w) DV_FAIL("dv_viode_mask: bad argument");
    if (nkeys < 1 || nkeys > 64) DV_FAIL("dv_viode_mask: 1..64 dynamic keys");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    const int sp = align_up(3 * w, 16), mp = align_up(w, 16);
    DV_CHECK(ctx->s0.ensure((size_t)sp * h));                             // label image
    DV_CHECK(ctx->s1.ensure((size_t)mp * h)); DV_CHECK(ctx->s2.ensure((size_t)mp * h));      // merge, inverse
    DV_CHECK(ctx->s3.ensure((size_t)4 * w * h + 4096));                    // key image | keys | boxes
    DV_CHECK(ctx->s4.ensure(4096));
    uint32_t* d_keys = (uint32_t*)ctx->s4.p; int32_t* d_box = (int32_t*)((uint8_t*)ctx->s4.p + 1024);
    int32_t init[256];
    for (int k = 0; k < 64; ++k) { init[4 * k] = 0x7fffffff; init[4 * k + 1] = -1; init[4 * k + 2] = 0x7fffffff; init[4 * k + 3] = -1; }
    DV_CHECK(hipMemcpy2DAsync(ctx->s0.p, sp, seg_bgr, stride, (size_t)3 * w, h, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(d_keys, dyn_keys, 4 * (size_t)nkeys, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(d_box, init, 16 * (size_t)nkeys, hipMemcpyHostToDevice, s));
    DV_CHECK(hipStreamSynchronize(s));                                     // init[] is a stack object
    dv_launch_viode_mask((const uint8_t*)ctx->s0.p, w, h, sp, d_keys, nkeys, (uint8_t*)ctx->s1.p, (uint8_t*)ctx->s2.p, mp, key_image ? (uint32_t*)ctx->s3.p : nullptr, d_box, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpy2DAsync(merge_mask, w, ctx->s1.p, mp, w, h, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipMemcpy2DAsync(inv_merge_mask, w, ctx->s2.p, mp, w, h, hipMemcpyDeviceToHost, s));
    if (key_image) DV_CHECK(hipMemcpyAsync(key_image, ctx->s3.p, (size_t)4 * w * h, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipMemcpyAsync(boxes, d_box, 16 * (size_t)nkeys, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < nkeys; ++k) if (boxes[4 * k + 1] < 0) { boxes[4 * k] = boxes[4 * k + 2] = -1; boxes[4 * k + 3] = -1; }      // key not present
    return 0;
}

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
    if (mem != DV_MEM_HOST && mem != DV_MEM_DEVICE && mem != DV_MEM_PINNED) DV_FAIL("dv_viode_frame_enqueue: unknown memory kind");
    if (ctx->viode && ctx->viode->pending) DV_FAIL("dv_viode_frame_enqueue: previous frame not collected");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    if (!ctx->viode) {
        ViodeFrame* N = new ViodeFrame();
        ctx->viode = N;          // (a half-built one is completed by the next call or released by dv_destroy)
    }
    ViodeFrame& V = *ctx->viode;
    if (!V.ev) DV_CHECK(hipEventCreateWithFlags(&V.ev, hipEventDisableTiming));
    if (!V.pinned) {
        void* p = nullptr;
        DV_CHECK(hipHostMalloc(&p, 1024 + 256 + 1024, hipHostMallocDefault));
        V.pinned = (uint8_t*)p;
        int32_t* init = (int32_t*)V.pinned;
        for (int k = 0; k < 64; ++k) { init[4 * k] = 0x7fffffff; init[4 * k + 1] = -1; init[4 * k + 2] = 0x7fffffff; init[4 * k + 3] = -1; }
    }
    const int mp = w, sp = align_up(3 * w, 16);          // the masks are tightly packed: the inverse mask goes to dv_track_stereo_enqueue as a DV_MEM_DEVICE mask beside gray frames of stride w
    const size_t plane = ((size_t)mp * h + 255) / 256 * 256;
    ViodeFrame::Set& Q = V.set[V.cur ^ 1];
    DV_CHECK(Q.inv.ensure(plane)); DV_CHECK(Q.keys0.ensure((size_t)4 * w * h));
    if (seg1_bgr_or_null) DV_CHECK(Q.keys1.ensure((size_t)4 * w * h));
    DV_CHECK(V.scratch.ensure(3 * plane)); DV_CHECK(V.small.ensure(256 + 2048));
    // the set about to be overwritten held the frame before the last: the objects of that frame may still read its key images on the object tracker's stream
    if (dv_inst_wait_before_next_frame(ctx, s, false)) DV_FAIL("dv_viode_frame_enqueue: hipStreamWaitEvent");
    uint32_t* d_keys = (uint32_t*)V.small.p; int32_t* d_box0 = (int32_t*)((uint8_t*)V.small.p + 256); int32_t* d_box1 = d_box0 + 256;
    if (V.keys_on_dev != nkeys || std::memcmp(V.keys, dyn_keys, 4 * (size_t)nkeys) != 0) {      // (no frame is in flight: the pinned copy of the table is not being read)
        std::memcpy(V.keys, dyn_keys, 4 * (size_t)nkeys); std::memcpy(V.pinned + 1024, dyn_keys, 4 * (size_t)nkeys);
        DV_CHECK(dv_copy_async(d_keys, V.pinned + 1024, 256, s));
        V.keys_on_dev = nkeys;
    }
    V.nkeys = nkeys;
    DV_CHECK(dv_copy_async(d_box0, V.pinned, 1024, s));          // the box buffers start every frame at (max, -1, max, -1)
    if (seg1_bgr_or_null) DV_CHECK(dv_copy_async(d_box1, V.pinned, 1024, s));
    const uint8_t* src[2] = { seg0_bgr, seg1_bgr_or_null }; int spitch = stride;
    if (mem == DV_MEM_HOST) {
        for (int i = 0; i < 2; ++i) if (src[i]) {
            DV_CHECK(V.seg[i].ensure((size_t)sp * h));
            DV_CHECK(hipMemcpy2DAsync(V.seg[i].p, sp, src[i], stride, (size_t)3 * w, h, hipMemcpyHostToDevice, s));
            src[i] = (const uint8_t*)V.seg[i].p;
        }
        spitch = sp;
    }
    uint8_t* sc = (uint8_t*)V.scratch.p;
    {
        StageScope sc_t(ctx, "viode_frame");
        dv_launch_viode_mask(src[0], w, h, spitch, d_keys, nkeys, sc, (uint8_t*)Q.inv.p, mp, (uint32_t*)Q.keys0.p, d_box0, s);
        if (src[1]) dv_launch_viode_mask(src[1], w, h, spitch, d_keys, nkeys, sc + plane, sc + 2 * plane, mp, (uint32_t*)Q.keys1.p, d_box1, s);
    }
    DV_CHECK(hipGetLastError());
    DV_CHECK(dv_copy_async(V.pinned + 1280, d_box0, 1024, s));
    DV_CHECK(hipEventRecord(V.ev, s));
    V.cur ^= 1; V.pending = true; V.has_right = seg1_bgr_or_null != nullptr;
    return 0;
}

int dv_viode_frame_collect(dv_ctx* ctx, int min_inst_size, dv_inst_det* dets, int cap, int* n_dets, const uint8_t** inv_mask_dev, const uint32_t** keys0_dev, const uint32_t** keys1_dev) {
    if (!ctx) return -1;
    if (!ctx->viode || !ctx->viode->pending) DV_FAIL("dv_viode_frame_collect: nothing enqueued");
    if (!n_dets || cap < 0 || (cap > 0 && !dets)) DV_FAIL("dv_viode_frame_collect: bad argument");
    ViodeFrame& V = *ctx->viode;
    DV_CHECK(hipEventSynchronize(V.ev));
    V.pending = false;
    const int n = dv_viode_build_dets((const int32_t*)(V.pinned + 1280), V.keys, V.nkeys, min_inst_size, dets, cap);
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
    if (ctx->istack && ctx->istack->pending) DV_FAIL("dv_inst_stack_frame_enqueue: previous frame not collected");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    if (!ctx->istack) ctx->istack = new InstStackFrame();          // (a half-built one is completed by the next call or released by dv_destroy)
    InstStackFrame& V = *ctx->istack;
    if (!V.ev) DV_CHECK(hipEventCreateWithFlags(&V.ev, hipEventDisableTiming));
    if (!V.pinned) {
        void* p = nullptr;
        DV_CHECK(hipHostMalloc(&p, 2048, hipHostMallocDefault));
        V.pinned = (uint8_t*)p;
        int32_t* init = (int32_t*)V.pinned;
        for (int k = 0; k < 64; ++k) { init[4 * k] = 0x7fffffff; init[4 * k + 1] = -1; init[4 * k + 2] = 0x7fffffff; init[4 * k + 3] = -1; }
    }
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
    DV_CHECK(dv_copy_async(d_box, V.pinned, 1024, s));          // the boxes start every frame at (max, -1, max, -1)
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
    DV_CHECK(hipGetLastError());
    DV_CHECK(dv_copy_async(V.pinned + 1024, d_box, 1024, s));
    DV_CHECK(hipEventRecord(V.ev, s));
    if (st.mem == DV_MEM_HOST) { Q.from = st; Q.has_staged = true; }
    V.cur ^= 1; V.pending = true; V.n_planes = st.n_planes;
    return 0;
}

int dv_inst_stack_frame_collect(dv_ctx* ctx, int min_inst_size, dv_inst_det* dets, int32_t* planes, int cap, int* n_dets, const uint8_t** inv_mask_dev, const uint8_t** merge_mask_dev) {
    if (!ctx) return -1;
    if (!ctx->istack || !ctx->istack->pending) DV_FAIL("dv_inst_stack_frame_collect: nothing enqueued");
    if (!n_dets || cap < 0 || (cap > 0 && !dets)) DV_FAIL("dv_inst_stack_frame_collect: bad argument");
    InstStackFrame& V = *ctx->istack;
    DV_CHECK(hipEventSynchronize(V.ev));
    V.pending = false;
    const int n = dv_stack_build_dets((const int32_t*)(V.pinned + 1024), V.n_planes, min_inst_size, dets, planes, cap);
    if (n < 0) DV_FAIL("dv_inst_stack_frame_collect: more detections than `cap`");
    *n_dets = n;
    const InstStackFrame::Set& Q = V.set[V.cur];
    if (inv_mask_dev) *inv_mask_dev = (const uint8_t*)Q.inv.p;
    if (merge_mask_dev) *merge_mask_dev = (const uint8_t*)Q.merge.p;
    return 0;
}

int dv_bgr2gray(dv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* gray, int mem) {
    if (!ctx) return -1;
    if (!bgr || !gray || w <= 0 || h <= 0 || stride < 3 * w) DV_FAIL("dv_bgr2gray: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    const uint8_t* src = bgr; int sp = stride;
    if (mem != DV_MEM_DEVICE) {
        sp = align_up(3 * w, 16);
        DV_CHECK(ctx->s3.ensure((size_t)sp * h));
        DV_CHECK(hipMemcpy2DAsync(ctx->s3.p, sp, bgr, stride, (size_t)3 * w, h, hipMemcpyHostToDevice, s));
        src = (const uint8_t*)ctx->s3.p;
    }
    const int dp = align_up(w, 16);
    DV_CHECK(ctx->s4.ensure((size_t)dp * h));
    dv_launch_bgr2gray(src, nullptr, w, h, sp, (uint8_t*)ctx->s4.p, nullptr, dp, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpy2DAsync(gray, w, ctx->s4.p, dp, w, h, mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

int dv_remap(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, int channels, const int16_t* map1_xy, const uint16_t* map2, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst || !map1_xy || !map2 || w <= 0 || h <= 0 || (channels != 1 && channels != 3) || stride < channels * w) DV_FAIL("dv_remap: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    const bool dev = mem == DV_MEM_DEVICE;
    const uint8_t* d_src = src; int sp = stride;
    if (!dev) {
        sp = align_up(channels * w, 16);
        DV_CHECK(ctx->s3.ensure((size_t)sp * h));
        DV_CHECK(hipMemcpy2DAsync(ctx->s3.p, sp, src, stride, (size_t)channels * w, h, hipMemcpyHostToDevice, s));
        d_src = (const uint8_t*)ctx->s3.p;
    }
    const size_t npx = (size_t)w * h;
    DV_CHECK(ctx->s2.ensure(6 * npx));
    DV_CHECK(hipMemcpyAsync(ctx->s2.p, map1_xy, 4 * npx, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync((uint8_t*)ctx->s2.p + 4 * npx, map2, 2 * npx, hipMemcpyHostToDevice, s));
    const int dp = align_up(channels * w, 16);
    DV_CHECK(ctx->s4.ensure((size_t)dp * h));
    dv_launch_remap(d_src, nullptr, w, h, sp, channels, 0, (const int16_t*)ctx->s2.p, (const uint16_t*)((uint8_t*)ctx->s2.p + 4 * npx), nullptr, nullptr,
                    (uint8_t*)ctx->s4.p, nullptr, dp, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpy2DAsync(dst, (size_t)channels * w, ctx->s4.p, dp, (size_t)channels * w, h, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

int dv_set_undistort_maps(dv_ctx* ctx, int cam, const int16_t* map1_xy, const uint16_t* map2, int w, int h) {
    if (!ctx) return -1;
    if (cam < 0 || cam > 1) DV_FAIL("dv_set_undistort_maps: cam must be 0 or 1");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (ctx->pending) DV_FAIL("dv_set_undistort_maps: a frame is in flight");
    if (!map1_xy) {
        ctx->undist[cam] = false; if (cam == 0) ctx->undist[1] = false;
        if (ctx->cam_switched) {      // dv_undistort_setup re-parameterised the cameras for the undistorted frames: without the maps the original ones hold again
            ctx->cfg.cam1 = ctx->cam_orig[1];
            if (cam == 0) { ctx->cfg.cam0 = ctx->cam_orig[0]; ctx->cam_switched = false; }
        }
        return 0;
    }
    if (!map2 || w != ctx->cfg.width || h != ctx->cfg.height) DV_FAIL("dv_set_undistort_maps: maps must be width x height of the config");
    if (cam == 1 && !ctx->undist[0]) DV_FAIL("dv_set_undistort_maps: install camera 0 first");
    const size_t npx = (size_t)w * h;
    DV_CHECK(ctx->undist_buf[cam].ensure(6 * npx));
    DV_CHECK(hipMemcpyAsync(ctx->undist_buf[cam].p, map1_xy, 4 * npx, hipMemcpyHostToDevice, ctx->stream));
    DV_CHECK(hipMemcpyAsync((uint8_t*)ctx->undist_buf[cam].p + 4 * npx, map2, 2 * npx, hipMemcpyHostToDevice, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->undist[cam] = true; ctx->undist_w = w; ctx->undist_h = h;
    if (ctx->cam_switched) {      // the caller's own maps replace those of dv_undistort_setup: its (newK, 0) no longer describes this camera's frames — the camera the ctx was created with holds again
        if (cam == 0) ctx->cfg.cam0 = ctx->cam_orig[0]; else ctx->cfg.cam1 = ctx->cam_orig[1];
    }
    return 0;
}

int dv_pyr_down(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst) DV_FAIL("dv_pyr_down: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const uint8_t* d_src; int pitch;
    if (stage_image(ctx, ctx->s0, src, w, h, stride, mem, &d_src, &pitch)) return -1;
    const int dw = (w + 1) / 2, dh = (h + 1) / 2, dp = align_up(dw, 16);
    DV_CHECK(ctx->s1.ensure((size_t)dp * dh + 64));
    dv_launch_pyr_down2(d_src, nullptr, w, h, pitch, (uint8_t*)ctx->s1.p, nullptr, dp, nullptr, nullptr, 0, ctx->stream);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpy2DAsync(dst, dw, ctx->s1.p, dp, dw, dh, mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_circle_mask(dv_ctx* ctx, uint8_t* mask, int w, int h, int stride, const float* pts_xy, int n, int radius, int mem) {
    if (!ctx) return -1;
    if (!mask || (n > 0 && !pts_xy)) DV_FAIL("dv_circle_mask: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (dv_ensure_hw(ctx, radius)) return -1;
    uint8_t* d_mask = mask; int pitch = stride;
    if (mem != DV_MEM_DEVICE) {
        pitch = align_up(w, 16);
        DV_CHECK(ctx->s0.ensure((size_t)pitch * h));
        DV_CHECK(hipMemcpy2DAsync(ctx->s0.p, pitch, mask, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
        d_mask = (uint8_t*)ctx->s0.p;
    }
    if (stage_in(ctx, ctx->s1, pts_xy, (size_t)n * 8, mem)) return -1;
    dv_launch_circle_mask(d_mask, w, h, pitch, (const float2*)ctx->s1.p, n, radius, (const uint8_t*)ctx->hw_buf.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (mem != DV_MEM_DEVICE) DV_CHECK(hipMemcpy2DAsync(mask, stride, d_mask, pitch, w, h, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_erode(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, int k, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst || k < 1) DV_FAIL("dv_erode: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const uint8_t* d_src; int pitch;
    if (stage_image(ctx, ctx->s0, src, w, h, stride, mem, &d_src, &pitch)) return -1;
    const int p = align_up(w, 16);
    DV_CHECK(ctx->s1.ensure((size_t)p * h)); DV_CHECK(ctx->s2.ensure((size_t)p * h));
    dv_launch_erode(d_src, w, h, pitch, k, (uint8_t*)ctx->s1.p, p, (uint8_t*)ctx->s2.p, p, ctx->stream);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpy2DAsync(dst, mem == DV_MEM_DEVICE ? stride : w, ctx->s2.p, p, w, h,
                              mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_lift_projective(dv_ctx* ctx, const dv_cam* cam, const float* pts_xy, int n, float* out_xy, int mem) {
    return dv_lift_projective_offset(ctx, cam, pts_xy, n, 0.0, 0.0, out_xy, mem);
}

int dv_lift_projective_offset(dv_ctx* ctx, const dv_cam* cam, const float* pts_xy, int n, double off_x, double off_y, float* out_xy, int mem) {
    if (!ctx) return -1;
    if (!cam || (n > 0 && (!pts_xy || !out_xy))) DV_FAIL("dv_lift_projective: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (stage_in(ctx, ctx->s0, pts_xy, (size_t)n * 8, mem)) return -1;
    DV_CHECK(ctx->s1.ensure((size_t)std::max(n, 1) * 8));
    dv_launch_lift(*cam, (const float2*)ctx->s0.p, n, off_x, off_y, (float2*)ctx->s1.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (stage_out(ctx, out_xy, ctx->s1.p, (size_t)n * 8, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// FrameLines::UndistortedLineEndPoints (line_detector, front end of TrackImageLine): both end points through PinholeCamera::liftProjective; the Line keeps
// them as cv::Point2f, LineFeature widens to double (basic/line_feature.h:31-33)
int dv_undistort_lines(dv_ctx* ctx, const dv_cam* cam, const float* lines_xyxy, int n, double* out_xyxy) {
    if (!ctx) return -1;
    if (!cam || n < 0 || (n > 0 && (!lines_xyxy || !out_xyxy))) DV_FAIL("dv_undistort_lines: bad argument");
    if (n == 0) return 0;
    std::vector<float> un((size_t)4 * n);
    if (dv_lift_projective(ctx, cam, lines_xyxy, 2 * n, un.data(), DV_MEM_HOST)) return -1;
    for (size_t i = 0; i < (size_t)4 * n; ++i) out_xyxy[i] = (double)un[i];
    return 0;
}

} // extern "C"
