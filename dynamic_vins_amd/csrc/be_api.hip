// be_api.hip — host side of the bundle-adjustment entry points of include/dvins.h: uploads the flat problem
// tables, enqueues the fixed kernel schedule of the trust-region loop on the ctx's BA stream (no host round trip
// between iterations: every kernel is predicated on the device-resident BeCtl) and downloads the solved states.
#include <algorithm>
#include "be_host.h"
#include "est_window.h"

static_assert(sizeof(dv_ba_factor) == sizeof(BeFactor), "public/private factor layouts must match");
static_assert(sizeof(dv_ba_lm) == sizeof(BeLm), "public/private landmark layouts must match");
static_assert(sizeof(dv_ba_prior) == sizeof(BePriorHdr), "public/private prior layouts must match");

int be_ensure(dv_ctx* ctx, int nfac) {
    BeWork& w = ctx->be;
    if (w.ready && nfac <= w.fac_cap) return 0;
    const int fac_cap = std::max(nfac, BE_MAX_LM * BE_MAX_OBS_FACTORS);      // the worst case up front: a re-allocation would drop the device-resident prior
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t n = BE_MAX_STATE;
    // upload region first (mirrored 1:1 by the pinned staging buffer -> ONE H2D copy per solve), factors last (variable length)
    size_t o_ctl = take(sizeof(BeCtl)), o_x = take(sizeof(BeState)), o_imu = take(sizeof(BeImu) * BE_WIN), o_pr = take(sizeof(BePriorHdr)), o_i = take(4 * 4 * n),
           o_mt = take(4 * BE_MARG_TAB_INTS), o_lm = take(sizeof(BeLm) * BE_MAX_LM), o_fac = take(sizeof(BeFactor) * (size_t)fac_cap);
    const size_t upload_bytes = off;
    size_t o_c = take(sizeof(BeState)),
           o_pA = take(8 * (size_t)BE_MAX_PRIOR * BE_MAX_PRIOR), o_pb = take(8 * BE_MAX_PRIOR),
           o_pA2 = take(8 * (size_t)BE_MAX_PRIOR * BE_MAX_PRIOR), o_pb2 = take(8 * BE_MAX_PRIOR), o_ms = take(64), o_c0 = take(64),
           o_pk = take(8 * (size_t)BE_PK_SIZE * BE_PK_STRIDE), o_io = take(8 * (size_t)BE_WIN * IMU_OUT_STRIDE), o_po = take(8 * (BE_MAX_PRIOR + 1)),
           o_cc = take(8 * (BE_MAX_LM + BE_WIN + 1)), o_ob = take(4 * BE_MAX_LM), o_hd = take(8 * n * n), o_sc = take(8 * n * n), o_g = take(8 * 2 * n),
           o_pk1 = take(8 * (size_t)BE_PK_SIZE * BE_PK_STRIDE), o_io1 = take(8 * (size_t)BE_WIN * IMU_OUT_STRIDE), o_po1 = take(8 * (BE_MAX_PRIOR + 1)),
           o_hd1 = take(8 * n * n), o_sc1 = take(8 * n * n), o_g1 = take(8 * 2 * n),      // second linearisation set (speculative evaluation at the candidate)
           o_v = take(8 * 4 * n), o_vl = take(8 * 4 * (size_t)BE_MAX_LM);
    DV_CHECK(w.block.ensure(off));
    uint8_t* b = (uint8_t*)w.block.p;
    w.ctl = (BeCtl*)(b + o_ctl); w.x = (BeState*)(b + o_x); w.cand = (BeState*)(b + o_c); w.fac = (BeFactor*)(b + o_fac); w.lm = (BeLm*)(b + o_lm);
    w.imu = (BeImu*)(b + o_imu); w.prior = (BePriorHdr*)(b + o_pr);
    w.priorA_buf[0] = (double*)(b + o_pA); w.priorb_buf[0] = (double*)(b + o_pb); w.priorA_buf[1] = (double*)(b + o_pA2); w.priorb_buf[1] = (double*)(b + o_pb2);
    w.prior_cur = 0; w.priorA = w.priorA_buf[0]; w.priorb = w.priorb_buf[0]; w.prior_resident = false;
    w.marg_tab = (int32_t*)(b + o_mt); w.marg_scal = (double*)(b + o_ms); w.prior_c0 = (double*)(b + o_c0);
    w.packets[0] = (double*)(b + o_pk); w.imu_out[0] = (double*)(b + o_io); w.prior_out[0] = (double*)(b + o_po); w.cand_cost = (double*)(b + o_cc); w.lm_obs = (int32_t*)(b + o_ob);
    w.Hd[0] = (double*)(b + o_hd); w.Sc[0] = (double*)(b + o_sc); w.gvec[0] = (double*)(b + o_g);
    w.packets[1] = (double*)(b + o_pk1); w.imu_out[1] = (double*)(b + o_io1); w.prior_out[1] = (double*)(b + o_po1);
    w.Hd[1] = (double*)(b + o_hd1); w.Sc[1] = (double*)(b + o_sc1); w.gvec[1] = (double*)(b + o_g1);
    double* v = (double*)(b + o_v); w.scale_p = v; w.diag_p = v + n; w.grad_p = v + 2 * n; w.gn_p = v + 3 * n;
    double* vl = (double*)(b + o_vl); w.scale_l = vl; w.diag_l = vl + BE_MAX_LM; w.grad_l = vl + 2 * BE_MAX_LM; w.gn_l = vl + 3 * BE_MAX_LM;
    int32_t* iv = (int32_t*)(b + o_i); w.prior_col = iv; w.col_kind = iv + n; w.col_frame = iv + 2 * n; w.col_comp = iv + 3 * n;
    w.fac_cap = fac_cap;
    w.up_ctl = o_ctl; w.up_x = o_x; w.up_imu = o_imu; w.up_prior = o_pr; w.up_idx = o_i; w.up_mt = o_mt; w.up_lm = o_lm; w.up_fac = o_fac;
    const size_t need = upload_bytes + sizeof(BeState) + sizeof(BeCtl) + BE_DOWNLOAD_SLACK;        // staging mirror + download area (BeDownload, be_host.h)
    if (w.pinned_bytes < need) {
        if (w.pinned) (void)hipHostFree(w.pinned);
        w.pinned = nullptr;
        DV_CHECK(hipHostMalloc(&w.pinned, need, hipHostMallocDefault));
        w.pinned_bytes = need;
    }
    w.dl_off = upload_bytes;
    if (!w.ev_state) DV_CHECK(hipEventCreateWithFlags(&w.ev_state, hipEventDisableTiming));
    if (const char* e = std::getenv("DVINS_GPU_REJECT")) w.gpu_reject = std::atoi(e) != 0;
    w.ready = true;
    return 0;
}

// Everything the first frames of an estimator would otherwise create in the middle of the sequence: the work block and its pinned mirror (hipMalloc / hipHostMalloc),
// the marginalization scratch, events, the pinned flag arrays, the kernels' code objects and LDS attributes — together a
// 3 ms frame at the first window solve (scripts/dyn_cold_frames.py), where a 20 Hz estimator has 1 ms frames otherwise.  Called by dv_est_create.
int be_prepare(dv_ctx* ctx, bool dynamic) {
    BeWork& w = ctx->be;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (be_ensure(ctx, 0)) return -1;
    {       // marg_args' sizing at its maximum (BE_MAX_LM landmarks anchored in the oldest frame, D = 178)
        const size_t nlmax = (size_t)BE_MAX_LM, Dmax = 178;
        DV_CHECK(w.marg_buf.ensure(8 * (nlmax * (size_t)be_marg_wstride((int)Dmax) + ((size_t)be_marg_chunks((int)nlmax) + 1) * be_marg_part() + Dmax * Dmax + Dmax + nlmax + 512)));
    }
    if (!w.rej_pinned) DV_CHECK(hipHostMalloc((void**)&w.rej_pinned, BE_MAX_LM, hipHostMallocDefault));
    if (be_eval_prepare() || be_solve_prepare() || be_marg_prepare() || dv_copy_prepare()) DV_FAIL("be_prepare: cannot load the back end's kernels");
    if (dynamic && be_obj_solve_prepare(ctx, ctx->obj_buf, ctx->obj_pend)) return -1;
    // the scratch memory of the queues the back end launches on (see dv_warm_stream), then everything above has happened before the first frame
    if (dv_warm_stream(ctx->be_stream) || (dynamic && ctx->obj_stream && dv_warm_stream(ctx->obj_stream))) DV_FAIL("be_prepare: warm-up launch failed");
    DV_CHECK(hipStreamSynchronize(ctx->be_stream));
    if (dynamic && ctx->obj_stream) DV_CHECK(hipStreamSynchronize(ctx->obj_stream));
    return 0;
}

int be_fill_imu(const dv_ba_imu& in, BeImu& o, const double* sqrt_hint) {
    o.sum_dt = in.sum_dt;
    for (int k = 0; k < 3; ++k) { o.dp[k] = in.dp[k]; o.dv[k] = in.dv[k]; o.lin_ba[k] = in.lin_ba[k]; o.lin_bg[k] = in.lin_bg[k]; }
    for (int k = 0; k < 4; ++k) o.dq[k] = in.dq[k];
    auto blk = [&](int r0, int c0, double* dst) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) dst[i * 3 + j] = in.jacobian[(r0 + i) * 15 + c0 + j]; };
    blk(0, 9, o.dp_dba); blk(0, 12, o.dp_dbg); blk(3, 12, o.dq_dbg); blk(6, 9, o.dv_dba); blk(6, 12, o.dv_dbg);
    o.fi = in.fi; o.fj = in.fj; o.pad0 = o.pad1 = 0;
    if (sqrt_hint) { std::memcpy(o.sqrt_info, sqrt_hint, sizeof(o.sqrt_info)); return 0; }
    return estw::imu_sqrt_info(in.covariance, o.sqrt_info) ? 0 : -1;
}
bool be_imu_sqrt_info(const double* cov, double* U) { return estw::imu_sqrt_info(cov, U); }      // (est_window.h, beside the pre-integration that owns the covariance)

// The stages of one window's slots for be_run_slots (be_host.h): the member's arguments by value, the _ext launches of the free extrinsic / td blocks behind
// evaluation and reduce, and per-launch events when kernel_timing is on.
struct BeWindowStages {
    dv_ctx* ctx; BePending& pd; hipStream_t s;
    const bool kt = ctx->timing && ctx->kernel_timing;       // per-launch events (roofline measurement); off in the throughput run
    // sharded window (be_shard.hip): every reduce is followed by the exchange of the partial systems and their rank-ordered sum, every cost-only
    // evaluation by the exchange of the candidate costs.  The exchanges are enqueued unconditionally (all ranks hold identical control blocks).
    const bool sharded = pd.sa.sh.on != 0;
    void eval(int mode) {
        if (kt) { StageScope k(ctx, mode == BE_EVAL_CAND_COST ? "k_be_eval_cost" : "k_be_eval_full", s); be_launch_eval(pd.ea, mode, s); }
        else be_launch_eval(pd.ea, mode, s);
        be_launch_eval_ext(pd.ea, pd.xt, mode, s);      // (free extrinsic / td blocks only)
    }
    void reduce(int spec) {
        if (kt) { StageScope k(ctx, "k_be_reduce", s); be_launch_reduce(pd.sa, spec, s); }
        else be_launch_reduce(pd.sa, spec, s);
        be_launch_reduce_ext(pd.sa, spec, s);
    }
    int solve(int spec) {
        int rc;
        if (kt) { StageScope k(ctx, "k_be_solve", s); rc = be_launch_solve(pd.sa, spec, s); }
        else rc = be_launch_solve(pd.sa, spec, s);
        if (rc) DV_FAIL("dv_ba_solve: cannot set dynamic LDS size");
        return 0;
    }
    void accept(bool final_slot) {
        if (pd.fuse_accept_gauge && !kt && final_slot) return;      // (fused: be_enqueue_tail launches accept + gauge as one kernel)
        if (kt) { StageScope k(ctx, "k_be_accept", s); be_launch_accept(pd.sa, s); }
        else be_launch_accept(pd.sa, s);
    }
    void after(int it, int kind) { be_dbg_stage(ctx, it, kind, s); }
    int exchange_system(int spec) {
        if (!sharded) return 0;
        if (kt) { StageScope k(ctx, "k_be_exchange", s); if (be_exchange(ctx, (size_t)pd.sa.sh.len, s)) return -1; }
        else if (be_exchange(ctx, (size_t)pd.sa.sh.len, s)) return -1;
        if (kt) { StageScope k(ctx, "k_be_shard_finalize", s); be_launch_shard_finalize(pd.sa, spec, s); }
        else be_launch_shard_finalize(pd.sa, spec, s);
        return 0;
    }
    int exchange_cost() {
        if (!sharded) return 0;
        be_launch_shard_cost(pd.sa, 0, s);
        if (be_exchange(ctx, 8, s)) return -1;          // one partial sum per rank (padded to 64 bytes)
        be_launch_shard_cost(pd.sa, 1, s);
        return 0;
    }
    // every rank has moved its own landmarks only: one gather of the inverse depths of x behind the pass's last accept decision (whatever reads the whole state —
    // the gauge kernel's download, the outlier test, the marginalization, a spare-slot pass — comes behind it on the stream)
    int gather_depth() {
        if (!sharded) return 0;
        be_launch_shard_depth(pd.sa, 0, s);
        if (be_exchange(ctx, (size_t)pd.sa.sh.cap, s)) return -1;
        be_launch_shard_depth(pd.sa, 1, s);
        return 0;
    }
};
int be_enqueue_slots(dv_ctx* ctx, BePending& pd, int slots, bool speculative, hipStream_t s) {
    BeWindowStages st{ ctx, pd, s };
    return be_run_slots(st, slots, speculative);
}

// the gauge kernel's arguments of an estimator solve: it writes the gauge-fixed copy, the control block and (dynamic mode: body.para_pose as ceres leaves it, before
// Double2vector's gauge fix) the raw poses straight into the pinned buffer
void be_gauge_args(dv_ctx* ctx, const BePending& pd, BeGaugeArgs& ga) {
    BeWork& w = ctx->be;
    BeDownload* dl = be_download(w);
    ga = BeGaugeArgs{};
    ga.x = w.x; ga.out = w.cand; ga.nlm = pd.nlm; ga.nframes = pd.nframes; ga.use_imu = pd.use_imu;
    std::memcpy(ga.R0, pd.gauge_R0, sizeof(ga.R0)); std::memcpy(ga.ypr0, pd.gauge_ypr0, sizeof(ga.ypr0)); std::memcpy(ga.P0, pd.gauge_P0, sizeof(ga.P0));
    ga.h_out = &dl->x; ga.h_ctl = &dl->ctl; ga.ctl = w.ctl; ga.state_doubles = (int)((pd.state_bytes + 7) / 8);
    ga.h_raw_pose = pd.want_raw_pose ? dl->raw_pose : nullptr;
}
// gauge fix + download of the states (event) + marginalization, enqueued behind the slots on the same stream: the host
// waits only for the event, so the marginalization of frame k overlaps the host's turnaround and the upload of frame k+1;
// whatever reads its result (the next solve) is ordered behind it on the stream.
int be_enqueue_tail(dv_ctx* ctx, BePending& pd, hipStream_t s) {
    BeWork& w = ctx->be;
    BeDownload* dl = be_download(w);
    pd.ev_state_ext = nullptr;                                  // (a tail of its own: the host waits for w.ev_state again)
    BeGaugeArgs ga{};
    if (pd.fused_present) {        // estimator path
        be_gauge_args(ctx, pd, ga);
        const bool kt = ctx->timing && ctx->kernel_timing;
        if (pd.fuse_accept_gauge && !kt) be_launch_accept_gauge(pd.sa, ga, s); else be_launch_gauge(ga, s);
        DV_CHECK(hipGetLastError());
    } else {
        DV_CHECK(hipMemcpyAsync(&dl->x, w.x, pd.state_bytes, hipMemcpyDeviceToHost, s));
        DV_CHECK(hipMemcpyAsync(&dl->ctl, w.ctl, sizeof(BeCtl), hipMemcpyDeviceToHost, s));
    }
    if (pd.rej_on) { be_launch_reject(pd.rej, s); DV_CHECK(hipGetLastError()); }      // reads the gauge-fixed copy (w.cand), writes its flags to pinned memory: part of what ev_state covers
    DV_CHECK(hipEventRecord(w.ev_state, s));
    if (pd.fused_present && pd.do_marg && !pd.pl.empty) {
        if (marg_enqueue(ctx, pd.pl, w.cand, pd.g_norm, w.priorA, w.priorb, w.priorA_buf[pd.nxt], w.priorb_buf[pd.nxt], w.marg_scal, w.prior_c0 + pd.nxt, s)) return -1;
        DV_CHECK(dv_copy_async(dl->marg_scal[pd.scal_slot], w.marg_scal, 32, s));      // two alternating host slots
        pd.marg_in_flight = true;
    }
    return 0;
}


static int be_begin_impl(dv_ctx* ctx, dv_ba_problem* P, BeFused* fused, bool eval_only) {
    if (!ctx) return -1;
    BePending& pd = *ctx->be.pend;
    if (pd.active) DV_FAIL("dv_ba_solve: previous solve not collected");
    pd.trivial = false;
    const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
    if (!P || !P->pose || !P->ex_pose || !P->td) DV_FAIL("dv_ba_solve: null argument");
    if (P->nframes < 1 || P->nframes > BE_NF) DV_FAIL("dv_ba_solve: nframes out of range");
    if (P->nlm < 0 || P->nlm > BE_MAX_LM) DV_FAIL("dv_ba_solve: more than kNumFeat=1000 landmarks");
    if (P->nimu < 0 || P->nimu > BE_WIN) DV_FAIL("dv_ba_solve: bad IMU factor count");
    if (P->use_imu && !P->speed_bias) DV_FAIL("dv_ba_solve: speed_bias is null");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (be_ensure(ctx, P->nfac)) return -1;
    BeWork& w = ctx->be;
    hipStream_t s = ctx->be_stream;
    // ---- the bulk of the upload FIRST: landmark and factor tables (nine tenths of the bytes) are complete when the call begins (the estimator builds the factors in the pinned
    // mirror itself), so their staging copy — 15 of the 19 us the whole upload takes over PCIe, on the path between two frames' solves — runs while the host still works out the
    // column layout, the IMU records and the marginalization plan below; the head of the region (control block, states, IMU, prior header, index tables) follows at the end.
    // Measured (profiles/r06_experiments/upload_split_ab.json, 100-step blocks interleaved on one box): +0.1 - 0.7 %, i.e. noise level — the BA stream is still busy with the
    // previous frame's marginalization when the early copy arrives; kept because it cannot lose ----
    static const bool split_upload = [] { const char* e = std::getenv("DVINS_UPLOAD_SPLIT"); return !(e && e[0] == '0'); }();      // 0: one copy at the end (rounds 1 - 5; A/B)
    {
        uint8_t* hp0 = (uint8_t*)w.pinned;
        if (P->nlm) std::memcpy(hp0 + w.up_lm, P->landmarks, sizeof(BeLm) * (size_t)P->nlm);
        if (P->nfac && (const void*)P->factors != (const void*)(hp0 + w.up_fac)) std::memcpy(hp0 + w.up_fac, P->factors, sizeof(BeFactor) * (size_t)P->nfac);      // the estimator builds the table in place
        if (split_upload) DV_CHECK(dv_copy_async((uint8_t*)w.block.p + w.up_lm, hp0 + w.up_lm, (w.up_fac - w.up_lm) + sizeof(BeFactor) * (size_t)P->nfac, s));
    }
    // ---- column layout of the reduced system ----
    BeDims d{};
    d.nframes = P->nframes; d.nlm = P->nlm; d.nfac = P->nfac; d.nimu = P->nimu; d.use_imu = P->use_imu; d.plane_kind = P->plane_kind;
    std::vector<int32_t> idx(4 * BE_MAX_STATE, -1);
    int32_t* prior_col = idx.data(); int32_t* col_kind = prior_col + BE_MAX_STATE; int32_t* col_frame = col_kind + BE_MAX_STATE; int32_t* col_comp = col_frame + BE_MAX_STATE;
    int col = 0;
    for (int f = 0; f < BE_NF; ++f) { d.pose_col[f] = -1; d.sb_col[f] = -1; }
    for (int f = 0; f < P->nframes; ++f) {
        const bool pose_const = !P->use_imu && f == 0;              // estimator.cpp:83-84
        if (!pose_const) { d.pose_col[f] = col; for (int k = 0; k < 6; ++k) { col_kind[col] = 0; col_frame[col] = f; col_comp[col] = k; ++col; } }
        if (P->use_imu) { d.sb_col[f] = col; for (int k = 0; k < 9; ++k) { col_kind[col] = 1; col_frame[col] = f; col_comp[col] = k; ++col; } }
    }
    // free extrinsic / td blocks (estimator.cpp:87-100; dv_ba_problem::free_blocks): their columns follow the frames' (ceres' reduced program keeps the insertion order of
    // AddBodyParameterBlock: poses and speed-biases, the extrinsics, td); ext entry q = 0..5 ex0, 6..11 ex1, 12 td
    BeExt xt{};
    for (int q = 0; q <= BE_NX; ++q) xt.xcol[q] = -1;
    if (P->free_blocks & ~3) DV_FAIL("dv_ba_solve: unknown bits in free_blocks");
    if (P->free_blocks & 1) for (int cidx = 0; cidx < 2; ++cidx) for (int k = 0; k < 6; ++k) { xt.xcol[6 * cidx + k] = col; col_kind[col] = 2; col_frame[col] = 100 + cidx; col_comp[col] = k; ++col; }
    if (P->free_blocks & 2) { xt.xcol[12] = col; col_kind[col] = 3; col_frame[col] = 102; col_comp[col] = 0; ++col; }
    xt.on = (P->free_blocks & 3) ? 1 : 0;
    d.nstate = col;
    d.pad = 0;
    const bool has_prior = P->prior && P->prior->valid;
    const bool prior_on_device = has_prior && w.prior_resident && P->prior_A == w.priorA_buf[w.prior_cur];
    if (col == 0) {       // e.g. vision-only, first frame: pose 0 is constant and no landmark has 4 observations yet
        if (P->nlm > 0) DV_FAIL("dv_ba_solve: landmarks without a free pose block");
        if (fused && fused->marg_mode >= 0) DV_FAIL("dv_ba_solve: marginalization needs a full window");
        pd.active = true; pd.trivial = true;
        return 0;
    }
    BePriorHdr ph{};
    if (has_prior) {
        std::memcpy(&ph, P->prior, sizeof(ph));
        if (ph.n > BE_MAX_PRIOR || ph.nblocks > 16) DV_FAIL("dv_ba_solve: prior too large");
        for (int b = 0; b < ph.nblocks; ++b) {
            const BePriorBlock pb = ph.blocks[b];
            int c0 = -1;
            if (pb.type == 0) c0 = d.pose_col[pb.idx]; else if (pb.type == 1) c0 = d.sb_col[pb.idx];
            else if (pb.type == 2) c0 = xt.xcol[6 * pb.idx]; else if (pb.type == 3) c0 = xt.xcol[12];
            if (c0 >= 0) for (int k = 0; k < pb.size_local; ++k) prior_col[c0 + k] = pb.off + k;
        }
    }
    // ---- marginalization structure (does not depend on the solution): planned now so that its tables ride in the same upload ----
    MargPlan& pl = pd.pl;
    const bool do_marg = fused && fused->marg_mode >= 0;
    if (do_marg) {
        if (P->nframes != BE_NF) DV_FAIL("dv_marginalize: needs a full window (frame == kWinSize)");
        std::vector<int> sel;
        if (fused->marg_mode == 0) for (int l = 0; l < P->nlm; ++l) if (P->landmarks[l].anchor == 0) sel.push_back(l);
        const bool imu01 = P->nimu > 0 && P->imu[0].fi == 0 && P->imu[0].fj == 1;
        if (marg_plan(ctx, pl, fused->marg_mode, has_prior ? P->prior : nullptr, P->factors, P->landmarks, sel.data(), (int)sel.size(), imu01)) return -1;
    }
    // ---- upload: everything is staged in the pinned mirror of the device's upload region and travels in ONE copy ----
    uint8_t* hp = (uint8_t*)w.pinned;
    be_stage_state((BeState*)(hp + w.up_x), P, P->nlm);
    const size_t state_bytes = offsetof(BeState, inv_depth) + 8 * (size_t)P->nlm;
    BeCtl* hctl = (BeCtl*)(hp + w.up_ctl);
    std::memset(hctl, 0, sizeof(BeCtl));
    hctl->need_eval = 1; hctl->first = 1; hctl->max_iters = P->max_iters; hctl->radius = 1e4; hctl->mu = eval_only ? 0.0 : 1e-8; hctl->step_valid = 0;
    BeImu* himu = (BeImu*)(hp + w.up_imu);
    for (int k = 0; k < P->nimu; ++k) {
        const double* hint = (k < (int)w.sqrt_hint.size()) ? w.sqrt_hint[k] : nullptr;      // the estimator caches U per pre-integration (Q8)
        if (be_fill_imu(P->imu[k], himu[k], hint)) DV_FAIL("dv_ba_solve: IMU covariance is singular");
    }
    std::memcpy(hp + w.up_prior, &ph, sizeof(ph));
    std::memcpy(hp + w.up_idx, idx.data(), 4 * idx.size());
    if (do_marg && !pl.empty) std::memcpy(hp + w.up_mt, pl.tab, sizeof(pl.tab));
    DV_CHECK(dv_copy_async(w.block.p, hp, split_upload ? w.up_lm : w.up_fac + sizeof(BeFactor) * (size_t)P->nfac, s));      // the head of the upload region (the landmark / factor tables went first, see the top); kernels reading the pinned mirror: copy.hip
    if (has_prior && !prior_on_device) {               // a prior handed over in host memory (the estimator's stays in HBM)
        if (!P->prior_A || !P->prior_b) DV_FAIL("dv_ba_solve: prior without A / b");
        DV_CHECK(hipMemcpyAsync(w.priorA_buf[w.prior_cur], P->prior_A, 8 * (size_t)ph.n * ph.n, hipMemcpyHostToDevice, s));
        DV_CHECK(hipMemcpyAsync(w.priorb_buf[w.prior_cur], P->prior_b, 8 * (size_t)ph.n, hipMemcpyHostToDevice, s));
        double* hc0 = &be_download(w)->c0; *hc0 = ph.c0;
        DV_CHECK(hipMemcpyAsync(w.prior_c0 + w.prior_cur, hc0, 8, hipMemcpyHostToDevice, s));
        w.prior_resident = false;
    }
    w.priorA = w.priorA_buf[w.prior_cur]; w.priorb = w.priorb_buf[w.prior_cur];
    std::chrono::steady_clock::time_point t_up = std::chrono::steady_clock::now();
    // ---- schedule ----
    BeEvalArgs ea{};
    ea.ctl = w.ctl; ea.x = w.x; ea.cand = w.cand; ea.fac = w.fac; ea.lm = w.lm; ea.imu = w.imu; ea.prior = w.prior; ea.priorA = w.priorA; ea.priorb = w.priorb;
    ea.dims = d; ea.g_norm = P->g_norm; ea.cand_cost = w.cand_cost; ea.lm_obs = w.lm_obs; ea.prior_c0 = w.prior_c0 + w.prior_cur;
    ea.lm_lo = 0; ea.lm_hi = P->nlm;
    if (P->free_blocks & 3) {
        if (ctx->dist.transport != 0) DV_FAIL("dv_ba_solve: free extrinsic / td blocks are not built for the landmark-sharded window");
        if (xt.on) {
            DV_CHECK(w.xpk_buf.ensure(2 * 8 * (size_t)BX_SIZE * BE_PK_STRIDE));
            xt.xpk[0] = (double*)w.xpk_buf.p; xt.xpk[1] = xt.xpk[0] + (size_t)BX_SIZE * BE_PK_STRIDE;
        }
    }
    BeShard sh{};
    if (ctx->dist.transport != 0) {        // landmark-sharded window: contiguous ranges of cap = ceil(nlm / world) landmarks
        const DvDist& dd = ctx->dist;
        sh.on = 1; sh.rank = dd.rank; sh.world = dd.world;
        sh.cap = std::max(1, (P->nlm + dd.world - 1) / dd.world);
        sh.lo = std::min(P->nlm, dd.rank * sh.cap); sh.hi = std::min(P->nlm, sh.lo + sh.cap);
        sh.len = BE_XS_LEN;
        sh.xsend = (double*)dd.xsend.p; sh.xrecv = (const double*)dd.xrecv.p;
        sh.qf[0] = (double*)dd.qf.p; sh.qf[1] = sh.qf[0] + BE_QF_LEN;
        ea.lm_lo = sh.lo; ea.lm_hi = sh.hi;
    }
    for (int k = 0; k < 2; ++k) { ea.packets[k] = w.packets[k]; ea.imu_out[k] = w.imu_out[k]; ea.prior_out[k] = w.prior_out[k]; }
    BeSolveArgs sa{};
    sa.ctl = w.ctl; sa.x = w.x; sa.cand = w.cand; sa.lm = w.lm; sa.imu = w.imu; sa.prior = w.prior; sa.priorA = w.priorA; sa.dims = d;
    sa.cand_cost = w.cand_cost; sa.lm_obs = w.lm_obs;
    for (int k = 0; k < 2; ++k) { sa.packets[k] = w.packets[k]; sa.imu_out[k] = w.imu_out[k]; sa.prior_out[k] = w.prior_out[k]; sa.Hd[k] = w.Hd[k]; sa.Sc[k] = w.Sc[k]; sa.gvec[k] = w.gvec[k]; }
    sa.scale_p = w.scale_p; sa.diag_p = w.diag_p; sa.grad_p = w.grad_p; sa.gn_p = w.gn_p; sa.scale_l = w.scale_l; sa.diag_l = w.diag_l; sa.grad_l = w.grad_l; sa.gn_l = w.gn_l;
    sa.prior_col = w.prior_col; sa.col_kind = w.col_kind; sa.col_frame = w.col_frame; sa.col_comp = w.col_comp;
    sa.xnorm2_extra = P->x_norm2_extra; sa.sh = sh; sa.xt = xt;
    // the 16-wide MFMA factorisation (be_solve.hip MF16) wherever the system fits its tile budget (n <= 175: every window the estimator builds); "ldl_generic" selects the 4-wide panel form
    sa.ldl_mf16 = 0;
    if (!w.ldl_generic && !(P->free_blocks & 3)) {      // (free extrinsic / td blocks: the generic form carries the ext entries)
        uint8_t plan[64];
        if (be_mf16_plan(d.nstate, plan)) { std::memcpy(sa.ldl_col0, plan, sizeof(plan)); sa.ldl_mf16 = w.ldl_barriers ? 2 : 1; }
    }
    // The first pass enqueues exactly max_iters slots: enough unless a linear solve failed (mu *= 10 retry) or a step was
    // invalid; be_solve_fused_end checks the downloaded control block and, in that rare case, runs the spare slots and the
    // (idempotent) tail again.
    pd.rej_on = false;
    if (fused && fused->want_reject && w.gpu_reject && P->nlm > 0) {
        if (!w.rej_pinned) DV_CHECK(hipHostMalloc((void**)&w.rej_pinned, BE_MAX_LM, hipHostMallocDefault));
        BeRejectArgs& r = pd.rej;
        r.st = w.cand; r.fac = w.fac; r.lm = w.lm; r.nlm = P->nlm; r.nframes = P->nframes; r.focal = fused->rej_focal; r.flags = w.rej_pinned;
        std::memcpy(r.ric, fused->rej_ric, sizeof(r.ric)); std::memcpy(r.tic, fused->rej_tic, sizeof(r.tic));
        r.ex_from_state = (P->free_blocks & 1) ? 1 : 0; r.pad = 0;
        pd.rej_on = true;
    }
    pd.xt = xt; pd.copy_ex_td = (P->free_blocks & 3) != 0;
    pd.ea = ea; pd.sa = sa; pd.fused_present = fused != nullptr; pd.fuse_accept_gauge = fused != nullptr && !ctx->batch && !sh.on /* sharded: the last accept decision must stand before the gather of the inverse depths */; pd.max_iters = P->max_iters; pd.g_norm = P->g_norm; pd.nframes = P->nframes; pd.use_imu = P->use_imu; pd.nlm = P->nlm;
    pd.want_raw_pose = fused && fused->want_raw_pose;
    if (fused) { std::memcpy(pd.gauge_R0, fused->R0, sizeof(pd.gauge_R0)); std::memcpy(pd.gauge_ypr0, fused->ypr0, sizeof(pd.gauge_ypr0)); std::memcpy(pd.gauge_P0, fused->P0, sizeof(pd.gauge_P0)); }
    pd.do_marg = do_marg; pd.state_bytes = state_bytes; pd.nxt = 1 - w.prior_cur;
    if (eval_only) {        // dv_ba_eval: one evaluation + assembly of the reduced camera system at the given states (mu = 0)
        be_launch_eval(ea, BE_EVAL_X, s); be_launch_eval_ext(ea, xt, BE_EVAL_X, s);
        be_launch_reduce(sa, 0, s); be_launch_reduce_ext(sa, 0, s);
        if (sh.on) { if (be_exchange(ctx, (size_t)sh.len, s)) return -1; be_launch_shard_finalize(sa, 0, s); }
        DV_CHECK(hipGetLastError());
        return 0;
    }
    if (w.debug_hash_log && fused) {        // what the device holds when the round starts: the uploaded block as it arrived, the prior it will read
        if (!w.dbg_pinned) DV_CHECK(hipHostMalloc((void**)&w.dbg_pinned, 64, hipHostMallocDefault));
        const size_t up_bytes = w.up_fac + sizeof(BeFactor) * (size_t)P->nfac;
        be_dbg_hash(w.block.p, up_bytes & ~(size_t)7, w.dbg_pinned + 0, s);
        const bool pv = P->prior && P->prior->valid;
        if (pv) { be_dbg_hash(w.priorA, 8 * (size_t)P->prior->n * P->prior->n, w.dbg_pinned + 1, s); be_dbg_hash(w.priorb, 8 * (size_t)P->prior->n, w.dbg_pinned + 2, s); } else { w.dbg_pinned[1] = 0; w.dbg_pinned[2] = 0; }
    }
    const int first_slots = w.debug_short_first_pass ? std::max(1, P->max_iters - 2) : P->max_iters;      // dv_debug_set(ctx, "short_first_pass", 1): tests exercise the spare-slot path
    if (ctx->batch && fused && !sh.on) {       // member of a dv_batch: the upload is on its way; dv_batch_enqueue launches the slots of all members together
        pd.deferred = true; pd.first_slots = first_slots;
        pd.active = true; pd.t_begin = t_begin; pd.t_up = t_up; pd.t_enq = t_up;
        return 0;
    }
    { StageScope sc(ctx, "ba_solve", s); if (be_enqueue_slots(ctx, pd, first_slots, true, s)) return -1; }
    std::chrono::steady_clock::time_point t_enq = std::chrono::steady_clock::now();
    if (be_enqueue_tail(ctx, pd, s)) return -1;
    pd.active = true; pd.t_begin = t_begin; pd.t_up = t_up; pd.t_enq = t_enq;
    return 0;
}

void* be_staging_factors(dv_ctx* ctx, int* cap) {
    if (!ctx || ctx->be.pend->active) return nullptr;
    if (hipSetDevice(ctx->cfg.device) != hipSuccess || be_ensure(ctx, 0)) return nullptr;
    *cap = ctx->be.fac_cap;
    return (uint8_t*)ctx->be.pinned + ctx->be.up_fac;
}

int be_solve_fused_begin(dv_ctx* ctx, dv_ba_problem* P, BeFused* fused) { return be_begin_impl(ctx, P, fused, false); }

int be_solve_fused_end(dv_ctx* ctx, dv_ba_problem* P, dv_ba_summary* summary, BeFused* fused) {
    if (!ctx) return -1;
    BePending& pd = *ctx->be.pend;
    if (!pd.active) DV_FAIL("dv_ba_solve: nothing to collect");
    pd.active = false;
    if (pd.trivial) {
        if (summary) { summary->iterations = 0; summary->successful = 0; summary->termination = 1; summary->slots = 0; summary->initial_cost = 0; summary->final_cost = 0; }
        return 0;
    }
    BeWork& w = ctx->be;
    hipStream_t s = ctx->be_stream;
    if (pd.deferred) {        // a batch member collected without dv_batch_enqueue (the synchronous solves of the initialisation): enqueue it alone
        pd.deferred = false;
        if (be_enqueue_slots(ctx, pd, pd.first_slots, true, s)) return -1;
        if (be_enqueue_tail(ctx, pd, s)) return -1;
    }
    const MargPlan& pl = pd.pl;
    const BeDownload* dl = be_download(w);
    const BeState* hx = &dl->x; const BeCtl* hctl = &dl->ctl;
    DV_CHECK(hipEventSynchronize(pd.ev_state_ext ? pd.ev_state_ext : w.ev_state));      // (member of a dv_batch round: the group's event behind the shared gauge / reject launches)
    if (w.debug_wait_tail) DV_CHECK(hipStreamSynchronize(ctx->be_stream));      // dv_debug_set "wait_tail": the host does not move on until the marginalization behind ev_state has drained too (bisecting the open multi-sequence defect)
    if (be_dist_check(ctx)) return -1;      // sharded window, peer transport: a dead or late peer is an error of THIS solve, not garbage in its result
    // the previous frame's marginalization ran before this frame's upload (stream order), so its scalars have landed
    if (be_check_prev_marg(ctx, pd)) return -1;
    if (!hctl->done) {        // rare: a failed linear solve / invalid step used up slots -> the 3 spare slots, then the tail once more
        // (the raw solution is still in w.x: the gauge fix writes to the candidate buffer; the marginalization reads the untouched old prior)
        if (be_enqueue_slots(ctx, pd, 3, false, s)) return -1;
        if (be_enqueue_tail(ctx, pd, s)) return -1;
        DV_CHECK(hipEventSynchronize(w.ev_state));
        if (be_dist_check(ctx)) return -1;
    }
    if (pd.marg_in_flight) { pd.marg_in_flight = false; pd.marg_check_due = true; pd.check_slot = pd.scal_slot; pd.scal_slot ^= 1; }
    if (ctx->host_timing) {
        StageTimer* te = dv_timer_for(ctx, "h_solve_enqueue"); te->total_ms += std::chrono::duration<double, std::milli>(pd.t_enq - pd.t_up).count(); te->count++;
        StageTimer* tu = dv_timer_for(ctx, "h_solve_upload"); tu->total_ms += std::chrono::duration<double, std::milli>(pd.t_up - pd.t_begin).count(); tu->count++;
    }
    if (ctx->timing) {
        DV_CHECK(hipStreamSynchronize(s));         // measurement mode only: the timers are harvested from an idle stream
        StageTimer* te = dv_timer_for(ctx, "h_solve_enqueue"); te->total_ms += std::chrono::duration<double, std::milli>(pd.t_enq - pd.t_up).count(); te->count++;
        StageTimer* tu = dv_timer_for(ctx, "h_solve_upload"); tu->total_ms += std::chrono::duration<double, std::milli>(pd.t_up - pd.t_begin).count(); tu->count++;
        dv_harvest_timers(ctx, s);
    }
    for (int f = 0; f < P->nframes; ++f) { std::memcpy(P->pose + 7 * f, hx->pose[f], 56); if (P->use_imu) std::memcpy(P->speed_bias + 9 * f, hx->sb[f], 72); }
    if (P->nlm) std::memcpy(P->inv_depth, hx->inv_depth, 8 * (size_t)P->nlm);
    if (pd.copy_ex_td) { std::memcpy(P->ex_pose, hx->ex, 14 * 8); P->td[0] = hx->td; }      // free blocks: para_ex_pose / para_td as the solve left them
    if (w.debug_hash_log && fused && w.dbg_pinned) {      // what the device holds when the round is over: x (raw solution), the candidate buffer (gauge-fixed copy), the control block
        be_dbg_hash(w.x, pd.state_bytes & ~(size_t)7, w.dbg_pinned + 3, s);
        be_dbg_hash(w.cand, pd.state_bytes & ~(size_t)7, w.dbg_pinned + 4, s);
        be_dbg_hash(w.ctl, sizeof(BeCtl) & ~(size_t)7, w.dbg_pinned + 5, s);
        DV_CHECK(hipStreamSynchronize(s));
        w.dbg_dev_log.push_back(w.dbg_solve_no++);
        for (int k = 0; k < 6; ++k) w.dbg_dev_log.push_back(w.dbg_pinned[k]);
        if (w.dbg_slots) {
            const size_t nv = (size_t)BeWork::DBG_SLOTS * 5 * BeWork::DBG_RANGES;
            w.dbg_slot_log.insert(w.dbg_slot_log.end(), w.dbg_slots, w.dbg_slots + nv);
            std::memset(w.dbg_slots, 0, sizeof(unsigned long long) * nv);
        }
    }
    if (summary) {
        summary->iterations = hctl->iter; summary->successful = hctl->successful; summary->termination = hctl->done ? hctl->termination : 0;
        summary->slots = hctl->slots; summary->initial_cost = hctl->initial_cost; summary->final_cost = hctl->x_cost;
    }
    if (fused) fused->rej_flags = pd.rej_on ? w.rej_pinned : nullptr;
    if (fused && pd.want_raw_pose) std::memcpy(fused->raw_pose, dl->raw_pose, sizeof(fused->raw_pose));
    if (pd.do_marg) {
        std::memcpy(fused->diag, w.marg_last, sizeof(fused->diag));      // the scalars of THIS frame's marginalization are still in flight: the previous frame's (be_check_prev_marg)
        if (pl.empty) { std::memset(&fused->new_prior, 0, sizeof(fused->new_prior)); w.prior_resident = false; }
        else {
            // header only: A', b' and c0 are (being) written in HBM by the marginalization kernels still in flight
            marg_new_prior(pl, P->pose, P->speed_bias, P->ex_pose, P->td, std::nan(""), &fused->new_prior);      // x0 = the gauge-fixed states just downloaded
            w.prior_cur = pd.nxt; w.prior_resident = true;
            w.priorA = w.priorA_buf[pd.nxt]; w.priorb = w.priorb_buf[pd.nxt];
        }
    }
    return 0;
}

int be_solve_fused(dv_ctx* ctx, dv_ba_problem* P, dv_ba_summary* summary, BeFused* fused) {
    if (be_solve_fused_begin(ctx, P, fused)) return -1;
    return be_solve_fused_end(ctx, P, summary, fused);
}

extern "C" {

int dv_ba_solve(dv_ctx* ctx, dv_ba_problem* P, dv_ba_summary* summary) {
    if (!ctx) return -1;
    // an operator-level solve with a host prior would overwrite the prior buffer the estimator's next frame reads from HBM
    if (ctx->est && ctx->be.prior_resident && P && P->prior && P->prior->valid && P->prior_A != ctx->be.priorA_buf[ctx->be.prior_cur])
        DV_FAIL("dv_ba_solve: this ctx's estimator holds a device-resident prior; use a separate ctx for operator-level calls");
    return be_solve_fused(ctx, P, summary, nullptr);
}

int dv_ba_eval(dv_ctx* ctx, const dv_ba_problem* P, int* n_out, double* cost, double* S, double* g) {
    if (!ctx) return -1;
    if (!P || !n_out) DV_FAIL("dv_ba_eval: null argument");
    if (ctx->be.pend->active) DV_FAIL("dv_ba_eval: a solve is in flight");
    if (ctx->est && ctx->be.prior_resident && P->prior && P->prior->valid && P->prior_A != ctx->be.priorA_buf[ctx->be.prior_cur])
        DV_FAIL("dv_ba_eval: this ctx's estimator holds a device-resident prior; use a separate ctx for operator-level calls");
    if (be_begin_impl(ctx, const_cast<dv_ba_problem*>(P), nullptr, true)) return -1;
    BeWork& w = ctx->be;
    hipStream_t s = ctx->be_stream;
    const BePending& pd = *w.pend;
    if (pd.trivial) { w.pend->active = false; *n_out = 0; if (cost) *cost = 0; return 0; }
    const int n = pd.sa.dims.nstate, NBR = (n + 3) / 4, nblk = NBR * (NBR + 1) / 2;
    *n_out = n;
    std::vector<double> blk((size_t)nblk * 16), gv(2 * (size_t)n), lcost((size_t)std::max(P->nlm, 1)), io((size_t)std::max(P->nimu, 1) * IMU_OUT_STRIDE), pc(1);
    DV_CHECK(hipMemcpyAsync(blk.data(), w.Sc[0], 8 * blk.size(), hipMemcpyDeviceToHost, s));
    DV_CHECK(hipMemcpyAsync(gv.data(), w.gvec[0], 8 * gv.size(), hipMemcpyDeviceToHost, s));
    if (P->nlm) DV_CHECK(hipMemcpyAsync(lcost.data(), w.packets[0] + (size_t)BE_PK_COST * BE_PK_STRIDE, 8 * (size_t)P->nlm, hipMemcpyDeviceToHost, s));
    if (P->nimu) DV_CHECK(hipMemcpyAsync(io.data(), w.imu_out[0], 8 * (size_t)P->nimu * IMU_OUT_STRIDE, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipMemcpyAsync(pc.data(), w.prior_out[0], 8, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    if (be_dist_check(ctx)) return -1;
    if (cost) {
        double c = 0;
        if (pd.sa.sh.on) {          // sharded window: the landmark costs of the other ranks are known as their rank-ordered sum only (form scalar 10 of set 0)
            double lc = 0; DV_CHECK(hipMemcpy(&lc, pd.sa.sh.qf[0] + BE_QF_A + 10, 8, hipMemcpyDeviceToHost)); c = lc;
        } else for (int l = 0; l < P->nlm; ++l) c += lcost[l];
        for (int k = 0; k < P->nimu; ++k) c += io[(size_t)k * IMU_OUT_STRIDE];
        c += pc[0]; *cost = c;
    }
    if (g) for (int i = 0; i < n; ++i) g[i] = gv[i] - gv[n + i];
    if (S) for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) {          // unpack the block-packed lower triangle (be_solve.hip: blk_pos)
        const int bi = i >> 2, bj = j >> 2;
        const double v = blk[((size_t)bj * NBR - (size_t)bj * (bj - 1) / 2 + bi - bj) * 16 + (i & 3) * 4 + (j & 3)];
        S[(size_t)i * n + j] = v; S[(size_t)j * n + i] = v;
    }
    return 0;
}

int dv_proj_eval(dv_ctx* ctx, const dv_ba_factor* factors, int n, const double* pose_i, const double* pose_j, const double* ex0,
                 const double* ex1, const double* inv_depth, const double* td, double* out) {
    if (!ctx) return -1;
    if (!factors || n <= 0 || !out) DV_FAIL("dv_proj_eval: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->be_stream;
    const size_t nf = sizeof(BeFactor) * (size_t)n, np = 56 * (size_t)n, ns = 8 * (size_t)n, no = 8 * 54 * (size_t)n;
    DV_CHECK(ctx->s0.ensure(nf + 4 * np + 2 * ns + no + 1024));
    uint8_t* b = (uint8_t*)ctx->s0.p;
    BeFactor* dfac = (BeFactor*)b; double* dpi = (double*)(b + nf); double* dpj = dpi + 7 * n; double* de0 = dpj + 7 * n; double* de1 = de0 + 7 * n;
    double* dl = de1 + 7 * n; double* dtd = dl + n; double* dout = dtd + n;
    DV_CHECK(hipMemcpyAsync(dfac, factors, nf, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(dpi, pose_i, np, hipMemcpyHostToDevice, s)); DV_CHECK(hipMemcpyAsync(dpj, pose_j, np, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(de0, ex0, np, hipMemcpyHostToDevice, s)); DV_CHECK(hipMemcpyAsync(de1, ex1, np, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(dl, inv_depth, ns, hipMemcpyHostToDevice, s)); DV_CHECK(hipMemcpyAsync(dtd, td, ns, hipMemcpyHostToDevice, s));
    be_launch_proj_op(dfac, n, dpi, dpj, de0, de1, dl, dtd, dout, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpyAsync(out, dout, no, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

int dv_imu_eval(dv_ctx* ctx, const dv_ba_imu* imu, double g_norm, const double* pose_i, const double* sb_i, const double* pose_j,
                const double* sb_j, double* out) {
    if (!ctx) return -1;
    if (!imu || !out) DV_FAIL("dv_imu_eval: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->be_stream;
    BeImu h;
    if (be_fill_imu(*imu, h, nullptr)) DV_FAIL("dv_imu_eval: IMU covariance is singular");
    DV_CHECK(ctx->s0.ensure(sizeof(BeImu) + 8 * (32 + 465) + 256));
    uint8_t* b = (uint8_t*)ctx->s0.p;
    BeImu* dm = (BeImu*)b; double* dpar = (double*)(b + sizeof(BeImu)); double* dout = dpar + 32;
    double par[32];
    std::memcpy(par, pose_i, 56); std::memcpy(par + 7, sb_i, 72); std::memcpy(par + 16, pose_j, 56); std::memcpy(par + 23, sb_j, 72);
    DV_CHECK(hipMemcpyAsync(dm, &h, sizeof(h), hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(dpar, par, sizeof(par), hipMemcpyHostToDevice, s));
    be_launch_imu_op(dm, g_norm, dpar, dout, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpyAsync(out, dout, 8 * 465, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

// the BeState the tail kernels read, from the caller's flat blocks (absent blocks stay zero)
static void be_op_state(BeState& h, const double* pose, const double* sb, const double* ex, const double* inv_depth, int nlm) {
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.pose, pose, sizeof(h.pose));
    if (sb) std::memcpy(h.sb, sb, sizeof(h.sb));
    if (ex) std::memcpy(h.ex, ex, sizeof(h.ex));
    if (nlm > 0) std::memcpy(h.inv_depth, inv_depth, 8 * (size_t)nlm);
}

int dv_ba_gauge(dv_ctx* ctx, const double* pose, const double* speed_bias, const double* inv_depth, int nlm, int nframes, int use_imu,
                const double* R0, const double* ypr0, const double* P0, double* out_pose, double* out_speed_bias, double* out_inv_depth) {
    if (!ctx) return -1;
    if (!pose || !speed_bias || !R0 || !ypr0 || !P0 || !out_pose || !out_speed_bias) DV_FAIL("dv_ba_gauge: null argument");
    if (nframes < 1 || nframes > BE_NF || nlm < 0 || nlm > BE_MAX_LM || (nlm > 0 && (!inv_depth || !out_inv_depth))) DV_FAIL("dv_ba_gauge: bad argument");
    if (ctx->be.pend && ctx->be.pend->active) DV_FAIL("dv_ba_gauge: a solve is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->be_stream;
    DV_CHECK(ctx->s0.ensure(2 * sizeof(BeState) + 256));
    BeState* dx = (BeState*)ctx->s0.p; BeState* dout = dx + 1;
    std::vector<BeState> hs(1);
    BeState& h = hs[0];
    be_op_state(h, pose, speed_bias, nullptr, inv_depth, nlm);
    DV_CHECK(hipMemcpyAsync(dx, &h, sizeof(h), hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemsetAsync(dout, 0, sizeof(BeState), s));
    BeGaugeArgs ga{};
    ga.x = dx; ga.out = dout; ga.nframes = nframes; ga.use_imu = use_imu ? 1 : 0; ga.nlm = nlm;
    std::memcpy(ga.R0, R0, sizeof(ga.R0)); std::memcpy(ga.ypr0, ypr0, sizeof(ga.ypr0)); std::memcpy(ga.P0, P0, sizeof(ga.P0));
    be_launch_gauge(ga, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpyAsync(&h, dout, sizeof(h), hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    std::memcpy(out_pose, h.pose, sizeof(h.pose)); std::memcpy(out_speed_bias, h.sb, sizeof(h.sb));
    if (nlm > 0) std::memcpy(out_inv_depth, h.inv_depth, 8 * (size_t)nlm);
    return 0;
}

int dv_ba_reject(dv_ctx* ctx, const double* pose, const double* ex_pose, const double* inv_depth, const dv_ba_factor* factors, int nfac,
                 const dv_ba_lm* landmarks, int nlm, int nframes, const double* ric, const double* tic, double focal, int ex_from_state, uint8_t* flags) {
    if (!ctx) return -1;
    if (!pose || !ex_pose || !inv_depth || !factors || !landmarks || !ric || !tic || !flags) DV_FAIL("dv_ba_reject: null argument");
    if (nframes < 1 || nframes > BE_NF || nlm < 1 || nlm > BE_MAX_LM || nfac < 1) DV_FAIL("dv_ba_reject: bad argument");
    for (int l = 0; l < nlm; ++l) {        // everything the kernel indexes with: one half-wave (32 lanes) per landmark, frames < nframes
        const dv_ba_lm& L = landmarks[l];
        if (L.first < 0 || L.count < 1 || L.count > BE_MAX_OBS_FACTORS || L.first > nfac - L.count || L.anchor < 0 || L.anchor >= nframes) DV_FAIL("dv_ba_reject: bad landmark record");
        for (int k = 0; k < L.count; ++k) {
            const dv_ba_factor& f = factors[L.first + k];
            if (f.kind < 0 || f.kind > 2 || f.fj < 0 || f.fj >= nframes) DV_FAIL("dv_ba_reject: bad factor record");
        }
    }
    if (ctx->be.pend && ctx->be.pend->active) DV_FAIL("dv_ba_reject: a solve is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->be_stream;
    const size_t nf = sizeof(BeFactor) * (size_t)nfac, nl = sizeof(BeLm) * (size_t)nlm, nflag = ((size_t)nlm + 255) & ~(size_t)255;
    DV_CHECK(ctx->s0.ensure(sizeof(BeState) + nf + nl + nflag + 256));
    uint8_t* b = (uint8_t*)ctx->s0.p;
    BeState* dx = (BeState*)b; BeFactor* dfac = (BeFactor*)(b + sizeof(BeState)); BeLm* dlm = (BeLm*)(b + sizeof(BeState) + nf); uint8_t* dflag = b + sizeof(BeState) + nf + nl;
    std::vector<BeState> hs(1);
    be_op_state(hs[0], pose, nullptr, ex_pose, inv_depth, nlm);
    DV_CHECK(hipMemcpyAsync(dx, &hs[0], sizeof(BeState), hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(dfac, factors, nf, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(dlm, landmarks, nl, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemsetAsync(dflag, 0xff, nflag, s));        // a landmark the kernel skips shows as 255
    BeRejectArgs r{};
    r.st = dx; r.fac = dfac; r.lm = dlm; r.nlm = nlm; r.nframes = nframes; r.focal = focal; r.flags = dflag; r.ex_from_state = ex_from_state ? 1 : 0;
    std::memcpy(r.ric, ric, sizeof(r.ric)); std::memcpy(r.tic, tic, sizeof(r.tic));
    be_launch_reject(r, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpyAsync(flags, dflag, (size_t)nlm, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
