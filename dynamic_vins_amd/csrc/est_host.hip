// est_host.hip — host side of the back end (product code): the schedule of dynamic_vins' Estimator around the device kernels and the dv_est_* entries.
// The window bookkeeping and every piece of host arithmetic live in est_window.h (HIP-free); what is here needs a dv_ctx:
//   Estimator::{ProcessImage (with its object branch),InitEstimator,Optimization,SetMarginalizationInfo,OptimizationWithOnlyLine,ChangeSensorType}   estimator/estimator.cpp
// What runs where: IMU pre-integration, triangulation, PnP seeding and the window shuffling are O(100) flops per item and stay on the host; every
// residual/Jacobian evaluation, the Schur elimination, the trust-region loop and the marginalization run on the GPU through dv_ba_solve / dv_marginalize.
// Deviation from the reference that changes no result: IMUFactor's sqrt-information cached per solve (Q8).
#include "dv_ctx.h"
#include "est_window.h"

using namespace estw;
static_assert(kWin == BE_WIN, "est_window.h and be_types.h agree on kWinSize");

struct dv_estimator : EstWindow {
    bool open_ex = false;          // Estimator::openExEstimation (estimator.h:173): sticky until ClearState (estimator.cpp:632)
    dv_ba_prior prior{};          // header on the host, A' / b' device-resident
    dv_ba_summary last{};
    // dynamic mode (cfg.dynamic): Estimator::im + what body.para_pose holds when InstanceManager::Optimization reads it (estimator_insts.cpp:1043-1045):
    // the values the PREVIOUS frame's Optimization left there — ceres' raw output, or the gauge-fixed states where SetMarginalizationInfo called
    // Vector2double again (estimator.cpp:409,562)
    dvi::InstMgr im; double para_pose_ref[kWin + 1][7]; dv_ba_summary obj_last{}; bool dyn_frame = false;
    // line mode (cfg.use_line): body.para_line_features as Vector2double fills them
    std::vector<double> para_line; dv_ba_summary line_last{};

    explicit dv_estimator(const dv_est_config& c) : EstWindow(c) { clear(); }
    void clear() {
        EstWindow::clear();
        prior = dv_ba_prior{}; open_ex = false; para_line.clear(); line_last = dv_ba_summary{};
        im.clear(); im.cfg.use_det3d = cfg.use_det3d; im.cfg.init_min_num = cfg.instance_init_min_num; im.cfg.static_threshold = cfg.static_inst_threshold;
        im.cfg.plane_kind = cfg.plane_constraint ? (cfg.use_imu ? 1 : 2) : 0; im.cfg.max_iters = cfg.max_iters;
        std::memset(para_pose_ref, 0, sizeof(para_pose_ref)); obj_last = dv_ba_summary{}; dyn_frame = false; dyn_tail_deferred = false;
    }

    // ---------------- optimisation (device) ----------------
    dv_ba_problem P{}; BeFused fu;          // the solve in flight (optimization_begin .. optimization_end)
    // diagnostics (dv_debug_set "hash_log"; the open multi-sequence defect of round 4): per window solve [solve counter, hash of the states uploaded, hash of the tables
    // uploaded (factors, landmarks, IMU records, prior descriptor), hash of the states downloaded, hash of the outlier flags consumed, iterations]
    std::vector<unsigned long long> hash_log; unsigned long long solve_no = 0;
    static unsigned long long fnv(unsigned long long h, const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } return h; }
    unsigned long long hash_states() const {
        unsigned long long h = 1469598103934665603ull;
        h = fnv(h, pose, sizeof(pose)); h = fnv(h, sb, sizeof(sb)); h = fnv(h, ex, sizeof(ex)); h = fnv(h, tdv, sizeof(tdv)); h = fnv(h, invd.data(), invd.size() * sizeof(double));
        return h;
    }
    int optimization_begin(dv_ctx* ctx) {        // Estimator::Optimization (estimator.cpp:261-339) incl. SetMarginalizationInfo (:403-619)
        { HostScope h(ctx, "h_build");
          states_to_arrays();
          int cap = 0; dv_ba_factor* staging = (dv_ba_factor*)be_staging_factors(ctx, &cap);
          build_factors(false, staging, cap);
          imu.clear();
          ctx->be.sqrt_hint.clear();
          if (cfg.use_imu) for (int i = 0; i < frame; ++i) { if (pre[i + 1]->sum_dt > 10.0) continue; dv_ba_imu r; pre[i + 1]->fill(r, i, i + 1); imu.push_back(r); ctx->be.sqrt_hint.push_back(pre[i + 1]->sqrt_info()); }
          P = make_problem(frame + 1);
          if (prior.valid) { P.prior = &prior; P.prior_A = ctx->be.priorA_buf[ctx->be.prior_cur]; P.prior_b = ctx->be.priorb_buf[ctx->be.prior_cur]; }      // A', b' stay in HBM (written by the fused marginalization)
          {   // AddBodyParameterBlock (estimator.cpp:87-100): which of para_ex_pose / para_td this solve may move
              const double v0 = norm(Vs[0]);
              if (((cfg.estimate & 1) && frame == kWin && v0 > 0.2) || open_ex) { open_ex = true; P.free_blocks |= 1; }
              if ((cfg.estimate & 2) && !(v0 < 0.2)) P.free_blocks |= 2;
          }
          if (cfg.use_line) {          // Vector2double's line part + AddLineResidualBlock under zero weights: the blocks only count in |x| (see dv_ba_problem::x_norm2_extra)
              lines.get_orth(Rs, Ps, ric[0], tic[0], para_line);
              double sq = 0; for (double v : para_line) sq += v * v;
              P.x_norm2_extra = sq;
          }
          // gauge reference: yaw and position of frame 0 before the solve (Double2vector, estimator.cpp:1111-1128)
          const d3 y0 = r2ypr(Rs[0]);
          std::memcpy(fu.R0, Rs[0].m, sizeof(fu.R0)); put3(fu.ypr0, y0); put3(fu.P0, Ps[0]);
          fu.marg_mode = -1; fu.want_raw_pose = cfg.dynamic != 0;
          {   // OutliersRejection runs on the device behind the gauge fix (be_reject_kernel): the extrinsics it must use are the ones arrays_to_states will leave
              fu.want_reject = nonlinear; fu.rej_focal = kFocal;      // the initialisation solves never consume the flags (InitEstimator has no OutliersRejection)
              for (int c = 0; c < 2; ++c) {
                  const m33 r = cfg.use_imu ? qR(qnormalized(Q4(ex[c]))) : ric[c];
                  std::memcpy(fu.rej_ric[c], r.m, sizeof(r.m)); put3(fu.rej_tic[c], cfg.use_imu ? P3(ex[c]) : tic[c]);
              }
          }
          if (frame == kWin) {
              if (margin_old) fu.marg_mode = 0;
              else {
                  bool has9 = false;          // MARGIN_SECOND_NEW touches the prior only if it holds pose kWin-1 (estimator.cpp:557-560)
                  if (prior.valid) for (int i = 0; i < prior.nblocks; ++i) if (prior.blocks[i].type == 0 && prior.blocks[i].idx == kWin - 1) has9 = true;
                  if (has9) fu.marg_mode = 1;
              }
          }
        }
        if (ctx->be.debug_hash_log) {
            unsigned long long ht = 1469598103934665603ull;
            ht = fnv(ht, P.factors, (size_t)P.nfac * sizeof(dv_ba_factor)); ht = fnv(ht, lmt.data(), lmt.size() * sizeof(lmt[0])); ht = fnv(ht, imu.data(), imu.size() * sizeof(dv_ba_imu));
            const int pv = prior.valid ? 1 : 0; ht = fnv(ht, &pv, sizeof(pv));
            if (prior.valid) { ht = fnv(ht, &prior.n, sizeof(prior.n)); ht = fnv(ht, &prior.nblocks, sizeof(prior.nblocks)); ht = fnv(ht, prior.blocks, (size_t)prior.nblocks * sizeof(prior.blocks[0])); ht = fnv(ht, &fu.marg_mode, sizeof(fu.marg_mode)); }
            // the device-resident prior this solve starts from (written by the previous frame's marginalization): synchronises the solve stream — diagnostics only
            unsigned long long hp = 0;
            if (prior.valid && P.prior_A && P.prior_b) {
                std::vector<double> tmp((size_t)prior.n * prior.n + prior.n);
                (void)hipStreamSynchronize(ctx->be_stream);
                (void)hipMemcpy(tmp.data(), P.prior_A, (size_t)prior.n * prior.n * sizeof(double), hipMemcpyDeviceToHost);
                (void)hipMemcpy(tmp.data() + (size_t)prior.n * prior.n, P.prior_b, (size_t)prior.n * sizeof(double), hipMemcpyDeviceToHost);
                hp = fnv(1469598103934665603ull, tmp.data(), tmp.size() * sizeof(double));
            }
            hash_log.push_back(solve_no++); hash_log.push_back(hash_states()); hash_log.push_back(ht); hash_log.push_back(0); hash_log.push_back(hp); hash_log.push_back(0);
        }
        { HostScope h(ctx, "h_solve_begin"); const int rc = be_solve_fused_begin(ctx, &P, &fu); ctx->be.sqrt_hint.clear(); if (rc) return -1; }
        return 0;
    }
    int optimization_end(dv_ctx* ctx) {
        { HostScope h(ctx, "h_solve_wait"); if (be_solve_fused_end(ctx, &P, &last, &fu)) return -1; }
        if (ctx->be.debug_hash_log && hash_log.size() >= 6) {
            unsigned long long* r = hash_log.data() + hash_log.size() - 6;
            r[3] = hash_states(); r[5] = (unsigned long long)last.iterations;
            if (fu.rej_flags) r[3] = fnv(r[3], fu.rej_flags, (size_t)long_count());      // (the outlier flags consumed count as downloaded state)
        }
        { HostScope h(ctx, "h_post"); arrays_to_states(); }
        if (cfg.use_line && !para_line.empty()) lines.set_orth(Rs, Ps, ric[0], tic[0], para_line.data());      // Double2vector: SetLineOrth with the solved poses
        if (fu.marg_mode >= 0) prior = fu.new_prior;
        if (cfg.dynamic) {
            if (fu.marg_mode >= 0) {          // SetMarginalizationInfo re-ran Vector2double: para_pose = the gauge-fixed window
                for (int i = 0; i <= kWin; ++i) pack_pose(Ps[i], Rs[i], para_pose_ref[i]);
            } else if (ctx->be.pend->trivial) std::memcpy(para_pose_ref, pose, sizeof(para_pose_ref));
            else std::memcpy(para_pose_ref, fu.raw_pose, sizeof(para_pose_ref));
        }
        return 0;
    }
    int optimization(dv_ctx* ctx) { if (optimization_begin(ctx)) return -1; return optimization_end(ctx); }
    int init_estimator(dv_ctx* ctx) {        // InitEstimator (estimator.cpp:1424-1508), stereo paths
        if (cfg.stereo && cfg.use_imu) {
            pnp_frame(frame); triangulate();
            if (frame == kWin) {
                solve_gyro_bias();
                for (int j = 0; j <= kWin; ++j) pre[j]->repropagate(mk3(0, 0, 0), Bgs[j]);
                if (optimization(ctx)) return -1;
                nonlinear = true; slide_window();
            }
        } else if (cfg.stereo && !cfg.use_imu) {
            pnp_frame(frame); triangulate();
            if (optimization(ctx)) return -1;
            if (frame == kWin) { if (optimization(ctx)) return -1; nonlinear = true; slide_window(); }
        }
        if (frame < kWin) { frame++; const int p = frame - 1; Ps[frame] = Ps[p]; Vs[frame] = Vs[p]; Rs[frame] = Rs[p]; Bas[frame] = Bas[p]; Bgs[frame] = Bgs[p]; }
        return 0;
    }
    // Estimator::OptimizationWithOnlyLine (estimator.cpp:345-395): Vector2double, the line-only dogleg solve on the GPU (dv_line_solve; with the reference's zero
    // sqrt_info every residual and Jacobian is zero and ceres returns before its first step, so nothing is launched), Double2vector, RemoveLineOutlier.
    // Deviation (only reachable with non-zero weights): the reference leaves para_pose[kWinSize] a free 7-wide block here (its loop fixes poses 0..kWinSize-1);
    // dv_line_solve keeps all poses fixed.
    int optimization_only_line(dv_ctx* ctx) {
        lines.get_orth(Rs, Ps, ric[0], tic[0], para_line);
        line_last = dv_ba_summary{};
        if (!para_line.empty() && !line_zero_w()) {
            states_to_arrays();
            std::vector<dv_line_obs> obs; lines.observations(obs);
            dv_line_problem LP{};
            LP.n_lines = (int)para_line.size() / 4; LP.n_obs = (int)obs.size(); LP.max_iters = cfg.max_iters;
            LP.orth = para_line.data(); LP.pose = &pose[0][0]; LP.ex_pose = &ex[0][0]; std::memcpy(LP.sqrt_info, cfg.line_sqrt_info, sizeof(LP.sqrt_info)); LP.obs = obs.data();
            if (dv_line_solve(ctx, &LP, &line_last)) return -1;
        }
        if (!para_line.empty()) lines.set_orth(Rs, Ps, ric[0], tic[0], para_line.data());      // Double2vector (the poses did not move: re-normalises the Pluecker vectors)
        lines.remove_outliers(Rs, Ps, ric[0], tic[0]);
        return 0;
    }
    // the object branch of ProcessImage between TriangulatePoints and Optimization (estimator.cpp:1562-1622).  It neither reads what the window
    // solve writes nor writes what it reads (the joint factors are dead code), so it runs on the host + a third stream while the window
    // solve enqueued just before is in flight on the BA stream.
    int dynamic_branch(dv_ctx* ctx, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats, const double* points) {
        HostScope h(ctx, "h_dynamic");
        flush_dyn_tail(ctx);          // the previous frame's object tail (see BodySnap)
        const dvi::BodyView B = body_view();
        { HostScope h1(ctx, "h_dyn_push"); im.push_back(frame, B, insts, n_insts, inst_feats, points); im.set_output_inst_info(); }
        { HostScope h1(ctx, "h_dyn_propagate"); im.propagate_pose(B); }
        { HostScope h1(ctx, "h_dyn_triangulate"); im.triangulate(B); }
        { HostScope h1(ctx, "h_dyn_initial"); im.initial_instance(B); im.initial_velocity(B); im.set_dynamic_or_static(B); }
        obj_solved = false; obj_last = dv_ba_summary{};
        bool have;
        { HostScope h1(ctx, "h_dyn_build"); have = im.build_problem(OP, &para_pose_ref[0][0], ric[0]) && (OP.n_boxes > 0 || OP.n_points > 0); }
        if (have) {
            HostScope h1(ctx, "h_dyn_solve_begin");
            // enqueued; collected in dynamic_branch_finish.  Member of a dv_batch: uploaded on the group's object stream and left to dv_batch_enqueue, which launches the object
            // solves of all members as one grid (be_batch.hip); a member with stage timers keeps its own launch (the timers are per stream)
            hipStream_t gs = ctx->batch ? be_batch_obj_stream(ctx->batch) : nullptr;
            if (be_obj_solve_begin(ctx, &OP, gs ? gs : ctx->obj_stream, ctx->obj_buf, ctx->obj_pend, gs && !ctx->timing)) return -1;
            obj_solved = true;
        }
        return 0;
    }
    // second half of the object branch (InstanceManager::GetOptimizationParameters + OutliersRejection, estimator_insts.cpp:804, estimator.cpp:1615): needs the object
    // solve's result and still the PRE-optimisation body states, so it runs at the top of process_image_end, before the window solve's result is applied
    dv_obj_problem OP{}; bool obj_solved = false;
    // The object branch's tail of a frame — ManageTriangulatePoint + SlideWindow on the body window BEFORE it slides, the per-frame clean-up on the slid window
    // (estimator.cpp:1653-1676) — reads nothing the next frame's ego branch writes and writes nothing it reads: it is kept back, with snapshots of the two body views it needs,
    // and runs at the top of the next frame's object branch, i.e. beside that frame's window solve instead of in front of it (45 us of the host path the GPU waits for).
    // Anything that looks at the objects before that (dv_est_get_instances, a reset) runs it first: same calls on the same data in the same order.
    struct BodySnap {
        m33 Rs[kWin + 1]; d3 Ps[kWin + 1]; m33 ric[2]; d3 tic[2]; double headers[kWin + 1]; double td = 0; int frame = 0;
        dvi::BodyView view() const { return dvi::BodyView{ Rs, Ps, ric, tic, headers, td, frame }; }
        void take(const dvi::BodyView& v) { std::copy(v.Rs, v.Rs + kWin + 1, Rs); std::copy(v.Ps, v.Ps + kWin + 1, Ps); std::copy(v.headers, v.headers + kWin + 1, headers); std::copy(v.ric, v.ric + 2, ric); std::copy(v.tic, v.tic + 2, tic); td = v.td; frame = v.frame; }
    };
    BodySnap snap_pre, snap_post; bool dyn_tail_deferred = false, dyn_tail_margin_old = false;
    void flush_dyn_tail(dv_ctx* ctx) {
        if (!dyn_tail_deferred) return;
        dyn_tail_deferred = false;
        { HostScope h1(ctx, "h_dyn_slide"); const dvi::BodyView B = snap_pre.view(); im.manage_triangulate_point(B); im.slide_window(B, dyn_tail_margin_old); }
        { HostScope h1(ctx, "h_dyn_finish_frame"); im.finish_frame(snap_post.view()); }
    }
    int dynamic_branch_finish(dv_ctx* ctx) {
        HostScope h(ctx, "h_dynamic_finish");
        { HostScope h1(ctx, "h_dyn_solve_wait"); if (obj_solved && be_obj_solve_end(ctx, &OP, &obj_last, ctx->obj_pend)) return -1; }
        im.read_back(obj_solved);
        { HostScope h1(ctx, "h_dyn_reject"); im.outliers_rejection(body_view()); }
        return 0;
    }
    bool dyn_deferred = false;      // dv_est_process_dynamic_begin_ego: the object branch of this frame comes with dv_est_process_dynamic_attach
    int process_image_begin(dv_ctx* ctx, const dv_feat* feats, int n, double header, const dv_inst_obs* insts = nullptr, int n_insts = 0, const dv_feat* inst_feats = nullptr,
                            const double* points = nullptr, bool defer_dynamic = false) {      // ProcessImage (estimator.cpp:1516-1696), up to and including the enqueue of the window solve
        { HostScope h(ctx, "h_add_features");
          if (cfg.use_line) { lines.add(frame, pending_lines.data(), (int)pending_lines.size()); pending_lines.clear(); }
          margin_old = add_features(frame, feats, n); }
        headers[frame] = header;
        frame_pre.push_back(std::shared_ptr<Preint>(tmp_pre.release()));
        if (frame_pre.size() > (size_t)kWin + 1 && nonlinear) frame_pre.erase(frame_pre.begin());
        tmp_pre = new_preint(frame);
        in_flight = false; dyn_frame = false; dyn_deferred = false;
        if (!nonlinear) return init_estimator(ctx);      // initialisation: synchronous
        if (!cfg.use_imu) pnp_frame(frame);
        { HostScope h(ctx, "h_triangulate"); triangulate(); if (cfg.use_line) lines.triangulate(Rs, Ps, ric[0], tic[0]); }
        if (cfg.use_line) {
            if (!line_zero_w() && lines.count() > 0 && !line_weight_warned) { line_weight_warned = true; dv_set_error(ctx, "line mode: non-zero lineProjectionFactor::sqrt_info is honoured by OptimizationWithOnlyLine only; inside the window solve the line blocks stay inert"); }
            HostScope h(ctx, "h_line_only"); if (optimization_only_line(ctx)) return -1;
        }
        if (optimization_begin(ctx)) return -1;
        in_flight = true;
        dyn_frame = cfg.dynamic != 0;
        if (dyn_frame && defer_dynamic) { dyn_deferred = true; return 0; }
        if (dyn_frame && dynamic_branch(ctx, insts, n_insts, inst_feats, points)) return -1;
        return 0;
    }
    int process_image_end(dv_ctx* ctx) {
        if (!in_flight) return 0;
        in_flight = false;
        if (dyn_frame && dyn_deferred) { dyn_deferred = false; if (dynamic_branch(ctx, nullptr, 0, nullptr, nullptr)) return -1; }      // never attached: a frame without objects
        if (dyn_frame && dynamic_branch_finish(ctx)) return -1;      // before optimization_end: Rs / Ps are still the states the reference's object branch saw
        if (optimization_end(ctx)) return -1;
        if (dyn_frame) im.touch_in_main_optimization();      // AddInstanceParameterBlock / im.GetOptimizationParameters inside Estimator::Optimization
        { HostScope h(ctx, "h_reject"); reject_outliers(fu.rej_flags); fu.rej_flags = nullptr; if (cfg.use_line) lines.remove_outliers(Rs, Ps, ric[0], tic[0]); }
        if (dyn_frame) { flush_dyn_tail(ctx); snap_pre.take(body_view()); dyn_tail_margin_old = margin_old; }      // estimator.cpp:1653-1658 sees the body window BEFORE it slides ...
        { HostScope h(ctx, "h_slide"); slide_window(); }
        if (dyn_frame) { snap_post.take(body_view()); dyn_tail_deferred = true; }                                     // ... and :1663-1676 the slid one: both kept back (flush_dyn_tail)
        erase_if([](const Lm& l) { return l.solve_flag == 2; });      // RemoveFailures
        update_latest_states();          // unconditional in the reference (estimator.cpp:1688); the IMU replay inside is empty in vision-only mode
        return 0;
    }
    bool in_flight = false, begun = false, line_weight_warned = false;
};

// the entries' preamble: a null ctx has nowhere to leave a message; without an estimator, "<entry>: call dv_est_create first"
static bool have_est(dv_ctx* ctx, const char* entry) {
    if (ctx && !ctx->est) dv_set_error(ctx, std::string(entry) + ": call dv_est_create first");
    return ctx && ctx->est;
}

extern "C" {

int dv_est_create(dv_ctx* ctx, const dv_est_config* cfg) {
    if (!ctx) return -1;
    if (!cfg) DV_FAIL("dv_est_create: null config");
    if (!cfg->stereo) DV_FAIL("dv_est_create: monocular initialisation is out of scope (every BASELINE config is stereo)");
    if (cfg->estimate & ~3) DV_FAIL("dv_est_create: estimate: bit 0 estimate_extrinsic 1, bit 1 estimate_td 1 (estimate_extrinsic 2, the from-scratch calibration, is not built)");
    if (cfg->estimate && cfg->dynamic)      // the reference's static-instance factors take para_ex_pose[0] / para_td (estimator.cpp:205); the object branch here builds its problem with constant extrinsics
        DV_FAIL("dv_est_create: estimate != 0 (free extrinsic / td blocks) is not built for dynamic = 1: the object branch's factors carry no extrinsic / td Jacobians");
    delete ctx->est;
    ctx->est = new dv_estimator(*cfg);
    return be_prepare(ctx, cfg->dynamic != 0);      // nothing is allocated or created lazily in the middle of a sequence
}
// diagnostics (dv_debug_set "hash_log"): rows of six uint64 per window solve, see dv_estimator::hash_log
int dv_est_debug_hash_log(dv_ctx* ctx, unsigned long long* rows6, int cap, int* n_rows) {
    if (!ctx || !ctx->est) return -1;
    const int n = (int)(ctx->est->hash_log.size() / 6);
    if (n_rows) *n_rows = n;
    if (rows6) std::memcpy(rows6, ctx->est->hash_log.data(), sizeof(unsigned long long) * 6 * (size_t)std::min(n, std::max(cap, 0)));
    return 0;
}
int dv_est_reset(dv_ctx* ctx) { if (!ctx || !ctx->est) return -1; if (ctx->est->begun) { ctx->est->begun = false; (void)ctx->est->process_image_end(ctx); } ctx->est->clear(); return 0; }
int dv_est_input_imu(dv_ctx* ctx, double t, const double* acc, const double* gyr) {
    if (!ctx || !ctx->est) return -1;
    dv_estimator& E = *ctx->est;
    E.imu_buf.push_back({ t, { P3(acc), P3(gyr) } });
    if (E.nonlinear && E.latest_valid) E.fast_predict_imu(t, P3(acc), P3(gyr));      // InputIMU: FastPredictIMU + PubLatestOdometry (estimator.cpp:734-741)
    return 0;
}
int dv_est_set_lines(dv_ctx* ctx, const dv_line_row* rows, int n) {
    if (!have_est(ctx, "dv_est_set_lines")) return -1;
    if (n < 0 || (n > 0 && !rows)) DV_FAIL("dv_est_set_lines: bad argument");
    if (!ctx->est->cfg.use_line) DV_FAIL("dv_est_set_lines: the estimator was created with use_line = 0");
    ctx->est->pending_lines.assign(rows, rows + n);
    return 0;
}
int dv_est_get_lines(dv_ctx* ctx, dv_line_landmark* out, int cap, int* n_out) {
    if (!have_est(ctx, "dv_est_get_lines")) return -1;
    if (!n_out || cap < 0 || (cap > 0 && !out)) DV_FAIL("dv_est_get_lines: bad argument");
    int k = 0;
    for (auto& L : ctx->est->lines.lms) {
        if (k >= cap) break;
        dv_line_landmark& o = out[k++];
        std::memset(&o, 0, sizeof(o));
        o.id = L.id; o.start_frame = L.start; o.n_obs = (int)L.obs.size(); o.is_triangulation = L.tri;
        if (L.tri) { put3(o.plucker, L.plk.n); put3(o.plucker + 3, L.plk.v); put3(o.ptw1, L.ptw1); put3(o.ptw2, L.ptw2); }
    }
    *n_out = k;
    return 0;
}
// Estimator::ChangeSensorType (estimator.cpp:697-726)
int dv_est_change_sensor_type(dv_ctx* ctx, int use_imu, int use_stereo) {
    if (!have_est(ctx, "dv_est_change_sensor_type")) return -1;
    dv_estimator& E = *ctx->est;
    if (E.begun) DV_FAIL("dv_est_change_sensor_type: a frame is in flight");
    if (!use_imu && !use_stereo) DV_FAIL("dv_est_change_sensor_type: at least two sensors are needed (reference: message only)");
    if (!use_stereo) DV_FAIL("dv_est_change_sensor_type: monocular operation is out of scope (every BASELINE config is stereo)");
    bool restart = false;
    if ((E.cfg.use_imu != 0) != (use_imu != 0)) {
        E.cfg.use_imu = use_imu ? 1 : 0;
        if (use_imu) restart = true;
        else { E.prior = dv_ba_prior{}; ctx->be.prior_resident = false; E.tmp_pre.reset(); E.latest_valid = false; }      // last_marg_info, tmp_pre_integration dropped
    }
    E.cfg.stereo = 1;
    if (restart) E.clear();          // ClearState + SetParameter
    return 0;
}
// latest_P / latest_Q / latest_V (what Publisher::PubLatestOdometry gets, estimator.cpp:737-739)
int dv_est_get_latest(dv_ctx* ctx, double* t, double* P3o, double* Q4o, double* V3o) {
    if (!have_est(ctx, "dv_est_get_latest")) return -1;
    const dv_estimator& E = *ctx->est;
    if (!E.latest_valid) return 1;
    const quat q = qnormalized(E.latest_Q);
    if (t) *t = E.latest_time;
    if (P3o) put3(P3o, E.latest_P);
    if (Q4o) { Q4o[0] = q.x; Q4o[1] = q.y; Q4o[2] = q.z; Q4o[3] = q.w; }
    if (V3o) put3(V3o, E.latest_V);
    return 0;
}
// body.ric / body.tic / body.td as Double2vector left them (what pubOdometry writes to the extrinsic file when estimate_extrinsic is on, utils/io/visualization.cpp:94-118)
int dv_est_get_extrinsics(dv_ctx* ctx, double* ric18, double* tic6, double* td) {
    if (!have_est(ctx, "dv_est_get_extrinsics")) return -1;
    const dv_estimator& E = *ctx->est;
    for (int c = 0; c < 2; ++c) {
        if (ric18) std::memcpy(ric18 + 9 * c, E.ric[c].m, 72);
        if (tic6) put3(tic6 + 3 * c, E.tic[c]);
    }
    if (td) *td = E.td;
    return 0;
}
// feat_manager.point_landmarks as the point-cloud publishers read them (utils/io/visualization.cpp:214-249)
int dv_est_get_landmarks(dv_ctx* ctx, dv_landmark* out, int cap, int* n_out) {
    if (!have_est(ctx, "dv_est_get_landmarks")) return -1;
    if (!n_out || cap < 0 || (cap > 0 && !out)) DV_FAIL("dv_est_get_landmarks: bad argument");
    const dv_estimator& E = *ctx->est;
    int k = 0;
    for (auto& l : E.lms) {
        if (k >= cap) break;
        dv_landmark& o = out[k++];
        std::memset(&o, 0, sizeof(o));
        o.id = l.id; o.start_frame = l.start; o.n_obs = (int)l.obs.size(); o.solve_flag = l.solve_flag; o.depth = l.depth;
        const d3 pw = mul(E.Rs[l.start], mul(E.ric[0], l.obs[0].pt * l.depth) + E.tic[0]) + E.Ps[l.start];      // body.CamToWorld(point * depth, start_frame)
        put3(o.p_w, pw);
        const bool base = o.n_obs >= 2 && l.start < kWin - 2;
        o.in_point_cloud = base && !(l.start > kWin * 3.0 / 4.0 || l.solve_flag != 1);
        o.in_margin_cloud = base && l.start == 0 && o.n_obs <= 2 && l.solve_flag == 1;
    }
    *n_out = k;
    return 0;
}
static int est_begin(dv_ctx* ctx, const dv_feat* feats, int n, double t, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats, const double* points, bool defer_dynamic = false) {
    if (!have_est(ctx, "dv_est_process")) return -1;
    dv_estimator& E = *ctx->est;
    if (E.begun) DV_FAIL("dv_est_process_begin: previous frame not collected (dv_est_process_end)");
    E.cur_time = t + E.td;
    { HostScope h(ctx, "h_imu"); if (E.cfg.use_imu && !E.add_imu_until(E.cur_time)) return 1; }       // "wait for imu" (estimator.cpp:1801-1805)
    { HostScope h(ctx, "h_process_begin"); if (E.process_image_begin(ctx, feats, n, t, insts, n_insts, inst_feats, points, defer_dynamic)) return -1; }
    E.begun = true;
    return 0;
}
// Estimator::IMUAvailable (estimator.h:128-133) at cur_time = t + td, as ProcessMeasurements tests it before it pops the frame (estimator.cpp:1800-1805)
int dv_est_imu_available(dv_ctx* ctx, double t) {
    if (!have_est(ctx, "dv_est_imu_available")) return -1;
    const dv_estimator& E = *ctx->est;
    if (!E.cfg.use_imu) return 1;
    return (!E.imu_buf.empty() && t + E.td <= E.imu_buf.back().first) ? 1 : 0;
}
static int check_insts(dv_ctx* ctx, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats, const double* points) {
    if (n_insts < 0 || (n_insts > 0 && !insts)) DV_FAIL("dv_est_process_dynamic: bad instance list");
    for (int i = 0; i < n_insts; ++i) {
        if (insts[i].n_feats < 0 || insts[i].n_points < 0 || (insts[i].n_feats > 0 && !inst_feats) || (insts[i].n_points > 0 && !points)) DV_FAIL("dv_est_process_dynamic: bad instance record");
    }
    return 0;
}
int dv_est_process_begin(dv_ctx* ctx, const dv_feat* feats, int n, double t) { return est_begin(ctx, feats, n, t, nullptr, 0, nullptr, nullptr); }
int dv_est_process_dynamic_begin(dv_ctx* ctx, const dv_feat* feats, int n, double t, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats, const double* points) {
    if (!ctx) return -1;
    if (ctx->est && !ctx->est->cfg.dynamic) DV_FAIL("dv_est_process_dynamic: the estimator was created with dynamic = 0");
    if (check_insts(ctx, insts, n_insts, inst_feats, points)) return -1;
    return est_begin(ctx, feats, n, t, insts, n_insts, inst_feats, points);
}
// three-phase form: the window solve is enqueued with the background features alone (_begin_ego); the frame's instances follow (_attach: the object branch, host
// bookkeeping + dv_obj_solve on the third stream) while it is in flight — whatever the caller does between the two calls (enqueueing the next frame's tracking,
// collecting the object tracker) no longer sits in front of the window solve
int dv_est_process_dynamic_begin_ego(dv_ctx* ctx, const dv_feat* feats, int n, double t) {
    if (!ctx) return -1;
    if (ctx->est && !ctx->est->cfg.dynamic) DV_FAIL("dv_est_process_dynamic: the estimator was created with dynamic = 0");
    return est_begin(ctx, feats, n, t, nullptr, 0, nullptr, nullptr, true);
}
int dv_est_process_dynamic_attach(dv_ctx* ctx, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats, const double* points) {
    if (!ctx) return -1;
    if (!ctx->est || !ctx->est->begun) DV_FAIL("dv_est_process_dynamic_attach: no frame in flight (dv_est_process_dynamic_begin_ego)");
    if (check_insts(ctx, insts, n_insts, inst_feats, points)) return -1;
    dv_estimator& E = *ctx->est;
    if (!E.dyn_deferred) return 0;                      // initialisation frame (processed synchronously, no object branch) or already attached
    E.dyn_deferred = false;
    return E.dynamic_branch(ctx, insts, n_insts, inst_feats, points) ? -1 : 0;
}
int dv_est_process_dynamic(dv_ctx* ctx, const dv_feat* feats, int n, double t, const dv_inst_obs* insts, int n_insts, const dv_feat* inst_feats, const double* points, dv_est_state* out) {
    const int rc = dv_est_process_dynamic_begin(ctx, feats, n, t, insts, n_insts, inst_feats, points);
    return rc ? rc : dv_est_process_end(ctx, out);
}
int dv_est_get_instances(dv_ctx* ctx, dv_inst_state* out, int cap, int* n_out, double* summary4) {
    if (!have_est(ctx, "dv_est_get_instances")) return -1;
    if (!n_out || cap < 0 || (cap > 0 && !out)) DV_FAIL("dv_est_get_instances: bad argument");
    dv_estimator& E = *ctx->est;
    E.flush_dyn_tail(ctx);
    int k = 0;
    for (auto& kv : E.im.insts) {
        if (k >= cap) break;
        const dvi::Inst& I = kv.second; dv_inst_state& o = out[k++];
        std::memset(&o, 0, sizeof(o));
        o.id = I.id; o.is_initial = I.is_initial; o.is_tracking = I.is_tracking; o.is_curr_visible = I.is_curr_visible; o.is_static = I.is_static; o.is_init_velocity = I.is_init_velocity;
        o.age = I.age; o.lost_number = I.lost_number; o.static_frame = I.static_frame; o.n_landmarks = (int)I.lms.size(); o.n_valid = I.valid_size(); o.triangle_num = I.triangle_num;
        for (int c = 0; c < 3; ++c) { o.dims[c] = I.dims[c]; o.vel_v[c] = get(I.vel_v, c); o.vel_a[c] = get(I.vel_a, c); }
        for (int i = 0; i <= kWin; ++i) { pack_pose(I.P[i], I.R[i], o.window[i]); o.time[i] = I.time[i]; }
    }
    *n_out = k;
    if (summary4) { summary4[0] = E.obj_last.iterations; summary4[1] = E.obj_last.termination; summary4[2] = E.obj_last.initial_cost; summary4[3] = E.obj_last.final_cost; }
    return 0;
}
int dv_est_get_static_instances(dv_ctx* ctx, uint32_t* ids, int cap, int* n_out) {
    if (!have_est(ctx, "dv_est_get_static_instances")) return -1;
    if (!n_out || cap < 0 || (cap > 0 && !ids)) DV_FAIL("dv_est_get_static_instances: bad argument");
    const std::vector<uint32_t>& v = ctx->est->im.static_out;
    const int n = std::min((int)v.size(), cap);
    for (int i = 0; i < n; ++i) ids[i] = v[i];
    *n_out = n;
    return 0;
}
int dv_est_process_end(dv_ctx* ctx, dv_est_state* out) {
    if (!have_est(ctx, "dv_est_process")) return -1;
    dv_estimator& E = *ctx->est;
    if (!E.begun) DV_FAIL("dv_est_process_end: no frame in flight");
    E.begun = false;
    { HostScope h(ctx, "h_process_end"); if (E.process_image_end(ctx)) return -1; }
    E.prev_time = E.cur_time;
    if (out) {
        std::memset(out, 0, sizeof(*out));
        out->frame = E.frame; out->nonlinear = E.nonlinear; out->margin_old = E.margin_old; out->n_landmarks = (int)E.lms.size(); out->n_long = E.long_count();
        out->iterations = E.last.iterations; out->initial_cost = E.last.initial_cost; out->final_cost = E.last.final_cost;
        for (int i = 0; i <= kWin; ++i) {
            double* p = out->window[i];
            pack_pose(E.Ps[i], E.Rs[i], p); put3(p + 7, E.Vs[i]); put3(p + 10, E.Bas[i]); put3(p + 13, E.Bgs[i]);
        }
    }
    return 0;
}
int dv_est_process(dv_ctx* ctx, const dv_feat* feats, int n, double t, dv_est_state* out) {
    const int rc = dv_est_process_begin(ctx, feats, n, t);
    return rc ? rc : dv_est_process_end(ctx, out);
}

}  // extern "C"

void dv_est_destroy_internal(dv_estimator* e) { delete e; }
