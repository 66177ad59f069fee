// be_marg_host.hip — host side of the marginalization (kernels: be_marg.hip, be_marg_eig.hip): which blocks take part and where they sit ("plan"), the kernels'
// arguments and launches, the new prior's header, the health scalars of the previous frame's marginalization, and the operator-level entry dv_marginalize.
#include <algorithm>
#include "be_host.h"

// ================================ marginalization: structure ("plan"), launch, new header ================================
// Which parameter blocks take part (MarginalizationInfo::addResidualBlockInfo) and where they sit in the dense system:
// dropped dims first, then the kept ones in canonical order (poses, speed-bias, ex0, ex1, td)  (M1).
// sel[0..nsel): landmarks of `lms` whose residual blocks take part (all of them anchored in frame 0).
int marg_plan(dv_ctx* ctx, MargPlan& pl, int mode, const dv_ba_prior* prior, const dv_ba_factor* fac, const dv_ba_lm* lms, const int* sel, int nsel, bool imu01) {
    pl = MargPlan();
    pl.mode = mode;
    for (int i = 0; i < BE_MARG_TAB_INTS; ++i) pl.tab[i] = -1;
    bool pose_in[BE_NF] = { false }, sb_in[BE_NF] = { false }, ex_in[2] = { false, false }, td_in = false;
    const bool has_prior = prior && prior->valid;
    if (has_prior) for (int b = 0; b < prior->nblocks; ++b) {
        const dv_ba_prior_block& pb = prior->blocks[b];
        if (pb.type == 0) pose_in[pb.idx] = true; else if (pb.type == 1) sb_in[pb.idx] = true; else if (pb.type == 2) ex_in[pb.idx] = true; else td_in = true;
    }
    pl.nimu = (mode == 0 && imu01) ? 1 : 0;
    pl.nsel = (mode == 0) ? nsel : 0;
    if (pl.nimu) { pose_in[0] = sb_in[0] = pose_in[1] = sb_in[1] = true; }
    for (int q = 0; q < pl.nsel; ++q) {
        const dv_ba_lm& L = lms[sel[q]];
        if (L.anchor != 0) DV_FAIL("dv_marginalize: only landmarks anchored in frame 0 take part (estimator.cpp:446)");
        pl.tab[BE_MT_SEL + q] = sel[q];
        for (int f = L.first; f < L.first + L.count; ++f) {
            const dv_ba_factor& ff = fac[f];
            ex_in[0] = true; td_in = true;
            if (ff.kind != 0) ex_in[1] = true;
            if (ff.kind != 2) { pose_in[0] = true; pose_in[ff.fj] = true; }
        }
    }
    int32_t* dim_slot = pl.tab + BE_MT_SLOT; int32_t* dim_comp = pl.tab + BE_MT_COMP;
    int nd = 0;
    for (int k = 0; k < BE_NF; ++k) { pl.pose_dim[k] = -1; pl.sb_dim[k] = -1; }
    pl.ex_dim[0] = pl.ex_dim[1] = -1; pl.td_dim = -1;
    auto add_pose = [&](int k) { pl.pose_dim[k] = nd; for (int c = 0; c < 6; ++c) { dim_slot[nd] = k; dim_comp[nd] = c; ++nd; } };
    auto add_sb = [&](int k) { pl.sb_dim[k] = nd; for (int c = 0; c < 9; ++c) { dim_slot[nd] = -1; dim_comp[nd] = c; ++nd; } };
    const int drop_frame = (mode == 0) ? 0 : BE_WIN - 1;
    if (pose_in[drop_frame]) add_pose(drop_frame);
    if (mode == 0 && sb_in[0]) add_sb(0);
    pl.m = nd;
    if (pl.m == 0) { pl.empty = true; return 0; }             // "unstable tracking" (marginalization_factor.cpp:210-215)
    for (int k = 0; k < BE_NF; ++k) if (pose_in[k] && k != drop_frame) add_pose(k);
    for (int k = 0; k < BE_NF; ++k) if (sb_in[k] && !(mode == 0 && k == 0)) add_sb(k);
    for (int c = 0; c < 2; ++c) if (ex_in[c]) { pl.ex_dim[c] = nd; for (int q = 0; q < 6; ++q) { dim_slot[nd] = BE_NF + c; dim_comp[nd] = q; ++nd; } }
    if (td_in) { pl.td_dim = nd; dim_slot[nd] = BE_NF + 2; dim_comp[nd] = 0; ++nd; }
    pl.D = nd; pl.n = nd - pl.m;
    if (pl.n > BE_MAX_PRIOR || pl.n < 1 || nd > 256) DV_FAIL("dv_marginalize: bad kept size");
    // be_marg_finish holds the D x D system, A' and its workspace in LDS, in both forms: refused here, before anything is uploaded (6 dropped dims: n <= 89, 9: 88, 15: 85;
    // be_marg_eig's own 96 lies above all of them)
    if (be_marg_finish_smem(pl.D, pl.n) > BE_MARG_FINISH_LDS) {
        int nmax = pl.n;
        while (nmax > 1 && be_marg_finish_smem(pl.m + nmax, nmax) > BE_MARG_FINISH_LDS) --nmax;
        DV_FAIL("dv_marginalize: at most " + std::to_string(nmax) + " kept dims beside " + std::to_string(pl.m) + " dropped ones (the system and A' share " + std::to_string(BE_MARG_FINISH_LDS / 1024) +
                " KB of LDS), this prior has " + std::to_string(pl.n));
    }
    if (has_prior) for (int b = 0; b < prior->nblocks; ++b) {
        const dv_ba_prior_block& pb = prior->blocks[b];
        const int d0 = pb.type == 0 ? pl.pose_dim[pb.idx] : pb.type == 1 ? pl.sb_dim[pb.idx] : pb.type == 2 ? pl.ex_dim[pb.idx] : pl.td_dim;
        for (int k = 0; k < pb.size_local; ++k) pl.tab[BE_MT_PRIOR + pb.off + k] = d0 + k;
    }
    if (pl.nimu) {
        for (int k = 0; k < 6; ++k) { pl.tab[BE_MT_IMU + k] = pl.pose_dim[0] + k; pl.tab[BE_MT_IMU + 15 + k] = pl.pose_dim[1] + k; }
        for (int k = 0; k < 9; ++k) { pl.tab[BE_MT_IMU + 6 + k] = pl.sb_dim[0] + k; pl.tab[BE_MT_IMU + 21 + k] = pl.sb_dim[1] + k; }
    }
    return 0;
}

// the argument block of the three marginalization kernels; the index tables must already be (enqueued to be) in w.marg_tab
int marg_args(dv_ctx* ctx, const MargPlan& pl, const BeState* x, double g_norm, const double* priorA, const double* priorb, double* outA, double* outb, double* scal, double* c0_out, BeMargArgs& ma) {
    BeWork& w = ctx->be;
    ma = BeMargArgs{};
    ma.x = x; ma.nframes = BE_NF; ma.nlm = pl.nsel; ma.nimu = pl.nimu; ma.fac = w.fac; ma.lm = w.lm; ma.imu = w.imu;
    ma.prior = w.prior; ma.priorA = priorA; ma.priorb = priorb;
    ma.prior_map = w.marg_tab + BE_MT_PRIOR; ma.imu_map = w.marg_tab + BE_MT_IMU; ma.dim_slot = w.marg_tab + BE_MT_SLOT; ma.dim_comp = w.marg_tab + BE_MT_COMP;
    ma.lm_sel = w.marg_tab + BE_MT_SEL;
    ma.D = pl.D; ma.m = pl.m; ma.g_norm = g_norm; ma.outA = outA; ma.outb = outb; ma.out_scalars = scal; ma.c0_out = c0_out;
    const size_t slab = (size_t)pl.D * pl.D + pl.D;
    // sized once for BE_MAX_LM landmarks anchored in the oldest frame at the largest system (D = 178): growing it later would stall the stream
    const size_t nl = (size_t)std::max(pl.nsel, 1), nlmax = std::max(nl, (size_t)BE_MAX_LM), Dmax = (size_t)std::max(pl.D, 178);
    const size_t need = 8 * (nlmax * (size_t)be_marg_wstride((int)Dmax) + ((size_t)be_marg_chunks((int)nlmax) + 1) * be_marg_part() + Dmax * Dmax + Dmax + nlmax + 512);      // W | part | psum | sum | h | whitened IMU factor
    DV_CHECK(w.marg_buf.ensure(need));
    ma.W = (double*)w.marg_buf.p; ma.part = ma.W + nl * be_marg_wstride(pl.D); ma.psum = ma.part + (size_t)be_marg_chunks((int)nl) * be_marg_part(); ma.sum = ma.psum + be_marg_part();
    ma.lm_h = ma.sum + slab; ma.imu_w = ma.lm_h + nl; ma.anchor = 0;
    for (int k = 0; k < BE_NF; ++k) ma.pose_dim[k] = pl.pose_dim[k];
    ma.ex_dim[0] = pl.ex_dim[0]; ma.ex_dim[1] = pl.ex_dim[1]; ma.td_dim = pl.td_dim;
    ma.c0_mode = 0;
    {   // the finish kernel's factorisation on the matrix cores where the tiles fit (every window the estimator builds: D = 97, m = 15 -> 7 x 7 tiles)
        const int mt = (pl.m + 15) / 16, mf_n = 16 * mt + (pl.D - pl.m), NB = (mf_n + 16) >> 4;
        const size_t room = (size_t)pl.D * pl.D + pl.D + std::max((size_t)(pl.D - pl.m) * (pl.D - pl.m), (size_t)1024);      // A | b | W2 of the LDS image: the factor's fragments and the staged A', b' tiles take their place once the tiles are in registers
        ma.mf16 = 0; ma.mf_n = mf_n;
        if (pl.m > 0 && pl.D > pl.m && 2 * ((size_t)NB * (NB + 1) / 2 * 256) <= room && be_mf16_plan(mf_n, ma.mf_plan, false) && !std::getenv("DVINS_MARG_GENERIC")) ma.mf16 = 1;
    }
    return 0;
}
// launches the three kernels (DV_MARG_EIGEN: be_marg_finish leaves A', b' without c0, and be_marg_eig follows on the same stream)
int marg_enqueue(dv_ctx* ctx, const MargPlan& pl, const BeState* x, double g_norm, const double* priorA, const double* priorb, double* outA, double* outb, double* scal, double* c0_out, hipStream_t s) {
    BeWork& w = ctx->be;
    BeMargArgs ma;
    if (marg_args(ctx, pl, x, g_norm, priorA, priorb, outA, outb, scal, c0_out, ma)) return -1;
    const bool eig = w.marg_form == DV_MARG_EIGEN;
    ma.c0_mode = eig ? 1 : 0;
    {
        StageScope sc(ctx, "k_be_marg", s);
        const int rc = be_launch_marg(ma, s);
        if (rc == -2) DV_FAIL("dv_marginalize: system does not fit in LDS");
        if (rc) DV_FAIL("dv_marginalize: cannot set dynamic LDS size");
    }
    if (eig) {
        if (!w.eig_spec.p) DV_FAIL("dv_marginalize: DV_MARG_EIGEN without its spectrum buffer (dv_set_marg_form allocates it)");
        BeMargEigArgs ea{};
        ea.A = outA; ea.b = outb; ea.scal = scal; ea.c0_out = c0_out; ea.spec = (double*)w.eig_spec.p; ea.n = pl.n;
        StageScope sc(ctx, "k_be_marg_eig", s);
        const int rc = be_launch_marg_eig(ea, s);
        if (rc == -2) DV_FAIL("dv_marginalize: be_marg_eig holds at most 96 kept dims (marg_plan refuses what be_marg_finish cannot hold: fewer)");
        if (rc) DV_FAIL("dv_marginalize: cannot set dynamic LDS size of be_marg_eig");
        DV_CHECK(hipGetLastError());
        w.eig_ran = true;
    }
    return 0;
}

// new prior header: kept blocks, indices shifted like addr_shift (estimator.cpp:537-548 / 591-612); x0 = the states the system was linearised at
void marg_new_prior(const MargPlan& pl, const double* pose, const double* sb, const double* ex, const double* td, double c0, dv_ba_prior* out) {
    std::memset(out, 0, sizeof(*out));
    if (pl.empty) return;
    out->valid = 1; out->n = pl.n; out->c0 = c0;
    int nb = 0;
    auto put = [&](int type, int new_idx, int dim0, int size_local, const double* x0, int gs) {
        dv_ba_prior_block& pb = out->blocks[nb];
        pb.type = type; pb.idx = new_idx; pb.off = dim0 - pl.m; pb.size_local = size_local;
        for (int k = 0; k < gs; ++k) out->x0[nb][k] = x0[k];
        ++nb;
    };
    auto shift = [&](int k) { return pl.mode == 0 ? k - 1 : (k == BE_WIN ? BE_WIN - 1 : k); };
    for (int k = 0; k < BE_NF; ++k) if (pl.pose_dim[k] >= pl.m) put(0, shift(k), pl.pose_dim[k], 6, pose + 7 * k, 7);
    for (int k = 0; k < BE_NF; ++k) if (pl.sb_dim[k] >= pl.m) put(1, shift(k), pl.sb_dim[k], 9, sb + 9 * k, 9);
    for (int c = 0; c < 2; ++c) if (pl.ex_dim[c] >= 0) put(2, c, pl.ex_dim[c], 6, ex + 7 * c, 7);
    if (pl.td_dim >= 0) put(3, 0, pl.td_dim, 1, td, 1);
    out->nblocks = nb;
}

// the marginalization enqueued by the PREVIOUS frame reports its health here (its 4 scalars were downloaded behind it)
int be_check_prev_marg(dv_ctx* ctx, BePending& pd) {
    if (!pd.marg_check_due) return 0;
    pd.marg_check_due = false;
    const double* hscal = be_download(ctx->be)->marg_scal[pd.check_slot];
    // hscal[2] != 0: a pivot of A_mm was <= 1e-8 and was skipped on the device (pseudo-inverse, as the reference's eigen clamp does,
    // marginalization_factor.cpp:286-289).  The prior stays finite and usable, so the frame is never aborted half-way; the event is only counted.
    if (hscal[2] != 0.0) ctx->be.marg_clamped++;
    std::memcpy(ctx->be.marg_last, hscal, 32); ctx->be.marg_checked++;
    if (hscal[3] < 0.0) DV_FAIL("marginalization (DV_MARG_EIGEN): the Jacobi eigen-decomposition of A' did not converge in 30 sweeps");
    return 0;
}

extern "C" {

int dv_set_marg_form(dv_ctx* ctx, int form) {
    if (!ctx) return -1;
    if (form != DV_MARG_INFO && form != DV_MARG_EIGEN) DV_FAIL("dv_set_marg_form: form must be DV_MARG_INFO (0) or DV_MARG_EIGEN (1)");
    if (ctx->be.pend->active) DV_FAIL("dv_set_marg_form: a solve or marginalization is in flight on this ctx");
    if (ctx->batch) DV_FAIL("dv_set_marg_form: this ctx is a dv_batch member; batched groups marginalize in DV_MARG_INFO form only");
    if (form == DV_MARG_EIGEN && !ctx->be.eig_spec.p) {
        DV_CHECK(hipSetDevice(ctx->cfg.device));
        DV_CHECK(ctx->be.eig_spec.ensure(8 * 128));
        DV_CHECK(hipMemset(ctx->be.eig_spec.p, 0, 8 * 128));
    }
    ctx->be.marg_form = form;
    return 0;
}
int dv_get_marg_form(dv_ctx* ctx, int* form) {
    if (!ctx) return -1;
    if (!form) DV_FAIL("dv_get_marg_form: null argument");
    *form = ctx->be.marg_form;
    return 0;
}
int dv_marg_last_spectrum(dv_ctx* ctx, double* ev, int cap, int* n, int* sweeps) {
    if (!ctx) return -1;
    BeWork& w = ctx->be;
    if (!w.eig_ran) DV_FAIL("dv_marg_last_spectrum: no DV_MARG_EIGEN marginalization has run on this ctx");
    double spec[128];
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(hipStreamSynchronize(ctx->be_stream));
    DV_CHECK(hipMemcpy(spec, w.eig_spec.p, sizeof(spec), hipMemcpyDeviceToHost));
    const int nn = (int)spec[97];
    if (ev && cap < nn) DV_FAIL("dv_marg_last_spectrum: cap is smaller than n = " + std::to_string(nn));
    if (ev) std::memcpy(ev, spec, 8 * (size_t)nn);
    if (n) *n = nn;
    if (sweeps) *sweeps = (int)spec[96];
    return 0;
}
int dv_est_get_marg_health(dv_ctx* ctx, long long* checked, long long* clamped, double* last4) {
    if (!ctx) return -1;
    if (checked) *checked = ctx->be.marg_checked;
    if (clamped) *clamped = ctx->be.marg_clamped;
    if (last4) std::memcpy(last4, ctx->be.marg_last, 32);
    return 0;
}

int dv_marginalize(dv_ctx* ctx, const dv_ba_problem* P, int mode, dv_ba_prior* out_prior, double* out_A, double* out_b, double* diag4) {
    if (!ctx) return -1;
    if (!P || !out_prior || !out_A || !out_b) DV_FAIL("dv_marginalize: null argument");
    if (ctx->be.pend->active) DV_FAIL("dv_marginalize: a solve is in flight on this ctx");
    if (ctx->est && ctx->be.prior_resident) DV_FAIL("dv_marginalize: this ctx's estimator holds a device-resident prior; use a separate ctx for operator-level calls");
    if (mode != 0 && mode != 1) DV_FAIL("dv_marginalize: mode must be 0 (kMarginOld) or 1 (kMarginSecondNew)");
    if (P->nframes != BE_NF) DV_FAIL("dv_marginalize: needs a full window (frame == kWinSize)");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (be_ensure(ctx, P->nfac)) return -1;
    BeWork& w = ctx->be;
    hipStream_t s = ctx->be_stream;
    const bool has_prior = P->prior && P->prior->valid;
    std::memset(out_prior, 0, sizeof(*out_prior));
    const int nimu = (mode == 0) ? P->nimu : 0, nlm = (mode == 0) ? P->nlm : 0, nfac = (mode == 0) ? P->nfac : 0;
    if (nimu > 1) DV_FAIL("dv_marginalize: at most the IMU factor (0,1)");
    for (int f = 0; f < nfac; ++f) if (P->factors[f].fi != 0) DV_FAIL("dv_marginalize: only landmarks anchored in frame 0 take part (estimator.cpp:446)");
    static thread_local MargPlan pl;
    std::vector<int> sel(nlm);
    for (int l = 0; l < nlm; ++l) sel[l] = l;
    if (marg_plan(ctx, pl, mode, has_prior ? P->prior : nullptr, P->factors, P->landmarks, sel.data(), nlm, nimu == 1)) return -1;
    if (pl.empty) { out_prior->valid = 0; if (diag4) diag4[0] = diag4[1] = diag4[2] = diag4[3] = 0; return 0; }
    const int n = pl.n;
    // ---- upload (pinned mirror of the upload region, one copy) ----
    uint8_t* hp = (uint8_t*)w.pinned;
    BeState* hx = (BeState*)(hp + w.up_x);
    int max_lm = 0;
    for (int f = 0; f < nfac; ++f) max_lm = std::max(max_lm, P->factors[f].lm + 1);
    if (max_lm > BE_MAX_LM) DV_FAIL("dv_marginalize: landmark index out of range");
    be_stage_state(hx, P, max_lm);      // (every inverse depth a factor names, not nlm of them)
    BeImu* himu = (BeImu*)(hp + w.up_imu);
    if (nimu == 1 && be_fill_imu(P->imu[0], himu[0], nullptr)) DV_FAIL("dv_marginalize: IMU covariance is singular");
    BePriorHdr ph{};
    if (has_prior) std::memcpy(&ph, P->prior, sizeof(ph));
    std::memcpy(hp + w.up_prior, &ph, sizeof(ph));
    std::memcpy(hp + w.up_mt, pl.tab, sizeof(pl.tab));
    if (nlm) std::memcpy(hp + w.up_lm, P->landmarks, sizeof(BeLm) * (size_t)nlm);
    if (nfac) std::memcpy(hp + w.up_fac, P->factors, sizeof(BeFactor) * (size_t)nfac);
    DV_CHECK(hipMemcpyAsync(w.block.p, hp, w.up_fac + sizeof(BeFactor) * (size_t)nfac, hipMemcpyHostToDevice, s));
    if (has_prior) {
        DV_CHECK(hipMemcpyAsync(w.priorA_buf[w.prior_cur], P->prior_A, 8 * (size_t)ph.n * ph.n, hipMemcpyHostToDevice, s));
        DV_CHECK(hipMemcpyAsync(w.priorb_buf[w.prior_cur], P->prior_b, 8 * (size_t)ph.n, hipMemcpyHostToDevice, s));
        w.prior_resident = false;
    }
    double* d_outA = w.Sc[0]; double* d_outb = w.gvec[0]; double* d_scal = w.marg_scal;      // Sc / gvec are idle outside a solve
    if (marg_enqueue(ctx, pl, w.x, P->g_norm, w.priorA_buf[w.prior_cur], w.priorb_buf[w.prior_cur], d_outA, d_outb, d_scal, nullptr, s)) return -1;
    DV_CHECK(hipGetLastError());
    double scal[4];
    DV_CHECK(hipMemcpyAsync(out_A, d_outA, 8 * (size_t)n * n, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipMemcpyAsync(out_b, d_outb, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipMemcpyAsync(scal, d_scal, 32, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    if (ctx->timing) dv_harvest_timers(ctx, s);
    if (diag4) std::memcpy(diag4, scal, 32);
    std::memcpy(w.marg_last, scal, 32); w.marg_checked++;
    if (scal[3] < 0.0) DV_FAIL("dv_marginalize: DV_MARG_EIGEN: the Jacobi eigen-decomposition of A' did not converge in 30 sweeps");
    if (scal[2] != 0.0) w.marg_clamped++;          // pivots <= 1e-8 skipped on the device (pseudo-inverse like the reference's eigen clamp); reported through diag4[2]
    marg_new_prior(pl, P->pose, P->speed_bias, P->ex_pose, P->td, scal[0], out_prior);
    return 0;
}

}  // extern "C"
