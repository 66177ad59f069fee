// be_solve_body.inc — the body of be_solve_kernel, textually included by its two entry forms (be_solve.hip): kernel arguments by value (one window) and an
// argument table in HBM (dv_batch).  `a` (BeSolveArgs, value or reference) and `spec` are in scope.  Not a translation unit.
    extern __shared__ __attribute__((aligned(16))) double sm[];
    BeCtl* ctl = a.ctl;
    BeCtl c = *ctl;
    const int n = a.dims.nstate, nlm = a.dims.nlm, tid = threadIdx.x;
    // SHARD (be_solve_shard_kernel: one window sharded by landmark): this workgroup back-substitutes, norms and moves the landmarks [lm0, lm0 + nown) only; every sum over ALL
    // landmarks comes from the rank-ordered form coefficients qf (be_kernels.h) — identical bits on every rank
    const int lm0 = SHARD ? a.sh.lo : 0, nown = SHARD ? a.sh.hi - a.sh.lo : nlm;
    if (c.done) return;
    // column tables in LDS: a lane-dependent index into the kernel arguments is a memory load with a ~1 us round trip, paid on the critical path of every
    // phase that asked (the gathers of the pose entries, the candidate)
    __shared__ int s_pcol[BE_NF], s_scol[BE_NF];
    if (tid < BE_NF) { s_pcol[tid] = tid < a.dims.nframes ? a.dims.pose_col[tid] : -1; s_scol[tid] = tid < a.dims.nframes ? a.dims.sb_col[tid] : -1; }
    // free extrinsic / td blocks (be_kernels.h BeExt; the generic factorisation only — the MF16 kernels compile none of it): the columns of the 13 ext entries, and the ext
    // entries of whatever vector the landmarks' coupling rows are multiplied with (qx beside q66)
    __shared__ int s_xcol[MF16 ? 1 : 16]; __shared__ double qx[MF16 ? 1 : 16];
    bool xt_on = false;
    if constexpr (!MF16) { xt_on = a.xt.on != 0; if (tid >= 64 && tid < 80) s_xcol[tid - 64] = (xt_on && tid - 64 < BE_NX) ? a.xt.xcol[tid - 64] : -1; }
    TS(15);
    // MF16: what the factorisation and the scaling phase read of the linearisation is requested BEFORE the accept decision below (a block reduction over the candidate
    // costs, ~1.5 us): the candidate's set (cur ^ 1) when a decision is pending — nearly every step of a tracking window is accepted; after a rejection the kept
    // factorisation is reused and nothing of this is consumed — else the set of x.  The loads' round trip then runs beside the decision instead of behind it.
    const int cur_spec = (spec && c.pending) ? (c.cur ^ 1) : c.cur;
    // (the candidate costs of the decision are requested FIRST: loads return in order, and the decision must not wait behind the 24 loads of the prefetch)
    double dec_cv[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (MF16 && spec && c.pending && tid < 256) {
        const int ncost0 = nlm + a.dims.nimu + 1;
#pragma unroll
        for (int u = 0; u < 4; ++u) dec_cv[u] = a.cand_cost[tid + 256 * u < ncost0 ? tid + 256 * u : 0];
    }
    mf_d4 mfU[MF_SLOTS];
    double pre_h = 0.0, pre_g0 = 0.0, pre_g1 = 0.0, pre_s = 0.0;      // this thread's column of the scaling phase (n <= 175 < SOL_THREADS)
    if (MF16 && !(c.reuse && !(spec && c.pending))) {
        mf_prefetch(a.Sc[cur_spec], reinterpret_cast<const uint8_t*>(a.ldl_col0), n, mfU);
        if (tid < n) { pre_h = a.Hd[cur_spec][(size_t)tid * n + tid]; pre_g0 = a.gvec[cur_spec][tid]; pre_g1 = a.gvec[cur_spec][n + tid]; pre_s = a.scale_p[tid]; }
    }
    if (spec && c.pending) {
        // ---- decision on the candidate of the previous slot: be_accept_kernel's rule, taken here because the candidate's linearisation
        // (set cur ^ 1) is already in place.  Every thread evaluates the same scalars; thread 0 publishes the control block. ----
        __shared__ double red4[4];
        const int ncost = nlm + a.dims.nimu + 1;
        double part = 0;
        if (tid < 256) {      // the summation tree of be_accept_kernel, bit for bit: <= 4 costs per thread, requested together, added in index order
            double cv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cv[u] = MF16 ? dec_cv[u] : a.cand_cost[tid + 256 * u < ncost ? tid + 256 * u : 0];
#pragma unroll
            for (int u = 0; u < 4; ++u) if (tid + 256 * u < ncost) part += cv[u];
        }
        part = wave_sum_f64(part);
        if (tid < 256 && (tid & 63) == 0) red4[tid >> 6] = part;
        lds_barrier();
        const double cand_cost = red4[0] + red4[1] + red4[2] + red4[3];
        c.slots += 1; c.iter += 1; c.cand_cost = cand_cost; c.invalid = 0; c.pending = 0;
        bool done = false, accept = false; int term = 0;
        if (c.step_norm <= 1e-8 * (c.x_norm + 1e-8)) { done = true; term = 1; }                       // parameter tolerance
        else if (fabs(c.x_cost - cand_cost) <= 1e-6 * c.x_cost) { done = true; term = 1; }           // function tolerance
        else {
            const double rel = (c.x_cost - cand_cost) / c.model_cost_change;
            if (rel > 1e-3) {
                accept = true;
                double radius = c.radius;
                if (rel < 0.25) radius *= 0.5;
                if (rel > 0.75) radius = fmax(radius, 3.0 * c.dogleg_norm);
                c.radius = radius; c.mu = fmax(1e-8, 2.0 * c.mu / 10.0);
                c.x_cost = cand_cost; c.successful += 1; c.reuse = 0; c.need_eval = 0; c.cur ^= 1;      // the candidate's set becomes x's
            } else {
                c.radius = c.radius * 0.5; c.reuse = 1; c.need_eval = 0;
                if (c.radius < 1e-32) { done = true; term = 1; }
            }
            if (!done && c.iter >= c.max_iters) { done = true; term = 0; }
        }
        if (accept) {
            double* dst = reinterpret_cast<double*>(a.x);
            const double* src = reinterpret_cast<const double*>(a.cand);
            const int used = (int)(offsetof(BeState, inv_depth) / sizeof(double)) + nlm;
            for (int k = tid; k < used; k += SOL_THREADS) dst[k] = src[k];
        }
        if (done) { c.done = 1; c.termination = term; }
        if (tid == 0) *ctl = c;
        if (done) return;
        lds_barrier();            // (x is re-read only behind the factorisation, whose workgroup barriers order the copy's stores before those loads)
    }
    const int mf_nb = (n + 16) >> 4;
    // MF16: the tile region (the factor as MFMA fragments) takes the place of the packed factor; it is dead after the back substitution and then serves as `scratch`
    const int npk = MF16 ? (mf_nb * (mf_nb + 1) / 2 * 256 > 3072 ? mf_nb * (mf_nb + 1) / 2 * 256 : 3072) : n * (n + 1) / 2;
    double* Lm = sm;                                   // npk: unit-lower factor, packed row-major
    double* v_s = Lm + npk;                            // scale
    double* v_d = v_s + n;                             // diag
    double* v_grad = v_d + n;
    double* v_gn = v_grad + n;
    double* v_t = v_gn + n;                            // u_p / s.y / delta_p
    double* v_t2 = v_t + n;                            // H * v_t
    double* v_x = v_t2 + n;                            // back-substitution vector
    double* zfin = v_x + n;                            // L^-1 rhs
    double* dvec = zfin + n;                           // D
    double* q66 = dvec + n;                            // 66 (+6 pad): v_t gathered into packet (frame, comp) order
    double* red = q66 + 72;                            // 80: block-sum exchange (16 per value)
    double* misc = red + 80;                           // 8: [0] alpha
    double* scratch = MF16 ? Lm : misc + 8;            // 3072: gemv partial sums, aliased with the LDL^T panel buffers (two alternating sets in the wave-column form)
    MfLds mf; mf.Tl = Lm; mf.gat = misc + 8; mf.dv = mf.gat + 1024; mf.iv = mf.dv + 16 * mf_nb; mf.yv = mf.iv + 16 * mf_nb;      // (MF16 only)
    double* PL = scratch, *PD = scratch + 4 * 184;     // panel of L and of L D, [row][4]
    double* dinfo = red;                               // 2 x 16 (red[] is idle during the factorisation)
    __shared__ int s_fail;
    const double mu = c.mu;
    const double* pk = a.packets[c.cur];
    const double* const xpk = MF16 ? nullptr : a.xt.xpk[c.cur];
    const double* const Hd = a.Hd[c.cur]; const double* const gvec = a.gvec[c.cur];
    const double* const imu_out = a.imu_out[c.cur]; const double* const prior_out = a.prior_out[c.cur];
    auto gather66 = [&](const double* v) {             // q66[a*6+r] = v[pose_col[a] + r] (0 for constant / absent poses)
        if (tid < 66) { const int fa = tid / 6, r = tid - fa * 6; const int col = s_pcol[fa]; q66[tid] = col >= 0 ? v[col + r] : 0.0; }
        if constexpr (!MF16) { if (xt_on && tid >= 128 && tid < 128 + BE_NX) { const int col = s_xcol[tid - 128]; qx[tid - 128] = col >= 0 ? v[col] : 0.0; } }
        lds_barrier();
    };
    auto xdot = [&](int l) {                           // the ext entries' share of w_l . v (landmark l of the window)
        double s0 = 0;
        if constexpr (!MF16) { for (int q = 0; q < BE_NX; ++q) s0 += BE_PK(xpk, BX_W + q, l) * qx[q]; }
        return s0;
    };
    // wd[l] = w_l . q66 for every landmark: the 66 terms are split over npart thread groups (lane = landmark, so the
    // packet reads stay coalesced); partial sums meet in LDS and are added in a fixed order.  Result in scratch[l].
    const int nlm_pad = (nown + 63) & ~63;
    const int npart = nlm_pad * 6 <= SOL_THREADS ? 6 : (nlm_pad * 3 <= SOL_THREADS ? 3 : (nlm_pad * 2 <= SOL_THREADS ? 2 : 1));
    auto wdot_all = [&]() {
        const int per = 66 / npart;
        if (npart > 1) {
            const int part = tid / nlm_pad, l = tid - part * nlm_pad;
            if (part < npart && l < nown) {
                double s0 = 0;
                const int q0 = part * per;
#pragma unroll 11
                for (int q = 0; q < per; ++q) s0 += BE_PK(pk, BE_PK_W + q0 + q, lm0 + l) * q66[q0 + q];
                if constexpr (!MF16) { if (xt_on && part == 0) s0 += xdot(lm0 + l); }
                scratch[part * nlm_pad + l] = s0;
            }
            lds_barrier();
            if (tid < nown) { double s0 = scratch[tid]; for (int p = 1; p < npart; ++p) s0 += scratch[p * nlm_pad + tid]; scratch[tid] = s0; }
        } else {
            for (int l = tid; l < nown; l += SOL_THREADS) {
                double s0 = 0;
#pragma unroll 11
                for (int q = 0; q < 66; ++q) s0 += BE_PK(pk, BE_PK_W + q, lm0 + l) * q66[q];
                if constexpr (!MF16) { if (xt_on) s0 += xdot(lm0 + l); }
                scratch[l] = s0;
            }
        }
        lds_barrier();
    };
    const double* wd = scratch;
    TS(0);
    // this thread's landmark (l = tid: BE_MAX_LM <= SOL_THREADS).  Its scalars stay in registers from the phase that produces them to the end of the kernel:
    // every phase that re-read them from HBM paid a dependent ~1 us round trip
    const bool lm_live = tid < nown;
    const int lmi = lm0 + tid;                         // this thread's landmark
    double lm_h = 0, lm_g = 0, lm_scale = 1, lm_diag = 1, lm_grad = 0, lm_gn = 0, lm_wgn = 0;      // lm_wgn = w_l . (s_p y_p) of the Gauss-Newton step
    auto lm_diag_own = [&]() {
        if (lm_live) {
            const double h = BE_PK(pk, BE_PK_H, lmi), gl = BE_PK(pk, BE_PK_G, lmi), s = a.scale_l[lmi];
            double d2 = h * s * s; d2 = fmin(fmax(d2, 1e-6), 1e32);
            const double d = sqrt(d2);
            a.diag_l[lmi] = d; a.grad_l[lmi] = gl * s / d;
            lm_h = h; lm_g = gl; lm_scale = s; lm_diag = d; lm_grad = gl * s / d;
        }
    };
    const double* const qfc = SHARD ? a.sh.qf[c.cur] : nullptr;      // (c.cur after the accept decision above: the set of x)
    // work that does not feed the factorisation, for threads that would otherwise wait (t = index among the nt participating threads); reduced per wave
    // into red[wave] / red[16 + wave] and combined behind the back substitution's closing barrier
    auto side_sums = [&](int t, int nt, bool warm_up) {
        double part = 0, gm = 0;
        {
        if (c.first) {        // x_cost: fixed-order sum of the per-block costs at x
            if (!SHARD) for (int l = t; l < nlm; l += nt) part += BE_PK(pk, BE_PK_COST, l);
            for (int k = t; k < a.dims.nimu; k += nt) part += imu_out[(size_t)k * IMU_OUT_STRIDE];
            if (t == 0) part += prior_out[0];
            if (SHARD && t == 0) part += qfc[BE_QF_A + 10];
        }
        // gradient tolerance (trust_region_minimizer.cc: gradient_max_norm <= gradient_tolerance = 1e-10), checked on every new gradient
        for (int i = t; i < n; i += nt) gm = fmax(gm, fabs(gvec[i]));
        if (!SHARD) for (int l = t; l < nlm; l += nt) gm = fmax(gm, fabs(BE_PK(pk, BE_PK_G, l)));
        else if (t == 0) gm = fmax(gm, qfc[BE_QF_A + 11]);
        }
        lm_diag_own();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { gm = fmax(gm, __shfl_xor(gm, o)); part += __shfl_xor(part, o); }
        if ((tid & 63) == 0) { red[tid >> 6] = gm; red[16 + (tid >> 6)] = part; }
        if (warm_up) {
        double warm = 0.0;
        const int lpr = (nlm + 15) >> 4;                                   // lines per packet row
        for (int e = t; e < 66 * lpr; e += nt) { const int q = e / lpr, l16 = e - q * lpr; warm += __builtin_nontemporal_load(&BE_PK(pk, BE_PK_W + q, l16 * 16)); }
        for (int e = t; e < (n * n + 15) >> 4; e += nt) warm += __builtin_nontemporal_load(Hd + (size_t)e * 16);
        const int nst = ((int)(offsetof(BeState, inv_depth) / sizeof(double)) + nlm + 15) >> 4;
        for (int e = t; e < nst; e += nt) warm += __builtin_nontemporal_load(reinterpret_cast<const double*>(a.x) + (size_t)e * 16);
        if (warm == 1.2345e-300) misc[6] = warm;
        }
    };
    if (!c.reuse) {
        // ---------------- scaling, diagonal, gradient ----------------
        for (int i = tid; i < n; i += SOL_THREADS) {
            const bool pre = MF16 && cur_spec == c.cur;          // (always, when this branch runs: the speculation only misses on a rejection, which takes the reuse branch)
            const double hii = pre ? pre_h : Hd[(size_t)i * n + i];
            const double s = c.first ? 1.0 / (1.0 + sqrt(hii)) : (pre ? pre_s : a.scale_p[i]);
            double d2 = hii * s * s; d2 = fmin(fmax(d2, 1e-6), 1e32);
            const double d = sqrt(d2);
            const double g0 = pre ? pre_g0 : gvec[i];
            v_s[i] = s; v_d[i] = d; v_grad[i] = g0 * s / d;
            v_x[i] = g0 - (pre ? pre_g1 : gvec[n + i]);          // right-hand side of the reduced system (unscaled), for the factorisation's forward substitution: fetched here, in the round trip of this phase
            // (MF16: these three stores leave AFTER the back substitution — an outstanding store holds the vmcnt wait that guards the prefetched tiles' first use)
            if (!MF16) { if (c.first) a.scale_p[i] = s; a.diag_p[i] = d; a.grad_p[i] = v_grad[i]; }
        }
        lds_barrier();
        // cost at x, gradient tolerance and the landmark part of the diagonal: none of it feeds the factorisation, so the wave-column form runs it BEHIND the
        // factorisation (the prefetched blocks need not stay in registers across three block reductions)
        auto cost_and_tolerance = [&]() -> bool {
            if (c.first) {        // x_cost: fixed-order sum of the per-block costs at x
                double part = 0;
                if (!SHARD) for (int l = tid; l < nlm; l += SOL_THREADS) part += BE_PK(pk, BE_PK_COST, l);
                for (int k = tid; k < a.dims.nimu; k += SOL_THREADS) part += imu_out[(size_t)k * IMU_OUT_STRIDE];
                if (tid == 0) part += prior_out[0];
                if (SHARD && tid == 0) part += qfc[BE_QF_A + 10];
                const double xc = block_sum(part, red);
                if (tid == 0) { ctl->x_cost = xc; ctl->initial_cost = xc; }
            }
            // gradient tolerance (trust_region_minimizer.cc: gradient_max_norm <= gradient_tolerance = 1e-10), checked on every new gradient
            {
                double gm = 0;
                for (int i = tid; i < n; i += SOL_THREADS) gm = fmax(gm, fabs(gvec[i]));
                if (!SHARD) for (int l = tid; l < nlm; l += SOL_THREADS) gm = fmax(gm, fabs(BE_PK(pk, BE_PK_G, l)));
                else if (tid == 0) gm = fmax(gm, qfc[BE_QF_A + 11]);
    #pragma unroll
                for (int o = 32; o > 0; o >>= 1) gm = fmax(gm, __shfl_xor(gm, o));
                __syncthreads();
                if ((tid & 63) == 0) red[tid >> 6] = gm;
                __syncthreads();
                gm = 0; for (int k = 0; k < SOL_THREADS / 64; ++k) gm = fmax(gm, red[k]);
                __syncthreads();
                if (gm <= 1e-10) { if (tid == 0) { ctl->done = 1; ctl->termination = 1; ctl->first = 0; } return true; }
            }
            TS(1);
            // landmark part of the diagonal and of the scaled gradient (the Cauchy point itself is computed lazily, see below)
            if (lm_live) {
                const int l = lmi;
                const double h = BE_PK(pk, BE_PK_H, l), gl = BE_PK(pk, BE_PK_G, l), s = a.scale_l[l];
                double d2 = h * s * s; d2 = fmin(fmax(d2, 1e-6), 1e32);
                const double d = sqrt(d2);
                a.diag_l[l] = d; a.grad_l[l] = gl * s / d;
                lm_h = h; lm_g = gl; lm_scale = s; lm_diag = d; lm_grad = gl * s / d;
            }
            return false;
        };
        if (!MF16) { if (cost_and_tolerance()) return; }      // (MF16: beside the first diagonal tile, below — the sums only, one round trip; with the L2 warm-up loads, inside the
                                                                         // loop or in the prefetch's round trip they cost more than they hid: spilled registers, a longer prologue — DESIGN.md)
        TS(3);
        // ---------------- Gauss-Newton step: LDL^T of the Schur complement ----------------
        bool ok_f;
        if (MF16) ok_f = ldlt_mf16<MF_DF>(mfU, reinterpret_cast<const uint8_t*>(a.ldl_col0), n, mu, v_s, v_d, v_x, mf, &s_fail, [&](int excl) { side_sums(tid < 64 * excl ? tid : tid - 64, SOL_THREADS - 64, false); },
                                   [&]() { lm_diag_own(); if ((tid & 63) == 0) { red[tid >> 6] = 0.0; red[16 + (tid >> 6)] = 0.0; } });
        else ok_f = ldlt_blocked<NSLOT>(a.Sc[c.cur], gvec, n, mu, v_s, v_d, Lm, PL, PD, dinfo, zfin, dvec, &s_fail);
        if (!ok_f) {
            if (MF16) { if (cost_and_tolerance()) return; }      // (MF16 takes these checks beside the factorisation's first tile; a failed factorisation never reaches the sums behind the back substitution)
            // Ceres: LINEAR_SOLVER_FAILURE -> mu *= 10 and retry (dogleg_strategy.cc ComputeGaussNewtonStep)
            if (tid == 0) {
                ctl->mu = mu * 10.0; ctl->chol_fail = 1; ctl->first = 0; ctl->alpha_valid = 0;
                ctl->slots = c.slots + 1; ctl->reuse = 0; ctl->need_eval = 0; ctl->pending = 0;      // the slot is spent; the next reduce rebuilds Sc with the larger mu
                if (mu * 10.0 > 1.0) { ctl->done = 1; ctl->termination = 2; }
            }
            return;
        }
        TS(6);
        // back substitution L^T x = D^-1 z on ONE wave with x distributed over lanes (3 registers cover n <= 192):
        // the pivot is broadcast with v_readlane, row k-1 of L is prefetched from LDS while row k is applied.
        if (MF16) bs_mf16(reinterpret_cast<const uint8_t*>(a.ldl_col0), n, mf, v_x);
        else if ((tid >> 6) == 0) {
            __builtin_amdgcn_s_setprio(3);
            const int lane = tid & 63, nn = n;
            double x0 = lane < nn ? zfin[lane] / dvec[lane] : 0.0;
            double x1 = 64 + lane < nn ? zfin[64 + lane] / dvec[64 + lane] : 0.0;
            double x2 = 128 + lane < nn ? zfin[128 + lane] / dvec[128 + lane] : 0.0;
            int k = nn - 1;
            for (; k >= 0 && ((k + 1) & 7); --k) bs_rows<1>(Lm, k, lane, x0, x1, x2);      // until the chunks are 8-aligned (a chunk never straddles a segment)
            if (k >= 128 + BS_R - 1) k = bs_segment<2, BS_R>(Lm, k, lane, x0, x1, x2);      // segment by segment, software-pipelined
            if (k >= 64 + BS_R - 1) k = bs_segment<1, BS_R>(Lm, k, lane, x0, x1, x2);
            if (k >= BS_R - 1) k = bs_segment<0, BS_R>(Lm, k, lane, x0, x1, x2);
            __builtin_amdgcn_s_setprio(0);
            if (lane < nn) v_x[lane] = x0;
            if (64 + lane < nn) v_x[64 + lane] = x1;
            if (128 + lane < nn) v_x[128 + lane] = x2;
        }
        lds_barrier();
        if (MF16) {
            double gm = 0, xc = 0;
            for (int k = 0; k < SOL_THREADS / 64; ++k) { gm = fmax(gm, red[k]); xc += red[16 + k]; }
            if (c.first && tid == 0) { ctl->x_cost = xc; ctl->initial_cost = xc; }
            if (gm <= 1e-10) { if (tid == 0) { ctl->done = 1; ctl->termination = 1; ctl->first = 0; } return; }
        }
        TS(24);
        if (MF16) for (int i = tid; i < n; i += SOL_THREADS) { if (c.first) a.scale_p[i] = v_s[i]; a.diag_p[i] = v_d[i]; a.grad_p[i] = v_grad[i]; }
        TS(7);
        for (int i = tid; i < n; i += SOL_THREADS) { v_gn[i] = -v_d[i] * v_x[i]; a.gn_p[i] = v_gn[i]; v_t[i] = v_s[i] * v_x[i]; }   // v_t = s_p . y_p
        lds_barrier();
        gather66(v_t);
        wdot_all();
        if (lm_live) {
            const double rho = 1.0 / (lm_h + mu * lm_diag * lm_diag / (lm_scale * lm_scale));
            lm_wgn = wd[tid];
            const double yl = rho / lm_scale * (lm_g - lm_wgn);
            lm_gn = -lm_diag * yl;
            a.gn_l[lmi] = lm_gn;
        }
        lds_barrier();
    } else {
        for (int i = tid; i < n; i += SOL_THREADS) { v_s[i] = a.scale_p[i]; v_d[i] = a.diag_p[i]; v_grad[i] = a.grad_p[i]; v_gn[i] = a.gn_p[i]; }
        if (lm_live) { lm_h = BE_PK(pk, BE_PK_H, lmi); lm_g = BE_PK(pk, BE_PK_G, lmi); lm_scale = a.scale_l[lmi]; lm_diag = a.diag_l[lmi]; lm_grad = a.grad_l[lmi]; lm_gn = a.gn_l[lmi]; }
        __syncthreads();
    }
    TS(8);
    // ---------------- traditional dogleg (dogleg_strategy.cc ComputeTraditionalDoglegStep) ----------------
    double p_gg = 0, p_nn = 0, p_gn = 0;
    for (int i = tid; i < n; i += SOL_THREADS) { p_gg += v_grad[i] * v_grad[i]; p_nn += v_gn[i] * v_gn[i]; p_gn += v_grad[i] * v_gn[i]; }
    if (!SHARD && lm_live) { p_gg += lm_grad * lm_grad; p_nn += lm_gn * lm_gn; p_gn += lm_grad * lm_gn; }
    // SHARD: the landmark parts as forms in v = s_p y_p = -(s_p / d_p) gn_p, gathered into the 66-space (vq): nine sums over the 66 x 66 images / the vectors, one exchange
    double f_Q2 = 0, f_Q6 = 0, f_Q9 = 0, f_L2 = 0, f_LGS = 0, f_L5 = 0, f_L6 = 0, f_L8 = 0, f_L9 = 0;
    __shared__ double vq[SHARD ? 72 : 1];
    if (SHARD) {
        if (tid < 66) { const int fa = tid / 6, r = tid - fa * 6; const int col = s_pcol[fa]; vq[tid] = col >= 0 ? -(v_s[col + r] / v_d[col + r]) * v_gn[col + r] : 0.0; }
        lds_barrier();
        double q2 = 0, q6 = 0, q9 = 0;
        for (int e = tid; e < 4356; e += SOL_THREADS) { const int i = e / 66, j = e - i * 66; const double vv = vq[i] * vq[j]; q2 += qfc[BE_QF_M(1) + e] * vv; q6 += qfc[BE_QF_M(2) + e] * vv; q9 += qfc[BE_QF_M(3) + e] * vv; }
        double l5[5] = { q2, q6, q9, 0, 0 }, l4[4] = { 0, 0, 0, 0 };          // (red holds five values per exchange)
        if (tid < 66) { const double v = vq[tid]; l5[3] = v * qfc[BE_QF_V(1) + tid]; l5[4] = v * qfc[BE_QF_V(0) + tid]; l4[0] = v * qfc[BE_QF_V(3) + tid]; l4[1] = v * qfc[BE_QF_V(4) + tid]; l4[2] = v * qfc[BE_QF_V(5) + tid]; l4[3] = v * qfc[BE_QF_V(6) + tid]; }
        block_sum_n_dpp<5>(l5, red);
        block_sum_n_dpp<4>(l4, red);
        f_Q2 = l5[0]; f_Q6 = l5[1]; f_Q9 = l5[2]; f_L2 = l5[3]; f_LGS = l5[4]; f_L5 = l4[0]; f_L6 = l4[1]; f_L8 = l4[2]; f_L9 = l4[3];
        if (tid == 0) {
            const double* A = qfc + BE_QF_A;
            p_gg += A[0]; p_nn += (A[1] - 2.0 * f_L2) + f_Q2; p_gn += f_LGS - A[2];
        }
    }
    double sv3[3] = {p_gg, p_nn, p_gn};
    block_sum_n_dpp<3>(sv3, red);
    const double gnorm = sqrt(sv3[0]), gnn = sqrt(sv3[1]), gdot = sv3[2];
    const double radius = c.radius;
    // Cauchy point alpha = |gradient_|^2 / (u^T H u), u = S (gradient_ / diag): only the dogleg's second and third case read it, so it is
    // computed when the Gauss-Newton step first leaves the trust region (possibly slots later, after rejections: the linearisation of x
    // is still in place) and kept in the control block from then on.  Same arithmetic whenever it is evaluated.
    double alpha = c.alpha;
    bool have_alpha = c.reuse && c.alpha_valid;
    if (!(gnn <= radius) && !have_alpha) {
        for (int i = tid; i < n; i += SOL_THREADS) { const double sp = v_s[i], dp = v_d[i]; v_t[i] = sp * sp * gvec[i] / (dp * dp); }
        __syncthreads();
        gemv_hd(Hd, n, v_t, v_t2, scratch, tid);
        gather66(v_t);
        if (!SHARD) wdot_all();
        double uHu = 0, gg = 0;
        for (int i = tid; i < n; i += SOL_THREADS) { uHu += v_t[i] * v_t2[i]; gg += v_grad[i] * v_grad[i]; }
        if (SHARD) {          // 2 q . (sum alpha g w) + sum h alpha^2 g^2 ; sum grad_l^2
            if (tid < 66) uHu += 2.0 * q66[tid] * qfc[BE_QF_V(2) + tid];
            if (tid == 0) { uHu += qfc[BE_QF_A + 3]; gg += qfc[BE_QF_A + 0]; }
        }
        for (int l = tid; l < (SHARD ? 0 : nlm); l += SOL_THREADS) {
            const double h = BE_PK(pk, BE_PK_H, l), gl = BE_PK(pk, BE_PK_G, l), sl = a.scale_l[l], dl = a.diag_l[l], grad = a.grad_l[l];
            const double u = sl * sl * gl / (dl * dl);
            uHu += 2.0 * u * wd[l] + h * u * u;
            gg += grad * grad;
        }
        { double sv2[2] = {uHu, gg}; block_sum_n<2>(sv2, red); uHu = sv2[0]; gg = sv2[1]; }
        alpha = gg / uHu;
        have_alpha = true;
        __syncthreads();
    }
    if (tid == 0) { ctl->alpha = alpha; ctl->alpha_valid = have_alpha ? 1 : 0; }
    double cg, cn, dnorm;
    if (gnn <= radius) { cg = 0; cn = 1; dnorm = gnn; }
    else if (gnorm * alpha >= radius) { cg = -(radius / gnorm); cn = 0; dnorm = radius; }
    else {
        const double b_dot_a = -alpha * gdot, a2 = (alpha * gnorm) * (alpha * gnorm), bma2 = a2 - 2 * b_dot_a + gnn * gnn;
        const double cc = b_dot_a - a2, dd = sqrt(cc * cc + bma2 * (radius * radius - a2));
        const double beta = (cc <= 0) ? (dd - cc) / bma2 : (radius * radius - a2) / (dd + cc);
        cg = -alpha * (1.0 - beta); cn = beta; dnorm = -1.0;
    }
    // delta = (cg*grad + cn*gn) / diag * scale   (v_t = delta_p)
    double p_dn = 0;
    for (int i = tid; i < n; i += SOL_THREADS) { const double st = cg * v_grad[i] + cn * v_gn[i]; p_dn += st * st; v_t[i] = st / v_d[i] * v_s[i]; }
    // this thread's landmark step; published in LDS for the (landmark, part) threads of the coupling term below (scratch is idle: wd has been consumed)
    const double lm_st = cg * lm_grad + cn * lm_gn, lm_dl = lm_st / lm_diag * lm_scale;
    if (lm_live) scratch[tid] = lm_dl;
    lds_barrier();
    TS(9);
    if (tid < 66) { const int fa = tid / 6, r = tid - fa * 6; const int col = s_pcol[fa]; q66[tid] = col >= 0 ? v_t[col + r] : 0.0; }      // gather66
    if constexpr (!MF16) { if (xt_on && tid >= 128 && tid < 128 + BE_NX) { const int col = s_xcol[tid - 128]; qx[tid - 128] = col >= 0 ? v_t[col] : 0.0; } }
    lds_barrier();
    // Model cost change, candidate and norms in ONE pass.  Only the scalar delta^T H delta is needed, not H * delta: every thread adds the products of its
    // share of Hd (the coalesced column partition of gemv_hd) and of the packets' w rows (the (landmark, part) partition of wdot_all) straight into its
    // partial sum, so the loads of this phase are mutually independent and share one round trip; the block reduction at the end is the only exchange.
    // Wave 15 holds no share of Hd or of the w rows: its lanes carry the candidate's state blocks (lanes 0..10 pose f, 16..26 speed-bias f, 32..46 one
    // extrinsic / td entry each), so the candidate is formed beside the sums of the other waves instead of after them.
    const int h_col = tid % 192, h_part = tid / 192, h_seg = (n + 4) / 5, h_j0 = h_part * h_seg;       // the coalesced column partition of gemv_hd
    const bool h_live = h_part < 5 && h_col < n;
    const int c_lane = tid - (SOL_THREADS - 64);
    const bool c_pose = c_lane >= 0 && c_lane < BE_NF, c_sb = c_lane >= 16 && c_lane < 16 + BE_NF, c_ex = c_lane >= 32 && c_lane < 47;
    const int c_f = c_pose ? c_lane : (c_sb ? c_lane - 16 : 0);
    double creg[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) creg[k] = 0.0;
    if (c_pose) { for (int k = 0; k < 7; ++k) creg[k] = a.x->pose[c_f][k]; }
    if (c_sb) { for (int k = 0; k < 9; ++k) creg[k] = a.x->sb[c_f][k]; }
    if (c_ex) creg[0] = c_lane - 32 < 14 ? a.x->ex[(c_lane - 32) / 7][(c_lane - 32) % 7] : a.x->td;
    const double lm_x0 = lm_live ? a.x->inv_depth[lmi] : 0.0;
    double p_sg = 0, p_sHs = 0, p_step = 0, p_xn = 0;
    // candidate poses / speed-bias / extrinsics from the blocks wave 15 holds
    TSW(25);
    if (c_pose) {
        const int pc = s_pcol[c_f];
        if (pc >= 0) {
            double out[7];
            pose_plus(creg, &v_t[pc], a.dims.plane_kind, out);
            for (int k = 0; k < 7; ++k) { const double d = out[k] - creg[k]; p_step += d * d; p_xn += creg[k] * creg[k]; a.cand->pose[c_f][k] = out[k]; }
        } else for (int k = 0; k < 7; ++k) a.cand->pose[c_f][k] = creg[k];
    }
    TSW(26);
    if (c_sb) {
        const int sc = s_scol[c_f];
        if (sc >= 0) for (int k = 0; k < 9; ++k) { const double d = v_t[sc + k]; p_step += d * d; p_xn += creg[k] * creg[k]; a.cand->sb[c_f][k] = creg[k] + d; }
        else for (int k = 0; k < 9; ++k) a.cand->sb[c_f][k] = creg[k];
    }
    TSW(27);
    bool c_ex_free = false;          // this lane's extrinsic / td entry belongs to a FREE block: lanes 48..50 below form it
    if constexpr (!MF16) { if (xt_on && c_ex) c_ex_free = s_xcol[c_lane - 32 < 14 ? 6 * ((c_lane - 32) / 7) : 12] >= 0; }
    if (c_ex && !c_ex_free) { if (c_lane - 32 < 14) a.cand->ex[(c_lane - 32) / 7][(c_lane - 32) % 7] = creg[0]; else a.cand->td = creg[0]; }
    if constexpr (!MF16) {
        if (xt_on && c_lane >= 48 && c_lane < 51) {          // free para_ex_pose[0 / 1] (PoseLocalParameterization) / para_td: part of ceres' reduced parameter vector, so of both norms
            const int k = c_lane - 48;
            const int col = s_xcol[k < 2 ? 6 * k : 12];
            if (col >= 0) {
                if (k < 2) {
                    double x7[7], out[7];
                    for (int j = 0; j < 7; ++j) x7[j] = a.x->ex[k][j];
                    pose_plus(x7, &v_t[col], 0, out);
                    for (int j = 0; j < 7; ++j) { const double d = out[j] - x7[j]; p_step += d * d; p_xn += x7[j] * x7[j]; a.cand->ex[k][j] = out[j]; }
                } else { const double x = a.x->td, d = v_t[col]; p_step += d * d; p_xn += x * x; a.cand->td = x + d; }
            }
        }
    }
    TSW(28);
    if (h_part < 5) {
        double sh = 0;
#pragma unroll 12
        for (int q = 0; q < 36; ++q) {            // (reading only the lower triangle, off-diagonal entries twice, halves the bytes but measured 3.5 us slower)
            const int j = h_j0 + q;
            const bool ok = h_live && q < h_seg && j < n;
            const double h = Hd[ok ? (size_t)j * n + h_col : 0];
            const double xv = v_t[ok ? j : 0];
            sh += ok ? h * xv : 0.0;
        }
        if (h_live) p_sHs += sh * v_t[h_col];
    }
    TS(11);
    // coupling term 2 dl (w_l . delta_p).  A pure Gauss-Newton step of this linearisation (the common case) has delta_p = -(s_p y_p), whose products with the w
    // rows were formed for the landmark part of the step: no second pass over the packets.  Otherwise (Cauchy / interpolated step, or a step re-cut from a
    // kept linearisation) the rows are read again.
    const bool gn_pure = !c.reuse && cg == 0.0 && cn == 1.0;
    if (SHARD) {
        // every landmark term of the model cost change, the step norms and the state norm from the forms: delta-dependent parts (delta_p gathered in q66) first
        double d3[3] = { 0, 0, 0 };
        {
            double m = 0;
            for (int e = tid; e < 4356; e += SOL_THREADS) { const int i = e / 66, j = e - i * 66; m += qfc[BE_QF_M(0) + e] * (vq[i] * q66[j]); }
            d3[0] = m;
            if (tid < 66) { d3[1] = q66[tid] * qfc[BE_QF_V(2) + tid]; d3[2] = q66[tid] * qfc[BE_QF_V(0) + tid]; }
        }
        lds_barrier();
        block_sum_n_dpp<3>(d3, red);
        lds_barrier();
        if (tid == 0) {
            const double* A = qfc + BE_QF_A;
            const double nn = (A[1] - 2.0 * f_L2) + f_Q2, gnl = f_LGS - A[2];
            p_dn += cg * cg * A[0] + 2.0 * cg * cn * gnl + cn * cn * nn;
            p_sg += cg * A[0] - cn * A[2] + cn * f_LGS;
            p_sHs += (cg * cg * A[3] - 2.0 * cg * cn * A[4] + cn * cn * A[5]) + 2.0 * cn * (cg * f_L5 - cn * f_L6) + cn * cn * f_Q6
                     + 2.0 * (cg * d3[1] - cn * d3[2]) + 2.0 * cn * d3[0];
            p_step += (cg * cg * A[6] - 2.0 * cg * cn * A[7] + cn * cn * A[8]) + 2.0 * cn * (cg * f_L8 - cn * f_L9) + cn * cn * f_Q9;
            p_xn += A[9];
        }
    } else if (gn_pure) { if (lm_live) p_sHs += 2.0 * lm_dl * (-lm_wgn); }
    else {
        const int per = 66 / npart;
        const int part = npart > 1 ? tid / nlm_pad : 0;
        if (npart > 1) {
            const int l = tid - part * nlm_pad;
            if (part < npart && l < nlm) {
                double s0 = 0;
                const int q0 = part * per;
#pragma unroll 11
                for (int q = 0; q < per; ++q) s0 += BE_PK(pk, BE_PK_W + q0 + q, l) * q66[q0 + q];
                if constexpr (!MF16) { if (xt_on && part == 0) s0 += xdot(l); }
                p_sHs += 2.0 * scratch[l] * s0;
            }
        } else {
            for (int l = tid; l < nlm; l += SOL_THREADS) {
                double s0 = 0;
#pragma unroll 11
                for (int q = 0; q < 66; ++q) s0 += BE_PK(pk, BE_PK_W + q, l) * q66[q];
                if constexpr (!MF16) { if (xt_on) s0 += xdot(l); }
                p_sHs += 2.0 * scratch[l] * s0;
            }
        }
    }
    TS(12);
    for (int i = tid; i < n; i += SOL_THREADS) p_sg += v_t[i] * gvec[i];
    if (lm_live) {
        if (!SHARD) {
            p_dn += lm_st * lm_st;
            p_sg += lm_dl * lm_g;
            p_sHs += lm_h * lm_dl * lm_dl;
            p_step += lm_dl * lm_dl; p_xn += lm_x0 * lm_x0;
        }
        a.cand->inv_depth[lmi] = lm_x0 + lm_dl;
    }
    TS(13);
    TSW(29);
    double sv5[5] = {p_dn, p_sg, p_sHs, p_step, p_xn};
    block_sum_n_dpp<5>(sv5, red);          // LDS-only barriers: the candidate's stores drain behind the reduction
    const double dn2 = sv5[0], sg = sv5[1], sHs = sv5[2], step2 = sv5[3], xn2 = sv5[4] + a.xnorm2_extra;
    TS(10);
    if (tid == 0) {
        const double mcc = -(sg + 0.5 * sHs);
        ctl->model_cost_change = mcc;
        ctl->dogleg_norm = dnorm >= 0 ? dnorm : sqrt(dn2);
        ctl->step_valid = mcc > 0.0 ? 1 : 0;
        ctl->step_norm = sqrt(step2);
        ctl->x_norm = sqrt(xn2);
        ctl->chol_fail = 0;
        ctl->first = 0;
        if (mcc > 0.0) ctl->pending = 1;            // the candidate awaits its cost and the accept / reject decision
        else {                                      // HandleInvalidStep: needs no evaluation, so it is settled here
            ctl->pending = 0;
            ctl->slots = c.slots + 1; ctl->iter = c.iter + 1; ctl->invalid = c.invalid + 1; ctl->mu = c.mu * 10.0; ctl->reuse = 0; ctl->need_eval = 0;
            ctl->chol_fail = 1;                     // forces the reduce to rebuild Sc with the new mu
            if (c.invalid + 1 >= 5) { ctl->done = 1; ctl->termination = 2; }
            else if (c.iter + 1 >= c.max_iters) { ctl->done = 1; ctl->termination = 0; }
        }
    }
