// be_host.h — what the host side of the window solve shares between its files: be_api.hip (workspace, upload, single-window schedule, tail, operator entries),
// be_marg_host.hip (marginalization plan / arguments / enqueue), be_batch.hip (dv_batch) and be_debug.hip (hash logs, dv_debug_set).
#pragma once
#include "dv_ctx.h"

// ---- the pinned download area (BeWork::pinned + dl_off, behind the mirror of the upload region) ----
// The gauge kernel writes x, ctl and raw_pose straight into it; the marginalization's 4 health scalars land in marg_scal[slot] (two alternating slots: the
// scalars of frame k are read while frame k + 1's are in flight); c0 stages the constant of a prior handed over in host memory on its way to the device.
struct BeDownload {
    BeState x; BeCtl ctl;
    double marg_scal[2][4]; double pad0[8];
    double c0; double pad1[15];
    double raw_pose[77];
};
constexpr size_t BE_DOWNLOAD_SLACK = 4096;      // what be_ensure reserves behind the state and the control block
static_assert(sizeof(BeCtl) % sizeof(double) == 0 && sizeof(BeState) % sizeof(double) == 0, "downloaded as doubles");
static_assert(offsetof(BeDownload, ctl) == sizeof(BeState) && offsetof(BeDownload, marg_scal) == sizeof(BeState) + sizeof(BeCtl), "state and control block are downloaded back to back");
static_assert(offsetof(BeDownload, c0) == offsetof(BeDownload, marg_scal) + 128 && offsetof(BeDownload, raw_pose) == offsetof(BeDownload, marg_scal) + 256, "the download area's layout");
static_assert(sizeof(BeDownload) <= sizeof(BeState) + sizeof(BeCtl) + BE_DOWNLOAD_SLACK, "the download area fits what be_ensure reserves");
static inline BeDownload* be_download(const BeWork& w) { return (BeDownload*)((uint8_t*)w.pinned + w.dl_off); }

// the states of a problem into the pinned BeState of the upload region; n_inv_depth: how many inverse depths travel (a solve: its nlm landmarks; dv_marginalize: up to
// the largest landmark index its factors name, whatever nlm says)
static inline void be_stage_state(BeState* hx, const dv_ba_problem* P, int n_inv_depth) {
    std::memset(hx, 0, offsetof(BeState, inv_depth));
    for (int f = 0; f < P->nframes; ++f) { std::memcpy(hx->pose[f], P->pose + 7 * f, 56); if (P->use_imu) std::memcpy(hx->sb[f], P->speed_bias + 9 * f, 72); }
    std::memcpy(hx->ex, P->ex_pose, 14 * 8); hx->td = P->td[0];
    if (n_inv_depth) std::memcpy(hx->inv_depth, P->inv_depth, 8 * (size_t)n_inv_depth);
}

// ---- the slot schedule, written once for the single window (be_api.hip: BeWindowStages) and the dv_batch group (be_batch.hip: BeGroupStages) ----
// `slots` trust-region iterations.  speculative: the candidate of every slot but the last is linearised in full (evaluation + reduce into
// the other set) and judged by the next solve kernel; the last one gets the cost-only evaluation and the accept kernel.  The classic form
// (spare slots after a failed / invalid step) spends 5 launches per slot and needs no look-ahead.
// Stages: eval(mode), reduce(spec), solve(spec) and accept(final_slot) launch; after(it, kind) runs behind launch `kind` of slot `it` (BE_ST_*: the debug hashes, the
// group's timing events); exchange_system(spec) / exchange_cost() / gather_depth() are the sharded window's exchanges (no-ops otherwise).  Whatever returns an int
// returns -1 with the error set.
enum { BE_ST_HEAD_EVAL = 0, BE_ST_HEAD_REDUCE = 1, BE_ST_SOLVE = 2, BE_ST_CAND_EVAL = 3, BE_ST_CAND_REDUCE = 4 };
template <class Stages> static inline int be_run_slots(Stages& st, int slots, bool speculative) {
    for (int it = 0; it < slots; ++it) {
        const bool head = !speculative || it == 0, last = !speculative || it == slots - 1;
        if (head) { st.eval(BE_EVAL_X); st.after(it, BE_ST_HEAD_EVAL); st.reduce(0); st.after(it, BE_ST_HEAD_REDUCE); if (st.exchange_system(0)) return -1; }
        if (st.solve(head ? 0 : 1)) return -1;
        st.after(it, BE_ST_SOLVE);
        if (last) { st.eval(BE_EVAL_CAND_COST); st.after(it, BE_ST_CAND_EVAL); if (st.exchange_cost()) return -1; st.accept(it == slots - 1); }
        else { st.eval(BE_EVAL_CAND_FULL); st.after(it, BE_ST_CAND_EVAL); st.reduce(1); st.after(it, BE_ST_CAND_REDUCE); if (st.exchange_system(1)) return -1; }
    }
    if (!speculative || slots > 0) return st.gather_depth();
    return 0;
}

// be_api.hip
int be_ensure(dv_ctx* ctx, int nfac);
int be_fill_imu(const dv_ba_imu& in, BeImu& o, const double* sqrt_hint);
int be_enqueue_slots(dv_ctx* ctx, BePending& pd, int slots, bool speculative, hipStream_t s);
void be_gauge_args(dv_ctx* ctx, const BePending& pd, BeGaugeArgs& ga);
int be_enqueue_tail(dv_ctx* ctx, BePending& pd, hipStream_t s);
// be_marg_host.hip
int marg_plan(dv_ctx* ctx, MargPlan& pl, int mode, const dv_ba_prior* prior, const dv_ba_factor* fac, const dv_ba_lm* lms, const int* sel, int nsel, bool imu01);
int marg_args(dv_ctx* ctx, const MargPlan& pl, const BeState* x, double g_norm, const double* priorA, const double* priorb, double* outA, double* outb, double* scal, double* c0_out, BeMargArgs& ma);
int marg_enqueue(dv_ctx* ctx, const MargPlan& pl, const BeState* x, double g_norm, const double* priorA, const double* priorb, double* outA, double* outb, double* scal, double* c0_out, hipStream_t s);
void marg_new_prior(const MargPlan& pl, const double* pose, const double* sb, const double* ex, const double* td, double c0, dv_ba_prior* out);
int be_check_prev_marg(dv_ctx* ctx, BePending& pd);
// be_debug.hip
void be_dbg_stage(dv_ctx* c, int it, int kind, hipStream_t s);
void be_dbg_hash(const void* dev, size_t bytes, unsigned long long* out_pinned, hipStream_t s);
