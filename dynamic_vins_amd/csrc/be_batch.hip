// be_batch.hip — dv_batch: the group object, its shared round of window solves (the slot schedule of be_host.h over the batched launches), the rendezvous of the
// members' threads and the group's timing / counters.
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include "be_host.h"

// ---- dv_batch: several independent windows (one estimator each, same device) whose solve slots share every launch -----------------------------------
// Each member keeps its own BA stream for the upload, the gauge fix, the state download and the marginalization; the iteration slots — the launch-bound
// part: 3 launches per iteration and window — run on the batch's stream as ONE launch per stage for all windows (argument tables in HBM, window index in
// the grid).  Per round: S event waits (uploads done), 3 x iterations launches, one event, S event waits (tails).
struct dv_batch {
    std::vector<dv_ctx*> members;
    hipStream_t stream = nullptr;
    DevBuf tab; void* tab_pinned = nullptr; size_t tab_bytes = 0;      // [S] BeEvalArgs | [S] BeSolveArgs | [S] BeGaugeArgs | [S] BeRejectArgs | [S] BeMargArgs
    long long batched_rounds = 0, single_rounds = 0;
    DvFrontBatch* front = nullptr;                // the members' front ends in shared launches (dv_batch_track_enqueue, front_track.hip)
    hipEvent_t ev_state = nullptr;                // behind the shared accept + gauge + reject launches of a round: what the members' dv_est_process_end wait for
    std::mutex mu; std::condition_variable cv; int arrived = 0; long long generation = 0; int last_rc = 0;      // dv_batch_arrive
    bool aborted = false;                         // dv_batch_abort: every waiting and every later dv_batch_arrive returns -1
    // dv_batch_timing: HIP events around the three launches of the SECOND iteration slot of every round (a steady-state slot: candidate evaluation, reduce, solve with
    // the accept decision), on the batch stream they are launched on; harvested when the next round starts (the events of the previous round have completed by then)
    bool timing = false; hipEvent_t tev[4] = { nullptr, nullptr, nullptr, nullptr }; bool tev_pending = false;
    double t_ms[3] = { 0, 0, 0 }; long long t_n = 0; int t_windows = 0;
    // the members' object solves (dynamic members; dv_batch_obj_solve): their uploads and ONE bd_solve_group_kernel launch per round on the group's object stream, beside the
    // window solves on `stream`.  Job table: pinned block -> HBM per launch, double-buffered (ev_obj_copy[k] behind the upload that last read pinned block k); ev_obj behind the launch
    // All of it is created by the FIRST object solve that comes the group's way (obj_ensure): a group without dynamic members owns exactly the streams it always did — one more
    // stream per group shifts the runtime's round-robin of streams onto hardware queues for every stream created after it, and 16 raw sequences in four groups lost a third
    // of their rate to that (7100 -> 4700 frames/s, measured)
    std::mutex obj_mu; int device = 0; size_t obj_cap = 0;
    hipStream_t obj_stream = nullptr; hipEvent_t ev_obj = nullptr, ev_obj_copy[2] = { nullptr, nullptr };
    DevBuf obj_tab[2]; void* obj_tab_pinned[2] = { nullptr, nullptr }; int obj_parity = 0; bool obj_copy_used[2] = { false, false };
    long long obj_launches = 0, obj_jobs = 0, obj_single = 0;      // shared launches, the jobs in them, solves launched alone (dv_batch_obj_info)
};
DvFrontBatch*& be_batch_front(dv_batch* B) { return B->front; }
static void obj_release(dv_batch* B) {
    if (B->obj_stream) (void)hipStreamDestroy(B->obj_stream);
    if (B->ev_obj) (void)hipEventDestroy(B->ev_obj);
    B->obj_stream = nullptr; B->ev_obj = nullptr;
    for (int k = 0; k < 2; ++k) { if (B->ev_obj_copy[k]) (void)hipEventDestroy(B->ev_obj_copy[k]); B->ev_obj_copy[k] = nullptr; B->obj_tab[k].release(); if (B->obj_tab_pinned[k]) (void)hipHostFree(B->obj_tab_pinned[k]); B->obj_tab_pinned[k] = nullptr; }
}
// the group's object stream, its events and job tables: created on first use (members' threads of a team may come here together)
static bool obj_ensure(dv_batch* B) {
    std::lock_guard<std::mutex> lk(B->obj_mu);
    if (B->obj_stream) return true;
    const size_t bytes = B->obj_cap * be_obj_job_bytes();
    bool ok = hipSetDevice(B->device) == hipSuccess && hipEventCreateWithFlags(&B->ev_obj, hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < 2; ++k)
        ok = ok && hipEventCreateWithFlags(&B->ev_obj_copy[k], hipEventDisableTiming) == hipSuccess && B->obj_tab[k].ensure(bytes) == hipSuccess &&
             hipHostMalloc(&B->obj_tab_pinned[k], bytes, hipHostMallocDefault) == hipSuccess;
    hipStream_t s = nullptr;
    ok = ok && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
    if (!ok) { obj_release(B); return false; }
    B->obj_stream = s;
    return true;
}
hipStream_t be_batch_obj_stream(dv_batch* B) { return obj_ensure(B) ? B->obj_stream : nullptr; }      // nullptr: out of resources — the caller keeps its own stream and launch
// a member leaves (dv_destroy, dv_batch_destroy) with an object solve on the group's object stream — drained by the caller: the upload has landed, a launched solve has
// written its result — so what is left of it no longer needs the group: a deferred job is launched on the member's own stream when it is collected, a launched one has no event to wait for
static void obj_member_leaves(dv_ctx* c) {
    for (ObjPending* p : { &c->obj_pend, &c->obj_op_pend }) { p->ev_ext = nullptr; p->stream = c->obj_stream; }
    c->be.pend->ev_state_ext = nullptr;      // the same for a window solve inside a shared round: the group's event goes with the group (its stream is drained: the states have landed)
}
const std::vector<dv_ctx*>& be_batch_members(dv_batch* B) { return B->members; }
// dv_destroy of a member: the batch forgets it (a destroyed ctx must never be reached through B->members); threads waiting in dv_batch_arrive
// for a round this member will never join are released with an error
void be_batch_detach(dv_ctx* ctx) {
    dv_batch* B = ctx->batch;
    if (!B) return;
    {
        std::lock_guard<std::mutex> lk(B->mu);
        B->members.erase(std::remove(B->members.begin(), B->members.end(), ctx), B->members.end());
        ctx->batch = nullptr;
        if (B->stream) (void)hipStreamSynchronize(B->stream);
        if (B->obj_stream) (void)hipStreamSynchronize(B->obj_stream);      // an uploaded (deferred) or launched object solve of this member reads / writes its buffers
        obj_member_leaves(ctx);
        dv_front_batch_sync(B->front);
        if (ctx->be_stream_own) { ctx->be_stream = ctx->be_stream_own; ctx->be_stream_own = nullptr; }
        if (B->arrived > 0) { B->last_rc = -1; B->arrived = 0; ++B->generation; dv_set_error(nullptr, "dv_batch_arrive: a member was destroyed during the round"); }
    }
    B->cv.notify_all();
}
// The stages of a group's round for be_run_slots: one launch per stage for all windows (argument tables in HBM), nothing sharded (a member of a sharded window is
// never deferred to the group), the last slot's accept decision rides in the tail's first launch.
struct BeGroupStages {
    dv_batch* B; const std::vector<dv_ctx*>& M; const BeEvalArgs* dea; const BeSolveArgs* dsa; int S, max_grid, max_n;
    // bisecting switches (dv_debug_set on the group's FIRST member; the open multi-sequence defect of round 4): one stage of the round goes through the members' own
    // single-window launches instead of the shared launch — same stream, same order, only the kernel form differs
    int single;      // bit 0: evaluation, 1: reduce, 2: solve
    bool time_round; hipStream_t s;
    void eval(int mode) { if (single & 1) { for (dv_ctx* c : M) be_launch_eval(c->be.pend->ea, mode, s); } else be_launch_eval_batch(dea, S, max_grid, mode, s); }
    void reduce(int spec) { if (single & 2) { for (dv_ctx* c : M) be_launch_reduce(c->be.pend->sa, spec, s); } else be_launch_reduce_batch(dsa, S, max_n, spec, s); }
    int solve(int spec) {
        int rc = 0;
        if (single & 4) { for (dv_ctx* c : M) if (be_launch_solve(c->be.pend->sa, spec, s)) { rc = -1; break; } }
        else rc = be_launch_solve_batch(dsa, S, max_n, spec, s);
        if (rc) dv_set_error(M[0], "dv_batch_enqueue: cannot set dynamic LDS size");
        return rc ? -1 : 0;
    }
    void accept(bool) {}
    // dv_batch_timing: slot 1 (solve with the accept decision + factorisation, then the candidate's evaluation and reduce) between four events.  tev[0] stands where slot 0
    // ends, i.e. in front of slot 1's solve; the timed slot keeps the hashes behind its solve and leaves out those behind its evaluation and reduce.
    void after(int it, int kind) {
        if (time_round && it == 1) {
            if (kind == BE_ST_SOLVE) { dbg_all(it, kind); (void)hipEventRecord(B->tev[1], s); }
            else if (kind == BE_ST_CAND_EVAL) (void)hipEventRecord(B->tev[2], s);
            else { (void)hipEventRecord(B->tev[3], s); B->tev_pending = true; }
            return;
        }
        dbg_all(it, kind);
        if (time_round && it == 0 && kind == BE_ST_CAND_REDUCE) { (void)hipEventRecord(B->tev[0], s); B->t_windows = S; }
    }
    void dbg_all(int it, int kind) { for (dv_ctx* c : M) be_dbg_stage(c, it, kind, s); }
    int exchange_system(int) { return 0; } int exchange_cost() { return 0; } int gather_depth() { return 0; }
};

// The object solves the members' object branches left deferred (est_host.hip dynamic_branch -> be_obj_solve_begin with defer): one job table, one launch, one event.
// `which` picks the estimator's ObjPending (dv_batch_enqueue) or the operator-level one (dv_batch_obj_solve).
static int batch_enqueue_objects(dv_batch* B, const std::vector<dv_ctx*>& M, ObjPending dv_ctx::* which) {
    if (M.empty()) return 0;
    dv_ctx* ctx = M[0];
    if (M.size() == 1) {      // nothing to share: the member's own single-workgroup launch
        B->obj_single++;
        if (be_obj_solve_launch(M[0], M[0]->*which)) return -1;
        return 0;
    }
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const int par = B->obj_parity; B->obj_parity ^= 1;
    if (B->obj_copy_used[par]) DV_CHECK(hipEventSynchronize(B->ev_obj_copy[par]));      // the upload that last read this pinned block (two launches ago) has run
    std::vector<ObjPending*> pends;
    for (dv_ctx* c : M) pends.push_back(&(c->*which));
    if (be_obj_solve_group_launch(ctx, pends.data(), (int)pends.size(), B->obj_tab_pinned[par], B->obj_tab[par].p, B->obj_stream, B->ev_obj)) return -1;
    DV_CHECK(hipEventRecord(B->ev_obj_copy[par], B->obj_stream)); B->obj_copy_used[par] = true;
    B->obj_launches++; B->obj_jobs += (long long)M.size();
    return 0;
}
static int batch_enqueue_windows(dv_batch* B);
// a round: the window solves' slots and tails on the group's stream, then — beside them, on the group's object stream — the object solves of the dynamic members
static int batch_enqueue_impl(dv_batch* B) {
    if (batch_enqueue_windows(B)) return -1;
    std::vector<dv_ctx*> O;
    for (dv_ctx* c : B->members) if (c->obj_pend.active && c->obj_pend.deferred) O.push_back(c);
    if (!O.empty() && batch_enqueue_objects(B, O, &dv_ctx::obj_pend)) { if (O[0] != B->members[0]) dv_set_error(B->members[0], O[0]->err); return -1; }
    return 0;
}
static int batch_enqueue_windows(dv_batch* B) {
    std::vector<dv_ctx*> M;
    for (dv_ctx* c : B->members) if (c->be.pend->active && c->be.pend->deferred && !c->be.pend->trivial) M.push_back(c);
    if (M.empty()) return 0;
    dv_ctx* ctx = M[0];
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = B->stream;                    // == every member's be_stream: their uploads (and the marginalizations of their previous frames) are ordered before the slots
    bool uniform = true; int slots = M[0]->be.pend->first_slots, max_grid = 0, max_n = 0;
    for (dv_ctx* c : M) {
        const BePending& pd = *c->be.pend;
        if (pd.sa.ldl_mf16 == 0 || pd.first_slots != slots || (c->timing && c->kernel_timing) || !pd.fused_present) uniform = false;
        max_grid = std::max(max_grid, be_eval_batch_blocks(pd.ea.dims.nlm, pd.ea.dims.nimu)); max_n = std::max(max_n, pd.sa.dims.nstate);
    }
    if (!uniform || M.size() == 1) {      // mixed kernel variants (or nothing to share): every member's own launches, one member after the other
        for (dv_ctx* c : M) { BePending& pd = *c->be.pend; pd.deferred = false; if (be_enqueue_slots(c, pd, pd.first_slots, true, s) || be_enqueue_tail(c, pd, s)) { dv_set_error(ctx, c->err); return -1; } }
        B->single_rounds++;
        return 0;
    }
    const int S = (int)M.size();
    const size_t cap = B->members.size();
    BeEvalArgs* hea = (BeEvalArgs*)B->tab_pinned; BeSolveArgs* hsa = (BeSolveArgs*)(hea + cap);
    BeGaugeArgs* hga = (BeGaugeArgs*)(hsa + cap); BeRejectArgs* hrj = (BeRejectArgs*)(hga + cap); BeMargArgs* hma = (BeMargArgs*)(hrj + cap);
    // the frame tails' arguments are known now as well (nothing in them depends on the solve): accept + gauge + download, outlier test, marginalization
    int max_rej = 0, max_mlm = 0, any_imu = 0, max_D = 0, n_marg = 0; size_t max_fin = 0;
    for (int i = 0; i < S; ++i) {
        dv_ctx* c = M[i]; BePending& pd = *c->be.pend; BeWork& w = c->be;
        hea[i] = pd.ea; hsa[i] = pd.sa;
        be_gauge_args(c, pd, hga[i]);
        hrj[i] = BeRejectArgs{};
        if (pd.rej_on) { hrj[i] = pd.rej; max_rej = std::max(max_rej, pd.rej.nlm); }
        hma[i] = BeMargArgs{};                    // D = 0: no marginalization for this member this frame
        if (pd.do_marg && !pd.pl.empty) {
            double* hscal = be_download(w)->marg_scal[pd.scal_slot];      // the health scalars go straight to the member's pinned slot
            if (marg_args(c, pd.pl, w.cand, pd.g_norm, w.priorA, w.priorb, w.priorA_buf[pd.nxt], w.priorb_buf[pd.nxt], hscal, w.prior_c0 + pd.nxt, hma[i])) { dv_set_error(ctx, c->err); return -1; }
            max_mlm = std::max(max_mlm, hma[i].nlm); any_imu |= hma[i].nimu > 0; max_D = std::max(max_D, hma[i].D);
            max_fin = std::max(max_fin, be_marg_finish_smem(hma[i].D, hma[i].D - hma[i].m)); ++n_marg;
        }
    }
    const BeEvalArgs* dea = (const BeEvalArgs*)B->tab.p; const BeSolveArgs* dsa = (const BeSolveArgs*)(dea + cap);
    const BeGaugeArgs* dga = (const BeGaugeArgs*)(dsa + cap); const BeRejectArgs* drj = (const BeRejectArgs*)(dga + cap); const BeMargArgs* dma = (const BeMargArgs*)(drj + cap);
    DV_CHECK(dv_copy_async(B->tab.p, B->tab_pinned, B->tab_bytes, s));
    if (B->timing && B->tev_pending && hipEventQuery(B->tev[3]) == hipSuccess) {      // the previous round's three stages
        float ms;
        for (int k = 0; k < 3; ++k) if (hipEventElapsedTime(&ms, B->tev[k], B->tev[k + 1]) == hipSuccess) B->t_ms[k] += ms;
        B->t_n++; B->tev_pending = false;
    }
    const bool time_round = B->timing && !B->tev_pending && slots >= 3;
    const int dbg = M[0]->be.debug_batch_single;      // dv_debug_set "batch_single_*" on the group's first member: bits 0 - 2 see BeGroupStages, bit 3 the tail below
    BeGroupStages st{ B, M, dea, dsa, S, max_grid, max_n, dbg, time_round, s };
    if (be_run_slots(st, slots, true)) return -1;
    // ---- the tails of all members: 2 + 3 launches per group instead of 5 - 6 per member on S streams ----
    // Round 4: a member's result intermittently left the single-sequence result in this launch when a second group was in flight (located by per-launch hashes,
    // scripts/dbg/multiseq_first_diff.py).  Cause: be_accept_body let thread 0 store into the control block before every wave had loaded it (be_kernels.h; fixed by a workgroup
    // barrier — shared launch 8 of 30 runs differing before, 0 of 60 after).  dv_debug_set "batch_single_tail" issues the members' own launches of the same bodies instead (A/B).
    if (dbg & 8) { for (dv_ctx* c : M) { BeGaugeArgs ga{}; be_gauge_args(c, *c->be.pend, ga); be_launch_accept_gauge(c->be.pend->sa, ga, s); } }
    else be_launch_accept_gauge_batch(dsa, dga, S, s);
    be_launch_reject_batch(drj, S, max_rej, s);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipEventRecord(B->ev_state, s));
    if (n_marg > 0) {
        const int rc = be_launch_marg_batch(dma, S, max_mlm, any_imu, max_D, max_fin, s);
        if (rc == -2) DV_FAIL("dv_marginalize: system does not fit in LDS");
        if (rc) DV_FAIL("dv_marginalize: cannot set dynamic LDS size");
        DV_CHECK(hipGetLastError());
    }
    for (dv_ctx* c : M) {
        BePending& pd = *c->be.pend;
        pd.deferred = false; pd.t_enq = std::chrono::steady_clock::now();
        pd.ev_state_ext = B->ev_state;
        if (pd.do_marg && !pd.pl.empty) pd.marg_in_flight = true;
    }
    B->batched_rounds++;
    return 0;
}

extern "C" {

dv_batch* dv_batch_create(dv_ctx* const* ctxs, int n) {
    if (!ctxs || n < 1 || n > 256) { dv_set_error(nullptr, "dv_batch_create: bad arguments"); return nullptr; }
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || ctxs[i]->batch || ctxs[i]->cfg.device != ctxs[0]->cfg.device || ctxs[i]->be.pend->active) { dv_set_error(nullptr, "dv_batch_create: members must be idle contexts of one device that belong to no other batch"); return nullptr; }
        for (int j = 0; j < i; ++j) if (ctxs[j] == ctxs[i]) { dv_set_error(nullptr, "dv_batch_create: duplicate member"); return nullptr; }
        if (ctxs[i]->be.marg_form != DV_MARG_INFO) { dv_set_error(nullptr, "dv_batch_create: a member uses DV_MARG_EIGEN; dv_batch groups marginalize in DV_MARG_INFO form only"); return nullptr; }
    }
    if (hipSetDevice(ctxs[0]->cfg.device) != hipSuccess) { dv_set_error(nullptr, "dv_batch_create: hipSetDevice failed"); return nullptr; }
    dv_batch* B = new dv_batch();
    B->members.assign(ctxs, ctxs + n);
    bool ok = hipStreamCreateWithFlags(&B->stream, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&B->ev_state, hipEventDisableTiming) == hipSuccess;
    const size_t bytes = (size_t)n * (sizeof(BeEvalArgs) + sizeof(BeSolveArgs) + sizeof(BeGaugeArgs) + sizeof(BeRejectArgs) + sizeof(BeMargArgs));
    B->tab_bytes = bytes;
    ok = ok && B->tab.ensure(bytes) == hipSuccess && hipHostMalloc(&B->tab_pinned, bytes, hipHostMallocDefault) == hipSuccess;
    B->device = ctxs[0]->cfg.device; B->obj_cap = (size_t)n;
    if (!ok) { dv_set_error(nullptr, "dv_batch_create: out of resources"); B->members.clear(); dv_batch_destroy(B); return nullptr; }
    // from now on the batch's stream IS every member's BA stream: uploads, window solves (shared or alone), tails and marginalizations of all members are ordered on
    // it — one hardware queue per group instead of one per member (48 streams on 12 queues made unrelated launches wait behind each other's event waits)
    for (int i = 0; i < n; ++i) {
        dv_ctx* c = ctxs[i];
        (void)hipStreamSynchronize(c->be_stream);
        c->be_stream_own = c->be_stream; c->be_stream = B->stream; c->batch = B;
    }
    return B;
}
void dv_batch_destroy(dv_batch* B) {
    if (!B) return;
    if (B->stream) (void)hipStreamSynchronize(B->stream);
    if (B->obj_stream) (void)hipStreamSynchronize(B->obj_stream);
    { std::lock_guard<std::mutex> lk(B->mu); for (dv_ctx* c : B->members) if (c->batch == B) { obj_member_leaves(c); c->batch = nullptr; if (c->be_stream_own) { c->be_stream = c->be_stream_own; c->be_stream_own = nullptr; } } B->members.clear(); }
    if (B->front) { dv_front_batch_release(B->front); B->front = nullptr; }
    if (B->stream) (void)hipStreamDestroy(B->stream);
    if (B->ev_state) (void)hipEventDestroy(B->ev_state);
    for (hipEvent_t e : B->tev) if (e) (void)hipEventDestroy(e);
    obj_release(B);
    B->tab.release();
    if (B->tab_pinned) (void)hipHostFree(B->tab_pinned);
    delete B;
}
int dv_batch_enqueue(dv_batch* B) {
    if (!B) return -1;
    return batch_enqueue_impl(B);
}
// Rendezvous form for one host thread per member: every thread calls it after its member's dv_est_process_begin; the call returns in all of them once the
// last one has arrived and enqueued the round (a barrier inside the library: no interpreter lock is held while waiting).
int dv_batch_arrive(dv_batch* B) {
    if (!B) return -1;
    std::unique_lock<std::mutex> lk(B->mu);
    if (B->aborted) { dv_set_error(nullptr, "dv_batch_arrive: the batch was aborted"); return -1; }
    const long long gen = B->generation;
    if (++B->arrived >= (int)B->members.size()) {
        B->last_rc = batch_enqueue_impl(B);
        B->arrived = 0; ++B->generation;
        lk.unlock();
        B->cv.notify_all();
        return B->last_rc;
    }
    B->cv.wait(lk, [&] { return B->generation != gen; });
    return B->last_rc;
}
// A member thread that fails before it can arrive calls this (except / finally of the worker): the round is abandoned, every thread waiting in
// dv_batch_arrive — and every later arrival — returns -1 instead of blocking for ever.
int dv_batch_abort(dv_batch* B) {
    if (!B) return -1;
    {
        std::lock_guard<std::mutex> lk(B->mu);
        B->aborted = true; B->last_rc = -1; B->arrived = 0; ++B->generation;
    }
    dv_set_error(nullptr, "dv_batch_arrive: the batch was aborted");
    B->cv.notify_all();
    return 0;
}
// per-stage launch durations of the batched window solve, HIP events on the batch stream: out3 = average ms of [be_solve_batch, be_eval_batch (full), be_reduce_batch] over
// the rounds timed so far (one steady-state slot per round), *windows = windows per launch of the last timed round.  on != 0 switches the events on.
int dv_batch_timing(dv_batch* B, int on, double* out3, long long* rounds, int* windows) {
    if (!B) return -1;
    if (on && !B->tev[0]) for (auto& e : B->tev) if (hipEventCreate(&e) != hipSuccess) return -1;
    B->timing = on != 0;
    if (out3) for (int k = 0; k < 3; ++k) out3[k] = B->t_n ? B->t_ms[k] / (double)B->t_n : 0.0;
    if (rounds) *rounds = B->t_n;
    if (windows) *windows = B->t_windows;
    return 0;
}
// InstanceManager::Optimization (estimator/estimator_insts.cpp:772-807) of several members at once: problems[i] solved on member members[i], all in ONE launch
// (bd_solve_group_kernel, one workgroup per problem) on the group's object stream; every result carries the bits dv_obj_solve gives for the same problem.  All problems are
// checked and packed before anything is enqueued: one bad problem fails the call with dv_obj_solve's message (on its member and on the first member) and nothing is launched.
int dv_batch_obj_solve(dv_batch* B, const int* members, dv_obj_problem* const* problems, int n, dv_ba_summary* summaries) {
    if (!B) return -1;
    dv_ctx* first = B->members.empty() ? nullptr : B->members[0];
    auto bad = [&](dv_ctx* c, const std::string& m) { if (c && c != first) dv_set_error(c, m); dv_set_error(first, m); return -1; };
    if (!members || !problems || !summaries || n < 1) return bad(nullptr, "dv_obj_solve: null argument");
    if (!obj_ensure(B)) return bad(nullptr, "dv_batch_obj_solve: out of resources");
    std::vector<dv_ctx*> M;
    for (int i = 0; i < n; ++i) {
        if (members[i] < 0 || members[i] >= (int)B->members.size()) return bad(nullptr, "dv_batch_obj_solve: member index out of range");
        dv_ctx* c = B->members[members[i]];
        if (std::find(M.begin(), M.end(), c) != M.end()) return bad(c, "dv_batch_obj_solve: a member is listed twice (one object solve per member and launch)");
        if (!problems[i]) return bad(c, "dv_obj_solve: null argument");
        M.push_back(c);
    }
    for (int i = 0; i < n; ++i) if (be_obj_solve_pack(M[i], problems[i], M[i]->s1, M[i]->obj_op_pend)) return bad(M[i], M[i]->err);      // (nothing enqueued yet: the packed ones are simply dropped)
    int rc = 0;
    for (int i = 0; i < n && !rc; ++i) { ObjPending& p = M[i]->obj_op_pend; rc = be_obj_solve_upload(M[i], B->obj_stream, M[i]->s1, p); if (!rc) { p.deferred = true; p.active = true; } }
    if (!rc) rc = batch_enqueue_objects(B, M, &dv_ctx::obj_op_pend);
    if (rc) {      // a runtime failure half way: drain what was enqueued, drop the solves
        (void)hipStreamSynchronize(B->obj_stream);
        std::string m; for (dv_ctx* c : M) { if (m.empty() && !c->err.empty()) m = c->err; c->obj_op_pend.active = c->obj_op_pend.deferred = false; c->obj_op_pend.ev_ext = nullptr; }
        return bad(nullptr, m.empty() ? "dv_batch_obj_solve: launch failed" : m);
    }
    for (int i = 0; i < n; ++i) if (be_obj_solve_end(M[i], problems[i], &summaries[i], M[i]->obj_op_pend)) return bad(M[i], M[i]->err);
    return 0;
}
// shared object-solve launches of the group so far (dv_batch_enqueue rounds and dv_batch_obj_solve calls), the jobs in them, and the solves that were launched alone
int dv_batch_obj_info(dv_batch* B, long long* launches, long long* jobs, long long* single) {
    if (!B) return -1;
    if (launches) *launches = B->obj_launches;
    if (jobs) *jobs = B->obj_jobs;
    if (single) *single = B->obj_single;
    return 0;
}
int dv_batch_info(dv_batch* B, long long* batched_rounds, long long* single_rounds) {
    if (!B) return -1;
    if (batched_rounds) *batched_rounds = B->batched_rounds;
    if (single_rounds) *single_rounds = B->single_rounds;
    return 0;
}

}  // extern "C"
