// runner.hip — the per-frame host loop of the reference's threads T2 + T3 (system/main.cpp:178-330 FeatureTrack, :394-404 the estimator thread, the two queues
// between them) for one or many sequences, in C++ inside the library: dv_runner_*.  Host code only (no kernel here); everything goes through the public entries
// of include/dvins.h, so a runner is exactly what a caller could write against the ABI.
//
// ONE schedule per frame, whatever the sequence is (raw, with masks, dynamic, label images) and whoever drives it (group_round):
//     end(k-1) [seq_end: wait, outlier rejection, slide] -> [shared front end, first round only: track k] -> begin(k) [seq_begin -> est_frame: IMU up to t_k,
//     window solve enqueued, tracking(k+1) enqueued where this thread does that itself, object branch] -> [dv_batch: ONE enqueue] -> [shared front end: track k+1]
//     -> post(k) [seq_post: IMU up to t_k+1, collect tracking(k+1) where it is due]
// so that the front end of frame k+1 overlaps the back end of frame k on one host thread (Pipeline of dynamic_vins_amd/pipeline.py).  What frame k's tracking takes
// (mask, mode, detections ...) is said once, by track_input; seq_enqueue and the shared launches of group_track both read it.
// A DYNAMIC sequence runs the reference's two threads literally (dv_runner_set "tracker_thread", default on): T2 = a tracker thread (TrackSemanticImage + InstsTrack of
// frame after frame, collected into a small ring: the role of feature_queue, basic/feature_queue.h:19-73, blocking instead of dropping so that no frame is lost) beside
// T3 = the estimator loop on the calling thread (pop, IMU, window solve, object branch, end).  Tracker and estimator share nothing but the ring: the tracker API touches
// the context's tracker state and front-end streams, the estimator API its own state and the BA / object streams.
// Many sequences on one GPU (config 4 of BASELINE.json, "batched"): the sequences of a GROUP run their begin phases back to back, dv_batch_enqueue launches the
// iteration slots of all their window solves as one launch per stage, and while that runs the host turns to the next group; the end phases of a group follow when
// its turn comes again.  `threads` host threads each drive their own groups (the reference runs one process — three threads — per sequence), or a TEAM of threads
// drives one group: thread j of T takes members j, j + T, ... through the same phases with a barrier between them, thread 0 issuing the shared launches.
// Dynamic sequences may be members of such a group: per member end(k-1), begin_ego(k), attach(k); then ONE dv_batch_enqueue launches the window slots AND the object solves
// of all members; then ONE dv_batch_track_enqueue tracks the background of frame k+1 of all members (TrackSemanticImage in the group's shared launches, the members' static
// instances unmasked by one launch) and every member enqueues InstsTrack(k+1) on its object tracker's stream; then every member collects its frame k+1 (seq_post).  With
// "batch_front" 0, or a static-report lag of 1, a member enqueues tracking(k+1) itself between begin_ego(k) and attach(k), as a sequence outside a group does.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "dv_ctx.h"

// The entries of a label-image sequence (dv_runner_set_viode).  Weak references: this file is also linked, as plain C++, into host-only sanitizer harnesses whose
// stand-in C ABI knows only the entries of the pre-computed path; dv_runner_set_viode refuses when they are absent.  In the library they bind as usual.
#pragma weak dv_viode_frame_enqueue
#pragma weak dv_viode_frame_collect
#pragma weak dv_track_unmask_static_keys
#pragma weak dv_inst_track_enqueue_keys
// ... and of a mask-stack sequence (dv_runner_set_inst_stack), likewise
#pragma weak dv_inst_stack_frame_enqueue
#pragma weak dv_inst_stack_frame_collect
#pragma weak dv_track_unmask_static_planes
#pragma weak dv_inst_track_enqueue_planes

namespace {
// choice T1: DV_STATIC_REPORT_LAG (DVINS_STATIC_LAG in the environment: experiments only — the Python pipeline and the parity harness read the same variable)
int static_lag() { static const int v = [] { const char* e = std::getenv("DVINS_STATIC_LAG"); const int k = e ? std::atoi(e) : DV_STATIC_REPORT_LAG; return k >= 1 && k <= 3 ? k : DV_STATIC_REPORT_LAG; }(); return v; }
struct RSeq {
    dv_ctx* ctx = nullptr; dv_seq_input in{};
    int next = 0, k_imu = 0, w = 0, h = 0, stride = 0;
    bool enqueued = false, pending = false, skipped = false;
    std::vector<dv_feat> rows; int n_rows = 0;
    double pending_t = 0;
    dv_est_state last{};
    std::vector<double> poses;          // [t, px py pz qx qy qz qw] per frame solved in the non-linear phase
    std::vector<unsigned long long> row_log;      // per frame handed to the back end: [frame index k, rows collected, FNV-1a of the rows' bytes, solver iterations] (dv_runner_get_row_log: diagnostics)
    unsigned long long cur_rows_hash = 0; int cur_k = -1;
    std::vector<double> track_clock;    // tracker thread: host clock at which each frame was delivered into the ring (dv_runner_get_frame_clock with which = 1)
    std::vector<double> end_clock;      // host clock (seconds, steady) at which each frame's dv_est_process_end returned (dv_runner_get_frame_clock: diagnostics)
    std::vector<double> frames9;        // [t, px py pz qx qy qz qw, nonlinear] of EVERY frame handed to the back end (what SaveBodyTrajectory writes)
    long long iterations = 0, frames = 0;
    std::string err;
    // dynamic mode (dv_runner_set_dynamic): the frame's object hand-over, double-buffered — [cur] belongs to the frame in the back end, [cur ^ 1] receives the next
    // frame's while that one's window solve is in flight
    bool dynamic = false; dv_seq_dynamic dyn{};
    struct DynBuf {
        std::vector<dv_feat> rows; int n_rows = 0; std::vector<dv_inst_obs> insts; int n_insts = 0; std::vector<dv_feat> ifeats; int n_ifeats = 0; std::vector<double> pts; int n_pts = 0; bool valid = false;
        void reserve() { rows.resize(DV_MAX_FEATS); insts.resize(64); ifeats.resize(64 * 256); pts.resize((size_t)3 * 65536); valid = false; }
    };
    DynBuf db[2]; int cur = 0;
    // the one-thread order (tracker_thread 0, and every member of a dv_batch group): seq_begin leaves the collect of frame k+1's rows to seq_post, which a group runs
    // behind its shared launches — the member's host thread must not sit in its own tracker's collect while the solves of the whole group are not launched yet
    bool grouped = false, collect_due = false;
    // a frame of this dynamic sequence has been enqueued (by seq_enqueue or by the group's shared launches): from then on it always has its next frame in flight or
    // collected when a round starts, so group_track's first-round pass has nothing to do for it — and does not look at the fields its team thread may be writing
    bool started = false;
    int job_k = 0;      // group_track: the frame of this member in the round's shared launches
    // tracker thread (T2) -> estimator loop (T3): ring of collected frames.  ring_head = frame index of ring[ring_pos], ring_count frames are ready; tracked_next = the
    // next frame the tracker will take.  Guarded by ring_mu; the tracker fills ring[(ring_pos + ring_count) % RING] outside the lock (the slot is not visible yet).
    static constexpr int RING = 3;
    DynBuf ring[RING]; int ring_pos = 0, ring_count = 0, ring_head = 0, tracked_next = 0; bool ring_failed = false;
    int track_last = -1; bool track_stop = false, track_busy = false; std::thread tracker;      // the tracker thread lives as long as the runner (a thread's first HIP call costs milliseconds:
                                                                                                // a thread per dv_runner_run put that into the first frames of every call); track_last = the last frame it may take
    std::unique_ptr<std::mutex> ring_mu = std::make_unique<std::mutex>(); std::unique_ptr<std::condition_variable> ring_cv = std::make_unique<std::condition_variable>();
    long long detections = 0, object_features = 0, frames_with_objects = 0; int min_detections = 1 << 30;
    // para::is_static_inst_as_background (dv_seq_dynamic::static_as_background): FeatureTrack takes the pixels of the instances the estimator reported static out of the merged
    // mask (system/main.cpp:194,217-245).  In the reference T2 reads whatever T3 published last — a race whose outcome depends on the threads' timing; here the tracking of
    // frame f uses the snapshot of the newest back-end frame <= f - 2 (what the one-thread loop sees when it enqueues frame f: the object branch of frame f - 1 comes behind
    // that enqueue), in every host layout.  snaps / est_passed are guarded by ring_mu.
    struct StaticSnap { int frame = -1; std::vector<uint32_t> ids; };
    bool static_unmask = false; StaticSnap snaps[4]; int snap_next = 0, est_passed = -1;
    // dv_runner_set_viode: thread T1's stage per frame.  live_dets / live_* = what dv_viode_frame_collect handed back for the frame being enqueued; live_enq = the frame whose
    // stage is enqueued and not collected yet (-1: none).  Touched by the thread that enqueues the tracking alone (T2, or the one-thread loop)
    bool live = false; dv_seq_viode vio{}; std::vector<dv_inst_det> live_dets; int live_n = 0, live_enq = -1;
    const uint8_t* live_inv = nullptr; const uint32_t* live_k0 = nullptr; const uint32_t* live_k1 = nullptr;
    // dv_runner_set_inst_stack: the same stage from the detector's mask stack (live is set too).  live_planes[i] = the plane of live_dets[i]; live_st = the descriptor of the
    // frame whose stage was collected last — what the *_planes entries of that frame take
    bool live_stack = false; dv_seq_stack stk{}; std::vector<int32_t> live_planes; dv_mask_stack live_st{};
    // TrackImageNaive over the sequence (dv_runner_set_mask): per frame the inverse merged instance mask, and the tracking mode that takes it
    const uint8_t* const* raw_mask = nullptr; int raw_mode = DV_MODE_RAW;
};
// reusable barrier of a group's host threads (sense reversing; the waits are short — a member's host phase is ~0.1 ms — so it spins with a yield)
struct SpinBarrier {
    std::atomic<int> count{0}; std::atomic<int> sense{0}; std::atomic<int> failed{0}; int n = 1;
    bool wait() {          // -> false if any thread of the group reported a failure (everybody leaves the round; the flag is also polled INSIDE the spin, so a thread
                           //    that failed behind the round's last barrier cannot leave its teammates spinning in the next one)
        const int s = sense.load(std::memory_order_acquire);
        if (count.fetch_add(1, std::memory_order_acq_rel) + 1 == n) { count.store(0, std::memory_order_relaxed); sense.store(s ^ 1, std::memory_order_release); }
        else while (sense.load(std::memory_order_acquire) == s) {
            if (failed.load(std::memory_order_acquire)) return false;      // a teammate left the round with an error and will never arrive: nobody waits for it
            std::this_thread::yield();
        }
        return failed.load(std::memory_order_acquire) == 0;
    }
};
}
struct dv_runner {
    std::vector<RSeq> seqs;
    struct Group { std::vector<int> members; dv_batch* batch = nullptr; std::unique_ptr<SpinBarrier> bar; };
    std::vector<Group> groups;
    int threads = 1, threads_per_group = 1;      // threads > groups: every dv_batch group is driven by threads / groups host threads that split its members' host phases (group_round)
    bool teams = true;            // dv_runner_set "teams" (on by default since round 5: 100 of 100 runs of 16 sequences in four groups on eight threads bit-identical to the single-thread run, profiles/r05_experiments): several host threads per group.  First blamed for the round-4 trajectory defect, then cleared (the cause was the
                                  // accept decision's missing barrier, be_kernels.h be_accept_body); bit-identical to the single-thread run (tests/test_runner.py).
    int threads_requested = 1;
    bool tracker_thread = true;   // dynamic sequences: the reference's T2 beside T3 (dv_runner_set "tracker_thread"); 0 = the one-thread loop of round 4, kept for A/B and as the bit-identity reference
    bool batch_front = true;      // dv_batch groups: the members' tracking in shared launches too (dv_batch_track_enqueue); dv_runner_set(runner, "batch_front", 0) keeps one set of launches per sequence
    std::string err; std::mutex err_mu;
};

namespace {
// ---- errors: the runner's message is shared by its host threads (guarded); a sequence's own is its thread's ----
int set_err(dv_runner* R, const std::string& m) { std::lock_guard<std::mutex> lk(R->err_mu); R->err = m; return -1; }
int seq_err(dv_runner* R, RSeq& s, const std::string& m) { s.err = m; return set_err(R, m); }
int fail(dv_runner* R, RSeq& s, const char* what) { const char* m = dv_last_error(s.ctx); return seq_err(R, s, std::string(what) + ": " + (m ? m : "")); }
int batch_fail(dv_runner* R, const dv_runner::Group& g, const char* what) { const char* m = dv_last_error(R->seqs[g.members[0]].ctx); return set_err(R, std::string(what) + ": " + (m ? m : "")); }
RSeq* seq_at(dv_runner* R, int seq) { return R && seq >= 0 && seq < (int)R->seqs.size() ? &R->seqs[seq] : nullptr; }
bool seq_started(const RSeq& s) { return s.next != 0 || s.enqueued || s.pending || s.tracked_next != 0; }
// a getter's hand-over: rows of `width` values; the count goes out whole, the copy stops at the caller's cap
template <class T> void copy_rows(const std::vector<T>& v, int width, T* out, int cap, int* n_out) {
    const int n = (int)(v.size() / width);
    if (n_out) *n_out = n;
    if (out) std::memcpy(out, v.data(), sizeof(T) * width * (size_t)std::min(n, std::max(cap, 0)));
}

// ---- the tracking half of a frame ----
// What frame k's tracking takes: the background tracker's mask and mode; for a dynamic sequence the object tracker's detections, 3-D boxes, disparity map and
// right key image, and whether the static instances' rectangles leave the mask first.  keys: the left key image of a label-image frame, whose calls take their key-image forms.
struct TrackInput {
    const uint8_t* mask = nullptr; int mode = DV_MODE_RAW;
    const dv_inst_det* dets = nullptr; int n_dets = 0; const dv_box3d* boxes = nullptr; int n_boxes = 0;
    const float* disp = nullptr; const uint32_t* right_keys = nullptr; int right_keys_mem = 0;
    const uint32_t* keys = nullptr; bool unmask = false;
    const dv_mask_stack* stack = nullptr; const int32_t* planes = nullptr;      // a mask-stack frame: its calls take their plane forms
};
// raw sequence | sequence with dv_runner_set_mask | dynamic sequence | label-image sequence whose stage of frame k has been collected (viode_collect)
TrackInput track_input(const RSeq& s, int k) {
    TrackInput in;
    if (!s.dynamic) { in.mask = s.raw_mask ? s.raw_mask[k] : nullptr; in.mode = s.raw_mode; return in; }
    const dv_seq_dynamic& d = s.dyn;          // (a label-image sequence keeps its mode, disparity source and static_as_background here too)
    in.mode = d.mode ? d.mode : DV_MODE_SEMANTIC;
    in.boxes = d.boxes3d ? d.boxes3d[k] : nullptr; in.n_boxes = d.n_boxes3d ? d.n_boxes3d[k] : 0;
    in.disp = d.disp ? d.disp[k] : nullptr;
    if (s.live) {
        in.mask = s.live_inv; in.keys = s.live_k0; in.right_keys = s.live_k1; in.right_keys_mem = DV_MEM_DEVICE;
        if (s.live_stack) { in.stack = &s.live_st; in.planes = s.live_planes.data(); in.keys = nullptr; in.right_keys = nullptr; }
        in.dets = s.live_n ? s.live_dets.data() : nullptr; in.n_dets = s.live_n;
        in.unmask = s.static_unmask && s.live_n > 0;
    } else {
        in.mask = d.inv_mask ? d.inv_mask[k] : nullptr; in.right_keys = d.right_keys ? d.right_keys[k] : nullptr; in.right_keys_mem = d.right_keys_mem;
        in.dets = d.dets ? d.dets[k] : nullptr; in.n_dets = d.n_dets ? d.n_dets[k] : 0;
        in.unmask = s.static_unmask && d.inv_mask && d.dets && d.n_dets && d.n_dets[k] > 0;
    }
    return in;
}
// the static ids frame k's tracking takes out of its mask: the snapshot of the newest back-end frame <= k - lag (RSeq::snaps) -> their count
int static_ids(RSeq& s, int k, uint32_t* ids) {
    std::lock_guard<std::mutex> lk(*s.ring_mu);
    const RSeq::StaticSnap* best = nullptr;
    for (const RSeq::StaticSnap& sn : s.snaps) if (sn.frame >= 0 && sn.frame <= k - static_lag() && (!best || sn.frame > best->frame)) best = &sn;
    if (!best) return 0;
    std::copy(best->ids.begin(), best->ids.end(), ids);
    return (int)best->ids.size();
}
// The three steps of frame k's enqueue: the static instances' rectangles staged for it (seq_unmask) | the background tracking | what follows it (seq_enqueued: InstsTrack
// of a dynamic sequence).  seq_enqueue runs them back to back on the sequence's own stream; a dv_batch group with shared tracking launches (group_track) runs the first
// and the last per member around ONE dv_batch_track_enqueue.
int seq_unmask(dv_runner* R, RSeq& s, int k, const TrackInput& in) {
    if (!in.unmask) return 0;
    uint32_t ids[256];          // (a snapshot holds at most the 256 ids dyn_passed asks for)
    const int n = static_ids(s, k, ids);
    if (s.live_stack) { if (dv_track_unmask_static_planes(s.ctx, in.dets, in.planes, in.n_dets, n ? ids : nullptr, n, in.stack)) return fail(R, s, "dv_track_unmask_static_planes"); }
    else if (s.live) { if (dv_track_unmask_static_keys(s.ctx, in.dets, in.n_dets, n ? ids : nullptr, n, in.keys, 0, DV_MEM_DEVICE)) return fail(R, s, "dv_track_unmask_static_keys"); }
    else if (dv_track_unmask_static(s.ctx, in.dets, in.n_dets, n ? ids : nullptr, n)) return fail(R, s, "dv_track_unmask_static");
    return 0;
}
int seq_enqueued(dv_runner* R, RSeq& s, int k, const TrackInput& in) {
    if (s.dynamic) {
        const dv_seq_dynamic& d = s.dyn;
        if (in.disp && dv_inst_set_disparity(s.ctx, in.disp, d.disp_stride, d.disp_mem, d.baseline)) return fail(R, s, "dv_inst_set_disparity");
        if (in.right_keys && dv_inst_set_right_keys(s.ctx, in.right_keys, 0, in.right_keys_mem)) return fail(R, s, "dv_inst_set_right_keys");
        if (s.live_stack) { if (dv_inst_track_enqueue_planes(s.ctx, s.in.times[k], in.dets, in.planes, in.n_dets, in.stack, in.boxes, in.n_boxes)) return fail(R, s, "dv_inst_track_enqueue_planes"); }
        else if (s.live) { if (dv_inst_track_enqueue_keys(s.ctx, s.in.times[k], in.dets, in.n_dets, in.keys, 0, DV_MEM_DEVICE, in.boxes, in.n_boxes)) return fail(R, s, "dv_inst_track_enqueue_keys"); }
        else if (dv_inst_track_enqueue(s.ctx, s.in.times[k], in.dets, in.n_dets, in.boxes, in.n_boxes)) return fail(R, s, "dv_inst_track_enqueue");
    }
    s.enqueued = true; s.started = true;
    return 0;
}
// a label-image sequence (dv_runner_set_viode): T1's stage of frame k is collected (enqueued first, if frame k - 1 did not do it), then FeatureTrack's calls in their
// key-image forms, then T1's stage of frame k + 1 is enqueued behind them — its boxes arrive while the host is busy with frame k
// (a mask-stack sequence, dv_runner_set_inst_stack: the same two steps on dv_inst_stack_frame_*; behind the collect the upstream tracker's answer goes onto the detections —
// track id and class per plane, -1 = the plane is dropped: the reference's class filter, image_process/image_process.cpp:217-232)
dv_mask_stack stack_of(const RSeq& s, int k) {
    const dv_seq_stack& q = s.stk;
    dv_mask_stack st{}; st.data = q.stack[k]; st.n_planes = q.n_planes[k]; st.kind = q.kind; st.mem = q.mem; st.row_stride = q.row_stride; st.plane_stride = q.plane_stride; st.threshold = q.threshold;
    return st;
}
int viode_stage(dv_runner* R, RSeq& s, int k) {
    if (s.live_stack) {
        const dv_mask_stack st = stack_of(s, k);
        if (dv_inst_stack_frame_enqueue(s.ctx, &st, s.w, s.h, 0)) return fail(R, s, "dv_inst_stack_frame_enqueue");
        s.live_enq = k;
        return 0;
    }
    const dv_seq_viode& v = s.vio;
    if (dv_viode_frame_enqueue(s.ctx, v.seg0[k], v.seg1 ? v.seg1[k] : nullptr, s.w, s.h, v.stride, v.mem, v.dyn_keys, v.nkeys)) return fail(R, s, "dv_viode_frame_enqueue");
    s.live_enq = k;
    return 0;
}
int viode_collect(dv_runner* R, RSeq& s, int k) {
    if (s.live_enq != k && viode_stage(R, s, k)) return -1;
    s.live_enq = -1;
    if (s.live_stack) {
        if (dv_inst_stack_frame_collect(s.ctx, s.stk.min_inst_size, s.live_dets.data(), s.live_planes.data(), (int)s.live_dets.size(), &s.live_n, &s.live_inv, nullptr)) return fail(R, s, "dv_inst_stack_frame_collect");
        s.live_st = stack_of(s, k);
        int n = 0;
        for (int i = 0; i < s.live_n; ++i) {
            const int p = s.live_planes[i], tid = s.stk.track_id[k][p], cls = s.stk.class_id ? s.stk.class_id[k][p] : 0;
            if (tid < 0 || cls < 0) continue;
            dv_inst_det d = s.live_dets[i]; d.track_id = (uint32_t)tid; d.class_id = cls;
            s.live_dets[n] = d; s.live_planes[n] = p; ++n;
        }
        s.live_n = n;
        return 0;
    }
    if (dv_viode_frame_collect(s.ctx, s.vio.min_inst_size, s.live_dets.data(), (int)s.live_dets.size(), &s.live_n, &s.live_inv, &s.live_k0, &s.live_k1)) return fail(R, s, "dv_viode_frame_collect");
    return 0;
}
int seq_enqueue(dv_runner* R, RSeq& s, int k) {
    if (s.live && viode_collect(R, s, k)) return -1;
    const TrackInput in = track_input(s, k);
    if (seq_unmask(R, s, k, in)) return -1;
    // (frames and mask share `mem` in dv_track_stereo_enqueue: a device-resident sequence keeps both in HBM)
    if (dv_track_stereo_enqueue(s.ctx, s.in.left[k], s.in.right[k], s.w, s.h, s.stride, s.in.times[k], in.mask, in.mode, s.in.mem)) return fail(R, s, "dv_track_stereo_enqueue");
    if (seq_enqueued(R, s, k, in)) return -1;
    return s.live && k + 1 < s.in.n_frames ? viode_stage(R, s, k + 1) : 0;
}
// b = NULL: a raw sequence, into its own rows
int seq_collect(dv_runner* R, RSeq& s, RSeq::DynBuf* b) {
    if (dv_track_stereo_collect(s.ctx, b ? b->rows.data() : s.rows.data(), b ? &b->n_rows : &s.n_rows)) return fail(R, s, "dv_track_stereo_collect");
    if (b) {
        if (dv_inst_track_collect(s.ctx, b->insts.data(), (int)b->insts.size(), &b->n_insts, b->ifeats.data(), (int)b->ifeats.size(), &b->n_ifeats, b->pts.data(), (int)(b->pts.size() / 3), &b->n_pts)) return fail(R, s, "dv_inst_track_collect");
        b->valid = true;
    }
    s.enqueued = false;
    return 0;
}
// the frame the sequence tracks AHEAD of the one seq_begin has just taken (a track-only frame has already advanced s.next)
int frame_ahead(const RSeq& s) { return s.next + (s.skipped ? 0 : 1); }

// ---- the estimator half of a frame ----
int seq_feed_imu(dv_runner* R, RSeq& s, double t) {
    while (s.k_imu < s.in.n_imu && s.in.imu_t[s.k_imu] <= t + 0.006) {      // the samples up to the frame (+ the slack the reference's GetIMUInterval tolerates)
        if (dv_est_input_imu(s.ctx, s.in.imu_t[s.k_imu], s.in.imu_acc + 3 * (size_t)s.k_imu, s.in.imu_gyr + 3 * (size_t)s.k_imu)) return fail(R, s, "dv_est_input_imu");
        ++s.k_imu;
    }
    return 0;
}
// the estimator loop has passed frame k (its object branch ran, or the frame was track-only): publish the static-instance snapshot the tracker of frame >= k + 2 reads
int dyn_passed(dv_runner* R, RSeq& s, int k, bool with_snapshot) {
    uint32_t ids[256]; int n = 0;
    if (s.static_unmask && with_snapshot && dv_est_get_static_instances(s.ctx, ids, 256, &n)) return fail(R, s, "dv_est_get_static_instances");
    {
        std::lock_guard<std::mutex> lk(*s.ring_mu);
        if (s.static_unmask && with_snapshot) { RSeq::StaticSnap& sn = s.snaps[s.snap_next]; s.snap_next = (s.snap_next + 1) % 4; sn.frame = k; sn.ids.assign(ids, ids + n); }
        s.est_passed = k;
    }
    s.ring_cv->notify_all();
    return 0;
}
// The estimator calls of frame k, whose tracking has been collected: `rows`, and `obj` — instances, feature rows, points — of a dynamic sequence (NULL: raw).
//     IMU up to t_k -> begin / begin_ego [host bookkeeping + enqueue of the window solve] -> tracking(k+1), if this thread enqueues it itself (own_front: thread T2 of
//     the reference, independent of T3) -> attach [the object branch of ProcessImage beside the window solve] -> hand_back(): the caller's buffer is free
//     -> the static report of frame k published (dyn_passed)
// A frame the back end does not take (ba_stride) goes the same way without the estimator calls.  What seq_post does comes behind: the IMU samples up to t_k+1 and, in
// the one-thread order, the collect of frame k+1 while the solve is still in flight.
template <class HandBack>
int est_frame(dv_runner* R, RSeq& s, int k, const dv_feat* rows, int n_rows, const RSeq::DynBuf* obj, bool own_front, HandBack hand_back) {
    const double t = s.in.times[k];
    const bool enqueue_next = own_front && k + 1 < s.in.n_frames;
    s.n_rows = n_rows;
    // tracked only: outside KITTI the reference pushes a frame to feature_queue when cnt % 2 == 0, cnt counting tracked frames from 0 (system/main.cpp:181,300-312):
    // frames 0, 2, 4, ... — both trackers have seen the frame, the back end has not
    s.skipped = s.in.ba_stride > 1 && (k % s.in.ba_stride) != 0;
    if (s.skipped) {
        if (enqueue_next && seq_enqueue(R, s, k + 1)) return -1;
        hand_back();
        ++s.next;
        return obj ? dyn_passed(R, s, k, false) : 0;
    }
    if (seq_feed_imu(R, s, t)) return -1;
    const char* const begin = obj ? "dv_est_process_dynamic_begin_ego" : "dv_est_process_begin";
    const int rc = obj ? dv_est_process_dynamic_begin_ego(s.ctx, rows, n_rows, t) : dv_est_process_begin(s.ctx, rows, n_rows, t);      // (the window solve goes to the GPU with the background rows alone)
    if (rc < 0) return fail(R, s, begin);
    if (rc > 0) return seq_err(R, s, "IMU stream does not cover the frame");
    if (enqueue_next && seq_enqueue(R, s, k + 1)) return -1;
    if (obj) {
        if (dv_est_process_dynamic_attach(s.ctx, obj->n_insts ? obj->insts.data() : nullptr, obj->n_insts, obj->n_ifeats ? obj->ifeats.data() : nullptr, obj->n_pts ? obj->pts.data() : nullptr)) return fail(R, s, "dv_est_process_dynamic_attach");
        s.detections += obj->n_insts; s.object_features += obj->n_ifeats; s.frames_with_objects += obj->n_insts > 0; s.min_detections = std::min(s.min_detections, obj->n_insts);
    }
    hand_back();          // (rows, detections, feature rows and points are copied into the estimator's own tables by the calls above)
    s.pending = true; s.pending_t = t;
    return obj ? dyn_passed(R, s, k, true) : 0;
}
// what the back end is handed: frame index + a hash of the collected rows (row log: the bit-identity checks compare it run against run).  Taken BEHIND the enqueue of the
// window solve — a byte-serial FNV over 32 KB was 20 - 25 us on the path between two frames' solves — and over 64-bit words
void hash_rows(RSeq& s, int k) {
    static_assert(sizeof(dv_feat) % 8 == 0, "rows are hashed as 64-bit words");
    unsigned long long h = 1469598103934665603ull; const unsigned long long* p = reinterpret_cast<const unsigned long long*>(s.rows.data());
    for (size_t i = 0, n = (size_t)s.n_rows * sizeof(dv_feat) / 8; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    s.cur_rows_hash = h; s.cur_k = k;
}
// Do the dynamic members of a dv_batch group track in the group's shared launches?  With shared tracking launches on, and a static-report lag of two frames or more:
// the shared launches of frame k+1 come BEHIND the object branch of frame k (dyn_passed), where the member's own enqueue comes before it — with lag 1 the snapshot of
// frame k would be read in one order and not in the other, so lag 1 keeps the enqueue inside est_frame (fourth finding).  A constant of the run.
bool dyn_shares_front(const dv_runner* R) { return R->batch_front && static_lag() >= 2; }
// First half of a step: frame k's buffer — where it comes from, and where it goes when the estimator has taken it — and est_frame on it.
//     raw:                  collected here into the sequence's rows (enqueued here too, if nobody has); hashed for the row log
//     dynamic, one thread:  db[cur], collected by the previous frame's seq_post (here, for the first frame); then the other buffer becomes current and seq_post fills it
//     dynamic, T2 + T3:     the ring's oldest slot, which goes back to the tracker
// own_front = false: member of a dv_batch group whose tracking runs in the group's shared launches (group_track has enqueued frame k, and enqueues frame k+1 behind the
// group's dv_batch_enqueue).
int seq_begin(dv_runner* R, RSeq& s, bool own_front) {
    const int k = s.next;
    if (k >= s.in.n_frames) return seq_err(R, s, "sequence exhausted");
    auto fetch = [&](RSeq::DynBuf* b) {
        if (!s.enqueued) { if (!own_front) return seq_err(R, s, "internal: frame not enqueued"); if (seq_enqueue(R, s, k)) return -1; }
        return seq_collect(R, s, b);
    };
    if (!s.dynamic) {
        if (fetch(nullptr)) return -1;
        return est_frame(R, s, k, s.rows.data(), s.n_rows, nullptr, own_front, [&] { hash_rows(s, k); });
    }
    if (R->tracker_thread && !s.grouped) {          // (a group member tracks on the group's host thread: the ring is a group_size 0 feature)
        RSeq::DynBuf* b;
        {
            std::unique_lock<std::mutex> lk(*s.ring_mu);
            s.ring_cv->wait(lk, [&] { return s.ring_count > 0 || s.ring_failed; });
            if (s.ring_failed) return -1;
            if (s.ring_head != k) return seq_err(R, s, "internal: the tracker ring is out of step with the estimator");
            b = &s.ring[s.ring_pos];
        }
        return est_frame(R, s, k, b->rows.data(), b->n_rows, b, false, [&] {          // (a track-only frame's slot goes back to the tracker unread)
            { std::lock_guard<std::mutex> lk(*s.ring_mu); b->valid = false; s.ring_pos = (s.ring_pos + 1) % RSeq::RING; --s.ring_count; ++s.ring_head; }
            s.ring_cv->notify_all();
        });
    }
    own_front = own_front || !dyn_shares_front(R);
    RSeq::DynBuf& b = s.db[s.cur];
    if (!b.valid && fetch(&b)) return -1;
    return est_frame(R, s, k, b.rows.data(), b.n_rows, &b, own_front, [&] { b.valid = false; s.cur ^= 1; s.collect_due = k + 1 < s.in.n_frames; });
}
// Last phase of a step, behind a group's dv_batch_enqueue and shared tracking launches: the IMU samples up to the sequence's next frame and, in the one-thread order of a
// dynamic sequence, the collect of that frame's rows (into the buffer seq_begin has already made the current one)
int seq_post(dv_runner* R, RSeq& s) {
    const int k1 = frame_ahead(s);
    if (k1 >= s.in.n_frames) return 0;
    if (!s.skipped && seq_feed_imu(R, s, s.in.times[k1])) return -1;
    if (!s.collect_due) return 0;
    s.collect_due = false;
    return seq_collect(R, s, &s.db[s.cur]);
}
int seq_end(dv_runner* R, RSeq& s) {
    if (!s.pending) return 0;
    if (dv_est_process_end(s.ctx, &s.last)) return fail(R, s, "dv_est_process_end");
    s.pending = false;
    s.row_log.push_back((unsigned long long)s.cur_k); s.row_log.push_back((unsigned long long)s.n_rows); s.row_log.push_back(s.cur_rows_hash); s.row_log.push_back((unsigned long long)s.last.iterations);
    s.end_clock.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count());
    s.frames9.push_back(s.pending_t);
    for (int i = 0; i < 7; ++i) s.frames9.push_back(s.last.window[10][i]);
    s.frames9.push_back((double)s.last.nonlinear);
    if (s.last.nonlinear) {
        s.poses.push_back(s.pending_t);
        for (int i = 0; i < 7; ++i) s.poses.push_back(s.last.window[10][i]);      // body.Ps / Rs[kWinSize]: what SaveBodyTrajectory writes (utils/io/output.cpp:199-227)
    }
    s.iterations += s.last.iterations; ++s.frames; ++s.next;
    return 0;
}

// ---- dynamic mode on two threads ----
// T2: tracks frames tracked_next .. track_last (inclusive; dv_runner_run moves the bound), each into the next free ring slot; parks while the ring is full (the reference's queue drops instead: 100 deep, never
// reached by a tracker that is faster than its estimator — here nothing may be lost because the run must equal the one-thread loop frame for frame)
void dyn_tracker_thread(dv_runner* R, RSeq& s) {
    for (;;) {
        int f, slot;
        {
            std::unique_lock<std::mutex> lk(*s.ring_mu);
            s.track_busy = false; s.ring_cv->notify_all();
            s.ring_cv->wait(lk, [&] { return s.track_stop || (!s.ring_failed && s.tracked_next <= s.track_last && s.ring_count < RSeq::RING &&
                                                                  (!s.static_unmask || s.tracked_next < static_lag() || s.est_passed >= s.tracked_next - static_lag())); });      // (the static-instance snapshot of frame f - lag must exist)
            if (s.track_stop) return;
            s.track_busy = true;
            f = s.tracked_next; slot = (s.ring_pos + s.ring_count) % RSeq::RING;
        }
        const bool bad = seq_enqueue(R, s, f) || seq_collect(R, s, &s.ring[slot]);
        {
            std::lock_guard<std::mutex> lk(*s.ring_mu);
            if (bad) s.ring_failed = true;
            else { if (s.ring_count == 0) s.ring_head = f; ++s.ring_count; ++s.tracked_next; s.track_clock.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count()); }
        }
        s.ring_cv->notify_all();
    }
}

// ---- a group's round ----
// The tracking of every member of a dv_batch group in shared launches (dv_batch_track_enqueue): of frame s.next (first round: nothing is enqueued yet), or of the frame
// AHEAD of the one the members have just begun.  Dynamic members (dyn_shares_front): per member its static instances' rectangles are staged first (seq_unmask), then the
// ONE dv_batch_track_enqueue, then per member InstsTrack of the same frame on its object tracker's own stream (seq_enqueued: not shared, like the extra-point stages).
int group_track(dv_runner* R, dv_runner::Group& g, bool ahead) {
    std::vector<dv_track_job> jobs;
    const bool dyn_shared = dyn_shares_front(R);
    for (size_t m = 0; m < g.members.size(); ++m) {
        RSeq& s = R->seqs[g.members[m]];
        // `enqueued` first: in a team round thread 0 comes here (first-round pass) while its teammates may still be inside seq_end of THEIR members, advancing s.next — every
        // member is `enqueued` then (set by this thread in the previous round, two barriers ago) and its counters are not looked at.  Reading s.next before this test was a
        // data race ThreadSanitizer reported (tests/host/runner_tsan.cpp); the value read was never used, so no result depended on it.
        // A dynamic member's flags (`enqueued`, its buffers) are written by seq_post, which a teammate may still be running for the previous round: in the first-round pass
        // `started` alone is read — written by this thread or before the threads started — and a started member is left alone.
        if (s.dynamic ? (!dyn_shared || (!ahead && s.started)) : s.enqueued) continue;          // (dynamic member with its own front end: it enqueues its tracking inside est_frame)
        const int k = ahead ? frame_ahead(s) : s.next;
        if (k >= s.in.n_frames || (s.dynamic && s.enqueued)) continue;
        const TrackInput in = track_input(s, k);
        if (seq_unmask(R, s, k, in)) return -1;
        dv_track_job j{};
        j.member = (int)m; j.mem = s.in.mem; j.gray0 = s.in.left[k]; j.gray1 = s.in.right[k]; j.stride = s.stride; j.t = s.in.times[k];
        j.mode = in.mode; j.mask = in.mask;      // (naive members with masks share the round's launches when the round holds two or more naive / semantic jobs; a lone one keeps its own: dv_batch_track_enqueue)
        s.job_k = k;
        jobs.push_back(j);
    }
    if (jobs.empty()) return 0;
    if (dv_batch_track_enqueue(g.batch, jobs.data(), (int)jobs.size())) return batch_fail(R, g, "dv_batch_track_enqueue");
    for (const dv_track_job& j : jobs) { RSeq& s = R->seqs[g.members[j.member]]; if (seq_enqueued(R, s, s.job_k, track_input(s, s.job_k))) return -1; }      // (sets `enqueued`)
    return 0;
}
// One round of a group: end(k-1) -> [shared front end, first round only: track k] -> begin(k) -> [dv_batch: ONE enqueue of the window solves' slots (and the object
// solves)] -> [shared front end: ONE set of tracking launches for the members' frames k+1] -> post.  `drain`: the members' last frames are ended, nothing begins.
// Run by ONE host thread over all members (j 0 of T 1: no barrier), or by thread j of a TEAM of T: it does the host phases of members j, j + T, ..., thread 0 issues the
// shared launches, and a barrier stands between the phases.  The window solves of a LARGE group share every launch (kernel efficiency) while its host work — ~0.1 ms
// per member and frame, serial on one thread — runs T wide.
int group_round(dv_runner* R, dv_runner::Group& g, int j, int T, bool drain) {
    SpinBarrier* const B = T > 1 ? g.bar.get() : nullptr;
    const bool shared = g.batch && R->batch_front;
    int rc = 0;
    auto mine = [&](auto f) { for (size_t m = j; m < g.members.size() && !rc; m += T) if (f(R->seqs[g.members[m]])) rc = -1; };
    auto phase_done = [&] { if (rc && B) B->failed.store(1); return B ? B->wait() : rc == 0; };      // -> false: somebody failed, everybody leaves the round
    // (the group keeps no "frames in flight" flag of its own: seq_end is a no-op for a member without one, and a flag written by thread 0 could be read by a teammate in
    //  the drain round, which has no barrier, after thread 0 cleared it — the teammate would skip its members' last frames)
    mine([&](RSeq& s) { return seq_end(R, s); });
    if (!drain) {
        if (j == 0 && !rc && shared && group_track(R, g, false)) rc = -1;
        if (!phase_done()) return -1;                                  // every member collected its previous frame; frame k of all members is enqueued
        mine([&](RSeq& s) { return seq_begin(R, s, !shared); });
        if (!phase_done()) return -1;                                  // all begins (uploads on the group's stream) are in
        if (j == 0) {
            if (g.batch && dv_batch_enqueue(g.batch)) rc = batch_fail(R, g, "dv_batch_enqueue");
            if (!rc && shared && group_track(R, g, true)) rc = -1;
        }
        if (!phase_done()) return -1;                                  // the next frames are enqueued (their `enqueued` flags are set)
        mine([&](RSeq& s) { return seq_post(R, s); });
    }
    if (rc && B) B->failed.store(1);
    return rc;
}
// host threads: one per group (at most `threads_requested`), or — dv_runner::teams, on by default — threads_requested / groups per dv_batch group
void runner_layout(dv_runner* R) {
    const int ng = (int)R->groups.size(), threads = R->threads_requested;
    bool all_batched = R->batch_front; for (auto& g : R->groups) if (!g.batch) all_batched = false;          // (teams need the shared front end)
    R->threads_per_group = 1;
    for (auto& g : R->groups) g.bar.reset();
    if (R->teams && threads > ng && all_batched && threads % ng == 0) {
        R->threads = threads; R->threads_per_group = threads / ng;
        for (auto& g : R->groups) { g.bar = std::make_unique<SpinBarrier>(); g.bar->n = R->threads_per_group; }
    } else R->threads = std::max(1, std::min(threads, ng));
}
// n host threads, each running body(t) -> status; -> -1 if any failed.  One thread: the caller's own.
template <class Body> int run_threads(int n, Body body) {
    if (n <= 1) return body(0);
    std::vector<std::thread> th; std::vector<int> rcs(n, 0);
    for (int t = 0; t < n; ++t) th.emplace_back([&, t] { rcs[t] = body(t); });
    for (auto& t : th) t.join();
    int rc = 0; for (int v : rcs) if (v) rc = -1;
    return rc;
}
}

extern "C" {

dv_runner* dv_runner_create(dv_ctx* const* ctxs, const dv_seq_input* seqs, int n_seq, int group_size, int threads) {
    if (!ctxs || !seqs || n_seq < 1 || n_seq > 4096) { dv_set_error(nullptr, "dv_runner_create: bad arguments"); return nullptr; }
    auto R = std::make_unique<dv_runner>();
    R->seqs.resize(n_seq);
    for (int i = 0; i < n_seq; ++i) {
        RSeq& s = R->seqs[i];
        if (!ctxs[i] || !ctxs[i]->est || !seqs[i].left || !seqs[i].right || !seqs[i].times || seqs[i].n_frames < 1) { dv_set_error(nullptr, "dv_runner_create: every sequence needs a ctx with an estimator (dv_est_create) and its frames"); return nullptr; }
        s.ctx = ctxs[i]; s.in = seqs[i];
        s.w = ctxs[i]->cfg.width; s.h = ctxs[i]->cfg.height; s.stride = seqs[i].stride > 0 ? seqs[i].stride : s.w;
        s.rows.resize(DV_MAX_FEATS);
    }
    // groups: group_size <= 0 -> no batching (every sequence its own group, window solves on its own stream); else dv_batch groups of that size
    const int gs = group_size <= 0 ? 1 : group_size;
    for (int a = 0; a < n_seq; a += gs) {
        dv_runner::Group g;
        for (int i = a; i < std::min(n_seq, a + gs); ++i) g.members.push_back(i);
        if (group_size > 0 && g.members.size() > 1) {
            std::vector<dv_ctx*> m; for (int i : g.members) m.push_back(R->seqs[i].ctx);
            g.batch = dv_batch_create(m.data(), (int)m.size());
            if (!g.batch) { for (auto& gg : R->groups) if (gg.batch) dv_batch_destroy(gg.batch); return nullptr; }
            for (int i : g.members) R->seqs[i].grouped = true;
        }
        R->groups.push_back(std::move(g));
    }
    R->threads_requested = threads;
    runner_layout(R.get());
    return R.release();
}

void dv_runner_destroy(dv_runner* R) {
    if (!R) return;
    for (auto& s : R->seqs) if (s.tracker.joinable()) {
        { std::lock_guard<std::mutex> lk(*s.ring_mu); s.track_stop = true; }
        s.ring_cv->notify_all(); s.tracker.join();
    }
    for (auto& g : R->groups) if (g.batch) dv_batch_destroy(g.batch);      // (the contexts stay the caller's)
    delete R;
}

// n_rounds frames of EVERY sequence.  wall_seconds (optional): the host wall clock of the call, all streams drained (dv_sync of every ctx inside the region).
int dv_runner_run(dv_runner* R, int n_rounds, double* wall_seconds) {
    if (!R) return -1;
    if (n_rounds < 0) return set_err(R, "dv_runner_run: negative round count");
    for (auto& s : R->seqs) if (s.next + n_rounds > s.in.n_frames) return set_err(R, "dv_runner_run: a sequence has fewer frames left than rounds asked");
    const auto t0 = std::chrono::steady_clock::now();
    // T2 of every dynamic sequence: may track up to ONE frame past what this call hands to the back end (as the one-thread loop does)
    if (R->tracker_thread && n_rounds > 0)
        for (auto& s : R->seqs) if (s.dynamic && !s.grouped) {
            {
                std::lock_guard<std::mutex> lk(*s.ring_mu);
                s.ring_failed = false; s.track_last = std::min(s.next + n_rounds, s.in.n_frames - 1);
                if (!s.tracker.joinable()) s.tracker = std::thread(dyn_tracker_thread, R, std::ref(s));
            }
            s.ring_cv->notify_all();
        }
    // host thread t: member share t % T of the groups t / T, t / T + threads / T, ..., round after round and a last one that drains.  (Teams, T > 1: threads / T is the
    // group count, so the thread stays with group t / T.  T = 1: a thread's groups are t, t + threads, ...)
    const int T = R->threads_per_group;
    int rc = run_threads(R->threads, [&](int t) {
        int bad = 0;
        for (int r = 0; r <= n_rounds && !bad; ++r)
            for (size_t gi = t / T; gi < R->groups.size() && !bad; gi += R->threads / T) if (group_round(R, R->groups[gi], t % T, T, r == n_rounds)) bad = -1;
        if (bad && T > 1) R->groups[t / T].bar->failed.store(1);
        return bad;
    });
    for (auto& g : R->groups) if (g.bar) { g.bar->failed.store(0); g.bar->count.store(0); }
    // the call ends when every tracker has delivered its last frame of this call (or has failed); an estimator-side failure takes the bound back so that a parked tracker stays parked
    if (R->tracker_thread && n_rounds > 0)
        for (auto& s : R->seqs) if (s.dynamic && !s.grouped) {
            std::unique_lock<std::mutex> lk(*s.ring_mu);
            if (rc) s.track_last = s.tracked_next - 1;
            s.ring_cv->wait(lk, [&] { return !s.track_busy && (s.ring_failed || s.tracked_next > s.track_last || s.ring_count >= RSeq::RING); });
            if (s.ring_failed && !rc) rc = -1;
        }
    for (auto& s : R->seqs) (void)dv_sync(s.ctx);
    if (wall_seconds) *wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int dv_runner_get(dv_runner* R, int seq, dv_est_state* last, double* poses8, int cap, int* n_poses, long long* iterations, long long* frames, int* n_rows_last) {
    const RSeq* s = seq_at(R, seq);
    if (!s) return -1;
    if (last) *last = s->last;
    copy_rows(s->poses, 8, poses8, cap, n_poses);
    if (iterations) *iterations = s->iterations;
    if (frames) *frames = s->frames;
    if (n_rows_last) *n_rows_last = s->n_rows;
    return 0;
}

int dv_runner_get_frames(dv_runner* R, int seq, double* rows9, int cap, int* n_rows) {
    const RSeq* s = seq_at(R, seq);
    if (s) copy_rows(s->frames9, 9, rows9, cap, n_rows);
    return s ? 0 : -1;
}

int dv_runner_get_frame_clock(dv_runner* R, int seq, int which, double* seconds, int cap, int* n_out) {
    RSeq* s = seq_at(R, seq);
    if (!s) return -1;
    std::lock_guard<std::mutex> lk(*s->ring_mu);
    copy_rows(which == 1 ? s->track_clock : s->end_clock, 1, seconds, cap, n_out);
    return 0;
}

int dv_runner_get_row_log(dv_runner* R, int seq, unsigned long long* rows4, int cap, int* n_rows) {
    const RSeq* s = seq_at(R, seq);
    if (s) copy_rows(s->row_log, 4, rows4, cap, n_rows);
    return s ? 0 : -1;
}

// batched groups: switch the per-stage events of every group's dv_batch on / read their averages (dv_batch_timing), averaged over the groups
int dv_runner_batch_timing(dv_runner* R, int on, double* out3, long long* rounds, int* windows) {
    if (!R) return -1;
    double acc[3] = { 0, 0, 0 }; long long n = 0; int w = 0, ng = 0;
    for (auto& g : R->groups) if (g.batch) {
        double o[3]; long long r = 0; int ww = 0;
        if (dv_batch_timing(g.batch, on, o, &r, &ww)) return -1;
        if (r > 0) { for (int k = 0; k < 3; ++k) acc[k] += o[k]; n += r; w = ww; ++ng; }
    }
    if (out3) for (int k = 0; k < 3; ++k) out3[k] = ng ? acc[k] / ng : 0.0;
    if (rounds) *rounds = n;
    if (windows) *windows = w;
    return 0;
}

// diagnostics: rounds of the groups' dv_batch objects that shared their launches / that fell back to every member's own launches (dv_batch_info), summed
int dv_runner_batch_rounds(dv_runner* R, long long* batched_rounds, long long* single_rounds) {
    if (!R) return -1;
    long long a = 0, b = 0;
    for (auto& g : R->groups) if (g.batch) { long long x = 0, y = 0; if (dv_batch_info(g.batch, &x, &y)) return -1; a += x; b += y; }
    if (batched_rounds) *batched_rounds = a;
    if (single_rounds) *single_rounds = b;
    return 0;
}

// A dynamic sequence inside a dv_batch group (RSeq::grouped): the one-thread order of seq_begin whatever "tracker_thread" says, its window solve in the group's shared
// slots, its object solve in the group's ONE object launch (both deferred by the estimator calls, launched by dv_batch_enqueue), its background tracking in the group's
// shared tracking launches (group_track; its own launches with "batch_front" 0 or a static-report lag of 1), InstsTrack and the extra-point stages in its own launches.
int dv_runner_set_dynamic(dv_runner* R, int seq, const dv_seq_dynamic* dyn) {
    RSeq* sp = seq_at(R, seq);
    if (!sp || !dyn) return -1;
    RSeq& s = *sp;
    if (seq_started(s)) return set_err(R, "dv_runner_set_dynamic: the sequence has already started");
    if (!s.ctx->inst) return set_err(R, "dv_runner_set_dynamic: call dv_inst_config on the sequence's context first");
    if (dyn->inv_mask && dyn->mask_mem != s.in.mem) return set_err(R, "dv_runner_set_dynamic: mask_mem must equal the frames' mem (dv_track_stereo_enqueue takes frames and mask from one memory kind)");
    s.dynamic = true; s.live = false; s.live_stack = false; s.dyn = *dyn; s.static_unmask = dyn->static_as_background != 0;
    for (auto& b : s.db) b.reserve();
    for (auto& b : s.ring) b.reserve();
    return 0;
}
// A label-image sequence: the dynamic loop above with T1's stage inside it (viode_collect / viode_stage around seq_enqueue's calls)
int dv_runner_set_viode(dv_runner* R, int seq, const dv_seq_viode* v) {
    RSeq* sp = seq_at(R, seq);
    if (!sp || !v) return -1;
    RSeq& s = *sp;
    if (s.grouped) return set_err(R, "dv_runner_set_viode: a sequence of a dv_batch group is not supported (the group's shared unmask launch reads host masks)");
    if (seq_started(s)) return set_err(R, "dv_runner_set_viode: the sequence has already started");
    if (!dv_viode_frame_enqueue || !dv_viode_frame_collect || !dv_track_unmask_static_keys || !dv_inst_track_enqueue_keys) return set_err(R, "dv_runner_set_viode: the label-image entries are not linked into this build");
    if (!s.ctx->inst) return set_err(R, "dv_runner_set_viode: call dv_inst_config on the sequence's context first");
    if (!v->seg0 || !v->dyn_keys || v->nkeys < 1 || v->nkeys > 64) return set_err(R, "dv_runner_set_viode: label images and 1..64 dynamic keys are needed");
    if (!dv_mem_known(v->mem)) return set_err(R, "dv_runner_set_viode: unknown memory kind of the label images");
    if (s.in.mem != DV_MEM_DEVICE && s.in.mem != DV_MEM_PINNED) return set_err(R, "dv_runner_set_viode: the frames must be DV_MEM_DEVICE or DV_MEM_PINNED (the inverse mask stays on the device and travels with them)");
    if (s.stride != s.w) return set_err(R, "dv_runner_set_viode: the frames' row stride must equal the width (the inverse mask is tightly packed)");
    dv_seq_dynamic d{};          // what the stage does not produce per frame travels as in a dynamic sequence (track_input)
    d.mode = DV_MODE_SEMANTIC; d.disp = v->disp; d.disp_mem = v->disp_mem; d.disp_stride = v->disp_stride; d.baseline = v->baseline; d.static_as_background = v->static_as_background;
    if (dv_runner_set_dynamic(R, seq, &d)) return -1;
    s.live = true; s.live_stack = false; s.vio = *v; s.live_enq = -1; s.live_dets.assign(64, dv_inst_det{});
    return 0;
}
// A mask-stack sequence: the same loop with the detector branch of T1's stage inside it
int dv_runner_set_inst_stack(dv_runner* R, int seq, const dv_seq_stack* q) {
    RSeq* sp = seq_at(R, seq);
    if (!sp || !q) return -1;
    RSeq& s = *sp;
    if (s.grouped) return set_err(R, "dv_runner_set_inst_stack: a sequence of a dv_batch group is not supported (the group's shared unmask launch reads host masks)");
    if (seq_started(s)) return set_err(R, "dv_runner_set_inst_stack: the sequence has already started");
    if (!dv_inst_stack_frame_enqueue || !dv_inst_stack_frame_collect || !dv_track_unmask_static_planes || !dv_inst_track_enqueue_planes) return set_err(R, "dv_runner_set_inst_stack: the mask-stack entries are not linked into this build");
    if (!s.ctx->inst) return set_err(R, "dv_runner_set_inst_stack: call dv_inst_config on the sequence's context first");
    if (!q->stack || !q->n_planes || !q->track_id) return set_err(R, "dv_runner_set_inst_stack: per frame a stack, its number of planes and the planes' track ids are needed");
    if (q->kind != DV_STACK_U8 && q->kind != DV_STACK_F32) return set_err(R, "dv_runner_set_inst_stack: unknown element kind");
    if (!dv_mem_known(q->mem)) return set_err(R, "dv_runner_set_inst_stack: unknown memory kind of the stacks");
    for (int k = 0; k < s.in.n_frames; ++k)
        if (!q->stack[k] || !q->track_id[k] || q->n_planes[k] < 1 || q->n_planes[k] > DV_STACK_MAX_PLANES) return set_err(R, "dv_runner_set_inst_stack: every frame needs a stack of 1..64 planes and their track ids (a frame without instances: one empty plane)");
    if (s.in.mem != DV_MEM_DEVICE && s.in.mem != DV_MEM_PINNED) return set_err(R, "dv_runner_set_inst_stack: the frames must be DV_MEM_DEVICE or DV_MEM_PINNED (the inverse mask stays on the device and travels with them)");
    if (s.stride != s.w) return set_err(R, "dv_runner_set_inst_stack: the frames' row stride must equal the width (the inverse mask is tightly packed)");
    dv_seq_dynamic d{};          // what the stage does not produce per frame travels as in a dynamic sequence (track_input)
    d.mode = DV_MODE_SEMANTIC; d.boxes3d = q->boxes3d; d.n_boxes3d = q->n_boxes3d; d.disp = q->disp; d.disp_mem = q->disp_mem; d.disp_stride = q->disp_stride; d.baseline = q->baseline;
    d.static_as_background = q->static_as_background;
    if (dv_runner_set_dynamic(R, seq, &d)) return -1;
    s.live = true; s.live_stack = true; s.stk = *q; s.live_enq = -1; s.live_dets.assign(64, dv_inst_det{}); s.live_planes.assign(64, 0);
    return 0;
}
// slam_type naive over a sequence (system/main.cpp:263-265 FeatureTrack -> TrackImageNaive): per frame the inverse merged instance mask (0 = object) the tracker takes,
// in the frames' memory kind; mode DV_MODE_NAIVE (or DV_MODE_RAW with inv_mask NULL to go back).  The estimator stays the raw one.  Before the first dv_runner_run.
int dv_runner_set_mask(dv_runner* R, int seq, const uint8_t* const* inv_mask, int mask_mem, int mode) {
    RSeq* sp = seq_at(R, seq);
    if (!sp) return -1;
    RSeq& s = *sp;
    if (seq_started(s)) return set_err(R, "dv_runner_set_mask: the sequence has already started");
    if (mode != DV_MODE_RAW && mode != DV_MODE_NAIVE) return set_err(R, "dv_runner_set_mask: mode must be DV_MODE_RAW or DV_MODE_NAIVE (DV_MODE_SEMANTIC belongs to dv_runner_set_dynamic)");
    if (inv_mask && mask_mem != s.in.mem) return set_err(R, "dv_runner_set_mask: mask_mem must equal the frames' mem");
    if (s.dynamic) return set_err(R, "dv_runner_set_mask: the sequence is dynamic (its mask travels in dv_seq_dynamic)");
    s.raw_mask = inv_mask; s.raw_mode = mode;
    return 0;
}
int dv_runner_dynamic_stats(dv_runner* R, int seq, long long* detections, long long* object_features, long long* frames_with_objects, int* min_detections) {
    const RSeq* s = seq_at(R, seq);
    if (!s) return -1;
    if (detections) *detections = s->detections;
    if (object_features) *object_features = s->object_features;
    if (frames_with_objects) *frames_with_objects = s->frames_with_objects;
    if (min_detections) *min_detections = s->frames ? s->min_detections : 0;
    return 0;
}
int dv_runner_get_batches(dv_runner* R, dv_batch** out, int cap, int* n_out) {
    if (!R) return -1;
    int n = 0;
    for (auto& g : R->groups) if (g.batch) { if (out && n < cap) out[n] = g.batch; ++n; }
    if (n_out) *n_out = n;
    return 0;
}
// "tracker_thread" governs the dynamic sequences OUTSIDE dv_batch groups; a dynamic member of a group has the group's host thread (or its team thread) as its T3 and tracks on
// it: the one-thread order, bit-identical to the sequence's own run with group_size 0 and tracker_thread 0.
int dv_runner_set(dv_runner* R, const char* key, int value) {
    if (!R || !key) return -1;
    if (std::strcmp(key, "batch_front") == 0) { R->batch_front = value != 0; runner_layout(R); return 0; }      // (teams need the shared front end)
    if (std::strcmp(key, "tracker_thread") == 0) {          // dynamic sequences: T2 beside T3 (default) or the one-thread loop; before the first dv_runner_run
        for (auto& s : R->seqs) if (seq_started(s)) return set_err(R, "dv_runner_set: tracker_thread must be chosen before the first dv_runner_run");
        R->tracker_thread = value != 0; return 0;
    }
    if (std::strcmp(key, "teams") == 0) { R->teams = value != 0; runner_layout(R); return 0; }                  // before the first dv_runner_run; see dv_runner::teams
    return set_err(R, std::string("dv_runner_set: unknown key ") + key);
}
int dv_runner_track_info(dv_runner* R, long long* rounds, long long* members_batched, long long* members_single) {
    if (!R) return -1;
    long long a = 0, b = 0, c = 0;
    for (auto& g : R->groups) if (g.batch) { long long x = 0, y = 0, z = 0; if (dv_batch_track_info(g.batch, &x, &y, &z)) return -1; a += x; b += y; c += z; }
    if (rounds) *rounds = a;
    if (members_batched) *members_batched = b;
    if (members_single) *members_single = c;
    return 0;
}
const char* dv_runner_error(dv_runner* R) { return R ? R->err.c_str() : "null runner"; }

} // extern "C"
