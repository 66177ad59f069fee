// runner.hip — the per-frame host loop of the reference's threads T2 + T3 (system/main.cpp:178-330 FeatureTrack, :394-404 the estimator thread, the two queues
// between them) for one or many sequences, in C++ inside the library: dv_runner_*.  Host code only (no kernel here); everything goes through the public entries
// of include/dvins.h, so a runner is exactly what a caller could write against the ABI.
//
// One sequence (Pipeline of dynamic_vins_amd/pipeline.py, the order that overlaps the front end of frame k+1 with the back end of frame k on one host thread):
//     collect tracking(k) -> feed IMU up to t_k -> dv_est_process_begin(k) [host bookkeeping + enqueue of the window solve]
//     -> enqueue tracking(k+1) -> feed IMU up to t_k+1 -> dv_est_process_end(k) [wait, outlier rejection, slide]
// A DYNAMIC sequence runs the reference's two threads literally (dv_runner_set "tracker_thread", default on): T2 = a tracker thread (TrackSemanticImage + InstsTrack of
// frame after frame, collected into a small ring: the role of feature_queue, basic/feature_queue.h:19-73, blocking instead of dropping so that no frame is lost) beside
// T3 = the estimator loop on the calling thread (pop, IMU, window solve, object branch, end).  Tracker and estimator share nothing but the ring: the tracker API touches
// the context's tracker state and front-end streams, the estimator API its own state and the BA / object streams.
// Many sequences on one GPU (config 4 of BASELINE.json, "batched"): the sequences of a GROUP run their begin phases back to back, dv_batch_enqueue launches the
// iteration slots of all their window solves as one launch per stage, and while that runs the host turns to the next group; the end phases of a group follow when
// its turn comes again.  `threads` host threads each drive their own groups (the reference runs one process — three threads — per sequence).
// Dynamic sequences may be members of such a group: per member end(k-1), begin_ego(k), attach(k); then ONE dv_batch_enqueue launches the window slots AND the object solves
// of all members; then ONE dv_batch_track_enqueue tracks the background of frame k+1 of all members (TrackSemanticImage in the group's shared launches, the members' static
// instances unmasked by one launch) and every member enqueues InstsTrack(k+1) on its object tracker's stream; then every member collects its frame k+1 (dyn_post).  With
// "batch_front" 0, or a static-report lag of 1, a member enqueues tracking(k+1) itself between begin_ego(k) and attach(k), as a sequence outside a group does.
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
    struct DynBuf { std::vector<dv_feat> rows; int n_rows = 0; std::vector<dv_inst_obs> insts; int n_insts = 0; std::vector<dv_feat> ifeats; int n_ifeats = 0; std::vector<double> pts; int n_pts = 0; bool valid = false; };
    DynBuf db[2]; int cur = 0;
    // member of a dv_batch group: always the one-thread order (dyn_begin), and the collect of frame k+1's rows waits until the group has enqueued its round (dyn_post) —
    // the member's host thread must not sit in its own tracker's collect while the solves of the whole group are not launched yet
    bool grouped = false, collect_due = false; int collect_k1 = 0;
    // a frame of this dynamic sequence has been enqueued (by dyn_enqueue or by the group's shared launches): from then on it always has its next frame in flight or
    // collected when a round starts, so group_track's first-round pass has nothing to do for it — and does not look at the fields its team thread may be writing
    bool started = false;
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
    // TrackImageNaive over the sequence (dv_runner_set_mask): per frame the inverse merged instance mask, and the tracking mode that takes it
    const uint8_t* const* raw_mask = nullptr; int raw_mode = DV_MODE_RAW;
};
}
namespace {
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
    struct Group { std::vector<int> members; dv_batch* batch = nullptr; bool pending = false; std::unique_ptr<SpinBarrier> bar; };
    std::vector<Group> groups;
    int threads = 1, threads_per_group = 1;      // threads > groups: every dv_batch group is driven by threads / groups host threads that split its members' host phases (runner_team)
    bool teams = true;            // dv_runner_set "teams" (on by default since round 5: 100 of 100 runs of 16 sequences in four groups on eight threads bit-identical to the single-thread run, profiles/r05_experiments): several host threads per group.  First blamed for the round-4 trajectory defect, then cleared (the cause was the
                                  // accept decision's missing barrier, be_kernels.h be_accept_body); bit-identical to the single-thread run (tests/test_runner.py).
    int threads_requested = 1;
    bool tracker_thread = true;   // dynamic sequences: the reference's T2 beside T3 (dv_runner_set "tracker_thread"); 0 = the one-thread loop of round 4 (dyn_begin), kept for A/B and as the bit-identity reference
    bool batch_front = true;      // dv_batch groups: the members' tracking in shared launches too (dv_batch_track_enqueue); dv_runner_set(runner, "batch_front", 0) keeps one set of launches per sequence
    std::string err; std::mutex err_mu;
};

namespace {
void set_err(dv_runner* R, const std::string& m) { std::lock_guard<std::mutex> lk(R->err_mu); R->err = m; }      // several host threads drive their own groups: the shared message is guarded (per-sequence ones are each thread's own)
int fail(dv_runner* R, RSeq& s, const char* what) {
    const char* m = dv_last_error(s.ctx);
    s.err = std::string(what) + ": " + (m ? m : "");
    set_err(R, s.err);
    return -1;
}
int seq_enqueue(dv_runner* R, RSeq& s, int k) {
    if (dv_track_stereo_enqueue(s.ctx, s.in.left[k], s.in.right[k], s.w, s.h, s.stride, s.in.times[k], s.raw_mask ? s.raw_mask[k] : nullptr, s.raw_mode, s.in.mem)) return fail(R, s, "dv_track_stereo_enqueue");
    s.enqueued = true;
    return 0;
}
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
// ---- dynamic mode: TrackSemanticImage + InstsTrack of frame k (one enqueue), their collect, and the three-phase back end ----
// the three steps of frame k's enqueue: the static instances' rectangles staged for it | TrackSemanticImage | InstsTrack.  dyn_enqueue runs them back to back on the
// member's own stream; a dv_batch group with shared tracking launches (group_track) runs the first and the last per member around ONE dv_batch_track_enqueue
int dyn_stage_unmask(dv_runner* R, RSeq& s, int k) {
    const dv_seq_dynamic& d = s.dyn;
    if (s.static_unmask && d.inv_mask && d.dets && d.n_dets && d.n_dets[k] > 0) {
        std::vector<uint32_t> ids;
        { std::lock_guard<std::mutex> lk(*s.ring_mu); int best = -1; for (const RSeq::StaticSnap& sn : s.snaps) if (sn.frame >= 0 && sn.frame <= k - static_lag() && sn.frame > best) { best = sn.frame; ids = sn.ids; } }
        if (dv_track_unmask_static(s.ctx, d.dets[k], d.n_dets[k], ids.data(), (int)ids.size())) return fail(R, s, "dv_track_unmask_static");
    }
    return 0;
}
int dyn_enqueue_objects(dv_runner* R, RSeq& s, int k) {
    const dv_seq_dynamic& d = s.dyn;
    if (d.disp && d.disp[k] && dv_inst_set_disparity(s.ctx, d.disp[k], d.disp_stride, d.disp_mem, d.baseline)) return fail(R, s, "dv_inst_set_disparity");
    if (d.right_keys && d.right_keys[k] && dv_inst_set_right_keys(s.ctx, d.right_keys[k], 0, d.right_keys_mem)) return fail(R, s, "dv_inst_set_right_keys");
    if (dv_inst_track_enqueue(s.ctx, s.in.times[k], d.dets ? d.dets[k] : nullptr, d.n_dets ? d.n_dets[k] : 0, d.boxes3d ? d.boxes3d[k] : nullptr, d.n_boxes3d ? d.n_boxes3d[k] : 0)) return fail(R, s, "dv_inst_track_enqueue");
    s.enqueued = true; s.started = true;
    return 0;
}
// a label-image sequence (dv_runner_set_viode): T1's stage of frame k is collected (enqueued first, if frame k - 1 did not do it), then FeatureTrack's calls in their
// key-image forms, then T1's stage of frame k + 1 is enqueued behind them — its boxes arrive while the host is busy with frame k
int dyn_viode_stage(dv_runner* R, RSeq& s, int k) {
    const dv_seq_viode& v = s.vio;
    if (dv_viode_frame_enqueue(s.ctx, v.seg0[k], v.seg1 ? v.seg1[k] : nullptr, s.w, s.h, v.stride, v.mem, v.dyn_keys, v.nkeys)) return fail(R, s, "dv_viode_frame_enqueue");
    s.live_enq = k;
    return 0;
}
int dyn_enqueue_live(dv_runner* R, RSeq& s, int k) {
    const dv_seq_dynamic& d = s.dyn;
    if (s.live_enq != k && dyn_viode_stage(R, s, k)) return -1;
    s.live_enq = -1;
    if (dv_viode_frame_collect(s.ctx, s.vio.min_inst_size, s.live_dets.data(), (int)s.live_dets.size(), &s.live_n, &s.live_inv, &s.live_k0, &s.live_k1)) return fail(R, s, "dv_viode_frame_collect");
    if (s.static_unmask && s.live_n > 0) {
        std::vector<uint32_t> ids;
        { std::lock_guard<std::mutex> lk(*s.ring_mu); int best = -1; for (const RSeq::StaticSnap& sn : s.snaps) if (sn.frame >= 0 && sn.frame <= k - static_lag() && sn.frame > best) { best = sn.frame; ids = sn.ids; } }
        if (dv_track_unmask_static_keys(s.ctx, s.live_dets.data(), s.live_n, ids.data(), (int)ids.size(), s.live_k0, 0, DV_MEM_DEVICE)) return fail(R, s, "dv_track_unmask_static_keys");
    }
    if (dv_track_stereo_enqueue(s.ctx, s.in.left[k], s.in.right[k], s.w, s.h, s.stride, s.in.times[k], s.live_inv, DV_MODE_SEMANTIC, s.in.mem)) return fail(R, s, "dv_track_stereo_enqueue");
    if (d.disp && d.disp[k] && dv_inst_set_disparity(s.ctx, d.disp[k], d.disp_stride, d.disp_mem, d.baseline)) return fail(R, s, "dv_inst_set_disparity");
    if (s.live_k1 && dv_inst_set_right_keys(s.ctx, s.live_k1, 0, DV_MEM_DEVICE)) return fail(R, s, "dv_inst_set_right_keys");
    if (dv_inst_track_enqueue_keys(s.ctx, s.in.times[k], s.live_n ? s.live_dets.data() : nullptr, s.live_n, s.live_k0, 0, DV_MEM_DEVICE, nullptr, 0)) return fail(R, s, "dv_inst_track_enqueue_keys");
    s.enqueued = true; s.started = true;
    if (k + 1 < s.in.n_frames && dyn_viode_stage(R, s, k + 1)) return -1;
    return 0;
}
int dyn_enqueue(dv_runner* R, RSeq& s, int k) {
    if (s.live) return dyn_enqueue_live(R, s, k);
    const dv_seq_dynamic& d = s.dyn;
    const int mode = d.mode ? d.mode : DV_MODE_SEMANTIC;
    if (dyn_stage_unmask(R, s, k)) return -1;
    // (frames and mask share `mem` in dv_track_stereo_enqueue: a device-resident sequence keeps both in HBM)
    if (dv_track_stereo_enqueue(s.ctx, s.in.left[k], s.in.right[k], s.w, s.h, s.stride, s.in.times[k], d.inv_mask ? d.inv_mask[k] : nullptr, mode, s.in.mem)) return fail(R, s, "dv_track_stereo_enqueue");
    return dyn_enqueue_objects(R, s, k);
}
int dyn_collect(dv_runner* R, RSeq& s, RSeq::DynBuf& b) {
    if (dv_track_stereo_collect(s.ctx, b.rows.data(), &b.n_rows)) return fail(R, s, "dv_track_stereo_collect");
    if (dv_inst_track_collect(s.ctx, b.insts.data(), (int)b.insts.size(), &b.n_insts, b.ifeats.data(), (int)b.ifeats.size(), &b.n_ifeats, b.pts.data(), (int)(b.pts.size() / 3), &b.n_pts)) return fail(R, s, "dv_inst_track_collect");
    b.valid = true; s.enqueued = false;
    return 0;
}
// own_front = false: member of a dv_batch group whose tracking runs in the group's shared launches — group_track has enqueued frame k before the first round and
// enqueues frame k+1 behind the group's dv_batch_enqueue; what is left here is the order of the estimator calls and the hand-over to dyn_post
int dyn_begin(dv_runner* R, RSeq& s, bool own_front = true) {
    const int k = s.next;
    if (k >= s.in.n_frames) { s.err = "sequence exhausted"; set_err(R, s.err); return -1; }
    RSeq::DynBuf& b = s.db[s.cur];
    if (!b.valid) {
        if (!s.enqueued) { if (!own_front) { s.err = "internal: frame not enqueued"; set_err(R, s.err); return -1; } if (dyn_enqueue(R, s, k)) return -1; }
        if (dyn_collect(R, s, b)) return -1;
    }
    const double t = s.in.times[k];
    s.n_rows = b.n_rows;
    if (s.in.ba_stride > 1 && (k % s.in.ba_stride) != 0) {      // tracked only: both trackers have seen the frame, the back end has not (system/main.cpp:300-312: frames 0, 2, 4, ... outside KITTI)
        if (k + 1 < s.in.n_frames) {
            if (own_front && dyn_enqueue(R, s, k + 1)) return -1;
            if (s.grouped) { s.collect_due = true; s.collect_k1 = k + 1; }
            else if (dyn_collect(R, s, s.db[s.cur ^ 1])) return -1;
        }
        b.valid = false; s.cur ^= 1; ++s.next; s.skipped = true;
        return dyn_passed(R, s, k, false);
    }
    s.skipped = false;
    if (seq_feed_imu(R, s, t)) return -1;
    // the window solve goes to the GPU with the background rows alone; then the next frame's tracking (thread T2 of the reference, independent of T3); then the object
    // branch of ProcessImage beside the window solve; then the next frame's rows are collected while the solve is still in flight
    const int rc = dv_est_process_dynamic_begin_ego(s.ctx, b.rows.data(), b.n_rows, t);
    if (rc < 0) return fail(R, s, "dv_est_process_dynamic_begin_ego");
    if (rc > 0) { s.err = "IMU stream does not cover the frame"; set_err(R, s.err); return -1; }
    if (own_front && k + 1 < s.in.n_frames && dyn_enqueue(R, s, k + 1)) return -1;
    if (dv_est_process_dynamic_attach(s.ctx, b.n_insts ? b.insts.data() : nullptr, b.n_insts, b.n_ifeats ? b.ifeats.data() : nullptr, b.n_pts ? b.pts.data() : nullptr)) return fail(R, s, "dv_est_process_dynamic_attach");
    s.detections += b.n_insts; s.object_features += b.n_ifeats; s.frames_with_objects += b.n_insts > 0; s.min_detections = std::min(s.min_detections, b.n_insts);
    if (dyn_passed(R, s, k, true)) return -1;
    if (k + 1 < s.in.n_frames) {
        if (s.grouped) { s.collect_due = true; s.collect_k1 = k + 1; }      // behind the group's dv_batch_enqueue: dyn_post
        else {
            if (seq_feed_imu(R, s, s.in.times[k + 1])) return -1;
            if (dyn_collect(R, s, s.db[s.cur ^ 1])) return -1;
        }
    }
    b.valid = false; s.cur ^= 1;
    s.pending = true; s.pending_t = t;
    return 0;
}
// a dynamic member of a dv_batch group, behind the group's dv_batch_enqueue: what dyn_begin left out — the IMU samples up to frame k+1 and the collect of its rows (into the
// buffer dyn_begin has already made the current one)
int dyn_post(dv_runner* R, RSeq& s) {
    if (!s.collect_due) return 0;
    s.collect_due = false;
    if (!s.skipped && seq_feed_imu(R, s, s.in.times[s.collect_k1])) return -1;
    return dyn_collect(R, s, s.db[s.cur]);
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
        RSeq::DynBuf& b = s.ring[slot];
        const bool bad = dyn_enqueue(R, s, f) || dyn_collect(R, s, b);
        {
            std::lock_guard<std::mutex> lk(*s.ring_mu);
            if (bad) s.ring_failed = true;
            else { if (s.ring_count == 0) s.ring_head = f; ++s.ring_count; ++s.tracked_next; s.track_clock.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count()); }
        }
        s.ring_cv->notify_all();
    }
}
// T3, first half of a step: frame k from the ring -> IMU -> window solve -> object branch -> IMU up to k+1 (the same estimator calls in the same order as dyn_begin)
int dyn_begin_threaded(dv_runner* R, RSeq& s) {
    const int k = s.next;
    if (k >= s.in.n_frames) { s.err = "sequence exhausted"; set_err(R, s.err); return -1; }
    RSeq::DynBuf* bp;
    {
        std::unique_lock<std::mutex> lk(*s.ring_mu);
        s.ring_cv->wait(lk, [&] { return s.ring_count > 0 || s.ring_failed; });
        if (s.ring_failed) return -1;
        if (s.ring_head != k) { s.err = "internal: the tracker ring is out of step with the estimator"; set_err(R, s.err); return -1; }
        bp = &s.ring[s.ring_pos];
    }
    RSeq::DynBuf& b = *bp;
    const double t = s.in.times[k];
    s.n_rows = b.n_rows;
    if (s.in.ba_stride > 1 && (k % s.in.ba_stride) != 0) {      // tracked only (see dyn_begin): the slot goes back to the tracker unread
        { std::lock_guard<std::mutex> lk(*s.ring_mu); b.valid = false; s.ring_pos = (s.ring_pos + 1) % RSeq::RING; --s.ring_count; ++s.ring_head; }
        s.ring_cv->notify_all();
        ++s.next; s.skipped = true;
        return dyn_passed(R, s, k, false);
    }
    s.skipped = false;
    if (seq_feed_imu(R, s, t)) return -1;
    const int rc = dv_est_process_dynamic_begin_ego(s.ctx, b.rows.data(), b.n_rows, t);
    if (rc < 0) return fail(R, s, "dv_est_process_dynamic_begin_ego");
    if (rc > 0) { s.err = "IMU stream does not cover the frame"; set_err(R, s.err); return -1; }
    if (dv_est_process_dynamic_attach(s.ctx, b.n_insts ? b.insts.data() : nullptr, b.n_insts, b.n_ifeats ? b.ifeats.data() : nullptr, b.n_pts ? b.pts.data() : nullptr)) return fail(R, s, "dv_est_process_dynamic_attach");
    s.detections += b.n_insts; s.object_features += b.n_ifeats; s.frames_with_objects += b.n_insts > 0; s.min_detections = std::min(s.min_detections, b.n_insts);
    {   // the estimator has taken what it needs of the slot (rows, detections, feature rows and points are copied into its own tables by the two calls above)
        std::lock_guard<std::mutex> lk(*s.ring_mu);
        b.valid = false; s.ring_pos = (s.ring_pos + 1) % RSeq::RING; --s.ring_count; ++s.ring_head;
    }
    s.ring_cv->notify_all();
    if (dyn_passed(R, s, k, true)) return -1;
    if (k + 1 < s.in.n_frames && seq_feed_imu(R, s, s.in.times[k + 1])) return -1;
    s.pending = true; s.pending_t = t;
    return 0;
}

// Do the dynamic members of a dv_batch group track in the group's shared launches?  With shared tracking launches on, and a static-report lag of two frames or more:
// the shared launches of frame k+1 come BEHIND the object branch of frame k (dyn_passed), where the member's own enqueue comes before it — with lag 1 the snapshot of
// frame k would be read in one order and not in the other, so lag 1 keeps the enqueue inside dyn_begin (fourth finding).  A constant of the run.
bool dyn_shares_front(const dv_runner* R) { return R->batch_front && static_lag() >= 2; }
// first half of a step: everything up to and including the enqueue of frame k's window solve and of frame k+1's tracking.  own_front = false: the caller enqueues
// the tracking of the group's frames itself, in shared launches (group_round), and feeds the IMU samples of frame k+1 afterwards.
int seq_begin(dv_runner* R, RSeq& s, bool own_front = true) {
    if (s.dynamic) return (R->tracker_thread && !s.grouped) ? dyn_begin_threaded(R, s) : dyn_begin(R, s, own_front || !dyn_shares_front(R));      // (a group member tracks on the group's host thread: the ring is a group_size 0 feature)
    const int k = s.next;
    if (k >= s.in.n_frames) { s.err = "sequence exhausted"; set_err(R, s.err); return -1; }
    if (!s.enqueued) { if (!own_front) { s.err = "internal: frame not enqueued"; set_err(R, s.err); return -1; } if (seq_enqueue(R, s, k)) return -1; }
    if (dv_track_stereo_collect(s.ctx, s.rows.data(), &s.n_rows)) return fail(R, s, "dv_track_stereo_collect");
    s.enqueued = false;
    // what the back end is handed: frame index + a hash of the collected rows (row log: the bit-identity checks compare it run against run).  Taken BEHIND the enqueue of the
    // window solve — a byte-serial FNV over 32 KB was 20 - 25 us on the path between two frames' solves — and over 64-bit words
    auto hash_rows = [&]() {
        static_assert(sizeof(dv_feat) % 8 == 0, "rows are hashed as 64-bit words");
        unsigned long long h = 1469598103934665603ull; const unsigned long long* p = reinterpret_cast<const unsigned long long*>(s.rows.data());
        for (size_t i = 0, n = (size_t)s.n_rows * sizeof(dv_feat) / 8; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
        s.cur_rows_hash = h; s.cur_k = k;
    };
    const double t = s.in.times[k];
    const int stride = s.in.ba_stride > 1 ? s.in.ba_stride : 1;
    if (stride > 1 && (k % stride) != 0) {      // tracked only: outside KITTI the reference pushes a frame to feature_queue when cnt % 2 == 0, cnt counting tracked frames from 0 (system/main.cpp:181,300-312): frames 0, 2, 4, ...
        if (own_front && k + 1 < s.in.n_frames && seq_enqueue(R, s, k + 1)) return -1;
        hash_rows();
        ++s.next; s.skipped = true;
        return 0;
    }
    s.skipped = false;
    if (seq_feed_imu(R, s, t)) return -1;
    const int rc = dv_est_process_begin(s.ctx, s.rows.data(), s.n_rows, t);
    if (rc < 0) return fail(R, s, "dv_est_process_begin");
    if (rc > 0) { s.err = "IMU stream does not cover the frame"; set_err(R, s.err); return -1; }
    if (own_front && k + 1 < s.in.n_frames) { if (seq_enqueue(R, s, k + 1) || seq_feed_imu(R, s, s.in.times[k + 1])) return -1; }
    hash_rows();
    s.pending = true; s.pending_t = t;
    return 0;
}
// the tracking of frame `s.next + ahead` of every member of a dv_batch group in shared launches (dv_batch_track_enqueue)
// Dynamic members (dyn_shares_front): per member its static instances' rectangles are staged first (dv_track_unmask_static, the snapshot dyn_enqueue would pick), then the
// ONE dv_batch_track_enqueue, then per member InstsTrack of the same frame on its object tracker's own stream (dv_inst_track_enqueue: not shared, like the extra-point stages).
int group_track(dv_runner* R, dv_runner::Group& g, int ahead) {
    std::vector<dv_track_job> jobs;
    const bool dyn_shared = dyn_shares_front(R);
    for (size_t m = 0; m < g.members.size(); ++m) {
        RSeq& s = R->seqs[g.members[m]];
        // `enqueued` first: in a team round thread 0 comes here (ahead = 0) while its teammates may still be inside seq_end of THEIR members, advancing s.next — every
        // member is `enqueued` then (set by this thread in the previous round, two barriers ago) and its counters are not looked at.  Reading s.next before this test was a
        // data race ThreadSanitizer reported (tests/host/runner_tsan.cpp); the value read was never used, so no result depended on it.
        // A dynamic member's flags (`enqueued`, its buffers) are written by dyn_post, which a teammate may still be running for the previous round: in the first-round pass
        // `started` alone is read — written by this thread or before the threads started — and a started member is left alone.
        if (s.dynamic ? (!dyn_shared || (ahead == 0 && s.started)) : s.enqueued) continue;          // (dynamic member with its own front end: it enqueues its tracking inside dyn_begin)
        const int k = s.next + ahead - (s.skipped && ahead ? 1 : 0);      // (a track-only frame has already advanced s.next)
        if (k >= s.in.n_frames) continue;
        dv_track_job j{};
        j.member = (int)m; j.mem = s.in.mem; j.gray0 = s.in.left[k]; j.gray1 = s.in.right[k]; j.stride = s.stride; j.t = s.in.times[k];
        if (s.dynamic) {
            if (s.enqueued) continue;
            if (dyn_stage_unmask(R, s, k)) return -1;
            j.mode = s.dyn.mode ? s.dyn.mode : DV_MODE_SEMANTIC; j.mask = s.dyn.inv_mask ? s.dyn.inv_mask[k] : nullptr;
        } else { j.mode = s.raw_mode; j.mask = s.raw_mask ? s.raw_mask[k] : nullptr; }      // (naive members with masks share the round's launches when the round holds two or more naive / semantic jobs; a lone one keeps its own: dv_batch_track_enqueue)
        jobs.push_back(j);
    }
    if (jobs.empty()) return 0;
    if (dv_batch_track_enqueue(g.batch, jobs.data(), (int)jobs.size())) { const char* m = dv_last_error(R->seqs[g.members[0]].ctx); set_err(R, std::string("dv_batch_track_enqueue: ") + (m ? m : "")); return -1; }
    for (const dv_track_job& j : jobs) {
        RSeq& s = R->seqs[g.members[j.member]];
        if (s.dynamic) { if (dyn_enqueue_objects(R, s, s.next + ahead - (s.skipped && ahead ? 1 : 0))) return -1; }      // (sets `enqueued`)
        else s.enqueued = true;
    }
    return 0;
}
// last phase of a group's round, behind dv_batch_enqueue and the shared tracking launches: the IMU samples up to the member's next frame (and, dynamic member, its rows)
int seq_post(dv_runner* R, RSeq& s) {
    if (s.dynamic) return dyn_post(R, s);
    const int k1 = s.next + (s.skipped ? 0 : 1);
    return (!s.skipped && k1 < s.in.n_frames) ? seq_feed_imu(R, s, s.in.times[k1]) : 0;
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
int group_round(dv_runner* R, dv_runner::Group& g) {
    if (g.pending) { for (int i : g.members) if (seq_end(R, R->seqs[i])) return -1; g.pending = false; }
    if (g.batch && R->batch_front) {
        // a dv_batch group with shared front-end launches: (first round only) track frame k of all members; per member collect k + begin k; ONE enqueue of the
        // window solves' slots; ONE set of tracking launches for the members' frames k+1; then their IMU samples up to k+1
        if (group_track(R, g, 0)) return -1;
        for (int i : g.members) if (seq_begin(R, R->seqs[i], false)) return -1;
        if (dv_batch_enqueue(g.batch)) { set_err(R, std::string("dv_batch_enqueue: ") + (dv_last_error(R->seqs[g.members[0]].ctx) ? dv_last_error(R->seqs[g.members[0]].ctx) : "")); return -1; }
        if (group_track(R, g, 1)) return -1;
        for (int i : g.members) if (seq_post(R, R->seqs[i])) return -1;
        g.pending = true;
        return 0;
    }
    for (int i : g.members) if (seq_begin(R, R->seqs[i])) return -1;
    if (g.batch && dv_batch_enqueue(g.batch)) { set_err(R, std::string("dv_batch_enqueue: ") + (dv_last_error(R->seqs[g.members[0]].ctx) ? dv_last_error(R->seqs[g.members[0]].ctx) : "")); return -1; }
    for (int i : g.members) if (dyn_post(R, R->seqs[i])) return -1;      // (raw members have fed their samples inside seq_begin)
    g.pending = true;
    return 0;
}
// One round of a dv_batch group driven by a TEAM of host threads: thread `j` of `T` does the host phases (end of frame k-1, collect + begin of frame k, IMU feed) of
// members j, j + T, ...; thread 0 issues the shared launches (the window solves' slots, the tracking of the members' next frames) between two barriers.  The window
// solves of a LARGE group share every launch (kernel efficiency) while its host work — ~0.1 ms per member and frame, serial in group_round — runs T wide.
int team_round(dv_runner* R, dv_runner::Group& g, int j, int T, bool last) {
    SpinBarrier& B = *g.bar;
    int rc = 0;
    auto mine = [&](auto f) { for (size_t m = j; m < g.members.size() && !rc; m += T) if (f(R->seqs[g.members[m]])) rc = -1; };
    // (no look at g.pending here: seq_end is a no-op for a member without a frame in flight, and the group's flag is written by thread 0 alone — in the drain round,
    //  which has no barrier, a teammate could otherwise read the flag after thread 0 cleared it and skip its members' last frames)
    mine([&](RSeq& s) { return seq_end(R, s); });
    if (!last) {
        if (j == 0 && !rc && group_track(R, g, 0)) rc = -1;          // (first round only: nothing is enqueued yet)
        if (rc) B.failed.store(1);
        if (!B.wait()) return -1;                                      // every member collected its previous frame; frame k of all members is enqueued
        mine([&](RSeq& s) { return seq_begin(R, s, false); });
        if (rc) B.failed.store(1);
        if (!B.wait()) return -1;                                      // all begins (uploads on the group's stream) are in
        if (j == 0) {
            if (dv_batch_enqueue(g.batch)) { set_err(R, std::string("dv_batch_enqueue: ") + (dv_last_error(R->seqs[g.members[0]].ctx) ? dv_last_error(R->seqs[g.members[0]].ctx) : "")); rc = -1; }
            if (!rc && group_track(R, g, 1)) rc = -1;
            g.pending = true;
        }
        if (rc) B.failed.store(1);
        if (!B.wait()) return -1;                                      // the next frames are enqueued (their `enqueued` flags are set)
        mine([&](RSeq& s) { return seq_post(R, s); });
    }          // (drain round: g.pending is cleared behind the join in dv_runner_run)
    if (rc) B.failed.store(1);
    return rc;
}
int group_drain(dv_runner* R, dv_runner::Group& g) {
    if (g.pending) { for (int i : g.members) if (seq_end(R, R->seqs[i])) return -1; g.pending = false; }
    return 0;
}
}

namespace {
// host threads: one per group (at most `threads_requested`), or — opt-in only, dv_runner::teams — threads_requested / groups per dv_batch group
void runner_layout(dv_runner* R) {
    const int ng = (int)R->groups.size(), threads = R->threads_requested;
    bool all_batched = R->batch_front; for (auto& g : R->groups) if (!g.batch) all_batched = false;
    R->threads_per_group = 1;
    for (auto& g : R->groups) g.bar.reset();
    if (R->teams && threads > ng && all_batched && threads % ng == 0) {
        R->threads = threads; R->threads_per_group = threads / ng;
        for (auto& g : R->groups) { g.bar = std::make_unique<SpinBarrier>(); g.bar->n = R->threads_per_group; }
    } else R->threads = std::max(1, std::min(threads, ng));
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
    if (n_rounds < 0) { R->err = "dv_runner_run: negative round count"; return -1; }
    for (auto& s : R->seqs) if (s.next + n_rounds > s.in.n_frames) { R->err = "dv_runner_run: a sequence has fewer frames left than rounds asked"; return -1; }
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
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
    auto drive = [&](int first, int step) -> int {          // one host thread: its groups, round after round
        for (int r = 0; r < n_rounds; ++r) for (size_t gi = first; gi < R->groups.size(); gi += step) if (group_round(R, R->groups[gi])) return -1;
        for (size_t gi = first; gi < R->groups.size(); gi += step) if (group_drain(R, R->groups[gi])) return -1;
        return 0;
    };
    if (R->threads_per_group > 1 && R->batch_front) {
        const int T = R->threads_per_group;
        std::vector<std::thread> th; std::vector<int> rcs(R->threads, 0);
        for (int t = 0; t < R->threads; ++t) th.emplace_back([&, t] {
            dv_runner::Group& g = R->groups[t / T];
            const int j = t % T;
            for (int r = 0; r < n_rounds && !rcs[t]; ++r) if (team_round(R, g, j, T, false)) rcs[t] = -1;
            if (!rcs[t] && team_round(R, g, j, T, true)) rcs[t] = -1;      // drain: the members' last frames
            if (rcs[t]) g.bar->failed.store(1);
        });
        for (auto& t : th) t.join();
        for (int v : rcs) if (v) rc = -1;
        for (auto& g : R->groups) { g.pending = false; g.bar->failed.store(0); g.bar->count.store(0); }
    }
    else if (R->threads <= 1) rc = drive(0, 1);
    else {
        std::vector<std::thread> th; std::vector<int> rcs(R->threads, 0);
        for (int t = 0; t < R->threads; ++t) th.emplace_back([&, t] { rcs[t] = drive(t, R->threads); });
        for (auto& t : th) t.join();
        for (int v : rcs) if (v) rc = -1;
    }
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
    if (!R || seq < 0 || seq >= (int)R->seqs.size()) return -1;
    const RSeq& s = R->seqs[seq];
    if (last) *last = s.last;
    const int n = (int)(s.poses.size() / 8);
    if (n_poses) *n_poses = n;
    if (poses8) std::memcpy(poses8, s.poses.data(), sizeof(double) * 8 * (size_t)std::min(n, std::max(cap, 0)));
    if (iterations) *iterations = s.iterations;
    if (frames) *frames = s.frames;
    if (n_rows_last) *n_rows_last = s.n_rows;
    return 0;
}

int dv_runner_get_frames(dv_runner* R, int seq, double* rows9, int cap, int* n_rows) {
    if (!R || seq < 0 || seq >= (int)R->seqs.size()) return -1;
    const RSeq& s = R->seqs[seq];
    const int n = (int)(s.frames9.size() / 9);
    if (n_rows) *n_rows = n;
    if (rows9) std::memcpy(rows9, s.frames9.data(), sizeof(double) * 9 * (size_t)std::min(n, std::max(cap, 0)));
    return 0;
}

int dv_runner_get_frame_clock(dv_runner* R, int seq, int which, double* seconds, int cap, int* n_out) {
    if (!R || seq < 0 || seq >= (int)R->seqs.size()) return -1;
    RSeq& s = R->seqs[seq];
    std::lock_guard<std::mutex> lk(*s.ring_mu);
    const std::vector<double>& v = which == 1 ? s.track_clock : s.end_clock;
    const int n = (int)v.size();
    if (n_out) *n_out = n;
    if (seconds) std::memcpy(seconds, v.data(), sizeof(double) * (size_t)std::min(n, std::max(cap, 0)));
    return 0;
}

int dv_runner_get_row_log(dv_runner* R, int seq, unsigned long long* rows4, int cap, int* n_rows) {
    if (!R || seq < 0 || seq >= (int)R->seqs.size()) return -1;
    const RSeq& s = R->seqs[seq];
    const int n = (int)(s.row_log.size() / 4);
    if (n_rows) *n_rows = n;
    if (rows4) std::memcpy(rows4, s.row_log.data(), sizeof(unsigned long long) * 4 * (size_t)std::min(n, std::max(cap, 0)));
    return 0;
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

// A dynamic sequence inside a dv_batch group (RSeq::grouped): the one-thread order of dyn_begin whatever "tracker_thread" says, its window solve in the group's shared
// slots, its object solve in the group's ONE object launch (both deferred by the estimator calls, launched by dv_batch_enqueue), its background tracking in the group's
// shared tracking launches (group_track; its own launches with "batch_front" 0 or a static-report lag of 1), InstsTrack and the extra-point stages in its own launches.
int dv_runner_set_dynamic(dv_runner* R, int seq, const dv_seq_dynamic* dyn) {
    if (!R || seq < 0 || seq >= (int)R->seqs.size() || !dyn) return -1;
    RSeq& s = R->seqs[seq];
    if (s.next != 0 || s.enqueued || s.pending) { R->err = "dv_runner_set_dynamic: the sequence has already started"; return -1; }
    if (!s.ctx->inst) { R->err = "dv_runner_set_dynamic: call dv_inst_config on the sequence's context first"; return -1; }
    if (dyn->inv_mask && dyn->mask_mem != s.in.mem) { R->err = "dv_runner_set_dynamic: mask_mem must equal the frames' mem (dv_track_stereo_enqueue takes frames and mask from one memory kind)"; return -1; }
    s.dynamic = true; s.live = false; s.dyn = *dyn; s.static_unmask = dyn->static_as_background != 0;
    for (auto& b : s.db) { b.rows.resize(DV_MAX_FEATS); b.insts.resize(64); b.ifeats.resize(64 * 256); b.pts.resize((size_t)3 * 65536); b.valid = false; }
    for (auto& b : s.ring) { b.rows.resize(DV_MAX_FEATS); b.insts.resize(64); b.ifeats.resize(64 * 256); b.pts.resize((size_t)3 * 65536); b.valid = false; }
    return 0;
}
// A label-image sequence: the dynamic loop above with T1's stage inside it (dyn_enqueue_live)
int dv_runner_set_viode(dv_runner* R, int seq, const dv_seq_viode* v) {
    if (!R || seq < 0 || seq >= (int)R->seqs.size() || !v) return -1;
    RSeq& s = R->seqs[seq];
    if (s.grouped) { R->err = "dv_runner_set_viode: a sequence of a dv_batch group is not supported (the group's shared unmask launch reads host masks)"; return -1; }
    if (s.next != 0 || s.enqueued || s.pending || s.tracked_next != 0) { R->err = "dv_runner_set_viode: the sequence has already started"; return -1; }
    if (!dv_viode_frame_enqueue || !dv_viode_frame_collect || !dv_track_unmask_static_keys || !dv_inst_track_enqueue_keys) { R->err = "dv_runner_set_viode: the label-image entries are not linked into this build"; return -1; }
    if (!s.ctx->inst) { R->err = "dv_runner_set_viode: call dv_inst_config on the sequence's context first"; return -1; }
    if (!v->seg0 || !v->dyn_keys || v->nkeys < 1 || v->nkeys > 64) { R->err = "dv_runner_set_viode: label images and 1..64 dynamic keys are needed"; return -1; }
    if (v->mem != DV_MEM_HOST && v->mem != DV_MEM_DEVICE && v->mem != DV_MEM_PINNED) { R->err = "dv_runner_set_viode: unknown memory kind of the label images"; return -1; }
    if (s.in.mem != DV_MEM_DEVICE && s.in.mem != DV_MEM_PINNED) { R->err = "dv_runner_set_viode: the frames must be DV_MEM_DEVICE or DV_MEM_PINNED (the inverse mask stays on the device and travels with them)"; return -1; }
    if (s.stride != s.w) { R->err = "dv_runner_set_viode: the frames' row stride must equal the width (the inverse mask is tightly packed)"; return -1; }
    s.dynamic = true; s.live = true; s.vio = *v; s.live_enq = -1; s.live_dets.assign(64, dv_inst_det{});
    s.dyn = dv_seq_dynamic{}; s.dyn.mode = DV_MODE_SEMANTIC; s.dyn.disp = v->disp; s.dyn.disp_mem = v->disp_mem; s.dyn.disp_stride = v->disp_stride; s.dyn.baseline = v->baseline;
    s.dyn.static_as_background = v->static_as_background; s.static_unmask = v->static_as_background != 0;
    for (auto& b : s.db) { b.rows.resize(DV_MAX_FEATS); b.insts.resize(64); b.ifeats.resize(64 * 256); b.pts.resize((size_t)3 * 65536); b.valid = false; }
    for (auto& b : s.ring) { b.rows.resize(DV_MAX_FEATS); b.insts.resize(64); b.ifeats.resize(64 * 256); b.pts.resize((size_t)3 * 65536); b.valid = false; }
    return 0;
}
// slam_type naive over a sequence (system/main.cpp:263-265 FeatureTrack -> TrackImageNaive): per frame the inverse merged instance mask (0 = object) the tracker takes,
// in the frames' memory kind; mode DV_MODE_NAIVE (or DV_MODE_RAW with inv_mask NULL to go back).  The estimator stays the raw one.  Before the first dv_runner_run.
int dv_runner_set_mask(dv_runner* R, int seq, const uint8_t* const* inv_mask, int mask_mem, int mode) {
    if (!R || seq < 0 || seq >= (int)R->seqs.size()) return -1;
    RSeq& s = R->seqs[seq];
    if (s.next != 0 || s.enqueued || s.pending) { R->err = "dv_runner_set_mask: the sequence has already started"; return -1; }
    if (mode != DV_MODE_RAW && mode != DV_MODE_NAIVE) { R->err = "dv_runner_set_mask: mode must be DV_MODE_RAW or DV_MODE_NAIVE (DV_MODE_SEMANTIC belongs to dv_runner_set_dynamic)"; return -1; }
    if (inv_mask && mask_mem != s.in.mem) { R->err = "dv_runner_set_mask: mask_mem must equal the frames' mem"; return -1; }
    if (s.dynamic) { R->err = "dv_runner_set_mask: the sequence is dynamic (its mask travels in dv_seq_dynamic)"; return -1; }
    s.raw_mask = inv_mask; s.raw_mode = mode;
    return 0;
}
int dv_runner_dynamic_stats(dv_runner* R, int seq, long long* detections, long long* object_features, long long* frames_with_objects, int* min_detections) {
    if (!R || seq < 0 || seq >= (int)R->seqs.size()) return -1;
    const RSeq& s = R->seqs[seq];
    if (detections) *detections = s.detections;
    if (object_features) *object_features = s.object_features;
    if (frames_with_objects) *frames_with_objects = s.frames_with_objects;
    if (min_detections) *min_detections = s.frames ? s.min_detections : 0;
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
// it: dyn_begin's order, bit-identical to the sequence's own run with group_size 0 and tracker_thread 0.
int dv_runner_set(dv_runner* R, const char* key, int value) {
    if (!R || !key) return -1;
    if (std::strcmp(key, "batch_front") == 0) { R->batch_front = value != 0; runner_layout(R); return 0; }      // (teams need the shared front end)
    if (std::strcmp(key, "tracker_thread") == 0) {          // dynamic sequences: T2 beside T3 (default) or the one-thread loop; before the first dv_runner_run
        for (auto& s : R->seqs) if (s.next != 0 || s.enqueued || s.pending || s.tracked_next != 0) { R->err = "dv_runner_set: tracker_thread must be chosen before the first dv_runner_run"; return -1; }
        R->tracker_thread = value != 0; return 0;
    }
    if (std::strcmp(key, "teams") == 0) { R->teams = value != 0; runner_layout(R); return 0; }                  // before the first dv_runner_run; see dv_runner::teams
    R->err = std::string("dv_runner_set: unknown key ") + key;
    return -1;
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
