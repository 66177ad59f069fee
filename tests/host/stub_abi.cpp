// stub_abi.cpp — a STAND-IN for libdvins_hip.so's C ABI for the ThreadSanitizer builds of the host-side machinery (tests/host/Makefile `tsan`): no GPU, no HIP
// runtime under TSan.  Every entry point the C++ runner (dynamic_vins_amd/csrc/runner.hip) and the header shim's concurrent surface (host/dvins_shim.hpp) call is
// here, doing three things instead of launching kernels:
//   * a state machine per context that refuses a call sequence the real library would refuse (enqueue twice, collect without enqueue, end without begin ...);
//   * plain (non-atomic) scratch words per context DOMAIN — tracker, estimator, IMU buffer — written by every call that touches that domain in the real library:
//     two host threads inside the same domain of one context without a happens-before edge are a data race TSan reports (the ABI's rule: "one ctx per thread",
//     relaxed by runner.hip to "tracker API on T2, estimator API on T3" for a dynamic sequence);
//   * deterministic outputs (functions of the frame index and of what the call was handed) after a short sleep, so that every threading layout of the runner must
//     produce the same logs as its single-thread loop.
// DVSTUB_FAIL="<ctx index>:<frame>" makes dv_est_process_begin of that context fail at that frame: the failure path through the team barriers.
// dvstub_trace(1 | 2) switches a CALL TRACE on: per context and domain (and per dv_batch) one record per entry called — its name, time argument, integer counts and
// modes, the id list of the unmask entries, and of every pointer only whether it is null; nothing derived from an address.  dvstub_trace_report(label) prints per
// (label, context, domain) the call count and the 64-bit FNV-1a of the records (level 2: the records too), so that the order of the ABI calls of two builds of
// runner.hip can be compared (tests/test_runner_calls.py against tests/golden/runner_calls_*.txt).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include "dv_ctx.h"

namespace {
struct Stub {
    int index = 0;
    // tracker domain
    int trk_scratch = 0; bool trk_pending = false; int trk_frame = 0; double trk_t = 0; unsigned long long trk_in = 0, unmask_hash = 0;
    bool inst_pending = false; int inst_frame = 0;
    // estimator domain
    int est_scratch = 0; bool begun = false, ego_begun = false; int est_frame = 0; unsigned long long est_hash = 0; double est_t = 0;
    // IMU-buffer domain
    int imu_scratch = 0; long long imu_n = 0; double imu_sum = 0, imu_last_t = -1;
    // call trace: the records of the three domains (appended by the thread that is inside the domain, like the scratch words)
    std::string calls[3]; long long n_calls[3] = { 0, 0, 0 };
};
std::mutex g_mu; std::unordered_map<dv_ctx*, Stub*> g_map; std::vector<dv_ctx*> g_order;
std::string g_err; std::atomic<long long> g_violations{0};
int g_fail_ctx = -1, g_fail_frame = -1, g_next_index = 0;

Stub& S(dv_ctx* c) { return *g_map.at(c); }      // (no lock: the map is complete before any thread starts, and a lock here would order the very accesses TSan is to judge)
void work(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }
int violation(const char* what) { g_violations.fetch_add(1); std::lock_guard<std::mutex> lk(g_mu); g_err = what; return -1; }
unsigned long long mix(unsigned long long h, unsigned long long v) { h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2); return h; }
unsigned long long bits(double d) { unsigned long long u; std::memcpy(&u, &d, 8); return u; }
// ---- call trace ----
enum { TRK = 0, EST = 1, IMU = 2 };
int g_trace = 0; size_t g_run_first = 0;
struct BatchCalls { std::string calls; long long n = 0; };
std::vector<BatchCalls> g_batch_calls;          // per dv_batch of the run, in creation order (a dv_batch dies with its runner, before the report)
void append(std::string& to, long long& n, const char* fmt, va_list ap) { char buf[4096]; std::vsnprintf(buf, sizeof buf, fmt, ap); to += buf; to += '\n'; ++n; }
std::string id_list(const uint32_t* ids, int n) { std::string o = "["; for (int i = 0; i < n; ++i) { if (i) o += ' '; o += std::to_string(ids[i]); } return o + "]"; }
}
void dvstub_record(dv_ctx* c, int domain, const char* fmt, ...) {          // (also called by stub_viode.cpp)
    if (!g_trace) return;
    Stub& s = S(c); va_list ap; va_start(ap, fmt); append(s.calls[domain], s.n_calls[domain], fmt, ap); va_end(ap);
}
namespace {
void batch_record(int index, const char* fmt, ...) {
    if (!g_trace) return;
    BatchCalls& b = g_batch_calls[index]; va_list ap; va_start(ap, fmt); append(b.calls, b.n, fmt, ap); va_end(ap);
}
void report_line(const char* label, const char* what, int index, const char* domain, const std::string& calls, long long n) {
    unsigned long long h = 1469598103934665603ull;
    for (unsigned char ch : calls) { h ^= ch; h *= 1099511628211ull; }
    std::printf("calls '%s' %s %d %s n=%lld fnv=%016llx\n", label, what, index, domain, n, h);
    if (g_trace > 1) for (size_t a = 0; a < calls.size();) { const size_t e = calls.find('\n', a); std::printf("call '%s' %s %d %s: %s\n", label, what, index, domain, calls.substr(a, e - a).c_str()); a = e + 1; }
}
}

// GCC 11's libtsan has no interceptor for pthread_cond_clockwait (what std::condition_variable::wait_for / wait_until(steady_clock) call on glibc >= 2.30): TSan then
// never sees the mutex released inside the wait and reports "double lock" and phantom races on everything the mutex guards.  The harness binaries route the call
// through pthread_cond_timedwait, which IS intercepted (test infrastructure only; the product is not built with this file).
#if defined(__SANITIZE_THREAD__)
#include <pthread.h>
#include <time.h>
extern "C" int pthread_cond_clockwait(pthread_cond_t* cond, pthread_mutex_t* mutex, clockid_t clock, const struct timespec* abstime) {
    struct timespec now_c, now_r, abs_r;
    clock_gettime(clock, &now_c); clock_gettime(CLOCK_REALTIME, &now_r);
    long long rel = (abstime->tv_sec - now_c.tv_sec) * 1000000000ll + (abstime->tv_nsec - now_c.tv_nsec);
    if (rel < 0) rel = 0;
    const long long t = now_r.tv_sec * 1000000000ll + now_r.tv_nsec + rel;
    abs_r.tv_sec = t / 1000000000ll; abs_r.tv_nsec = t % 1000000000ll;
    return pthread_cond_timedwait(cond, mutex, &abs_r);
}
#endif

void dv_set_error(dv_ctx*, const std::string& m) { std::lock_guard<std::mutex> lk(g_mu); g_err = m; }

extern "C" {
long long dvstub_violations() { return g_violations.load(); }
void dvstub_new_run() { g_next_index = 0; g_run_first = g_order.size(); g_batch_calls.clear(); }          // the contexts created from here on are numbered from 0 again (DVSTUB_FAIL addresses them per run)
void dvstub_trace(int level) { g_trace = level; }          // 0 = off (default), 1 = digests, 2 = digests + records
void dvstub_trace_report(const char* label) {          // the run's contexts and batches (everything created since dvstub_new_run), behind dv_runner_destroy
    if (!g_trace) return;
    static const char* const dom[3] = { "tracker", "estimator", "imu" };
    for (size_t i = g_run_first; i < g_order.size(); ++i) { const Stub& s = S(g_order[i]); for (int d = 0; d < 3; ++d) report_line(label, "ctx", s.index, dom[d], s.calls[d], s.n_calls[d]); }
    for (size_t i = 0; i < g_batch_calls.size(); ++i) report_line(label, "batch", (int)i, "batch", g_batch_calls[i].calls, g_batch_calls[i].n);
    std::fflush(stdout);
}
dv_ctx* dvstub_ctx(int w, int h, int dynamic) {          // what dv_create + dv_est_create (+ dv_inst_config) leave as far as runner.hip looks
    static int dummy_est, dummy_inst;
    if (const char* e = std::getenv("DVSTUB_FAIL")) std::sscanf(e, "%d:%d", &g_fail_ctx, &g_fail_frame);
    dv_ctx* c = new dv_ctx();
    c->cfg.width = w; c->cfg.height = h;
    c->est = reinterpret_cast<dv_estimator*>(&dummy_est);
    if (dynamic) c->inst = reinterpret_cast<dv_inst_tracker*>(&dummy_inst);
    std::lock_guard<std::mutex> lk(g_mu);
    Stub* s = new Stub(); s->index = g_next_index++; g_map[c] = s; g_order.push_back(c);
    return c;
}
const char* dv_last_error(dv_ctx*) { static thread_local std::string mine; std::lock_guard<std::mutex> lk(g_mu); mine = g_err; return mine.c_str(); }
int dv_sync(dv_ctx* c) { dvstub_record(c, EST, "dv_sync"); return 0; }          // (recorded with the estimator: the runner calls it behind its host threads' join)

// ---------------- tracker domain ----------------
int dv_track_stereo_enqueue(dv_ctx* c, const uint8_t* g0, const uint8_t* g1, int w, int h, int stride, double t, const uint8_t* mask, int mode, int mem) {
    Stub& s = S(c); s.trk_scratch++;
    dvstub_record(c, TRK, "dv_track_stereo_enqueue t=%.17g w=%d h=%d stride=%d mode=%d mem=%d g0=%d g1=%d mask=%d", t, w, h, stride, mode, mem, g0 != nullptr, g1 != nullptr, mask != nullptr);
    if (s.trk_pending) return violation("dv_track_stereo_enqueue: previous frame not collected");
    s.trk_pending = true; s.trk_t = t; s.trk_in = mix(mix(mix(mix((unsigned long long)(uintptr_t)g0, (unsigned long long)(uintptr_t)g1), (unsigned long long)(uintptr_t)mask), (unsigned long long)mode), s.unmask_hash);
    s.unmask_hash = 0;
    work(30);
    return 0;
}
int dv_track_stereo_collect(dv_ctx* c, dv_feat* out, int* n_out) {
    Stub& s = S(c); s.trk_scratch++;
    dvstub_record(c, TRK, "dv_track_stereo_collect out=%d n_out=%d", out != nullptr, n_out != nullptr);
    if (!s.trk_pending) return violation("dv_track_stereo_collect: nothing enqueued");
    work(60);
    const int n = 5 + s.trk_frame % 7;
    for (int i = 0; i < n; ++i) { dv_feat f{}; f.id = (uint32_t)(s.trk_frame * 100 + i); f.track_cnt = s.trk_frame + 1; f.left[0] = s.trk_t; f.left[1] = (double)(s.trk_in & 0xffff); f.left[3] = i; out[i] = f; }
    if (n_out) *n_out = n;
    s.trk_pending = false; s.trk_frame++;
    return 0;
}
int dv_inst_set_disparity(dv_ctx* c, const float* d, int stride, int mem, double baseline) { Stub& s = S(c); s.trk_scratch++; dvstub_record(c, TRK, "dv_inst_set_disparity stride=%d mem=%d baseline=%.17g disp=%d", stride, mem, baseline, d != nullptr); return 0; }
int dv_inst_set_right_keys(dv_ctx* c, const uint32_t* k, int stride, int mem) { Stub& s = S(c); s.trk_scratch++; dvstub_record(c, TRK, "dv_inst_set_right_keys stride=%d mem=%d keys=%d", stride, mem, k != nullptr); return 0; }
int dv_track_unmask_static(dv_ctx* c, const dv_inst_det* dets, int n_dets, const uint32_t* ids, int n) {          // the ids travel into the next frame's input hash: every layout must hand over the same list
    Stub& s = S(c); s.trk_scratch++;
    if (g_trace) dvstub_record(c, TRK, "dv_track_unmask_static n_dets=%d n_static=%d ids=%s dets=%d", n_dets, n, id_list(ids, n).c_str(), dets != nullptr);
    if (s.trk_pending) return violation("dv_track_unmask_static: behind the frame's enqueue");
    s.unmask_hash = 0x51ed; for (int i = 0; i < n; ++i) s.unmask_hash = mix(s.unmask_hash, ids[i]);
    return 0;
}
int dv_inst_track_enqueue(dv_ctx* c, double t, const dv_inst_det* dets, int n_dets, const dv_box3d* boxes, int n_boxes) {
    Stub& s = S(c); s.trk_scratch++;
    dvstub_record(c, TRK, "dv_inst_track_enqueue t=%.17g n_dets=%d n_boxes=%d dets=%d boxes=%d", t, n_dets, n_boxes, dets != nullptr, boxes != nullptr);
    if (s.inst_pending) return violation("dv_inst_track_enqueue: previous frame not collected");
    s.inst_pending = true; work(20);
    return 0;
}
int dv_inst_track_collect(dv_ctx* c, dv_inst_obs* insts, int cap_insts, int* n_insts, dv_feat* feats, int cap_feats, int* n_feats, double* points, int cap_points, int* n_points) {
    Stub& s = S(c); s.trk_scratch++;
    dvstub_record(c, TRK, "dv_inst_track_collect cap_insts=%d cap_feats=%d cap_points=%d insts=%d feats=%d points=%d", cap_insts, cap_feats, cap_points, insts != nullptr, feats != nullptr, points != nullptr);
    if (!s.inst_pending) return violation("dv_inst_track_collect: nothing enqueued");
    work(40);
    const int ni = 1 + s.inst_frame % 3, per = 4;
    if (ni > cap_insts || ni * per > cap_feats || ni * 2 > cap_points) return violation("dv_inst_track_collect: buffers too small");
    for (int i = 0; i < ni; ++i) { dv_inst_obs o{}; o.id = (uint32_t)(10 + i); o.first_feat = i * per; o.n_feats = per; o.first_point = 2 * i; o.n_points = 2; insts[i] = o; }
    for (int i = 0; i < ni * per; ++i) { dv_feat f{}; f.id = (uint32_t)(s.inst_frame * 1000 + i); f.left[0] = s.inst_frame; feats[i] = f; }
    for (int i = 0; i < ni * 2 * 3; ++i) points[i] = s.inst_frame + 0.25 * i;
    *n_insts = ni; *n_feats = ni * per; *n_points = ni * 2;
    s.inst_pending = false; s.inst_frame++;
    return 0;
}

// ---------------- IMU buffer + estimator domains ----------------
int dv_est_input_imu(dv_ctx* c, double t, const double* acc, const double* gyr) {
    Stub& s = S(c); s.imu_scratch++;
    dvstub_record(c, IMU, "dv_est_input_imu t=%.17g acc=%d gyr=%d", t, acc != nullptr, gyr != nullptr);
    if (t <= s.imu_last_t) return violation("dv_est_input_imu: samples out of order");
    s.imu_last_t = t; s.imu_n++; s.imu_sum += acc[0] + 2 * acc[1] + 3 * acc[2] + 5 * gyr[0] + 7 * gyr[1] + 11 * gyr[2];
    return 0;
}
int dv_est_imu_available(dv_ctx* c, double t) { Stub& s = S(c); s.imu_scratch++; return s.imu_last_t >= t ? 1 : 0; }
int dv_est_get_latest(dv_ctx* c, double* t, double* P, double* Q, double* V) { Stub& s = S(c); s.imu_scratch++; if (t) *t = s.imu_last_t; for (int k = 0; k < 3; ++k) { P[k] = s.imu_sum; V[k] = 0; } Q[0] = Q[1] = Q[2] = 0; Q[3] = 1; return s.imu_n ? 0 : 1; }
static int begin_common(Stub& s, const dv_feat* rows, int n, double t) {
    s.est_scratch++; s.imu_scratch++;
    if (s.begun) return violation("dv_est_process_begin: previous frame not ended");
    if (s.index == g_fail_ctx && s.est_frame == g_fail_frame) { std::lock_guard<std::mutex> lk(g_mu); g_err = "stub: injected failure"; return -1; }
    unsigned long long h = mix(bits(t), (unsigned long long)n);
    for (int i = 0; i < n; ++i) h = mix(mix(h, rows[i].id), bits(rows[i].left[0]));
    h = mix(mix(h, (unsigned long long)s.imu_n), bits(s.imu_sum));
    s.est_hash = h; s.est_t = t; s.begun = true;
    work(50);
    return 0;
}
int dv_est_process_begin(dv_ctx* c, const dv_feat* rows, int n, double t) { dvstub_record(c, EST, "dv_est_process_begin t=%.17g n=%d rows=%d", t, n, rows != nullptr); return begin_common(S(c), rows, n, t); }
int dv_est_process_dynamic_begin_ego(dv_ctx* c, const dv_feat* rows, int n, double t) { Stub& s = S(c); dvstub_record(c, EST, "dv_est_process_dynamic_begin_ego t=%.17g n=%d rows=%d", t, n, rows != nullptr); const int rc = begin_common(s, rows, n, t); if (!rc) s.ego_begun = true; return rc; }
int dv_est_process_dynamic_attach(dv_ctx* c, const dv_inst_obs* insts, int n_insts, const dv_feat* feats, const double* points) {
    Stub& s = S(c); s.est_scratch++;
    dvstub_record(c, EST, "dv_est_process_dynamic_attach n_insts=%d insts=%d feats=%d points=%d", n_insts, insts != nullptr, feats != nullptr, points != nullptr);
    if (!s.ego_begun) return violation("dv_est_process_dynamic_attach: no ego solve in flight");
    s.ego_begun = false;
    for (int i = 0; i < n_insts; ++i) { s.est_hash = mix(s.est_hash, insts[i].id); for (int k = 0; k < insts[i].n_feats; ++k) s.est_hash = mix(s.est_hash, feats[insts[i].first_feat + k].id); for (int k = 0; k < 3 * insts[i].n_points; ++k) s.est_hash = mix(s.est_hash, bits(points[3 * insts[i].first_point + k])); }
    work(40);
    return 0;
}
int dv_est_process_end(dv_ctx* c, dv_est_state* out) {
    Stub& s = S(c); s.est_scratch++;
    dvstub_record(c, EST, "dv_est_process_end out=%d", out != nullptr);
    if (!s.begun) return violation("dv_est_process_end: nothing begun");
    if (s.ego_begun) return violation("dv_est_process_end: the object branch was not attached");
    work(80);
    dv_est_state st{};
    st.frame = s.est_frame; st.nonlinear = s.est_frame >= 3; st.iterations = 1 + (int)(s.est_hash % 5);
    for (int k = 0; k < 7; ++k) st.window[10][k] = (double)((s.est_hash >> (8 * k)) & 0xff) + s.est_t;
    if (out) *out = st;
    s.begun = false; s.est_frame++;
    return 0;
}
int dv_est_process(dv_ctx* c, const dv_feat* rows, int n, double t, dv_est_state* out) {          // the shim's one-call form
    Stub& s = S(c);
    if (s.imu_last_t < t) { s.imu_scratch++; return 1; }          // the IMU stream does not cover the frame yet
    if (begin_common(s, rows, n, t)) return -1;
    return dv_est_process_end(c, out);
}
int dv_est_set_lines(dv_ctx* c, const dv_line_row*, int) { S(c).est_scratch++; return 0; }
int dv_est_get_static_instances(dv_ctx* c, uint32_t* ids, int cap, int* n) {          // "static" instances as a function of the frames processed so far
    Stub& s = S(c); s.est_scratch++;
    dvstub_record(c, EST, "dv_est_get_static_instances cap=%d ids=%d n=%d", cap, ids != nullptr, n != nullptr);
    const int k = std::min(cap, s.est_frame % 3);
    for (int i = 0; i < k; ++i) ids[i] = (uint32_t)(10 + (s.est_frame + i) % 3);
    *n = k;
    return 0;
}

// ---------------- dv_batch: the shared launches touch every member ----------------
struct dv_batch { std::vector<dv_ctx*> m; long long rounds = 0, track_rounds = 0, members = 0; int index = 0; };
dv_batch* dv_batch_create(dv_ctx* const* ctxs, int n) { dv_batch* b = new dv_batch(); b->m.assign(ctxs, ctxs + n); b->index = (int)g_batch_calls.size(); g_batch_calls.emplace_back(); return b; }
void dv_batch_destroy(dv_batch* b) { delete b; }
int dv_batch_enqueue(dv_batch* b) {
    batch_record(b->index, "dv_batch_enqueue");
    for (dv_ctx* c : b->m) { Stub& s = S(c); s.est_scratch++; if (s.begun == false) { /* a member without a frame this round: allowed */ } }
    b->rounds++; work(40);
    return 0;
}
int dv_batch_track_enqueue(dv_batch* b, const dv_track_job* jobs, int n) {
    batch_record(b->index, "dv_batch_track_enqueue n=%d jobs=%d", n, jobs != nullptr);
    for (int i = 0; i < n; ++i) batch_record(b->index, "  job member=%d t=%.17g stride=%d mode=%d mem=%d gray0=%d gray1=%d mask=%d", jobs[i].member, jobs[i].t, jobs[i].stride, jobs[i].mode, jobs[i].mem, jobs[i].gray0 != nullptr, jobs[i].gray1 != nullptr, jobs[i].mask != nullptr);
    for (int i = 0; i < n; ++i) {
        if (jobs[i].member < 0 || jobs[i].member >= (int)b->m.size()) return violation("dv_batch_track_enqueue: member index out of range");
        if (dv_track_stereo_enqueue(b->m[jobs[i].member], jobs[i].gray0, jobs[i].gray1, 0, 0, 0, jobs[i].t, jobs[i].mask, jobs[i].mode, jobs[i].mem)) return -1;
    }
    b->track_rounds++; b->members += n;
    return 0;
}
int dv_batch_info(dv_batch* b, long long* a, long long* s) { if (a) *a = b->rounds; if (s) *s = 0; return 0; }
int dv_batch_track_info(dv_batch* b, long long* r, long long* mb, long long* ms) { if (r) *r = b->track_rounds; if (mb) *mb = b->members; if (ms) *ms = 0; return 0; }
int dv_batch_timing(dv_batch*, int, double* o, long long* r, int* w) { if (o) o[0] = o[1] = o[2] = 0; if (r) *r = 0; if (w) *w = 0; return 0; }

// ---------------- what the header shim's classes call besides the above (host/dvins_shim.hpp): construction, the one-call forms, the getters ----------------
dv_ctx* dv_create(const dv_config* cfg) { dv_ctx* c = dvstub_ctx(cfg ? cfg->width : 64, cfg ? cfg->height : 48, 0); if (cfg) c->cfg = *cfg; return c; }
void dv_destroy(dv_ctx*) {}
int dv_est_create(dv_ctx* c, const dv_est_config*) { S(c).est_scratch++; return 0; }
int dv_est_reset(dv_ctx* c) { Stub& s = S(c); s.est_scratch++; s.imu_scratch++; s.begun = s.ego_begun = false; s.est_frame = 0; s.imu_n = 0; s.imu_sum = 0; s.imu_last_t = -1; return 0; }
int dv_est_change_sensor_type(dv_ctx* c, int, int) { S(c).est_scratch++; return 0; }
int dv_est_get_lines(dv_ctx* c, dv_line_landmark*, int, int* n) { S(c).est_scratch++; if (n) *n = 0; return 0; }
int dv_est_get_landmarks(dv_ctx* c, dv_landmark*, int, int* n) { S(c).est_scratch++; if (n) *n = 0; return 0; }
int dv_est_get_instances(dv_ctx* c, dv_inst_state*, int, int* n, double*) { S(c).est_scratch++; if (n) *n = 0; return 0; }
int dv_est_process_dynamic(dv_ctx* c, const dv_feat* rows, int n, double t, const dv_inst_obs* insts, int n_insts, const dv_feat* feats, const double* points, dv_est_state* out) {
    Stub& s = S(c);
    if (s.imu_last_t < t) { s.imu_scratch++; return 1; }
    if (dv_est_process_dynamic_begin_ego(c, rows, n, t) || dv_est_process_dynamic_attach(c, insts, n_insts, feats, points)) return -1;
    return dv_est_process_end(c, out);
}
int dv_track_stereo(dv_ctx* c, const uint8_t* g0, const uint8_t* g1, int w, int h, int stride, double t, const uint8_t* mask, int mode, int mem, dv_feat* out, int* n_out) {
    if (dv_track_stereo_enqueue(c, g0, g1, w, h, stride, t, mask, mode, mem)) return -1;
    return dv_track_stereo_collect(c, out, n_out);
}
void* dv_pinned_alloc(size_t n) { return std::malloc(n); }
void dv_pinned_free(void* p) { std::free(p); }
int dv_inst_config(dv_ctx* c, int, int, int) { S(c).trk_scratch++; return 0; }
int dv_undistort_lines(dv_ctx*, const dv_cam*, const float*, int, double*) { return 0; }
int dv_set_undistort_maps(dv_ctx* c, int, const int16_t*, const uint16_t*, int, int) { S(c).trk_scratch++; return 0; }
int dv_remap(dv_ctx* c, const uint8_t*, int, int, int, int, const int16_t*, const uint16_t*, uint8_t*, int) { S(c).trk_scratch++; return 0; }
int dv_obj_solve(dv_ctx* c, dv_obj_problem*, dv_ba_summary*) { S(c).est_scratch++; return 0; }
}
