// runner_group_tsan.cpp — ThreadSanitizer harness of dv_batch groups WITH DYNAMIC MEMBERS in the library's C++ host loop (dynamic_vins_amd/csrc/runner.hip compiled as
// plain C++ with -fsanitize=thread) on the stand-in C ABI of stub_abi.cpp; the recipe of runner_tsan.cpp, which covers raw groups and ungrouped dynamic sequences.
// A dynamic member of a group runs the one-thread order on the group's host thread — or on its team thread: end(k-1) | begin_ego(k), enqueue tracking(k+1),
// attach(k) | ONE dv_batch_enqueue | collect tracking(k+1) — between the team's barriers, beside raw members whose tracking thread 0 enqueues in shared launches.
// The stub's outputs are functions of what every call was handed, so every layout must leave, per sequence, the logs of that sequence's own one-thread loop
// (group_size 0, tracker_thread 0); TSan reports what the bit-identity checks of tests/test_runner_dynamic_group.py cannot see.
//   runner_group_tsan layouts | fail [--calls | --calls-full]       (--calls: per run, context and domain the digest of the stub's call trace)        exit 0 = logs identical / failure reported without a hang; TSan's own exit code (66) on a report
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "dvins.h"

extern "C" dv_ctx* dvstub_ctx(int w, int h, int dynamic);
extern "C" long long dvstub_violations();
extern "C" void dvstub_new_run();
extern "C" void dvstub_trace(int level);
extern "C" void dvstub_trace_report(const char* label);

namespace {
struct Seq {
    std::vector<const uint8_t*> left, right; std::vector<double> times, imu_t, imu_a, imu_g;
    std::vector<const uint8_t*> masks; std::vector<const dv_inst_det*> dets; std::vector<int32_t> n_dets; dv_inst_det one_det{};
    dv_seq_input in{}; dv_seq_dynamic dyn{};
};
void make_seq(Seq& q, int frames, int id) {
    static uint8_t pixel[4096];
    for (int k = 0; k < frames; ++k) { q.left.push_back(pixel + (id * 64 + k) % 4000); q.right.push_back(pixel + (id * 64 + k + 7) % 4000); q.times.push_back(1.0 + 0.05 * k); q.masks.push_back(pixel + k % 100); q.dets.push_back(&q.one_det); q.n_dets.push_back(1); }
    q.one_det.track_id = 10; q.one_det.w = q.one_det.h = 4; q.one_det.mask = pixel;
    for (int i = 0; i < frames * 10 + 20; ++i) { q.imu_t.push_back(0.9 + 0.005 * i); for (int c = 0; c < 3; ++c) { q.imu_a.push_back(0.01 * i + c + id); q.imu_g.push_back(0.02 * i - c); } }
    q.in.left = q.left.data(); q.in.right = q.right.data(); q.in.times = q.times.data(); q.in.n_frames = frames; q.in.mem = DV_MEM_DEVICE; q.in.stride = 0; q.in.ba_stride = 1;
    q.in.imu_t = q.imu_t.data(); q.in.imu_acc = q.imu_a.data(); q.in.imu_gyr = q.imu_g.data(); q.in.n_imu = (int)q.imu_t.size();
    q.dyn.inv_mask = q.masks.data(); q.dyn.mask_mem = DV_MEM_DEVICE; q.dyn.mode = DV_MODE_SEMANTIC; q.dyn.dets = q.dets.data(); q.dyn.n_dets = q.n_dets.data();
}
struct Log { std::vector<double> frames; std::vector<unsigned long long> rows; long long iterations = 0; };
// the mix of a group of four: member 3 of every four is a raw sequence, member 1 feeds its static report back into its tracking, member 2 sends every 2nd frame to the back end
// (mix 1: member 2 feeds its static report back too — every 2nd frame to the back end AND the snapshot lookup)
bool is_dynamic(int i) { return i % 4 != 3; }
std::string g_label;          // the call trace's name of the next run
int run_layout(int n, int frames, int group, int threads, int teams, int batch_front, int tracker_thread, const std::vector<int>& cuts, std::vector<Log>& out, bool expect_fail = false, int mix = 0) {
    std::vector<Seq> seqs(n); std::vector<dv_ctx*> ctxs; std::vector<dv_seq_input> in;
    dvstub_new_run();
    for (int i = 0; i < n; ++i) {
        make_seq(seqs[i], frames, i);
        if (i % 4 == 1) seqs[i].dyn.static_as_background = 1;
        if (i % 4 == 2) { seqs[i].in.ba_stride = 2; if (mix == 1) seqs[i].dyn.static_as_background = 1; }
        ctxs.push_back(dvstub_ctx(64, 48, is_dynamic(i))); in.push_back(seqs[i].in);
    }
    dv_runner* R = dv_runner_create(ctxs.data(), in.data(), n, group, threads);
    if (!R) { std::fprintf(stderr, "dv_runner_create failed\n"); return 2; }
    dv_runner_set(R, "teams", teams); dv_runner_set(R, "batch_front", batch_front); dv_runner_set(R, "tracker_thread", tracker_thread);
    for (int i = 0; i < n; ++i) if (is_dynamic(i) && dv_runner_set_dynamic(R, i, &seqs[i].dyn)) { std::fprintf(stderr, "set_dynamic: %s\n", dv_runner_error(R)); return 2; }
    int rc = 0;
    for (int c : cuts) if ((rc = dv_runner_run(R, c, nullptr)) != 0) break;
    if (expect_fail) { dv_runner_destroy(R); return rc ? 0 : 3; }
    if (rc) { std::fprintf(stderr, "dv_runner_run: %s\n", dv_runner_error(R)); dv_runner_destroy(R); return 2; }
    out.assign(n, Log{});
    for (int i = 0; i < n; ++i) {
        out[i].frames.resize(9 * (size_t)frames); int nf = 0; dv_runner_get_frames(R, i, out[i].frames.data(), frames, &nf); out[i].frames.resize(9 * (size_t)nf);
        out[i].rows.resize(4 * (size_t)frames); int nr = 0; dv_runner_get_row_log(R, i, out[i].rows.data(), frames, &nr); out[i].rows.resize(4 * (size_t)nr);
        long long fr = 0; dv_runner_get(R, i, nullptr, nullptr, 0, nullptr, &out[i].iterations, &fr, nullptr);
    }
    dv_batch* b[8]; int nb = 0;
    if (dv_runner_get_batches(R, b, 8, &nb) || nb != (group > 1 ? (n + group - 1) / group : 0)) { std::fprintf(stderr, "dv_runner_get_batches: %d groups\n", nb); dv_runner_destroy(R); return 2; }
    dv_runner_destroy(R);
    dvstub_trace_report(g_label.c_str());
    return 0;
}
bool same(const std::vector<Log>& a, const std::vector<Log>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].frames != b[i].frames || a[i].rows != b[i].rows || a[i].iterations != b[i].iterations || a[i].frames.empty()) return false;
    return true;
}
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "layouts";
    std::thread watchdog([] { std::this_thread::sleep_for(std::chrono::seconds(240)); std::fprintf(stderr, "runner_group_tsan: HANG (watchdog)\n"); std::_Exit(9); });
    watchdog.detach();
    int bad = 0;
    for (int a = 1; a < argc; ++a) { if (!std::strcmp(argv[a], "--calls")) dvstub_trace(1); else if (!std::strcmp(argv[a], "--calls-full")) dvstub_trace(2); }          // the stub's call trace: digests / records per run (not for `fail`)
    if (mode == "layouts") {
        const int n = 8, frames = 36;
        std::vector<Log> ref, got;
        g_label = "group reference";
        if (run_layout(n, frames, 0, 1, 0, 1, 0, { frames }, ref)) return 2;                                  // every sequence's own one-thread loop: the reference
        struct L { int group, threads, teams, batch_front, tracker; std::vector<int> cuts; const char* name; };
        const L layouts[] = { { 4, 1, 0, 1, 1, { frames }, "two groups on one thread" }, { 4, 2, 0, 1, 1, { frames }, "one thread per group" }, { 4, 2, 0, 0, 0, { 20, 16 }, "one thread per group, own tracking launches, two calls" },
                              { 4, 4, 1, 1, 1, { frames }, "teams of two" }, { 4, 8, 1, 1, 0, { 7, 1, 13, 15 }, "teams of four, four calls" }, { 8, 4, 1, 1, 1, { 1, 1, 1, 33 }, "one group, team of four, one-frame calls" },
                              { 3, 3, 0, 1, 1, { frames }, "groups of three (the last one of two)" } };
        for (int mix = 0; mix <= 1; ++mix) {
            const std::string tag = mix ? "ba_stride 2 with static feedback: " : "";
            if (mix) { g_label = tag + "reference"; if (run_layout(n, frames, 0, 1, 0, 1, 0, { frames }, ref, false, mix)) return 2; }
            for (const L& l : layouts) {
                if (mix && l.group == 3) continue;
                g_label = tag + l.name;
                if (run_layout(n, frames, l.group, l.threads, l.teams, l.batch_front, l.tracker, l.cuts, got, false, mix)) return 2;
                const bool ok = same(ref, got);
                if (!ok) bad++, std::fprintf(stderr, "MISMATCH: %s%s\n", tag.c_str(), l.name);
                std::printf("%slayout '%s': %s\n", tag.c_str(), l.name, ok ? "same logs" : "DIFFERENT");
            }
        }
    } else if (mode == "fail") {          // DVSTUB_FAIL=<ctx>:<frame> names a DYNAMIC member: the run must return an error, not hang, in every layout
        std::vector<Log> got;
        const int frames = 30;
        if (run_layout(8, frames, 4, 4, 1, 1, 1, { frames }, got, true)) { bad++; std::fprintf(stderr, "teams: the injected failure was not reported\n"); }
        if (run_layout(8, frames, 4, 2, 0, 1, 1, { frames }, got, true)) { bad++; std::fprintf(stderr, "thread per group: the injected failure was not reported\n"); }
        if (run_layout(8, frames, 8, 1, 0, 0, 1, { frames }, got, true)) { bad++; std::fprintf(stderr, "one thread: the injected failure was not reported\n"); }
        std::printf("failure path: %s\n", bad ? "BROKEN" : "every layout returned the error");
    } else return 2;
    if (dvstub_violations() && mode != "fail") { std::fprintf(stderr, "stub: %lld call-sequence violations\n", dvstub_violations()); bad++; }
    return bad ? 1 : 0;
}
