// runner_stack_host.cpp — stand-alone host program for the mask-stack path's runner (dv_runner_set_inst_stack): the runner's scheduling of thread T1's per-frame stage and
// the hand-over stage -> collect -> tracking across threads (csrc/runner.hip compiled as plain C++) on the stand-in C ABI (stub_abi.cpp + stub_stack.cpp).  Built twice by
// inst_stack.mk: AddressSanitizer + UBSan, and ThreadSanitizer.  No GPU, no HIP runtime.
//   exit 0 = every layout leaves the one-thread loop's logs, dropped planes stay dropped, a grouped sequence is refused and the runner goes on
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
extern "C" long long dvstub_stack_violations();
extern "C" void dvstub_new_run();

namespace {
int g_bad = 0;
void expect(bool ok, const char* what) { if (!ok) { ++g_bad; std::fprintf(stderr, "FAILED: %s\n", what); } }

constexpr int PLANES = 4;
struct Seq {
    std::vector<const uint8_t*> left, right; std::vector<const void*> stack; std::vector<int32_t> n_planes; std::vector<double> times, imu_t, imu_a, imu_g;
    std::vector<std::vector<int32_t>> tid, cls; std::vector<const int32_t*> tid_p, cls_p;
    dv_seq_input in{}; dv_seq_stack stk{};
};
void make_seq(Seq& q, int frames, int id, int static_bg, int ba_stride) {
    static uint8_t pixel[8192]; static uint8_t planes[64 * 48 * PLANES + 4096];
    q.tid.resize(frames); q.cls.resize(frames);
    for (int k = 0; k < frames; ++k) {
        q.left.push_back(pixel + (id * 64 + k) % 4000); q.right.push_back(pixel + (id * 64 + k + 7) % 4000); q.stack.push_back(planes + k); q.n_planes.push_back(PLANES); q.times.push_back(1.0 + 0.05 * k);
        for (int p = 0; p < PLANES; ++p) { q.tid[k].push_back(p == 2 ? -1 : 100 + p); q.cls[k].push_back(p == 3 && k % 5 == 0 ? -1 : p); }          // plane 2 always dropped, plane 3 every 5th frame (by its class)
        q.tid_p.push_back(q.tid[k].data()); q.cls_p.push_back(q.cls[k].data());
    }
    for (int i = 0; i < frames * 10 + 20; ++i) { q.imu_t.push_back(0.9 + 0.005 * i); for (int c = 0; c < 3; ++c) { q.imu_a.push_back(0.01 * i + c + id); q.imu_g.push_back(0.02 * i - c); } }
    q.in.left = q.left.data(); q.in.right = q.right.data(); q.in.times = q.times.data(); q.in.n_frames = frames; q.in.mem = DV_MEM_DEVICE; q.in.stride = 0; q.in.ba_stride = ba_stride;
    q.in.imu_t = q.imu_t.data(); q.in.imu_acc = q.imu_a.data(); q.in.imu_gyr = q.imu_g.data(); q.in.n_imu = (int)q.imu_t.size();
    q.stk.stack = q.stack.data(); q.stk.n_planes = q.n_planes.data(); q.stk.kind = DV_STACK_U8; q.stk.mem = DV_MEM_PINNED; q.stk.min_inst_size = 8;
    q.stk.track_id = q.tid_p.data(); q.stk.class_id = q.cls_p.data(); q.stk.static_as_background = static_bg;
}
struct Log { std::vector<double> frames; std::vector<unsigned long long> rows; long long iterations = 0, dets = 0; };
int run_layout(int n, int frames, int threads, int tracker_thread, const std::vector<int>& cuts, int static_bg, int ba_stride, std::vector<Log>& out) {
    std::vector<Seq> seqs(n); std::vector<dv_ctx*> ctxs; std::vector<dv_seq_input> in;
    dvstub_new_run();
    for (int i = 0; i < n; ++i) { make_seq(seqs[i], frames, i, static_bg, ba_stride); ctxs.push_back(dvstub_ctx(64, 48, 1)); in.push_back(seqs[i].in); }
    dv_runner* R = dv_runner_create(ctxs.data(), in.data(), n, 0, threads);
    if (!R) return 2;
    dv_runner_set(R, "tracker_thread", tracker_thread);
    for (int i = 0; i < n; ++i) if (dv_runner_set_inst_stack(R, i, &seqs[i].stk)) { std::fprintf(stderr, "set_inst_stack: %s\n", dv_runner_error(R)); return 2; }
    for (int c : cuts) if (dv_runner_run(R, c, nullptr)) { std::fprintf(stderr, "dv_runner_run: %s\n", dv_runner_error(R)); dv_runner_destroy(R); return 2; }
    out.assign(n, Log{});
    for (int i = 0; i < n; ++i) {
        out[i].frames.resize(9 * (size_t)frames); int nf = 0; dv_runner_get_frames(R, i, out[i].frames.data(), frames, &nf); out[i].frames.resize(9 * (size_t)nf);
        out[i].rows.resize(4 * (size_t)frames); int nr = 0; dv_runner_get_row_log(R, i, out[i].rows.data(), frames, &nr); out[i].rows.resize(4 * (size_t)nr);
        long long fr = 0; dv_runner_get(R, i, nullptr, nullptr, 0, nullptr, &out[i].iterations, &fr, nullptr);
        dv_runner_dynamic_stats(R, i, &out[i].dets, nullptr, nullptr, nullptr);
    }
    dv_runner_destroy(R);
    return 0;
}
bool same(const std::vector<Log>& a, const std::vector<Log>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].frames != b[i].frames || a[i].rows != b[i].rows || a[i].iterations != b[i].iterations || a[i].dets != b[i].dets || a[i].frames.empty()) return false;
    return true;
}
}

int main() {
    std::thread watchdog([] { std::this_thread::sleep_for(std::chrono::seconds(240)); std::fprintf(stderr, "runner_stack_host: HANG (watchdog)\n"); std::_Exit(9); });
    watchdog.detach();
    const int n = 3, frames = 29;
    struct L { int threads, tracker; std::vector<int> cuts; const char* name; };
    const L layouts[] = { { 1, 1, { frames }, "T2 beside T3" }, { 3, 1, { frames }, "T2 beside T3, one estimator thread per sequence" }, { 1, 1, { 7, 1, 13, 8 }, "T2 beside T3, four calls" },
                          { 1, 0, { 7, 1, 13, 8 }, "one-thread loop, four calls" }, { 3, 0, { 11, 18 }, "one-thread loops on three threads" } };
    for (int static_bg = 0; static_bg <= 1; ++static_bg) for (int stride = 1; stride <= 2; ++stride) {
        std::vector<Log> ref, got;
        if (run_layout(n, frames, 1, 0, { frames }, static_bg, stride, ref)) return 2;          // the one-thread loop, uncut
        expect(!ref.empty() && ref[0].dets > 0, "the object branch was fed");
        expect(!ref.empty() && ref[0].dets < (long long)frames * 3, "dropped planes reach no detection (plane 2 never, plane 3 not every frame)");
        for (const L& l : layouts) {
            if (run_layout(n, frames, l.threads, l.tracker, l.cuts, static_bg, stride, got)) return 2;
            const bool ok = same(ref, got);
            if (!ok) ++g_bad;
            std::printf("static feedback %d, ba_stride %d, layout '%s': %s\n", static_bg, stride, l.name, ok ? "same logs" : "DIFFERENT");
        }
    }
    {   // a member of a dv_batch group is refused with the documented message; the runner goes on with what it had.  So are frames without planes.
        std::vector<Seq> seqs(2); std::vector<dv_ctx*> ctxs; std::vector<dv_seq_input> in;
        dvstub_new_run();
        for (int i = 0; i < 2; ++i) { make_seq(seqs[i], 12, i, 0, 1); ctxs.push_back(dvstub_ctx(64, 48, 1)); in.push_back(seqs[i].in); }
        dv_runner* R = dv_runner_create(ctxs.data(), in.data(), 2, 2, 1);
        expect(R != nullptr, "grouped runner");
        if (R) {
            expect(dv_runner_set_inst_stack(R, 0, &seqs[0].stk) == -1 && std::strstr(dv_runner_error(R), "dv_runner_set_inst_stack: a sequence of a dv_batch group is not supported") != nullptr, "grouped sequence refused with the documented message");
            expect(dv_runner_run(R, 12, nullptr) == 0, "the runner stays usable");
            dv_runner_destroy(R);
        }
        dvstub_new_run();
        dv_ctx* c = dvstub_ctx(64, 48, 1);
        R = dv_runner_create(&c, &seqs[0].in, 1, 0, 1);
        expect(R != nullptr, "single runner");
        if (R) {
            seqs[0].n_planes[3] = 0;
            expect(dv_runner_set_inst_stack(R, 0, &seqs[0].stk) == -1 && std::strstr(dv_runner_error(R), "1..64 planes") != nullptr, "a frame with 0 planes is refused");
            seqs[0].n_planes[3] = 65;
            expect(dv_runner_set_inst_stack(R, 0, &seqs[0].stk) == -1, "a frame with 65 planes is refused");
            seqs[0].n_planes[3] = PLANES;
            expect(dv_runner_set_inst_stack(R, 0, &seqs[0].stk) == 0 && dv_runner_run(R, 12, nullptr) == 0, "the same runner takes the mended sequence and runs it");
            dv_runner_destroy(R);
        }
    }
    if (dvstub_violations() || dvstub_stack_violations()) { std::fprintf(stderr, "stub: %lld + %lld call-sequence violations\n", dvstub_violations(), dvstub_stack_violations()); ++g_bad; }
    std::printf("runner_stack_host: %s\n", g_bad ? "BROKEN" : "ok");
    return g_bad ? 1 : 0;
}
