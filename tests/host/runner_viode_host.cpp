// runner_viode_host.cpp — stand-alone host program for the label-image path (dv_runner_set_viode): the detection-building rule (csrc/viode_host.h) and the runner's
// scheduling of thread T1's per-frame stage (csrc/runner.hip compiled as plain C++) on the stand-in C ABI (stub_abi.cpp + stub_viode.cpp).  Built twice by viode.mk:
// AddressSanitizer + UBSan, and ThreadSanitizer.  No GPU, no HIP runtime.
//   runner_viode_host [--calls | --calls-full]       (--calls: per run, context and domain the digest of the stub's call trace)        exit 0 = the rule holds, every layout leaves the one-thread logs, a grouped sequence is refused and the runner goes on
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "dvins.h"
#include "../../dynamic_vins_amd/csrc/viode_host.h"

extern "C" dv_ctx* dvstub_ctx(int w, int h, int dynamic);
extern "C" long long dvstub_violations();
extern "C" long long dvstub_viode_violations();
extern "C" void dvstub_new_run();
extern "C" void dvstub_trace(int level);
extern "C" void dvstub_trace_report(const char* label);

namespace {
int g_bad = 0;
void expect(bool ok, const char* what) { if (!ok) { ++g_bad; std::fprintf(stderr, "FAILED: %s\n", what); } }

void rule_checks() {
    // keys out of order, one absent, one below the size floor, one touching all four borders of a 70 x 23 image, one a single column (empty rectangle)
    const uint32_t keys[5] = { 900, 100, 500, 300, 700 };
    const int32_t boxes[20] = { 2, 12, 3, 20,   0x7fffffff, -1, 0x7fffffff, -1,   5, 8, 5, 30,   0, 22, 0, 69,   4, 14, 9, 9 };
    dv_inst_det d[8];
    int n = dv_viode_build_dets(boxes, keys, 5, 8, d, 8);
    expect(n == 2, "two detections survive");
    expect(n == 2 && d[0].track_id == 300 && d[0].x == 0 && d[0].y == 0 && d[0].w == 69 && d[0].h == 22, "ascending key, max row / column excluded");
    expect(n == 2 && d[1].track_id == 900 && d[1].x == 3 && d[1].y == 2 && d[1].w == 17 && d[1].h == 10 && d[1].mask == nullptr && d[1].points == nullptr && d[1].class_id == 0, "second detection");
    n = dv_viode_build_dets(boxes, keys, 5, 0, d, 8);
    expect(n == 3 && d[1].track_id == 500 && d[1].h == 3, "min size 0 keeps the thin box and still drops the empty rectangle");
    expect(dv_viode_build_dets(boxes, keys, 5, 0, d, 2) == -1, "cap too small");
    expect(dv_viode_build_dets(boxes, keys, 0, 8, d, 8) == 0 && dv_viode_build_dets(boxes, keys, 65, 8, d, 8) == -1, "key count");
    uint32_t k64[64]; int32_t b64[256]; dv_inst_det d64[64];
    for (int k = 0; k < 64; ++k) { k64[k] = 64 - k; b64[4 * k] = 0; b64[4 * k + 1] = 10 + k; b64[4 * k + 2] = 1; b64[4 * k + 3] = 12 + k; }
    n = dv_viode_build_dets(b64, k64, 64, 8, d64, 64);
    bool asc = n == 64; for (int k = 1; k < n; ++k) asc = asc && d64[k - 1].track_id < d64[k].track_id;
    expect(asc, "64 keys, ascending");
}

struct Seq {
    std::vector<const uint8_t*> left, right, seg0, seg1; std::vector<double> times, imu_t, imu_a, imu_g;
    uint32_t keys[3] = { 10, 11, 12 };
    dv_seq_input in{}; dv_seq_viode vio{};
};
void make_seq(Seq& q, int frames, int id, int static_bg, int ba_stride, bool right_seg) {
    static uint8_t pixel[8192];
    for (int k = 0; k < frames; ++k) { q.left.push_back(pixel + (id * 64 + k) % 4000); q.right.push_back(pixel + (id * 64 + k + 7) % 4000); q.seg0.push_back(pixel + 4096 + k); q.seg1.push_back(pixel + 6000 + k); q.times.push_back(1.0 + 0.05 * k); }
    for (int i = 0; i < frames * 10 + 20; ++i) { q.imu_t.push_back(0.9 + 0.005 * i); for (int c = 0; c < 3; ++c) { q.imu_a.push_back(0.01 * i + c + id); q.imu_g.push_back(0.02 * i - c); } }
    q.in.left = q.left.data(); q.in.right = q.right.data(); q.in.times = q.times.data(); q.in.n_frames = frames; q.in.mem = DV_MEM_DEVICE; q.in.stride = 0; q.in.ba_stride = ba_stride;
    q.in.imu_t = q.imu_t.data(); q.in.imu_acc = q.imu_a.data(); q.in.imu_gyr = q.imu_g.data(); q.in.n_imu = (int)q.imu_t.size();
    q.vio.seg0 = q.seg0.data(); q.vio.seg1 = right_seg ? q.seg1.data() : nullptr; q.vio.mem = DV_MEM_PINNED; q.vio.stride = 0; q.vio.dyn_keys = q.keys; q.vio.nkeys = 3; q.vio.min_inst_size = 8;
    q.vio.static_as_background = static_bg;
}
struct Log { std::vector<double> frames; std::vector<unsigned long long> rows; long long iterations = 0, dets = 0; };
std::string g_label;          // the call trace's name of the next run
int run_layout(int n, int frames, int threads, int tracker_thread, const std::vector<int>& cuts, int static_bg, int ba_stride, std::vector<Log>& out) {
    std::vector<Seq> seqs(n); std::vector<dv_ctx*> ctxs; std::vector<dv_seq_input> in;
    dvstub_new_run();
    for (int i = 0; i < n; ++i) { make_seq(seqs[i], frames, i, static_bg, ba_stride, i % 2 == 0); ctxs.push_back(dvstub_ctx(64, 48, 1)); in.push_back(seqs[i].in); }
    dv_runner* R = dv_runner_create(ctxs.data(), in.data(), n, 0, threads);
    if (!R) return 2;
    dv_runner_set(R, "tracker_thread", tracker_thread);
    for (int i = 0; i < n; ++i) if (dv_runner_set_viode(R, i, &seqs[i].vio)) { std::fprintf(stderr, "set_viode: %s\n", dv_runner_error(R)); return 2; }
    for (int c : cuts) if (dv_runner_run(R, c, nullptr)) { std::fprintf(stderr, "dv_runner_run: %s\n", dv_runner_error(R)); dv_runner_destroy(R); return 2; }
    out.assign(n, Log{});
    for (int i = 0; i < n; ++i) {
        out[i].frames.resize(9 * (size_t)frames); int nf = 0; dv_runner_get_frames(R, i, out[i].frames.data(), frames, &nf); out[i].frames.resize(9 * (size_t)nf);
        out[i].rows.resize(4 * (size_t)frames); int nr = 0; dv_runner_get_row_log(R, i, out[i].rows.data(), frames, &nr); out[i].rows.resize(4 * (size_t)nr);
        long long fr = 0; dv_runner_get(R, i, nullptr, nullptr, 0, nullptr, &out[i].iterations, &fr, nullptr);
        dv_runner_dynamic_stats(R, i, &out[i].dets, nullptr, nullptr, nullptr);
    }
    dv_runner_destroy(R);
    dvstub_trace_report(g_label.c_str());
    return 0;
}
bool same(const std::vector<Log>& a, const std::vector<Log>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (a[i].frames != b[i].frames || a[i].rows != b[i].rows || a[i].iterations != b[i].iterations || a[i].dets != b[i].dets || a[i].frames.empty()) return false;
    return true;
}
}

int main(int argc, char** argv) {
    std::thread watchdog([] { std::this_thread::sleep_for(std::chrono::seconds(240)); std::fprintf(stderr, "runner_viode_host: HANG (watchdog)\n"); std::_Exit(9); });
    watchdog.detach();
    rule_checks();
    for (int a = 1; a < argc; ++a) { if (!std::strcmp(argv[a], "--calls")) dvstub_trace(1); else if (!std::strcmp(argv[a], "--calls-full")) dvstub_trace(2); }          // the stub's call trace: digests / records per run (not for `fail`)
    const int n = 3, frames = 32;
    struct L { int threads, tracker; std::vector<int> cuts; const char* name; };
    const L layouts[] = { { 1, 1, { frames }, "T2 beside T3" }, { 3, 1, { frames }, "T2 beside T3, one estimator thread per sequence" }, { 1, 1, { 7, 1, 13, 11 }, "T2 beside T3, four calls" },
                          { 1, 0, { 5, 27 }, "one-thread loop, two calls" }, { 3, 0, { 11, 21 }, "one-thread loops on three threads" } };
    for (int static_bg = 0; static_bg <= 1; ++static_bg) for (int stride = 1; stride <= 2; ++stride) {
        std::vector<Log> ref, got;
        const std::string tag = "static feedback " + std::to_string(static_bg) + ", ba_stride " + std::to_string(stride) + ": ";
        g_label = tag + "reference";
        if (run_layout(n, frames, 1, 0, { frames }, static_bg, stride, ref)) return 2;          // the one-thread loop, uncut
        expect(!ref.empty() && ref[0].dets > 0, "the object branch was fed");
        for (const L& l : layouts) {
            g_label = tag + l.name;
            if (run_layout(n, frames, l.threads, l.tracker, l.cuts, static_bg, stride, got)) return 2;
            const bool ok = same(ref, got);
            if (!ok) ++g_bad;
            std::printf("static feedback %d, ba_stride %d, layout '%s': %s\n", static_bg, stride, l.name, ok ? "same logs" : "DIFFERENT");
        }
    }
    {   // a member of a dv_batch group is refused with the documented message; the runner goes on with what it had
        std::vector<Seq> seqs(2); std::vector<dv_ctx*> ctxs; std::vector<dv_seq_input> in;
        dvstub_new_run();
        for (int i = 0; i < 2; ++i) { make_seq(seqs[i], 12, i, 0, 1, true); ctxs.push_back(dvstub_ctx(64, 48, 1)); in.push_back(seqs[i].in); }
        dv_runner* R = dv_runner_create(ctxs.data(), in.data(), 2, 2, 1);
        expect(R != nullptr, "grouped runner");
        if (R) {
            expect(dv_runner_set_viode(R, 0, &seqs[0].vio) == -1 && std::strstr(dv_runner_error(R), "dv_runner_set_viode: a sequence of a dv_batch group is not supported") != nullptr, "grouped sequence refused with the documented message");
            expect(dv_runner_run(R, 12, nullptr) == 0, "the runner stays usable");
            dv_runner_destroy(R);
            dvstub_trace_report("refused label-image member: the group goes on raw");
        }
    }
    if (dvstub_violations() || dvstub_viode_violations()) { std::fprintf(stderr, "stub: %lld + %lld call-sequence violations\n", dvstub_violations(), dvstub_viode_violations()); ++g_bad; }
    std::printf("runner_viode_host: %s\n", g_bad ? "BROKEN" : "ok");
    return g_bad ? 1 : 0;
}
