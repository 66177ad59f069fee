// stub_stack.cpp — the stand-in C ABI (stub_abi.cpp, beside this file) for the entries a mask-stack sequence of the runner calls (dv_runner_set_inst_stack): thread T1's
// per-frame stage from the detector's stack and the plane forms of the tracker calls.  Same three duties as stub_abi.cpp / stub_viode.cpp: refuse a call sequence the
// library would refuse, touch plain per-context scratch words so that two threads inside the tracker domain without a happens-before edge are a reported race, return
// deterministic outputs.  The detections are built by the library's own rule (csrc/inst_stack_host.h) from boxes that are a function of the frame.
#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include "dv_ctx.h"
#include "inst_stack_host.h"

void dvstub_record(dv_ctx* c, int domain, const char* fmt, ...);          // stub_abi.cpp: the call trace (domain 0 = tracker)

namespace {
struct SStub { int scratch = 0; bool pending = false; int collected = 0, n_planes = 0; const void* data = nullptr; const void* collected_data = nullptr; };
std::mutex s_mu; std::unordered_map<dv_ctx*, SStub*> s_map;
SStub& S(dv_ctx* c) { std::lock_guard<std::mutex> lk(s_mu); SStub*& p = s_map[c]; if (!p) p = new SStub(); return *p; }      // (the lock guards the map alone, not the fields TSan is to judge)
uint8_t g_plane[2][4096];
long long g_bad = 0;
int violation(dv_ctx* c, const std::string& what) { dv_set_error(c, what); std::lock_guard<std::mutex> lk(s_mu); ++g_bad; return -1; }
}

extern "C" {
long long dvstub_stack_violations() { std::lock_guard<std::mutex> lk(s_mu); return g_bad; }
int dv_inst_stack_frame_enqueue(dv_ctx* c, const dv_mask_stack* st, int w, int h, int flags) {
    SStub& s = S(c); s.scratch++;
    dvstub_record(c, 0, "dv_inst_stack_frame_enqueue w=%d h=%d flags=%d n_planes=%d kind=%d mem=%d", w, h, flags, st ? st->n_planes : -1, st ? st->kind : -1, st ? st->mem : -1);
    DvStackLayout L;
    if (w != c->cfg.width || h != c->cfg.height) return violation(c, "dv_inst_stack_frame_enqueue: image size differs from config");
    if (const char* why = dv_stack_check(st, w, h, &L)) return violation(c, std::string("dv_inst_stack_frame_enqueue: ") + why);
    if (s.pending) return violation(c, "dv_inst_stack_frame_enqueue: previous frame not collected");
    s.pending = true; s.data = st->data; s.n_planes = st->n_planes;
    return 0;
}
int dv_inst_stack_frame_collect(dv_ctx* c, int min_inst_size, dv_inst_det* dets, int32_t* planes, int cap, int* n_dets, const uint8_t** inv, const uint8_t** merge) {
    SStub& s = S(c); s.scratch++;
    dvstub_record(c, 0, "dv_inst_stack_frame_collect min_inst_size=%d cap=%d dets=%d planes=%d n_dets=%d inv=%d", min_inst_size, cap, dets != nullptr, planes != nullptr, n_dets != nullptr, inv != nullptr);
    if (!s.pending) return violation(c, "dv_inst_stack_frame_collect: nothing enqueued");
    s.pending = false; s.collected_data = s.data;
    int32_t boxes[256];
    const int f = s.collected++;
    for (int k = 0; k < s.n_planes; ++k) {          // plane k: empty every (k + 3)-th frame, otherwise a box that grows and shrinks with the frame (sometimes below min_inst_size)
        const bool absent = (f + k) % (k + 3) == 0;
        const int side = 2 + (f * 3 + k * 5) % 17;
        boxes[4 * k] = absent ? 0x7fffffff : k; boxes[4 * k + 1] = absent ? -1 : k + side; boxes[4 * k + 2] = absent ? 0x7fffffff : 2 * k; boxes[4 * k + 3] = absent ? -1 : 2 * k + side + 1;
    }
    const int n = dv_stack_build_dets(boxes, s.n_planes, min_inst_size, dets, planes, cap);
    if (n < 0) return violation(c, "dv_inst_stack_frame_collect: more detections than cap");
    *n_dets = n;
    if (inv) *inv = g_plane[f & 1] + f % 100;
    if (merge) *merge = g_plane[f & 1] + 2048;
    return 0;
}
// the plane forms land in the tracker domain's state machine of stub_abi.cpp through the entries it has; the stack handed in must be the one whose stage was collected last
int dv_track_unmask_static_planes(dv_ctx* c, const dv_inst_det* dets, const int32_t* planes, int n_dets, const uint32_t* ids, int n_static, const dv_mask_stack* st) {
    SStub& s = S(c); s.scratch++;
    { std::string is; for (int i = 0; i < n_static; ++i) is += (i ? " " : "") + std::to_string(ids[i]);
      dvstub_record(c, 0, "dv_track_unmask_static_planes n_dets=%d n_static=%d ids=[%s] dets=%d planes=%d", n_dets, n_static, is.c_str(), dets != nullptr, planes != nullptr); }
    if (n_static > 0 && n_dets > 0) {
        DvStackLayout L;
        if (const char* why = dv_stack_check(st, c->cfg.width, c->cfg.height, &L)) return violation(c, std::string("dv_track_unmask_static_planes: ") + why);
        if (st->data != s.collected_data) return violation(c, "dv_track_unmask_static_planes: not the stack of the frame whose stage was collected");
        if (const char* why = dv_stack_check_dets(dets, planes, n_dets, st->n_planes, c->cfg.width, c->cfg.height, ids, n_static)) return violation(c, std::string("dv_track_unmask_static_planes: ") + why);
    }
    std::vector<uint32_t> hit;
    for (int i = 0; i < n_static; ++i) for (int k = 0; k < n_dets; ++k) if (dets[k].track_id == ids[i]) hit.push_back(ids[i]);
    return dv_track_unmask_static(c, dets, n_dets, hit.data(), (int)hit.size());
}
int dv_inst_track_enqueue_planes(dv_ctx* c, double t, const dv_inst_det* dets, const int32_t* planes, int n_dets, const dv_mask_stack* st, const dv_box3d* b, int nb) {
    SStub& s = S(c); s.scratch++;
    { std::string ps; for (int i = 0; i < n_dets; ++i) ps += (i ? " " : "") + std::to_string(planes[i]) + ":" + std::to_string(dets[i].track_id);
      dvstub_record(c, 0, "dv_inst_track_enqueue_planes t=%.17g n_dets=%d plane:id=[%s] n_boxes=%d", t, n_dets, ps.c_str(), nb); }
    DvStackLayout L;
    if (const char* why = dv_stack_check(st, c->cfg.width, c->cfg.height, &L)) return violation(c, std::string("dv_inst_track_enqueue_planes: ") + why);
    if (st->data != s.collected_data) return violation(c, "dv_inst_track_enqueue_planes: not the stack of the frame whose stage was collected");
    if (n_dets > 0) if (const char* why = dv_stack_check_dets(dets, planes, n_dets, st->n_planes, c->cfg.width, c->cfg.height, nullptr, 0)) return violation(c, std::string("dv_inst_track_enqueue_planes: ") + why);
    for (int k = 0; k < n_dets; ++k) if (dets[k].mask) return violation(c, "dv_inst_track_enqueue_planes: a detection of the frame stage carries a mask");
    return dv_inst_track_enqueue(c, t, dets, n_dets, b, nb);
}
}
