// stub_viode.cpp — the stand-in C ABI (stub_abi.cpp, beside this file) for the entries a label-image sequence of the runner calls (dv_runner_set_viode): thread T1's
// per-frame stage and the key-image forms of the tracker calls.  Same three duties as stub_abi.cpp: refuse a call sequence the library would refuse, touch plain
// per-context scratch words so that two threads inside the tracker domain without a happens-before edge are a reported race, return deterministic outputs.  The
// detections are built by the library's own rule (csrc/viode_host.h) from boxes that are a function of the frame.
#include <cstdint>
#include <mutex>
#include <string>
#include <unordered_map>
#include "dv_ctx.h"
#include "viode_host.h"

extern "C" long long dvstub_violations();
void dvstub_record(dv_ctx* c, int domain, const char* fmt, ...);          // stub_abi.cpp: the call trace (domain 0 = tracker)

namespace {
struct VStub { int scratch = 0; bool pending = false; int frame = 0, collected = 0; const uint8_t* seg0 = nullptr; const uint8_t* seg1 = nullptr; uint32_t keys[64]; int nkeys = 0; };
std::mutex v_mu; std::unordered_map<dv_ctx*, VStub*> v_map;
VStub& V(dv_ctx* c) { std::lock_guard<std::mutex> lk(v_mu); VStub*& p = v_map[c]; if (!p) p = new VStub(); return *p; }      // (the lock guards the map alone, not the fields TSan is to judge)
uint8_t g_plane[2][4096]; uint32_t g_keys[2][2][1024];
long long g_bad = 0;
int violation(dv_ctx* c, const char* what) { dv_set_error(c, what); std::lock_guard<std::mutex> lk(v_mu); ++g_bad; return -1; }
}

extern "C" {
long long dvstub_viode_violations() { std::lock_guard<std::mutex> lk(v_mu); return g_bad; }
int dv_viode_frame_enqueue(dv_ctx* c, const uint8_t* seg0, const uint8_t* seg1, int w, int h, int stride, int mem, const uint32_t* keys, int nkeys) {
    VStub& s = V(c); s.scratch++;
    { std::string ks; for (int k = 0; keys && k < nkeys && k < 64; ++k) ks += (k ? " " : "") + std::to_string(keys[k]);
      dvstub_record(c, 0, "dv_viode_frame_enqueue w=%d h=%d stride=%d mem=%d nkeys=%d keys=[%s] seg0=%d seg1=%d", w, h, stride, mem, nkeys, ks.c_str(), seg0 != nullptr, seg1 != nullptr); }
    if (!seg0 || !keys || nkeys < 1 || nkeys > 64 || w != c->cfg.width || h != c->cfg.height || mem < 0 || mem > 2) return violation(c, "dv_viode_frame_enqueue: bad argument");
    if (s.pending) return violation(c, "dv_viode_frame_enqueue: previous frame not collected");
    s.pending = true; s.seg0 = seg0; s.seg1 = seg1; s.nkeys = nkeys; for (int k = 0; k < nkeys; ++k) s.keys[k] = keys[k];
    return 0;
}
int dv_viode_frame_collect(dv_ctx* c, int min_inst_size, dv_inst_det* dets, int cap, int* n_dets, const uint8_t** inv, const uint32_t** k0, const uint32_t** k1) {
    VStub& s = V(c); s.scratch++;
    dvstub_record(c, 0, "dv_viode_frame_collect min_inst_size=%d cap=%d dets=%d n_dets=%d inv=%d k0=%d k1=%d", min_inst_size, cap, dets != nullptr, n_dets != nullptr, inv != nullptr, k0 != nullptr, k1 != nullptr);
    if (!s.pending) return violation(c, "dv_viode_frame_collect: nothing enqueued");
    s.pending = false;
    int32_t boxes[256];
    const int f = s.collected++;
    for (int k = 0; k < s.nkeys; ++k) {          // key k: absent every (k + 3)-th frame, otherwise a box that grows and shrinks with the frame (sometimes below min_inst_size)
        const bool absent = (f + k) % (k + 3) == 0;
        const int side = 2 + (f * 3 + k * 5) % 17;
        boxes[4 * k] = absent ? 0x7fffffff : k; boxes[4 * k + 1] = absent ? -1 : k + side; boxes[4 * k + 2] = absent ? 0x7fffffff : 2 * k; boxes[4 * k + 3] = absent ? -1 : 2 * k + side + 1;
    }
    const int n = dv_viode_build_dets(boxes, s.keys, s.nkeys, min_inst_size, dets, cap);
    if (n < 0) return violation(c, "dv_viode_frame_collect: more detections than cap");
    *n_dets = n;
    if (inv) *inv = g_plane[f & 1] + f % 100;
    if (k0) *k0 = g_keys[f & 1][0];
    if (k1) *k1 = s.seg1 ? g_keys[f & 1][1] : nullptr;
    return 0;
}
// the key forms land in the tracker domain's state machine of stub_abi.cpp through the entries it has: the ids / detections travel into the same hashes
int dv_track_unmask_static_keys(dv_ctx* c, const dv_inst_det* dets, int n_dets, const uint32_t* ids, int n_static, const uint32_t* key_image, int stride, int mem) {
    VStub& s = V(c); s.scratch++;
    { std::string is; for (int i = 0; i < n_static; ++i) is += (i ? " " : "") + std::to_string(ids[i]);
      dvstub_record(c, 0, "dv_track_unmask_static_keys n_dets=%d n_static=%d ids=[%s] stride=%d mem=%d dets=%d keys=%d", n_dets, n_static, is.c_str(), stride, mem, dets != nullptr, key_image != nullptr); }
    if (n_static > 0 && n_dets > 0 && (!key_image || mem < 0 || mem > 2)) return violation(c, "dv_track_unmask_static_keys: bad key image");
    std::vector<uint32_t> hit;
    for (int i = 0; i < n_static; ++i) for (int k = 0; k < n_dets; ++k) if (dets[k].track_id == ids[i]) hit.push_back(ids[i]);
    return dv_track_unmask_static(c, dets, n_dets, hit.data(), (int)hit.size());
}
int dv_inst_track_enqueue_keys(dv_ctx* c, double t, const dv_inst_det* dets, int n_dets, const uint32_t* key_image, int stride, int mem, const dv_box3d* b, int nb) {
    VStub& s = V(c); s.scratch++;
    dvstub_record(c, 0, "dv_inst_track_enqueue_keys t=%.17g n_dets=%d stride=%d mem=%d n_boxes=%d dets=%d keys=%d boxes=%d", t, n_dets, stride, mem, nb, dets != nullptr, key_image != nullptr, b != nullptr);
    if (!key_image || mem < 0 || mem > 2) return violation(c, "dv_inst_track_enqueue_keys: bad key image");
    for (int k = 0; k < n_dets; ++k) if (dets[k].mask || dets[k].w <= 0 || dets[k].h <= 0) return violation(c, "dv_inst_track_enqueue_keys: a detection of the frame stage carries a mask or an empty rectangle");
    return dv_inst_track_enqueue(c, t, dets, n_dets, b, nb);
}
}
