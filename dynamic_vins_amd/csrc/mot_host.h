// mot_host.h — the half of the multi-object tracker (mot.hip) that is plain C++: the refusals of a dv_mot_params, the layout of the resident track table, and the small
// rules the association kernel and the host share in ONE copy — KalmanTracker's rect() (mot/kalman_tracker.cpp:20-28), RectIou (mot/deep_sort.cpp:27-35),
// FeatureBundle::add (mot/feature_bundle.h:40-46), KalmanTracker::miss (mot/kalman_tracker.cpp:90-96) and the two gates of DeepSORT::update (mot/deep_sort.cpp:99,116).
// No HIP in here: dv_mot_* use it, and tests/host/mot_host.cpp compiles it under the sanitizers.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "dv_mem.h"

#ifdef __HIPCC__
#define DV_MOT_HD __host__ __device__
#else
#define DV_MOT_HD
#endif

constexpr int DV_MOT_TENTATIVE = 0, DV_MOT_CONFIRMED = 1, DV_MOT_DELETED = 2;      // TrackState (mot/kalman_tracker.h:19-23)
constexpr float DV_MOT_INVALID_DIST = 1000.0f;                                     // mot/tracker_manager.h:27
constexpr float DV_MOT_GATE_IOU1 = 0.8f, DV_MOT_GATE_FEAT = 0.2f, DV_MOT_GATE_IOU2 = 0.7f;

// the reason a parameter set is refused, or nullptr
static inline const char* dv_mot_check_host(const dv_mot_params* p) {
    if (!p) return "null argument";
    if (p->n_init < 0 || p->n_init > (1 << 20)) return "n_init outside 0..2^20";
    if (p->max_age < 0 || p->max_age > (1 << 20)) return "max_age outside 0..2^20";
    if (p->budget < 1 || p->budget > DV_MOT_MAX_BUDGET) return "budget outside 1..100";
    if (p->feat_dim < 1 || p->feat_dim > DV_MOT_MAX_FEAT_DIM) return "feat_dim outside 1..512";
    if (p->max_tracks < 1 || p->max_tracks > DV_MOT_MAX_TRACKS) return "max_tracks outside 1..128";
    return nullptr;
}
// the reason a frame is refused, or nullptr (n = 0 is the reference's "no detections: the tracker is not called", front_end/dynamic_tracker.cpp:795-796)
static inline const char* dv_mot_frame_check_host(const float* rects, const float* feats, int n, int mem) {
    if (n < 0 || n > DV_STACK_MAX_PLANES) return "0..64 detections";
    if (!dv_mem_known(mem)) return "unknown memory kind";
    if (n == 0) return nullptr;
    if (!rects || !feats) return "null rectangles or embeddings";
    if (((uintptr_t)rects | (uintptr_t)feats) & 3) return "rectangles and embeddings must be 4-byte aligned";
    return nullptr;
}
// the reason a cost matrix is refused by dv_mot_assign, or nullptr: Munkres on anything but finite non-negative costs need not end
static inline const char* dv_mot_assign_check_host(const float* cost, int rows, int cols, const int32_t* assignment) {
    if (rows < 0 || rows > DV_MOT_MAX_TRACKS) return "0..128 rows";
    if (cols < 0 || cols > DV_STACK_MAX_PLANES) return "0..64 columns";
    if (rows > 0 && !assignment) return "null assignment";
    if (rows > 0 && cols > 0 && !cost) return "null cost";
    for (long long i = 0; i < (long long)rows * cols; ++i) if (!(cost[i] >= 0.0f) || !std::isfinite(cost[i])) return "costs must be finite and non-negative";
    return nullptr;
}

// The resident table: a header, then one array per field over max_tracks rows IN TABLE ORDER, then the rows stored in each gallery slot (0 = the slot is free).
// Byte offsets, every array 256-byte aligned.
enum { DV_MOT_H_NTRACKS = 0, DV_MOT_H_NEXT_ID = 1, DV_MOT_H_WORDS = 16 };
struct DvMotLayout { size_t hdr, x, P, state, id, hits, tsu, slot, next, full, slot_rows, bytes; };
static inline DvMotLayout dv_mot_layout(int max_tracks) {
    DvMotLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t m = (size_t)max_tracks;
    L.hdr = take(DV_MOT_H_WORDS * 4); L.x = take(m * 7 * 4); L.P = take(m * 49 * 4);
    L.state = take(m * 4); L.id = take(m * 4); L.hits = take(m * 4); L.tsu = take(m * 4); L.slot = take(m * 4); L.next = take(m * 4); L.full = take(m * 4);
    L.slot_rows = take(m * 4);
    L.bytes = off;
    return L;
}

// get_rect_xysr, in float as written there.  s r < 0 gives NaN (remove_nan's way in); w = 0 gives inf or NaN
DV_MOT_HD static inline void dv_mot_rect_of(const float* x, float* r) {
    const float w = sqrtf(x[2] * x[3]);
    const float h = x[2] / w;
    r[0] = x[0] - w / 2; r[1] = x[1] - h / 2; r[2] = w; r[3] = h;
}
DV_MOT_HD static inline bool dv_mot_rect_nan(const float* r) { return r[0] != r[0] || r[1] != r[1] || r[2] != r[2] || r[3] != r[3]; }
// KalmanTracker::init / the measurement of update: [x + w / 2, y + h / 2, area, w / h]
DV_MOT_HD static inline void dv_mot_measure(const float* r, float* z) { z[0] = r[0] + r[2] / 2; z[1] = r[1] + r[3] / 2; z[2] = r[2] * r[3]; z[3] = r[2] / r[3]; }
// 1 - RectIou with cv::Rect2f's operator& (empty when the width or the height of the overlap is <= 0) and the union tested against DBL_EPSILON
DV_MOT_HD static inline float dv_mot_iou_dist(const float* a, const float* b) {
    const float x1 = a[0] > b[0] ? a[0] : b[0], y1 = a[1] > b[1] ? a[1] : b[1];
    const float ax2 = a[0] + a[2], bx2 = b[0] + b[2], ay2 = a[1] + a[3], by2 = b[1] + b[3];
    float w = (ax2 < bx2 ? ax2 : bx2) - x1, h = (ay2 < by2 ? ay2 : by2) - y1;
    if (w <= 0 || h <= 0) { w = 0; h = 0; }
    const float in = w * h;
    const float un = a[2] * a[3] + b[2] * b[3] - in;
    if ((double)un < DBL_EPSILON) return 1.0f;
    return 1 - in / un;
}
// stage 1 (deep_sort.cpp:99) and stage 2 (deep_sort.cpp:116).  A NaN distance — a NaN in the caller's embeddings; a NaN, infinite or zero-height rectangle, or a track with
// r = 0, in the IoU — counts as gated in BOTH stages: the declared difference (include/dvins.h), since Munkres on a NaN need not end
DV_MOT_HD static inline float dv_mot_cost1(float iou_dist, float feat) { return (iou_dist > DV_MOT_GATE_IOU1 || iou_dist != iou_dist || feat > DV_MOT_GATE_FEAT || feat != feat) ? DV_MOT_INVALID_DIST : feat; }
DV_MOT_HD static inline float dv_mot_cost2(float iou_dist) { return (iou_dist > DV_MOT_GATE_IOU2 || iou_dist != iou_dist) ? DV_MOT_INVALID_DIST : iou_dist; }
// FeatureBundle::add: the row the embedding goes to; next / full updated.  Rows a distance reads afterwards: dv_mot_ring_rows
DV_MOT_HD static inline int dv_mot_ring_add(int* next, int* full, int budget) {
    if (*next == budget) { *full = 1; *next = 0; }
    return (*next)++;
}
DV_MOT_HD static inline int dv_mot_ring_rows(int next, int full, int budget) { return full ? budget : next; }
// KalmanTracker::miss: the state after a frame without a match (time_since_update already counted by predict)
DV_MOT_HD static inline int dv_mot_miss(int state, int time_since_update, int max_age) {
    if (state == DV_MOT_TENTATIVE) return DV_MOT_DELETED;
    return time_since_update > max_age ? DV_MOT_DELETED : state;
}
