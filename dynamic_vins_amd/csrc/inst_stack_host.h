// inst_stack_host.h — host half of the detector branch of thread T1 behind inst_stack_kernel: BuildBoxes2D's Box2D list (det2d/detector2d.cpp:58-97) from the per-plane
// bounding boxes, and the checks of a dv_mask_stack descriptor every entry shares.  Plain C++ (no HIP): dv_inst_stack_frame_collect uses it, and tests/host compiles it
// under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include "dv_mem.h"
#include "pix_src.h"

// the membership rule of a stack element: written once, in pix_src.h
static inline bool dv_stack_u8_has(uint8_t b) { return dv_pix_u8_has(b); }
static inline bool dv_stack_f32_has(float v, float thr) { return dv_pix_f32_has(v, thr); }

// boxes[p] = row_min, row_max, col_min, col_max of plane p's pixels (row_max < row_min: the plane is empty — where the reference throws, torch::max of an empty tensor).
// One detection per non-empty plane in ASCENDING plane order: rect = cv::Rect(min_pt, max_pt), i.e. the max row / column excluded; track_id = plane (Box2D::id = i),
// class 0, mask / points NULL; planes_out[i] = the plane of dets[i].  A rectangle under min_size pixels on a side (and any empty one) is dropped, as viode_host.h does.
// -> number of detections, or -1 when `cap` is too small / n_planes out of range.
static inline int dv_stack_build_dets(const int32_t* boxes, int n_planes, int min_size, dv_inst_det* dets, int32_t* planes_out, int cap) {
    if (n_planes < 0 || n_planes > DV_STACK_MAX_PLANES) return -1;
    const int floor_px = std::max(min_size, 1);
    int n = 0;
    for (int p = 0; p < n_planes; ++p) {
        const int r0 = boxes[4 * p], r1 = boxes[4 * p + 1], c0 = boxes[4 * p + 2], c1 = boxes[4 * p + 3];
        if (r1 < r0 || c1 < c0) continue;
        const int w = c1 - c0, h = r1 - r0;
        if (w < floor_px || h < floor_px) continue;
        if (n >= cap) return -1;
        dv_inst_det d{};
        d.track_id = (uint32_t)p; d.class_id = 0; d.x = c0; d.y = r0; d.w = w; d.h = h; d.mask = nullptr; d.points = nullptr; d.n_points = 0;
        dets[n] = d;
        if (planes_out) planes_out[n] = p;
        ++n;
    }
    return n;
}

// A descriptor with the defaults filled in (strides in bytes), or the reason it is refused.  w x h: the configured image size.
struct DvStackLayout { int es, row_stride; long long plane_stride; };
static inline const char* dv_stack_check(const dv_mask_stack* s, int w, int h, DvStackLayout* out) {
    if (!s || !s->data) return "null stack";
    if (s->n_planes < 1 || s->n_planes > DV_STACK_MAX_PLANES) return "1..64 planes";
    if (s->kind != DV_STACK_U8 && s->kind != DV_STACK_F32) return "unknown element kind";
    if (!dv_mem_known(s->mem)) return "unknown memory kind";
    const int es = s->kind == DV_STACK_F32 ? 4 : 1;
    const long long row = s->row_stride ? (long long)s->row_stride : (long long)w * es;
    if (s->row_stride < 0 || row < (long long)w * es || row > 0x7fffffff) return "row stride below the row";
    const long long plane = s->plane_stride ? (long long)s->plane_stride : row * h;
    if (s->plane_stride < 0 || plane < row * (h - 1) + (long long)w * es) return "plane stride below the plane";
    if (es == 4 && ((row & 3) || (plane & 3) || ((uintptr_t)s->data & 3))) return "float planes must be 4-byte aligned";
    out->es = es; out->row_stride = (int)row; out->plane_stride = plane;
    return nullptr;
}
// every detection's rectangle inside the image and its plane inside the stack (only: restricts the check to the detections whose track_id is in the list)
static inline const char* dv_stack_check_dets(const dv_inst_det* dets, const int32_t* planes, int n_dets, int n_planes, int w, int h, const uint32_t* only, int n_only) {
    for (int i = 0; i < n_dets; ++i) {
        const dv_inst_det& d = dets[i];
        if (only && std::find(only, only + n_only, d.track_id) == only + n_only) continue;
        if (d.w <= 0 || d.h <= 0 || d.x < 0 || d.y < 0 || d.w > w || d.h > h || d.x > w - d.w || d.y > h - d.h) return "detection rectangle outside the image";
        if (planes[i] < 0 || planes[i] >= n_planes) return "plane index out of range";
    }
    return nullptr;
}
