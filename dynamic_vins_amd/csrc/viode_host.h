// viode_host.h — host half of VIODE::SetViodeMaskAndRoi (utils/dataset/viode_utils.cpp:177-218) behind viode_mask_kernel: the frame's Box2D list from the per-key
// bounding boxes.  Plain C++ (no HIP): dv_viode_frame_collect uses it, and tests/host compiles it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include "../../include/dvins.h"

// what the box buffers of viode_mask_kernel and inst_stack_kernel hold before a frame: (row_min, row_max, col_min, col_max) = (max, -1, max, -1) for each of 64 boxes
static inline void dv_boxes_init(int32_t* init /* [256] */) {
    for (int k = 0; k < 64; ++k) { init[4 * k] = 0x7fffffff; init[4 * k + 1] = -1; init[4 * k + 2] = 0x7fffffff; init[4 * k + 3] = -1; }
}

// boxes[k] = row_min, row_max, col_min, col_max of keys[k]'s pixels (row_max < row_min: key absent).  One detection per key present, in ASCENDING key (the reference walks
// an unordered_map; the object tracker visits its instances in ascending id either way): rect = cv::Rect(min_pt, max_pt), i.e. the max row / column excluded;
// track_id = key, class 0, mask / points NULL.  A rectangle under min_size pixels on a side (and any empty one) is dropped — the rule dvins_node and
// dynamic_vins_amd/viode.py detections() share (declared deviation).  -> number of detections, or -1 when `cap` is too small.
static inline int dv_viode_build_dets(const int32_t* boxes, const uint32_t* keys, int nkeys, int min_size, dv_inst_det* dets, int cap) {
    int order[64];
    if (nkeys < 0 || nkeys > 64) return -1;
    for (int k = 0; k < nkeys; ++k) order[k] = k;
    std::stable_sort(order, order + nkeys, [&](int a, int b) { return keys[a] < keys[b]; });
    const int floor_px = std::max(min_size, 1);
    int n = 0;
    for (int i = 0; i < nkeys; ++i) {
        const int k = order[i];
        const int r0 = boxes[4 * k], r1 = boxes[4 * k + 1], c0 = boxes[4 * k + 2], c1 = boxes[4 * k + 3];
        if (r1 < r0 || c1 < c0) continue;
        const int w = c1 - c0, h = r1 - r0;
        if (w < floor_px || h < floor_px) continue;
        if (n >= cap) return -1;
        dv_inst_det d{};
        d.track_id = keys[k]; d.class_id = 0; d.x = c0; d.y = r0; d.w = w; d.h = h; d.mask = nullptr; d.points = nullptr; d.n_points = 0;
        dets[n++] = d;
    }
    return n;
}
