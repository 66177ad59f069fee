// solo_input_host.h — host half of the detector's input stage (solo_input.hip): the refusals of a frame / dv_solo_input_params pair, and the per-axis source index and
// weights of upsample_bilinear2d with align_corners = true in float32, the rule Pipeline::ProcessInput's interpolate applies (det2d/pipeline.cpp:204-232).  The rectangle
// (Pipeline::GetXYWHS) and the float32 scale are solo_head_host.h's.  Plain C++ (no HIP): dv_solo_input_enqueue uses it, the kernel calls the ONE copy of the axis rule on
// the device, and tests/host compiles it under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include "solo_head_host.h"

constexpr int DV_SOLO_INPUT_MAX_SIDE = 16384;

// destination index dst of an axis resampled from `in` samples: r = scale * dst in float32, i0 = int(r), i1 = i0 + (i0 < in - 1), l1 = r - i0, l0 = 1 - l1.
// (scale * (out - 1) can round a hair over in - 1; int() still gives in - 1 there, and the clamp only states it.)
DV_SOLO_HD static inline void dv_solo_input_axis(float scale, int dst, int in, int* i0, int* i1, float* l0, float* l1) {
    const float r = scale * (float)dst;
    int a = (int)r;
    if (a > in - 1) a = in - 1;
    *i0 = a; *i1 = a + (a < in - 1 ? 1 : 0);
    *l1 = r - (float)a; *l0 = 1.0f - *l1;
}

// The bilinear value lh0 (lw0 p00 + lw1 p01) + lh1 (lw0 p10 + lw1 p11) with lh0 = 1 - lh1, lw0 = 1 - lw1, evaluated in float32 as nested differences:
// top = p00 + lw1 (p01 - p00), bot = p10 + lw1 (p11 - p10), top + lh1 (bot - top).  Same value, other roundings: four equal sources give the source's bits (the
// sum-of-products form with a rounded 1 - l1 leaves a constant image up to one ulp off the constant), and an upper weight of 0 gives the lower sample's bits.  With
// operands up to 2.64 every difference is below 5.3 (half an ulp 2.4e-7), every partial value below 2.64 (1.2e-7): top and bot carry at most 6e-7 each, the outer
// step adds 6e-7, and the rounding of the reference's 1 - l1 moves its own value by at most 1.6e-7 per axis: under 1.6e-6 from the reference's float64 value.
DV_SOLO_HD static inline float dv_solo_input_value(float p00, float p01, float p10, float p11, float lw1, float lh1) {
    const float top = p00 + lw1 * (p01 - p00), bot = p10 + lw1 * (p11 - p10);
    return top + lh1 * (bot - top);
}

// one normalised value: the byte as float, minus the mean, divided (IEEE) by the deviation — ((input_tensor - mean_t) / std_t).  Compile with -ffp-contract=off
DV_SOLO_HD static inline float dv_solo_input_norm(int byte, float mean, float sd) { return ((float)byte - mean) / sd; }

// the reason a frame of img_w x img_h with `stride` bytes per row is refused for these parameters, or nullptr; on success the rectangle of dv_solo_rect
static inline const char* dv_solo_input_check_host(int img_w, int img_h, int stride, const dv_solo_input_params* p, int* rx, int* ry, int* rw, int* rh) {
    if (!p) return "null parameters";
    if (img_w <= 0 || img_h <= 0 || p->model_w <= 0 || p->model_h <= 0) return "image and model sizes must be positive";
    if (img_w > DV_SOLO_INPUT_MAX_SIDE || img_h > DV_SOLO_INPUT_MAX_SIDE || p->model_w > DV_SOLO_INPUT_MAX_SIDE || p->model_h > DV_SOLO_INPUT_MAX_SIDE) return "image and model sides up to 16384";
    if (img_w < 2 || img_h < 2) return "image sides under 2 cannot be resampled with align_corners";
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(p->mean[c]) || !std::isfinite(p->std[c])) return "mean and std must be finite";
        if (p->std[c] == 0.0f) return "std must not be zero";
    }
    if (stride < 3 * img_w) return "row stride below 3 * width";
    int x, y, w, h;
    if (dv_solo_rect_host(p->model_w, p->model_h, img_w, img_h, &x, &y, &w, &h)) return "no rectangle";
    if (w < 2 || h < 2) return "rectangle sides under 2 cannot be resampled with align_corners";
    if (w > p->model_w || h > p->model_h) return "the rectangle rounded up to even leaves the model input";
    // the reference concatenates two pads of (model - rect) / 2: an odd difference hands the network a tensor one row or column short
    if ((p->model_h - h) % 2 != 0 || (p->model_w - w) % 2 != 0) return "model side minus rectangle side is odd: the reference's two pads leave the tensor one short";
    if (rx) *rx = x;
    if (ry) *ry = y;
    if (rw) *rw = w;
    if (rh) *rh = h;
    return nullptr;
}
