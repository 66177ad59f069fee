// solo_head_host.h — host half of the detector head (solo_head.hip): the refusals of a dv_solo_outputs / dv_solo_params pair, the cell tables the kernels index by, the
// pixel floor of a concatenated cell (Solov2::Solov2 + GetSegTensor, det2d/solo_head.cpp:24-28,454-465), Pipeline::GetXYWHS (det2d/pipeline.cpp:23-48) and the float32
// scale of upsample_bilinear2d with align_corners = true.  Plain C++ (no HIP): dv_solo_head_enqueue uses it, and tests/host compiles it under the sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include "dv_mem.h"

constexpr int DV_SOLO_MAX_CHANNELS = 256, DV_SOLO_MAX_CLASSES = 128, DV_SOLO_MAX_GRID = 64, DV_SOLO_MAX_PIXELS = 1 << 20;

// Pipeline::GetXYWHS: the ratios in float, the scaled side truncated and bumped to even, centred along the other axis.  (r_h > r_w: the width fills the input.)
static inline int dv_solo_rect_host(int model_w, int model_h, int img_w, int img_h, int* x, int* y, int* w, int* h) {
    if (model_w <= 0 || model_h <= 0 || img_w <= 0 || img_h <= 0 || !x || !y || !w || !h) return -1;
    const float r_w = static_cast<float>(model_w / (img_w * 1.0f)), r_h = static_cast<float>(model_h / (img_h * 1.0f));
    if (r_h > r_w) {
        *w = model_w; *h = static_cast<int>(r_w * img_h);
        if (*h % 2 == 1) ++*h;
        *x = 0; *y = (model_h - *h) / 2;
    } else {
        *w = static_cast<int>(r_h * img_w);
        if (*w % 2 == 1) ++*w;
        *h = model_h; *x = (model_w - *w) / 2; *y = 0;
    }
    return 0;
}

// cells of the levels as they are concatenated (the levels' OWN g: addressing) and the pixel-floor boundaries (num_grids[] ONLY: the reference's rule, see include/dvins.h)
struct DvSoloTables { int cell_off[DV_SOLO_MAX_LEVELS + 1]; int floor_end[DV_SOLO_MAX_LEVELS]; };
static inline void dv_solo_tables(const dv_solo_outputs* o, const dv_solo_params* p, DvSoloTables* t) {
    t->cell_off[0] = 0;
    long long cum = 0;
    for (int l = 0; l < DV_SOLO_MAX_LEVELS; ++l) {
        const bool in = l < o->n_levels;
        t->cell_off[l + 1] = t->cell_off[l] + (in ? o->grid[l] * o->grid[l] : 0);
        if (in) cum += (long long)p->num_grids[l] * p->num_grids[l];
        t->floor_end[l] = in ? (int)cum : 0;
    }
}
// strides.index({pred_index}) of the reference: ones, overwritten slice by slice.  The ONE copy of the rule: solo_emit_kernel calls it on the device
#ifdef __HIPCC__
#define DV_SOLO_HD __host__ __device__
#else
#define DV_SOLO_HD
#endif
DV_SOLO_HD static inline float dv_solo_floor_of(int cell, int n_levels, const int* floor_end, const float* strides) {
    for (int l = 0; l < n_levels; ++l) if (cell < floor_end[l]) return strides[l];
    return 1.0f;
}
// area_pixel_compute_scale<float>(in, out, align_corners = true)
static inline float dv_solo_scale(int in, int out) { return out > 1 ? static_cast<float>(in - 1) / (out - 1) : 0.0f; }

// the reason a head call is refused, or nullptr
static inline const char* dv_solo_check_host(const dv_solo_outputs* o, const dv_solo_params* p) {
    if (!o || !p) return "null argument";
    if (o->n_levels < 1 || o->n_levels > DV_SOLO_MAX_LEVELS) return "1..5 levels";
    if (o->channels < 1 || o->channels > DV_SOLO_MAX_CHANNELS) return "1..256 channels";
    if (o->n_classes < 1 || o->n_classes > DV_SOLO_MAX_CLASSES) return "1..128 classes";
    if (!dv_mem_known(o->mem)) return "unknown memory kind";
    for (int l = 0; l < o->n_levels; ++l) {
        if (o->grid[l] < 1 || o->grid[l] > DV_SOLO_MAX_GRID) return "level grid outside 1..64";
        if (!o->kernel[l] || !o->cate[l]) return "null level tensor";
        if (((uintptr_t)o->kernel[l] | (uintptr_t)o->cate[l]) & 3) return "tensors must be 4-byte aligned";
        if (p->num_grids[l] < 1 || p->num_grids[l] > 1024) return "num_grids outside 1..1024";
        if (!(p->strides[l] >= 0.0f)) return "negative or NaN stride";
    }
    if (!o->feature || ((uintptr_t)o->feature & 3)) return "null or unaligned mask feature";
    if (o->fh < 1 || o->fw < 1 || (long long)o->fh * o->fw > DV_SOLO_MAX_PIXELS) return "mask feature size outside 1..2^20 pixels";
    if (std::isnan(p->score_thr) || std::isnan(p->mask_thr) || std::isnan(p->update_thr)) return "NaN threshold";
    if (p->nms_kernel != DV_SOLO_NMS_GAUSSIAN && p->nms_kernel != DV_SOLO_NMS_LINEAR) return "unknown NMS kernel";
    if (p->nms_kernel == DV_SOLO_NMS_GAUSSIAN && !(p->nms_sigma > 0.0f && std::isfinite(p->nms_sigma))) return "nms_sigma must be positive";
    if (p->max_candidates < 1 || p->max_candidates > DV_SOLO_MAX_CANDIDATES) return "max_candidates outside 1..4096";
    if (p->nms_pre < 1 || p->nms_pre > DV_SOLO_MAX_NMS_PRE) return "nms_pre outside 1..512";
    if (p->max_per_img < 1 || p->max_per_img > DV_SOLO_MAX_PER_IMG) return "max_per_img outside 1..128";
    if (p->origin_w < 1 || p->origin_h < 1 || p->origin_w > 16384 || p->origin_h > 16384) return "origin size outside 1..16384";
    if (p->rect_w < 1 || p->rect_h < 1 || p->rect_x < 0 || p->rect_y < 0 || p->rect_w > 4 * o->fw || p->rect_h > 4 * o->fh || p->rect_x > 4 * o->fw - p->rect_w ||
        p->rect_y > 4 * o->fh - p->rect_h) return "image rectangle outside the 4x mask feature";
    return nullptr;
}
