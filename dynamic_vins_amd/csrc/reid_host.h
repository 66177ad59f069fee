// reid_host.h — the half of the ReID extractor (reid.hip) that is plain C++: the layer list of ReIdNetImpl (mot/reid_net.cpp:98-110) with the offsets ReIdNetImpl::load_form
// (mot/reid_net.cpp:123-135) reads its flat float32 file at, the accepted input sizes, the refusals, the eval-mode batch-norm fold, the weight layout the convolution kernel
// reads, and the rules the crop kernel and the host share in ONE copy: cvRound of a Rect2f's fields, the crop's validity, and cv::resize's INTER_LINEAR coordinates and
// short coefficients for 8-bit images (as remembered from OpenCV's imgproc/src/resize.cpp, unpinned: DESIGN.md section 2).
// No HIP in here: dv_reid_* use it, and tests/host/reid_host.cpp compiles it under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "dv_mem.h"

#ifdef __HIPCC__
#define DV_REID_HD __host__ __device__
#else
#define DV_REID_HD
#endif

constexpr int DV_REID_BLOCKS = 8, DV_REID_CONVS = 19;      // BasicBlocks of conv2; their convolutions (two per block, a third in each of the three down blocks)
constexpr int DV_REID_C1 = 64;                             // conv1: 3 -> 64, 3 x 3, stride 1, pad 1, WITH bias
constexpr float DV_REID_BN_EPS = 1e-5f;
struct DvReidBlock { int c_in, c_out, down; };
constexpr DvReidBlock DV_REID_BLOCK[DV_REID_BLOCKS] = {{64, 64, 0}, {64, 64, 0}, {64, 128, 1}, {128, 128, 0}, {128, 256, 1}, {256, 256, 0}, {256, 512, 1}, {512, 512, 0}};

// One convolution of conv2 in FILE order (per block: conv.0, conv.3, then the 1 x 1 of a down block).  w_off: its weight [c_out, c_in, k, k] in the flat file, bn_off: its
// batch-norm's weight, bias, running_mean, running_var (c_out floats each).  role 0: conv.0 (ReLU), 1: conv.3 (residual, ReLU), 2: the down branch (neither)
struct DvReidConv { int c_in, c_out, k, stride, role, block; size_t w_off, bn_off; };
struct DvReidPlan { size_t c1_w, c1_b, c1_bn; DvReidConv conv[DV_REID_CONVS]; size_t n_floats; };
constexpr DvReidPlan dv_reid_plan() {
    DvReidPlan P{};
    size_t off = 0;
    P.c1_w = off; off += (size_t)DV_REID_C1 * 27;
    P.c1_b = off; off += DV_REID_C1;
    P.c1_bn = off; off += 4 * (size_t)DV_REID_C1;
    int n = 0;
    for (int b = 0; b < DV_REID_BLOCKS; ++b) {
        const DvReidBlock B = DV_REID_BLOCK[b];
        for (int role = 0; role < (B.down ? 3 : 2); ++role) {
            DvReidConv c{};
            c.c_in = role == 1 ? B.c_out : B.c_in; c.c_out = B.c_out; c.k = role == 2 ? 1 : 3;
            c.stride = (role == 1 || !B.down) ? 1 : 2; c.role = role; c.block = b;
            c.w_off = off; off += (size_t)c.c_out * c.c_in * c.k * c.k;
            c.bn_off = off; off += 4 * (size_t)c.c_out;
            P.conv[n++] = c;
        }
    }
    P.n_floats = off;
    return P;
}
static_assert(dv_reid_plan().n_floats == DV_REID_N_FLOATS, "the float count of include/dvins.h is the layer list's");

// a stride-2 stage (the max-pool, the three down blocks) maps n -> ceil(n / 2)
constexpr int dv_reid_half(int n) { return (n + 1) / 2; }
constexpr int dv_reid_last(int n) { return dv_reid_half(dv_reid_half(dv_reid_half(dv_reid_half(n)))); }
// avg_pool2d({8, 4}, 1) must see exactly an 8 x 4 map: 512 values per crop (heights 113..128, widths 49..64)
constexpr bool dv_reid_size_ok(int in_w, int in_h) { return in_w > 0 && in_h > 0 && in_w <= 64 && in_h <= 128 && dv_reid_last(in_w) == 4 && dv_reid_last(in_h) == 8; }

// the reason a weight file / input size is refused, or nullptr
static inline const char* dv_reid_check_host(size_t n_floats, int in_w, int in_h) {
    if (n_floats != (size_t)DV_REID_N_FLOATS) return "weights: the flat file of ReIdNetImpl::load_form holds exactly 11178496 floats";
    if (!dv_reid_size_ok(in_w, in_h)) return "input size: the last map must be 8 x 4 (reid_input_height 113..128, reid_input_width 49..64)";
    return nullptr;
}
// the reason a frame is refused at the enqueue, or nullptr (n = 0: Extractor::extract returns an empty tensor, mot/extractor.cpp:32-34)
static inline const char* dv_reid_frame_check_host(const uint8_t* bgr, int img_w, int stride, const float* rects, int n, int mem) {
    if (n < 0 || n > DV_REID_MAX_CROPS) return "0..64 rectangles";
    if (!dv_mem_known(mem)) return "unknown memory kind";
    if (n == 0) return nullptr;
    if (!bgr || !rects) return "null image or rectangles";
    if (stride < 3 * img_w) return "row stride below 3 * width";
    if ((uintptr_t)rects & 3) return "rectangles must be 4-byte aligned";
    return nullptr;
}
// the reason dv_reid_layer refuses its shapes, or nullptr: the (kernel, stride) pairs of the net, channel counts the tiles divide
static inline const char* dv_reid_layer_check_host(int n, int c_in, int h, int w, int c_out, int k, int stride) {
    if (n < 1 || n > DV_REID_MAX_CROPS) return "1..64 images";
    if (h < 1 || h > 128 || w < 1 || w > 128) return "height and width 1..128";
    if (!((k == 3 && (stride == 1 || stride == 2)) || (k == 1 && stride == 2))) return "kernel 3 with stride 1 or 2, or kernel 1 with stride 2";
    if (c_in < 32 || c_in > 512 || c_in % 32) return "c_in a multiple of 32 up to 512";
    if (c_out < 64 || c_out > 512 || c_out % 64) return "c_out a multiple of 64 up to 512";
    // the operator is for small cases: twice the net's largest activation (64 crops x 64 x 32 x 64) bounds its host and device buffers
    if ((long long)n * h * w * (c_in > c_out ? c_in : c_out) > (1LL << 24)) return "n * h * w * channels beyond 2^24 elements";
    return nullptr;
}
// the reason dv_reid_stem refuses its shapes, or nullptr: at most 64 x 3 x 128 x 128 in and 64 x 64 x 64 x 64 out, the 2^24 elements of the layer operator
static inline const char* dv_reid_stem_check_host(int n, int h, int w) {
    if (n < 1 || n > DV_REID_MAX_CROPS) return "1..64 images";
    if (h < 1 || h > 128 || w < 1 || w > 128) return "height and width 1..128";
    return nullptr;
}
constexpr int dv_reid_out_size(int n, int k, int stride) { return (n + (k == 3 ? 2 : 0) - k) / stride + 1; }

// Eval-mode batch-norm as y = x * scale + shift, in float64, rounded once: scale = w / sqrt(var + eps), shift = b - mean * scale (+ conv_bias * scale).  A declared
// deviation: the reference's batch_norm evaluates (x - mean) / sqrt(var + eps) * w + b in float32
static inline void dv_reid_fold(const float* bn /* w, b, mean, var: c each */, const float* conv_bias_or_null, int c, float* scale, float* shift) {
    for (int i = 0; i < c; ++i) {
        const double s = (double)bn[i] / std::sqrt((double)bn[3 * c + i] + (double)DV_REID_BN_EPS);
        const double t = (double)bn[c + i] - (double)bn[2 * c + i] * s + (conv_bias_or_null ? (double)conv_bias_or_null[i] * s : 0.0);
        scale[i] = (float)s; shift[i] = (float)t;
    }
}
// The convolution kernel's B operand: [tap = ky * k + kx][c_in / 4][c_out][4] from torch's [c_out][c_in][k][k], so that a lane's four consecutive input channels are one
// 16-byte load and the 32 lanes of a half wave read 512 contiguous bytes
static inline void dv_reid_pack(const float* w, int c_in, int c_out, int k, float* out) {
    for (int tap = 0; tap < k * k; ++tap)
        for (int ci = 0; ci < c_in; ++ci)
            for (int co = 0; co < c_out; ++co)
                out[(((size_t)tap * (c_in / 4) + ci / 4) * c_out + co) * 4 + (ci & 3)] = w[((size_t)co * c_in + ci) * k * k + tap];
}
// conv1's weights as [t = (ci * 3 + ky) * 3 + kx][64]: a lane per output channel reads them coalesced
static inline void dv_reid_pack_c1(const float* w, float* out) {
    for (int co = 0; co < DV_REID_C1; ++co) for (int t = 0; t < 27; ++t) out[t * DV_REID_C1 + co] = w[co * 27 + t];
}
// (u * (1 / 255.f) - mean[c]) / std[c] in float32 for every byte: convertTo(CV_32F, 1 / 255) then sub_ / div_ (mot/extractor.cpp:45-48, mot/mot_parameter.h:26-27).
// Tensor channel c reads the image's byte 2 - c (cvtColor's swap).  Compile with -ffp-contract=off
static inline void dv_reid_lut(float* lut /* [3][256] */) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const float inv = 1 / 255.f;
    for (int c = 0; c < 3; ++c) for (int u = 0; u < 256; ++u) { const float v = (float)u * inv; lut[c * 256 + u] = (v - mean[c]) / sd[c]; }
}

// cvRound on a float: round half to even.  false where the value cannot be a pixel coordinate (NaN, infinite, beyond 2^24)
DV_REID_HD static inline bool dv_reid_round(float v, int* out) {
    if (!(v > -16777216.0f && v < 16777216.0f)) return false;
    *out = (int)rintf(v);
    return true;
}
// Rect2f -> Rect (cvRound per field) and ori_img(rect)'s assertion: 0 <= x, 0 <= w, x + w <= cols, the same in y; an empty crop fails cv::resize
DV_REID_HD static inline bool dv_reid_rect(const float* r, int img_w, int img_h, int* q /* x, y, w, h */) {
    if (!dv_reid_round(r[0], q) || !dv_reid_round(r[1], q + 1) || !dv_reid_round(r[2], q + 2) || !dv_reid_round(r[3], q + 3)) return false;
    return q[0] >= 0 && q[1] >= 0 && q[2] > 0 && q[3] > 0 && q[0] + q[2] <= img_w && q[1] + q[3] <= img_h;
}
// cv::resize INTER_LINEAR on 8-bit: source indices and the two short coefficients of destination index d.  Horizontally the index is clamped WITH its fraction (sx < 0 ->
// 0, f = 0; sx >= src - 1 -> src - 1, f = 0); vertically the fraction is kept and the two row indices are clamped to [0, src - 1].  Clamping is to the CROP
DV_REID_HD static inline void dv_reid_coef(int d, int src, int dst, bool vertical, int* i0, int* i1, int* c0, int* c1) {
    const double scale = src / (double)dst;
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (!vertical) {
        if (s < 0) { s = 0; f = 0; }
        if (s >= src - 1) { s = src - 1; f = 0; }
        *i0 = s; *i1 = s + 1 < src ? s + 1 : src - 1;
    } else {
        *i0 = s < 0 ? 0 : (s > src - 1 ? src - 1 : s);
        *i1 = s + 1 < 0 ? 0 : (s + 1 > src - 1 ? src - 1 : s + 1);
    }
    *c0 = (int)rintf((1.f - f) * 2048.f); *c1 = (int)rintf(f * 2048.f);
}
// the vertical pass on two horizontal sums
DV_REID_HD static inline int dv_reid_vert(int S0, int S1, int b0, int b1) {
    const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// INTER_LINEAR becomes the fast area path when both scales are exactly 2
DV_REID_HD static inline bool dv_reid_area2(int cw, int ch, int in_w, int in_h) { return cw == 2 * in_w && ch == 2 * in_h; }
// one prepared byte of crop q at destination (dx, dy), image channel ch (0 = B)
DV_REID_HD static inline int dv_reid_pixel(const uint8_t* bgr, int stride, const int* q, int in_w, int in_h, int dx, int dy, int ch) {
    const uint8_t* base = bgr + (size_t)q[1] * stride + (size_t)q[0] * 3 + ch;
    if (dv_reid_area2(q[2], q[3], in_w, in_h)) {
        const uint8_t* p = base + (size_t)(2 * dy) * stride + (size_t)(2 * dx) * 3;
        return (p[0] + p[3] + p[stride] + p[stride + 3] + 2) >> 2;
    }
    int x0, x1, a0, a1, y0, y1, b0, b1;
    dv_reid_coef(dx, q[2], in_w, false, &x0, &x1, &a0, &a1);
    dv_reid_coef(dy, q[3], in_h, true, &y0, &y1, &b0, &b1);
    const uint8_t* r0 = base + (size_t)y0 * stride; const uint8_t* r1 = base + (size_t)y1 * stride;
    const int S0 = r0[x0 * 3] * a0 + r0[x1 * 3] * a1, S1 = r1[x0 * 3] * a0 + r1[x1 * 3] * a1;
    return dv_reid_vert(S0, S1, b0, b1);
}
