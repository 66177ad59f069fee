// lbd_host.h — the half of the LBD stage (lbd.hip) that is plain C++: the refusals, the two weight tables of BinaryDescriptor's constructor
// (thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:217-259), the blur's weights, the band-pair table (:74-107), the pixel-count rule, the sample and
// end-point roundings, the tail of computeLBD behind the band sums (:1246-1340) and Detect's selection (line_detector/line_detector.cpp:82-96), each in ONE copy the
// kernels and the host share.  No HIP in here: dv_lbd_* use it, and tests/host/lbd_host.cpp compiles it under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "dv_mem.h"

#ifdef __HIPCC__
#define DV_LBD_HD __host__ __device__
#else
#define DV_LBD_HD
#endif

constexpr int DV_LBD_BANDS = 9, DV_LBD_BAND_W = 7, DV_LBD_ROWS = DV_LBD_BANDS * DV_LBD_BAND_W;      // NUM_OF_BANDS, Params::widthOfBand_, heightOfLSP
constexpr int DV_LBD_FLOATS = DV_LBD_BANDS * 8;                                                      // descriptor_size
constexpr int DV_LBD_MAX_DIM = 32767;                                                                // imageWidth / imageHeight are `short`
static_assert(DV_LBD_ROWS == 63 && DV_LBD_FLOATS == 72 && DV_LINE_DESC_BYTES == 32, "one wave per line, one lane per row");

// cv::GaussianBlur(img, Size(5, 5), 1) as a separable kernel in 8-bit fixed point: exp(-x^2 / 2) normalised and scaled by 256 is 13.95, 62.52, 103.07; the five
// weights must sum to 256.  Both passes accumulate exactly; ONE rounding at the end: (sum + 2^15) >> 16.  DECLARED CHOICE, unpinned: OpenCV is
// not available to pin its own integer rule against.
constexpr int DV_LBD_BLUR_W[5] = { 14, 62, 104, 62, 14 };
static_assert(DV_LBD_BLUR_W[0] + DV_LBD_BLUR_W[1] + DV_LBD_BLUR_W[2] + DV_LBD_BLUR_W[3] + DV_LBD_BLUR_W[4] == 256, "the blur keeps the mean");

// BORDER_REFLECT_101 (cv::borderInterpolate): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...
DV_LBD_HD static inline int dv_lbd_reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// combinations[32][2] (:74-107) by its rule: the pairs (a, b), a < b, of the 9 bands in lexicographic order without (0, 7), (0, 8), (1, 7), (1, 8)
DV_LBD_HD static inline void dv_lbd_pair(int k, int* a, int* b) {
    int c = 0;
    for (int i = 0; i < DV_LBD_BANDS; ++i)
        for (int j = i + 1; j < DV_LBD_BANDS; ++j) {
            if (i <= 1 && j >= 7) continue;
            if (c == k) { *a = i; *b = j; return; }
            ++c;
        }
    *a = *b = 0;
}

// gaussCoefG_ (63 global weights, u = sigma = 31) and gaussCoefL_ (21 local weights, u = 10, sigma = 7): the constructor's INTEGER divisions, exp in double, cast to
// float where computeLBD uses them (:1188,1202,1218,1231)
struct DvLbdTabs { float g[DV_LBD_ROWS]; float l[3 * DV_LBD_BAND_W]; };
static inline void dv_lbd_tables(DvLbdTabs* t) {
    double u = (DV_LBD_BAND_W * 3 - 1) / 2;
    double sigma = (DV_LBD_BAND_W * 2 + 1) / 2;
    double inv = -1 / (2 * sigma * sigma);
    for (int i = 0; i < 3 * DV_LBD_BAND_W; ++i) { const double d = i - u; t->l[i] = (float)std::exp(d * d * inv); }
    u = (DV_LBD_BANDS * DV_LBD_BAND_W - 1) / 2;
    sigma = u;
    inv = -1 / (2 * sigma * sigma);
    for (int i = 0; i < DV_LBD_ROWS; ++i) { const double d = i - u; t->g[i] = (float)std::exp(d * d * inv); }
}

// cv::Point(Point2f): saturate_cast<int>(float) = cvRound, nearest integer, ties to even.  Returned as a float (whole, or not finite): the caller compares before it converts
DV_LBD_HD static inline float dv_lbd_rint(float v) { return rintf(v); }
// the pixel of an end point when it lies inside a w x h mask
DV_LBD_HD static inline bool dv_lbd_mask_pixel(float x, float y, int w, int h, int* ix, int* iy) {
    const float rx = dv_lbd_rint(x), ry = dv_lbd_rint(y);
    if (!(rx >= 0.0f && rx < (float)w && ry >= 0.0f && ry < (float)h)) return false;
    *ix = (int)rx; *iy = (int)ry;
    return true;
}
// KeyLine::numOfPixels when the caller has none: cv::LineIterator's count (8-connected) for a segment inside the image.  Saturates far outside any accepted range
DV_LBD_HD static inline int dv_lbd_npix(float sx, float sy, float ex, float ey) {
    const double ax = fabs((double)dv_lbd_rint(ex) - (double)dv_lbd_rint(sx)), ay = fabs((double)dv_lbd_rint(ey) - (double)dv_lbd_rint(sy));
    const double m = (ax > ay ? ax : ay) + 1.0;
    return m < 1.0e9 ? (int)m : 1000000000;      // (NaN: the comparison is false)
}
// (short) round(v) clamped to [0, hi] (:1155-1158): half away from zero, then the x86-64 conversion — through int32, low 16 bits kept; out of int32's range, or NaN,
// the "integer indefinite" 0x80000000, whose low half is 0
DV_LBD_HD static inline int dv_lbd_coord(float v, int hi) {
    const float r = roundf(v);
    int t = 0;
    if (r > -2147483648.0f && r < 2147483648.0f) t = (int)(int16_t)(uint16_t)((uint32_t)(int32_t)r & 0xffffu);
    return t < 0 ? 0 : (t > hi ? hi : t);
}

// float32 sqrt and division, correctly rounded on both sides: sqrtf and `/` are IEEE operations on the host, and the device compiler's default
// (-fhip-fp32-correctly-rounded-divide-sqrt) keeps them so.  NOT __fsqrt_rn: the HIP headers map it to the native, 1-ulp square root
DV_LBD_HD static inline float dv_lbd_sqrt(float x) { return sqrtf(x); }
DV_LBD_HD static inline float dv_lbd_div(float a, float b) { return a / b; }

// computeLBD behind the row loop (:1246-1340).  band[q][b]: the band sums, q = 0 pgdL, 1 ngdL, 2 pgdL2, 3 ngdL2, 4 pgdO, 5 ngdO, 6 pgdO2, 7 ngdO2.  des: 72 floats.
// Every sum runs in the reference's order; no product is fused into an add (the translation units that include this are built with -ffp-contract=off).  NaN travels:
// a flat image gives 0 * (1 / sqrt(0)) everywhere
DV_LBD_HD static inline void dv_lbd_finish(const float (*band)[DV_LBD_BANDS], float* des) {
    const float invN2 = (float)(1.0 / (DV_LBD_BAND_W * 2.0)), invN3 = (float)(1.0 / (DV_LBD_BAND_W * 3.0));
    for (int b = 0; b < DV_LBD_BANDS; ++b) {
        const float invN = (b == 0 || b == DV_LBD_BANDS - 1) ? invN2 : invN3;
        float* d = des + b * 8;
        float t = band[0][b] * invN;
        d[0] = t; d[4] = dv_lbd_sqrt(band[2][b] * invN - t * t);
        t = band[1][b] * invN;
        d[1] = t; d[5] = dv_lbd_sqrt(band[3][b] * invN - t * t);
        t = band[4][b] * invN;
        d[2] = t; d[6] = dv_lbd_sqrt(band[6][b] * invN - t * t);
        t = band[5][b] * invN;
        d[3] = t; d[7] = dv_lbd_sqrt(band[7][b] * invN - t * t);
    }
    float tm = 0, ts = 0;
    for (int b = 0; b < DV_LBD_BANDS; ++b) {
        const float* d = des + b * 8;
        tm += d[0] * d[0]; tm += d[1] * d[1]; tm += d[2] * d[2]; tm += d[3] * d[3];
        ts += d[4] * d[4]; ts += d[5] * d[5]; ts += d[6] * d[6]; ts += d[7] * d[7];
    }
    tm = dv_lbd_div(1.0f, dv_lbd_sqrt(tm));
    ts = dv_lbd_div(1.0f, dv_lbd_sqrt(ts));
    for (int b = 0; b < DV_LBD_BANDS; ++b) {
        float* d = des + b * 8;
        for (int k = 0; k < 4; ++k) { d[k] = d[k] * tm; d[4 + k] = d[4 + k] * ts; }
    }
    for (int i = 0; i < DV_LBD_FLOATS; ++i) if ((double)des[i] > 0.4) des[i] = (float)0.4;      // the DOUBLE literal (:1324)
    float t = 0;
    for (int i = 0; i < DV_LBD_FLOATS; ++i) t += des[i] * des[i];
    t = dv_lbd_div(1.0f, dv_lbd_sqrt(t));
    for (int i = 0; i < DV_LBD_FLOATS; ++i) des[i] = des[i] * t;
}
// binaryConversion (:401-412) over pair k: bit i is f1[i] > f2[i]; a NaN sets no bit
DV_LBD_HD static inline uint8_t dv_lbd_byte(const float* des, int k) {
    int a, b;
    dv_lbd_pair(k, &a, &b);
    unsigned r = 0;
    for (int i = 0; i < 8; ++i) if (des[8 * a + i] > des[8 * b + i]) r |= 1u << i;
    return (uint8_t)r;
}

// a line as the kernels read it: the key line, dL = (cos, sin) of its angle and numOfPixels.  The direction is computed HERE, on the host, per line:
// (float)cos((double)angle) — DECLARED CHOICE: computeLBD's unqualified cos(float) is taken as the double overload, rounded by the store to float
struct DvLbdLine { dv_key_line k; float c, s; int32_t npix; };
static_assert(sizeof(DvLbdLine) == 36, "packed words");
static inline DvLbdLine dv_lbd_line(const dv_key_line& k, int npix) {
    DvLbdLine L;
    L.k = k; L.c = (float)std::cos((double)k.angle); L.s = (float)std::sin((double)k.angle); L.npix = npix;
    return L;
}

// the reason the VALUES of n lines are refused, or nullptr.  num_pixels may be NULL (the library's rule)
static inline const char* dv_lbd_values_check_host(int w, int h, const dv_key_line* lines, const int32_t* num_pixels, int n) {
    for (int i = 0; i < n; ++i) {
        const dv_key_line& k = lines[i];
        if (!std::isfinite(k.sx) || !std::isfinite(k.sy) || !std::isfinite(k.ex) || !std::isfinite(k.ey) || !std::isfinite(k.angle))
            return "a key line has a non-finite coordinate or angle";      // (the length only meets min_length: NaN drops the line, +inf always keeps it)
        const int np = num_pixels ? num_pixels[i] : dv_lbd_npix(k.sx, k.sy, k.ex, k.ey);
        if (np < 1 || np > w + h) return "num_pixels of a line is below 1 or above w + h";
    }
    return nullptr;
}
// the reason a frame is refused, or nullptr.  Lines in device memory cannot be read here: their values are checked by the enqueue, which fetches them anyway
static inline const char* dv_lbd_check_host(int w, int h, int stride, const dv_key_line* lines, const int32_t* num_pixels, int n, int lines_mem, const uint8_t* mask, int mask_stride) {
    if (!dv_mem_known(lines_mem)) return "unknown memory kind";
    if (w < 1 || h < 1) return "empty image";
    if (w > DV_LBD_MAX_DIM || h > DV_LBD_MAX_DIM) return "image wider or higher than 32767 (the descriptor's coordinates are 16-bit)";
    if (stride < w) return "stride below the width";
    if (mask && mask_stride < w) return "mask stride below the width";
    if (n < 0) return "negative line count";
    if (n > DV_LINE_MAX) return "more than DV_LINE_MAX (512) lines in one image";
    if (n == 0) return nullptr;
    if (!lines) return "null key lines";
    if (((uintptr_t)lines | (uintptr_t)num_pixels) & 3) return "key lines and num_pixels must be 4-byte aligned";
    if (lines_mem == DV_MEM_DEVICE) return nullptr;
    return dv_lbd_values_check_host(w, h, lines, num_pixels, n);
}

// Detect's selection (:82-96) of one line.  mask: w x h bytes or NULL.  DEVIATION, declared: an end point that rounds outside the mask drops the line (the reference
// reads outside the matrix there)
DV_LBD_HD static inline bool dv_lbd_keep(const dv_key_line& k, float min_length, const uint8_t* mask, int mask_stride, int w, int h) {
    if (!(k.length >= min_length)) return false;
    if (!mask) return true;
    int x, y;
    if (!dv_lbd_mask_pixel(k.sx, k.sy, w, h, &x, &y) || mask[(size_t)y * mask_stride + x] == 0) return false;
    if (!dv_lbd_mask_pixel(k.ex, k.ey, w, h, &x, &y) || mask[(size_t)y * mask_stride + x] == 0) return false;
    return true;
}

// The frame's device -> host block: the count, then src[DV_LINE_MAX]
enum { DV_LBD_O_NKEPT = 0, DV_LBD_O_WORDS = 16 };
constexpr size_t DV_LBD_OUT_BYTES = (size_t)(DV_LBD_O_WORDS + DV_LINE_MAX) * 4;
