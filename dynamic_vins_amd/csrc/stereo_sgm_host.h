// stereo_sgm_host.h — the rules of the stereo matcher (stereo_sgm.hip) that exist ONCE, for the host and the device: the census clamp and bit order, the matching
// cost, the path step, the uniqueness test, the floored subpixel division and the refusals of a frame / dv_sgm_params pair.  The stage stands where the reference's
// MyStereoMatcher::Launch / WaitResult (stereo/stereo.cpp) read an offline network's PNG into SemanticImage::disp; the specification is include/dvins.h's.  Plain C++
// (no HIP): dv_stereo_sgm_enqueue uses it, the kernels call these copies on the device, and tests/host compiles it under the sanitizers.
#pragma once
#include <cstdint>
#include "dv_mem.h"

#ifdef __HIPCC__
#define DV_SGM_HD __host__ __device__
#else
#define DV_SGM_HD
#endif

constexpr int DV_SGM_CENSUS_RX = 4, DV_SGM_CENSUS_RY = 3;      // the window is 9 wide and 7 high
constexpr int DV_SGM_OOB_COST = 64;                            // C(x, y, d) for x - d < 0
constexpr int DV_SGM_MAX_SIDE = 16384;

// replicate border: a source coordinate clamped to [0, n)
DV_SGM_HD static inline int dv_sgm_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// one position of the window enters the code: row-major over the window, the centre skipped, earlier positions in higher bits
DV_SGM_HD static inline uint64_t dv_sgm_census_push(uint64_t code, int neighbour, int centre) { return (code << 1) | (uint64_t)(neighbour < centre ? 1 : 0); }

// the census code of pixel (x, y) of a w x h image with `stride` bytes per row (the kernel walks the same positions in the same order over its LDS tile, which
// it fills through dv_sgm_clamp)
DV_SGM_HD static inline uint64_t dv_sgm_census(const uint8_t* img, int stride, int w, int h, int x, int y) {
    const int c = img[(size_t)y * stride + x];
    uint64_t code = 0;
    for (int dy = -DV_SGM_CENSUS_RY; dy <= DV_SGM_CENSUS_RY; ++dy)
        for (int dx = -DV_SGM_CENSUS_RX; dx <= DV_SGM_CENSUS_RX; ++dx) {
            if (dx == 0 && dy == 0) continue;
            code = dv_sgm_census_push(code, img[(size_t)dv_sgm_clamp(y + dy, h) * stride + dv_sgm_clamp(x + dx, w)], c);
        }
    return code;
}

DV_SGM_HD static inline int dv_sgm_popcount(uint64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

// C(x, y, d) from the left code at x and the right code at x - d (right_code is not read for x - d < 0: pass anything)
DV_SGM_HD static inline int dv_sgm_cost(uint64_t left_code, uint64_t right_code, int x, int d) { return x - d >= 0 ? dv_sgm_popcount(left_code ^ right_code) : DV_SGM_OOB_COST; }

// a term that is left out of the minimum (d - 1 < 0, d + 1 >= n_disp): above every L_r + p1, small enough to add p1 to
constexpr int DV_SGM_NO_TERM = 0x3fff;

// one step of a path: L_r(p, d) from C(p, d), the predecessor's L_r at d, d - 1, d + 1 (DV_SGM_NO_TERM where left out) and its minimum m over all d
DV_SGM_HD static inline int dv_sgm_path_step(int cost, int prev, int prev_lo, int prev_hi, int m, int p1, int p2) {
    int v = prev;
    if (prev_lo + p1 < v) v = prev_lo + p1;
    if (prev_hi + p1 < v) v = prev_hi + p1;
    if (m + p2 < v) v = m + p2;
    return cost + v - m;
}

// OpenCV's integer uniqueness rule for ONE other disparity d with |d - d*| > 1: true = that d makes the winner ambiguous.  s_other (100 - uniqueness) is monotone in
// s_other, so the kernel tests the smallest such S alone
DV_SGM_HD static inline bool dv_sgm_not_unique(int s_other, int s_best, int uniqueness) { return s_other * (100 - uniqueness) < s_best * 100; }

// floor(a / b) for b > 0: C++ division truncates towards zero, which is one too high for a negative a that b does not divide
DV_SGM_HD static inline int dv_sgm_floor_div(int a, int b) { const int q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }

// the disparity in sixteenths from the winner d and its neighbours' sums (sm, sp are not read at d = 0 and d = n_disp - 1)
DV_SGM_HD static inline int dv_sgm_subpixel(int d, int n_disp, int sm, int s0, int sp) {
    if (d <= 0 || d >= n_disp - 1) return 16 * d;
    int den = sm + sp - 2 * s0;
    if (den < 1) den = 1;
    return 16 * d + dv_sgm_floor_div(16 * (sm - sp) + den, 2 * den);
}

// the reason a w x h pair with `stride` bytes per row is refused for these parameters, or nullptr
static inline const char* dv_sgm_check_host(int w, int h, int stride, const dv_sgm_params* p) {
    if (!p) return "null parameters";
    if (w <= 0 || h <= 0) return "image sizes must be positive";
    if (w > DV_SGM_MAX_SIDE || h > DV_SGM_MAX_SIDE) return "image sides up to 16384";
    if (p->n_disp != 64 && p->n_disp != 128 && p->n_disp != 256) return "n_disp must be 64, 128 or 256";
    if (p->p1 < 0) return "p1 must not be negative";
    if (p->p2 < p->p1) return "p2 must not be below p1";
    if (p->p2 > 255) return "p2 above 255";
    if (p->uniqueness < 0 || p->uniqueness >= 100) return "uniqueness must lie in [0, 100)";
    for (int i = 0; i < 3; ++i) if (p->reserved[i] != 0) return "reserved words must be zero";
    if (stride < w) return "row stride below width";
    return nullptr;
}
