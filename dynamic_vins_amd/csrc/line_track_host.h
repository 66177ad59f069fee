// line_track_host.h — the half of the line tracker (line_track.hip) that is plain C++: the refusals of a frame and of a descriptor match, the layout of the resident
// previous frame and of the frame's device -> host block, and the small rules the kernel and the host share in ONE copy — the 256-bit distance with the Mihasher's
// first-equal-byte key (thirdparty/line_descriptor/src/binary_descriptor_matcher.cpp:635-753, bitops_custom.hpp:83-123), TrackLine's gate
// (line_detector/line_detector.cpp:116-124), its h / v split (:165-166) and its quota (:190-213).
// No HIP in here: dv_line_track_* / dv_line_match use it, and tests/host/line_track_host.cpp compiles it under the sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "dv_mem.h"

#ifdef __HIPCC__
#define DV_LT_HD __host__ __device__
#else
#define DV_LT_HD
#endif

constexpr int DV_LT_MATCH_DIST = 30;            // lsd_matches[i].distance < 30 (line_detector.cpp:116,258)
constexpr int DV_LT_QUOTA = 35;                 // 35 - h_line, 35 - v_line (line_detector.cpp:190-191)
constexpr int DV_LT_DESC_WORDS = DV_LINE_DESC_BYTES / 4;
constexpr uint32_t DV_LT_NO_ID = 0xFFFFFFFFu;   // line_ids.push_back(-1) into a vector<unsigned int> (line_detector.cpp:237,248)

// the reason one image's lines are refused, or nullptr (n = 0 is an ordinary frame: the pointers are not looked at)
static inline const char* dv_line_side_check_host(const dv_key_line* lines, const uint8_t* desc, int n) {
    if (n < 0) return "negative line count";
    if (n > DV_LINE_MAX) return "more than DV_LINE_MAX (512) lines in one image";
    if (n == 0) return nullptr;
    if (!lines || !desc) return "null key lines or descriptors";
    if (((uintptr_t)lines | (uintptr_t)desc) & 3) return "key lines and descriptors must be 4-byte aligned";
    return nullptr;
}
// the reason a frame is refused, or nullptr
static inline const char* dv_line_frame_check_host(const dv_key_line* left, const uint8_t* left_desc, int n_left, const dv_key_line* right, const uint8_t* right_desc, int n_right, int mem) {
    if (!dv_mem_known(mem)) return "unknown memory kind";
    if (const char* why = dv_line_side_check_host(left, left_desc, n_left)) return why;
    if (!right && !right_desc && n_right == 0) return nullptr;      // no right image
    return dv_line_side_check_host(right, right_desc, n_right);
}
// the reason dv_line_match refuses its arguments, or nullptr (host memory both)
static inline const char* dv_line_match_check_host(const uint8_t* query, int nq, const uint8_t* train, int nt, const int32_t* train_idx, const int32_t* distance) {
    if (nq < 0 || nt < 0) return "negative row count";
    if (nq > DV_LINE_MAX || nt > DV_LINE_MAX) return "more than DV_LINE_MAX (512) rows";
    if (nq > 0 && (!query || !train_idx || !distance)) return "null query or result";
    if (nt > 0 && !train) return "null train descriptors";
    return nullptr;
}
// the reason dv_line_track_collect refuses its arguments, or nullptr
static inline const char* dv_line_collect_check_host(const dv_line_row* rows, int cap, const int* n_rows) {
    if (!n_rows) return "null n_rows";
    if (cap < 0 || (cap > 0 && !rows)) return "bad row buffer";
    return nullptr;
}

// The resident previous left frame: a header, then one array per field over DV_LINE_MAX lines.  Byte offsets, every array 256-byte aligned.
enum { DV_LT_H_HAVE_PREV = 0, DV_LT_H_NPREV = 1, DV_LT_H_NEXT_ID = 2, DV_LT_H_WORDS = 16 };
struct DvLineLayout { size_t hdr, line, id, cnt, desc, bytes; };
static inline DvLineLayout dv_line_layout() {
    DvLineLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t m = DV_LINE_MAX;
    L.hdr = take(DV_LT_H_WORDS * 4); L.line = take(m * sizeof(dv_key_line)); L.id = take(m * 4); L.cnt = take(m * 4); L.desc = take(m * DV_LINE_DESC_BYTES);
    L.bytes = off;
    return L;
}
// The frame's device -> host block: counters, five arrays of DV_LINE_MAX words, then the rows
enum { DV_LT_O_NROWS = 0, DV_LT_O_NLEFT = 1, DV_LT_O_NRIGHT = 2, DV_LT_O_NEXT_ID = 3, DV_LT_O_WORDS = 16 };
struct DvLineOut { size_t left_ids, left_src, left_cnt, right_ids, right_src, rows, bytes; };
DV_LT_HD static inline DvLineOut dv_line_out_layout() {
    DvLineOut O{};
    const size_t m = (size_t)DV_LINE_MAX * 4;
    O.left_ids = DV_LT_O_WORDS * 4; O.left_src = O.left_ids + m; O.left_cnt = O.left_src + m; O.right_ids = O.left_cnt + m; O.right_src = O.right_ids + m;
    O.rows = (O.right_src + m + 255) / 256 * 256;
    O.bytes = O.rows + (size_t)DV_LINE_MAX * sizeof(dv_line_row);
    return O;
}

DV_LT_HD static inline int dv_lt_popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}
DV_LT_HD static inline int dv_lt_ctz(uint32_t x) {      // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)x) - 1;
#else
    return __builtin_ctz(x);
#endif
}
// the Hamming distance of two 32-byte rows given as 8 words read in memory order (cv::line_descriptor::match, bitops_custom.hpp:83-96)
DV_LT_HD static inline int dv_lt_distance(const uint32_t* q, const uint32_t* t) {
    int d = 0;
    for (int w = 0; w < DV_LT_DESC_WORDS; ++w) d += dv_lt_popc(q[w] ^ t[w]);
    return d;
}
// the index of the first byte, in memory order, at which the two rows are equal; 32 when there is none.  This is the substring table k in which Mihasher::query meets
// the train row at search radius s = 0: m = 32 makes every substring one byte, in byte order (split, bitops_custom.hpp:99-123).  Little-endian words.
// (x - 0x01010101) & ~x & 0x80808080 has its LOWEST set bit in the lowest zero byte of x; only the bytes above a zero byte can be flagged wrongly.
DV_LT_HD static inline int dv_lt_first_equal_byte(const uint32_t* q, const uint32_t* t) {
    for (int w = 0; w < DV_LT_DESC_WORDS; ++w) {
        const uint32_t x = q[w] ^ t[w];
        const uint32_t z = (x - 0x01010101u) & ~x & 0x80808080u;
        if (z) return 4 * w + (dv_lt_ctz(z) >> 3);
    }
    return DV_LINE_DESC_BYTES;
}
// the nearest train row below distance 30 as BinaryDescriptorMatcher::match returns it: least by (distance, first equal byte, train index).  train: nt rows of 8 words.
// *dist = 0 and -1 when no row is nearer than 30.
DV_LT_HD static inline int dv_lt_nearest(const uint32_t* q, const uint32_t* train, int nt, int* dist) {
    int bd = DV_LT_MATCH_DIST, bk = DV_LINE_DESC_BYTES + 1, bj = -1;
    for (int j = 0; j < nt; ++j) {
        const uint32_t* t = train + (size_t)j * DV_LT_DESC_WORDS;
        const int d = dv_lt_distance(q, t);
        if (d > bd || d >= DV_LT_MATCH_DIST) continue;
        const int k = dv_lt_first_equal_byte(q, t);
        if (d < bd || k < bk) { bd = d; bk = k; bj = j; }      // j ascends: an equal (distance, key) keeps the earlier row
    }
    *dist = bj < 0 ? 0 : bd;
    return bj;
}

// float32 products and one float32 add, never contracted (cv::Point2f::dot of a cv::Point2f difference)
DV_LT_HD static inline float dv_lt_dot2(float x, float y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y));
#else
    volatile float a = x * x, b = y * y;      // volatile: no contraction on the host either
    return a + b;
#endif
}
DV_LT_HD static inline float dv_lt_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
// TrackLine's gate behind distance < 30 (line_detector.cpp:118-123; TrackRightLine :260-265): q is the query line, t the train line.  BOTH errors are measured against the
// train line's END point, as written there.  abs() is taken as the float overload (declared choice).
DV_LT_HD static inline bool dv_lt_gate(const dv_key_line& q, const dv_key_line& t) {
    const float s = dv_lt_dot2(dv_lt_sub(q.sx, t.ex), dv_lt_sub(q.sy, t.ey));
    const float e = dv_lt_dot2(dv_lt_sub(q.ex, t.ex), dv_lt_sub(q.ey, t.ey));
    const float da = fabsf(dv_lt_sub(q.angle, t.angle));
    return s < 40000.0f && e < 40000.0f && (double)da < 0.1;
}
// "h" of the h / v split: the float angle against the DOUBLE literals 3.14 / 4 and 3 * 3.14 / 4 (line_detector.cpp:165-166,181-182)
DV_LT_HD static inline bool dv_lt_is_h(float angle) {
    const double a = (double)angle;
    return (a >= 3.14 / 4 && a <= 3 * 3.14 / 4) || (a <= -3.14 / 4 && a >= -3 * 3.14 / 4);
}
// how many of n_new new lines of a class the top-up takes when n_tracked of the class were tracked (line_detector.cpp:190-213)
DV_LT_HD static inline int dv_lt_take(int n_tracked, int n_new) {
    const int diff = DV_LT_QUOTA - n_tracked;
    if (diff <= 0) return 0;
    return diff > n_new ? n_new : diff;
}
