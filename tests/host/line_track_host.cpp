// Stand-alone check of dynamic_vins_amd/csrc/line_track_host.h (the line tracker's host half) under the sanitizers: tests/test_line_track_ref.py compiles and runs it.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../../dynamic_vins_amd/csrc/line_track_host.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void flip(uint8_t* row, int bit) { row[bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
static const uint32_t* W(const std::vector<uint8_t>& v, int row = 0) { return (const uint32_t*)(v.data() + 32 * row); }

int main() {
    std::vector<dv_key_line> L(DV_LINE_MAX + 1);
    std::vector<uint8_t> D((DV_LINE_MAX + 1) * 32, 0);
    EXPECT(!dv_line_frame_check_host(L.data(), D.data(), DV_LINE_MAX, L.data(), D.data(), DV_LINE_MAX, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(L.data(), D.data(), DV_LINE_MAX + 1, nullptr, nullptr, 0, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(L.data(), D.data(), 1, L.data(), D.data(), DV_LINE_MAX + 1, DV_MEM_PINNED));
    EXPECT(!dv_line_frame_check_host(nullptr, nullptr, 0, nullptr, nullptr, 0, DV_MEM_DEVICE));
    EXPECT(!dv_line_frame_check_host(L.data(), D.data(), 2, L.data(), D.data(), 0, DV_MEM_DEVICE));
    EXPECT(dv_line_frame_check_host(L.data(), D.data(), -1, nullptr, nullptr, 0, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(nullptr, D.data(), 1, nullptr, nullptr, 0, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(L.data(), nullptr, 1, nullptr, nullptr, 0, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(L.data(), D.data(), 1, nullptr, nullptr, 1, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(L.data(), D.data(), 1, L.data(), nullptr, 1, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(L.data(), D.data(), 1, nullptr, nullptr, 0, 7));
    EXPECT(dv_line_frame_check_host((const dv_key_line*)((const char*)L.data() + 2), D.data(), 1, nullptr, nullptr, 0, DV_MEM_HOST));
    EXPECT(dv_line_frame_check_host(L.data(), D.data() + 1, 1, nullptr, nullptr, 0, DV_MEM_HOST));

    std::vector<int32_t> idx(DV_LINE_MAX), dist(DV_LINE_MAX);
    EXPECT(!dv_line_match_check_host(D.data(), DV_LINE_MAX, D.data(), DV_LINE_MAX, idx.data(), dist.data()));
    EXPECT(!dv_line_match_check_host(nullptr, 0, nullptr, 0, nullptr, nullptr));
    EXPECT(!dv_line_match_check_host(D.data(), 4, nullptr, 0, idx.data(), dist.data()));
    EXPECT(dv_line_match_check_host(D.data(), DV_LINE_MAX + 1, D.data(), 1, idx.data(), dist.data()));
    EXPECT(dv_line_match_check_host(D.data(), 1, D.data(), DV_LINE_MAX + 1, idx.data(), dist.data()));
    EXPECT(dv_line_match_check_host(D.data(), 1, nullptr, 1, idx.data(), dist.data()));
    EXPECT(dv_line_match_check_host(D.data(), 1, D.data(), 1, nullptr, dist.data()));
    EXPECT(dv_line_match_check_host(D.data(), -1, D.data(), 1, idx.data(), dist.data()));
    int nr = 0;
    dv_line_row row;
    EXPECT(!dv_line_collect_check_host(&row, 1, &nr) && !dv_line_collect_check_host(nullptr, 0, &nr));
    EXPECT(dv_line_collect_check_host(&row, 1, nullptr) && dv_line_collect_check_host(nullptr, 1, &nr) && dv_line_collect_check_host(&row, -1, &nr));

    // the arrays of both blocks neither overlap nor leave the allocation
    {
        const DvLineLayout T = dv_line_layout();
        const size_t m = DV_LINE_MAX;
        EXPECT(T.hdr == 0 && T.line >= DV_LT_H_WORDS * 4 && T.id >= T.line + m * sizeof(dv_key_line) && T.cnt >= T.id + m * 4 && T.desc >= T.cnt + m * 4 && T.bytes >= T.desc + m * 32);
        EXPECT(T.line % 256 == 0 && T.id % 256 == 0 && T.cnt % 256 == 0 && T.desc % 256 == 0);
        const DvLineOut O = dv_line_out_layout();
        EXPECT(O.left_ids == DV_LT_O_WORDS * 4 && O.left_src == O.left_ids + m * 4 && O.left_cnt == O.left_src + m * 4 && O.right_ids == O.left_cnt + m * 4 && O.right_src == O.right_ids + m * 4);
        EXPECT(O.rows >= O.right_src + m * 4 && O.rows % 8 == 0 && O.bytes == O.rows + m * sizeof(dv_line_row));
        EXPECT(sizeof(dv_line_row) == 72 && sizeof(dv_key_line) == 24);
    }

    // distance, first equal byte and the nearest row: (distance, first equal byte, index)
    {
        std::vector<uint8_t> q(32), t(32 * 6);
        for (int i = 0; i < 32; ++i) q[i] = (uint8_t)(37 * i + 11);
        for (int r = 0; r < 6; ++r) std::memcpy(t.data() + 32 * r, q.data(), 32);
        EXPECT(dv_lt_distance(W(q), W(t)) == 0 && dv_lt_first_equal_byte(W(q), W(t)) == 0);
        std::vector<uint8_t> a = q;
        for (int i = 0; i < 32; ++i) { flip(a.data(), 8 * i + (i % 8)); EXPECT(dv_lt_distance(W(q), W(a)) == i + 1 && dv_lt_first_equal_byte(W(q), W(a)) == i + 1); }
        a = q; a[1] ^= 0x80; EXPECT(dv_lt_first_equal_byte(W(q), W(a)) == 0);
        a = q; a[0] ^= 0x01; a[1] ^= 0xFF; EXPECT(dv_lt_first_equal_byte(W(q), W(a)) == 2 && dv_lt_distance(W(q), W(a)) == 9);
        a = q; a[0] ^= 0x80; a[1] ^= 0x01; a[2] ^= 0x80; a[3] ^= 0x01; EXPECT(dv_lt_first_equal_byte(W(q), W(a)) == 4);      // the borrow of a low byte never flags early
        // rows: 0 far | 1 three flips, first equal byte 3 | 2 three flips, first equal byte 0 | 3 the same key as 2 | 4 four flips | 5 far
        for (int b = 0; b < 200; b += 3) { flip(t.data(), b); flip(t.data() + 32 * 5, b + 1); }
        flip(t.data() + 32, 1); flip(t.data() + 32, 9); flip(t.data() + 32, 17);
        flip(t.data() + 64, 41); flip(t.data() + 64, 49); flip(t.data() + 64, 57);
        flip(t.data() + 96, 80); flip(t.data() + 96, 90); flip(t.data() + 96, 100);
        flip(t.data() + 128, 0); flip(t.data() + 128, 2); flip(t.data() + 128, 4); flip(t.data() + 128, 6);
        int d = -1;
        EXPECT(dv_lt_nearest(W(q), W(t), 6, &d) == 2 && d == 3);
        EXPECT(dv_lt_nearest(W(q), W(t), 2, &d) == 1 && d == 3);
        EXPECT(dv_lt_nearest(W(q), W(t), 1, &d) == -1 && d == 0);
        EXPECT(dv_lt_nearest(W(q), W(t), 0, &d) == -1 && d == 0);
        // exactly 29 is a match, exactly 30 is none
        std::vector<uint8_t> e = q;
        for (int i = 0; i < 29; ++i) flip(e.data(), 8 * i);
        EXPECT(dv_lt_nearest(W(q), W(e), 1, &d) == 0 && d == 29);
        flip(e.data(), 8 * 29);
        EXPECT(dv_lt_nearest(W(q), W(e), 1, &d) == -1 && d == 0);
    }

    // the gate: both errors against the train line's END point; float abs; NaN fails
    {
        dv_key_line t{100.0f, 100.0f, 0.0f, 0.0f, 0.5f, 141.0f}, q{150.0f, 100.0f, 10.0f, 10.0f, 0.55f, 160.0f};
        EXPECT(dv_lt_gate(q, t));
        q.sx = 200.0f; q.sy = 0.0f; EXPECT(!dv_lt_gate(q, t));      // 40000 is not < 40000
        q.sx = 199.99f; EXPECT(dv_lt_gate(q, t));
        q.angle = 0.5f + 0.5f; EXPECT(!dv_lt_gate(q, t));           // |0.5| < 1: an int abs() would pass it
        q.angle = 0.5f - 0.11f; EXPECT(!dv_lt_gate(q, t));
        q.angle = std::numeric_limits<float>::quiet_NaN(); EXPECT(!dv_lt_gate(q, t));
        q.angle = 0.5f; q.ex = 300.0f; EXPECT(!dv_lt_gate(q, t));
        dv_key_line far = t; far.sx = 1000.0f; far.sy = 1000.0f; q.ex = 10.0f; EXPECT(dv_lt_gate(q, far));      // the train line's START is never read
    }
    // h / v with the double literals, the quota
    EXPECT(!dv_lt_is_h(0.7849f) && dv_lt_is_h(0.7852f) && dv_lt_is_h(0.7856f) && dv_lt_is_h(2.35f) && !dv_lt_is_h(2.36f));
    EXPECT(!dv_lt_is_h(-0.7849f) && dv_lt_is_h(-0.7852f) && dv_lt_is_h(-2.35f) && !dv_lt_is_h(-2.36f) && !dv_lt_is_h(0.0f) && !dv_lt_is_h(std::numeric_limits<float>::quiet_NaN()));
    EXPECT(dv_lt_take(0, 40) == 35 && dv_lt_take(0, 3) == 3 && dv_lt_take(30, 40) == 5 && dv_lt_take(35, 40) == 0 && dv_lt_take(50, 40) == 0 && dv_lt_take(34, 0) == 0);

    if (fails) { std::printf("line_track_host: %d failures\n", fails); return 1; }
    std::printf("line_track_host: ok\n");
    return 0;
}
