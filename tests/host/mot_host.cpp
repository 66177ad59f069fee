// Stand-alone check of dynamic_vins_amd/csrc/mot_host.h (the tracker's host half) under the sanitizers: tests/test_mot_host.py compiles and runs it.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../../dynamic_vins_amd/csrc/mot_host.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    dv_mot_params p{3, 5, 100, 512, 128, {0, 0, 0}};
    EXPECT(dv_mot_check_host(&p) == nullptr);
    EXPECT(dv_mot_check_host(nullptr) != nullptr);
    { dv_mot_params q = p; q.budget = 0; EXPECT(dv_mot_check_host(&q)); q.budget = 101; EXPECT(dv_mot_check_host(&q)); q.budget = 1; EXPECT(!dv_mot_check_host(&q)); }
    { dv_mot_params q = p; q.feat_dim = 0; EXPECT(dv_mot_check_host(&q)); q.feat_dim = 513; EXPECT(dv_mot_check_host(&q)); q.feat_dim = 1; EXPECT(!dv_mot_check_host(&q)); }
    { dv_mot_params q = p; q.max_tracks = 0; EXPECT(dv_mot_check_host(&q)); q.max_tracks = 129; EXPECT(dv_mot_check_host(&q)); }
    { dv_mot_params q = p; q.n_init = -1; EXPECT(dv_mot_check_host(&q)); q.n_init = 0; q.max_age = -1; EXPECT(dv_mot_check_host(&q)); }

    std::vector<float> r(64 * 4, 1.0f), f(64 * 512, 0.0f);
    EXPECT(!dv_mot_frame_check_host(r.data(), f.data(), 64, DV_MEM_HOST));
    EXPECT(dv_mot_frame_check_host(r.data(), f.data(), 65, DV_MEM_HOST));
    EXPECT(dv_mot_frame_check_host(r.data(), f.data(), -1, DV_MEM_HOST));
    EXPECT(!dv_mot_frame_check_host(nullptr, nullptr, 0, DV_MEM_DEVICE));
    EXPECT(dv_mot_frame_check_host(nullptr, f.data(), 1, DV_MEM_HOST));
    EXPECT(dv_mot_frame_check_host(r.data(), f.data(), 1, 7));
    EXPECT(dv_mot_frame_check_host((const float*)((const char*)r.data() + 1), f.data(), 1, DV_MEM_HOST));

    std::vector<float> c(128 * 64, 0.5f);
    std::vector<int32_t> a(128);
    EXPECT(!dv_mot_assign_check_host(c.data(), 128, 64, a.data()));
    EXPECT(dv_mot_assign_check_host(c.data(), 129, 64, a.data()));
    EXPECT(dv_mot_assign_check_host(c.data(), 128, 65, a.data()));
    EXPECT(!dv_mot_assign_check_host(nullptr, 4, 0, a.data()));
    c[128 * 64 - 1] = std::numeric_limits<float>::quiet_NaN(); EXPECT(dv_mot_assign_check_host(c.data(), 128, 64, a.data()));
    c[128 * 64 - 1] = -1.0f; EXPECT(dv_mot_assign_check_host(c.data(), 128, 64, a.data()));
    c[128 * 64 - 1] = std::numeric_limits<float>::infinity(); EXPECT(dv_mot_assign_check_host(c.data(), 128, 64, a.data()));

    // the table's arrays neither overlap nor leave the allocation
    for (int m : {1, 5, 128}) {
        const DvMotLayout L = dv_mot_layout(m);
        const size_t off[] = {L.hdr, L.x, L.P, L.state, L.id, L.hits, L.tsu, L.slot, L.next, L.full, L.slot_rows, L.bytes};
        const size_t need[] = {DV_MOT_H_WORDS * 4, (size_t)m * 28, (size_t)m * 196, (size_t)m * 4, (size_t)m * 4, (size_t)m * 4, (size_t)m * 4, (size_t)m * 4, (size_t)m * 4, (size_t)m * 4, (size_t)m * 4};
        for (int i = 0; i < 11; ++i) EXPECT(off[i] % 256 == 0 && off[i] + need[i] <= off[i + 1]);
        std::vector<unsigned char> buf(L.bytes);
        std::memset(buf.data() + L.slot_rows, 0, (size_t)m * 4);
    }

    // rect() and its NaN way in; the measurement is its inverse
    float x[7] = {50, 40, 2400, 1.5f, 0, 0, 0}, rc[4], z[4];
    dv_mot_rect_of(x, rc);
    EXPECT(rc[2] == 60.0f && rc[3] == 40.0f && rc[0] == 20.0f && rc[1] == 20.0f && !dv_mot_rect_nan(rc));
    dv_mot_measure(rc, z);
    EXPECT(z[0] == 50.0f && z[1] == 40.0f && z[2] == 2400.0f && z[3] == 1.5f);
    x[2] = -1.0f; dv_mot_rect_of(x, rc); EXPECT(dv_mot_rect_nan(rc));
    x[2] = 0.0f; dv_mot_rect_of(x, rc); EXPECT(dv_mot_rect_nan(rc));      // 0 / 0

    // 1 - IoU: identical, disjoint, touching (empty overlap), degenerate union
    const float A[4] = {0, 0, 10, 10}, B[4] = {5, 0, 10, 10}, Cc[4] = {10, 0, 10, 10}, Z[4] = {3, 3, 0, 0};
    EXPECT(dv_mot_iou_dist(A, A) == 0.0f);
    EXPECT(dv_mot_iou_dist(A, B) == 1.0f - 50.0f / 150.0f);
    EXPECT(dv_mot_iou_dist(A, Cc) == 1.0f);
    EXPECT(dv_mot_iou_dist(Z, Z) == 1.0f);

    // the gates: strict, float thresholds, NaN gated
    EXPECT(dv_mot_cost1(0.8f, 0.2f) == 0.2f && dv_mot_cost1(0.81f, 0.1f) == 1000.0f && dv_mot_cost1(0.5f, 0.21f) == 1000.0f);
    EXPECT(dv_mot_cost1(0.5f, std::numeric_limits<float>::quiet_NaN()) == 1000.0f);
    EXPECT(dv_mot_cost2(0.7f) == 0.7f && dv_mot_cost2(0.71f) == 1000.0f);
    EXPECT(dv_mot_cost2(std::numeric_limits<float>::quiet_NaN()) == 1000.0f && dv_mot_cost1(std::numeric_limits<float>::quiet_NaN(), 0.1f) == 1000.0f);

    // FeatureBundle::add over a ring of 3: rows 0 1 2 0 1, full from the fourth
    int next = 0, full = 0, rows[5], cnt[5];
    for (int k = 0; k < 5; ++k) { rows[k] = dv_mot_ring_add(&next, &full, 3); cnt[k] = dv_mot_ring_rows(next, full, 3); }
    EXPECT(rows[0] == 0 && rows[1] == 1 && rows[2] == 2 && rows[3] == 0 && rows[4] == 1);
    EXPECT(cnt[0] == 1 && cnt[1] == 2 && cnt[2] == 3 && cnt[3] == 3 && cnt[4] == 3 && full == 1 && next == 2);
    next = 0; full = 0;
    for (int k = 0; k < 3; ++k) EXPECT(dv_mot_ring_add(&next, &full, 1) == 0 && dv_mot_ring_rows(next, full, 1) == 1);

    // miss
    EXPECT(dv_mot_miss(DV_MOT_TENTATIVE, 1, 5) == DV_MOT_DELETED);
    EXPECT(dv_mot_miss(DV_MOT_CONFIRMED, 5, 5) == DV_MOT_CONFIRMED && dv_mot_miss(DV_MOT_CONFIRMED, 6, 5) == DV_MOT_DELETED);

    std::printf(fails ? "mot_host: %d FAILED\n" : "mot_host: ok\n", fails);
    return fails ? 1 : 0;
}
