// The detector head's host rules (csrc/solo_head_host.h) as a stand-alone program for the sanitizers: Pipeline::GetXYWHS, the cell tables, the pixel floor of a
// concatenated cell and every refusal.  Prints "solo_head_host ok"; any failed check aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "solo_head_host.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::abort(); } } while (0)

int main() {
    int x, y, w, h;
    // the reference's KITTI shapes: model 1152 x 384, image 1242 x 375 -> r_h > r_w, h = int(0.9275 * 375) = 347 -> 348
    CHECK(dv_solo_rect_host(1152, 384, 1242, 375, &x, &y, &w, &h) == 0 && x == 0 && y == 18 && w == 1152 && h == 348);
    CHECK(dv_solo_rect_host(288, 90, 70, 23, &x, &y, &w, &h) == 0 && x == 7 && y == 0 && w == 274 && h == 90);          // the other branch, w 273 -> 274
    CHECK(dv_solo_rect_host(288, 96, 64, 4, &x, &y, &w, &h) == 0 && x == 0 && y == 39 && w == 288 && h == 18);           // no bump: 18 is even
    CHECK(dv_solo_rect_host(0, 96, 64, 4, &x, &y, &w, &h) < 0 && dv_solo_rect_host(288, 96, 64, 4, nullptr, &y, &w, &h) < 0);

    std::vector<float> buf(64, 0.0f);
    dv_solo_outputs o{}; dv_solo_params p{};
    o.n_levels = 5; o.channels = 12; o.n_classes = 3; o.mem = DV_MEM_HOST; o.fh = 7; o.fw = 13; o.feature = buf.data();
    const int grids[5] = { 5, 4, 3, 2, 2 }, num_grids[5] = { 2, 2, 3, 4, 5 };
    const float strides[5] = { 4, 8, 16, 32, 32 };
    for (int l = 0; l < 5; ++l) { o.kernel[l] = o.cate[l] = buf.data(); o.grid[l] = grids[l]; p.num_grids[l] = num_grids[l]; p.strides[l] = strides[l]; }
    p.score_thr = 0.1f; p.mask_thr = 0.5f; p.update_thr = 0.05f; p.nms_sigma = 2.0f; p.nms_pre = 48; p.max_per_img = 8; p.nms_kernel = DV_SOLO_NMS_GAUSSIAN; p.max_candidates = 72;
    p.rect_x = 0; p.rect_y = 1; p.rect_w = 52; p.rect_h = 26; p.origin_w = 70; p.origin_h = 23;
    CHECK(dv_solo_check_host(&o, &p) == nullptr);

    DvSoloTables t;
    dv_solo_tables(&o, &p, &t);
    const int cell_off[6] = { 0, 25, 41, 50, 54, 58 }, floor_end[5] = { 4, 8, 17, 33, 58 };
    for (int l = 0; l <= 5; ++l) CHECK(t.cell_off[l] == cell_off[l]);
    for (int l = 0; l < 5; ++l) CHECK(t.floor_end[l] == floor_end[l]);
    // the boundaries fall INSIDE level 0 (25 cells): cells 0..3 -> 4, 4..7 -> 8, 8..16 -> 16, 17..32 -> 32 (level 1 starts at 25), ..., none beyond 58
    CHECK(dv_solo_floor_of(0, 5, t.floor_end, p.strides) == 4 && dv_solo_floor_of(3, 5, t.floor_end, p.strides) == 4 && dv_solo_floor_of(4, 5, t.floor_end, p.strides) == 8);
    CHECK(dv_solo_floor_of(16, 5, t.floor_end, p.strides) == 16 && dv_solo_floor_of(24, 5, t.floor_end, p.strides) == 32 && dv_solo_floor_of(57, 5, t.floor_end, p.strides) == 32);
    CHECK(dv_solo_floor_of(58, 5, t.floor_end, p.strides) == 1);          // past the last boundary: torch::ones
    o.n_levels = 2; dv_solo_tables(&o, &p, &t);
    CHECK(t.cell_off[2] == 41 && t.cell_off[5] == 41 && t.floor_end[1] == 8 && dv_solo_floor_of(8, 2, t.floor_end, p.strides) == 1);
    o.n_levels = 5;
    CHECK(dv_solo_scale(24, 96) == 23.0f / 95 && dv_solo_scale(5, 1) == 0.0f);

    // every refusal
    auto refused = [&](auto change) { dv_solo_outputs a = o; dv_solo_params b = p; change(a, b); return dv_solo_check_host(&a, &b) != nullptr; };
    CHECK(dv_solo_check_host(nullptr, &p) && dv_solo_check_host(&o, nullptr));
    CHECK(refused([](auto& a, auto&) { a.n_levels = 0; }) && refused([](auto& a, auto&) { a.n_levels = 6; }));
    CHECK(refused([](auto& a, auto&) { a.channels = 0; }) && refused([](auto& a, auto&) { a.channels = 257; }));
    CHECK(refused([](auto& a, auto&) { a.n_classes = 0; }) && refused([](auto& a, auto&) { a.n_classes = 129; }));
    CHECK(refused([](auto& a, auto&) { a.mem = 3; }) && refused([](auto& a, auto&) { a.grid[2] = 0; }) && refused([](auto& a, auto&) { a.grid[4] = 65; }));
    CHECK(refused([](auto& a, auto&) { a.kernel[1] = nullptr; }) && refused([](auto& a, auto&) { a.cate[3] = nullptr; }) && refused([](auto& a, auto&) { a.feature = nullptr; }));
    CHECK(refused([](auto& a, auto&) { a.feature = (const float*)((const char*)a.feature + 2); }));
    CHECK(refused([](auto& a, auto&) { a.fh = 0; }) && refused([](auto& a, auto&) { a.fh = 2048; a.fw = 1024; }));
    CHECK(refused([](auto&, auto& b) { b.num_grids[0] = 0; }) && refused([](auto&, auto& b) { b.strides[1] = -1.0f; }) && refused([](auto&, auto& b) { b.strides[1] = NAN; }));
    CHECK(refused([](auto&, auto& b) { b.mask_thr = NAN; }) && refused([](auto&, auto& b) { b.nms_kernel = 2; }) && refused([](auto&, auto& b) { b.nms_sigma = 0.0f; }));
    CHECK(refused([](auto&, auto& b) { b.max_candidates = 0; }) && refused([](auto&, auto& b) { b.max_candidates = 4097; }));
    CHECK(refused([](auto&, auto& b) { b.nms_pre = 0; }) && refused([](auto&, auto& b) { b.nms_pre = 513; }));
    CHECK(refused([](auto&, auto& b) { b.max_per_img = 0; }) && refused([](auto&, auto& b) { b.max_per_img = 129; }));
    CHECK(refused([](auto&, auto& b) { b.origin_w = 0; }) && refused([](auto&, auto& b) { b.origin_h = 20000; }));
    CHECK(refused([](auto&, auto& b) { b.rect_w = 53; }) && refused([](auto&, auto& b) { b.rect_y = 3; }) && refused([](auto&, auto& b) { b.rect_x = -1; }) && refused([](auto&, auto& b) { b.rect_h = 0; }));
    CHECK(!refused([](auto&, auto& b) { b.nms_kernel = DV_SOLO_NMS_LINEAR; b.nms_sigma = 0.0f; }));          // sigma is the gaussian kernel's
    std::puts("solo_head_host ok");
    return 0;
}
