// inst_stack_host.cpp — stand-alone check of the mask-stack path's host code (csrc/inst_stack_host.h): the membership rule, BuildBoxes2D's detection list from per-plane
// boxes, the descriptor and rectangle / plane checks every *_planes entry runs before it stages anything.  No GPU, no library: tests/test_inst_stack_host.py builds it
// under AddressSanitizer + UBSan and under ThreadSanitizer (the rule runs from several threads on separate outputs, as one context per thread would) and runs it.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include "inst_stack_host.h"

static std::atomic<int> failures{ 0 };
#define EXPECT(cond) do { if (!(cond)) { std::printf("BROKEN %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static void rule() {
    // bytes: everything but 0 and 128 (to(kInt8).abs().clamp(0, 1): abs(-128) wraps)
    int members = 0;
    for (int b = 0; b < 256; ++b) members += dv_stack_u8_has((uint8_t)b);
    EXPECT(members == 254 && !dv_stack_u8_has(0) && !dv_stack_u8_has(128) && dv_stack_u8_has(1) && dv_stack_u8_has(127) && dv_stack_u8_has(129) && dv_stack_u8_has(255));
    const float nan = std::nanf("");
    EXPECT(dv_stack_f32_has(0.50001f, 0.5f) && !dv_stack_f32_has(0.5f, 0.5f) && !dv_stack_f32_has(nan, 0.5f) && !dv_stack_f32_has(0.5f, nan));
}

static void detections() {
    // plane 0 touches the whole 640 x 360 image, 1 is empty, 2 a single pixel, 3 one pixel under the floor on one side, 4 exactly at the floor, 63 the last plane
    std::vector<int32_t> boxes(4 * 64);
    for (int p = 0; p < 64; ++p) { boxes[4 * p] = 0x7fffffff; boxes[4 * p + 1] = -1; boxes[4 * p + 2] = 0x7fffffff; boxes[4 * p + 3] = -1; }
    auto set = [&](int p, int r0, int r1, int c0, int c1) { boxes[4 * p] = r0; boxes[4 * p + 1] = r1; boxes[4 * p + 2] = c0; boxes[4 * p + 3] = c1; };
    set(0, 0, 359, 0, 639); set(2, 17, 17, 90, 90); set(3, 10, 17, 10, 18); set(4, 10, 18, 10, 18); set(63, 100, 130, 600, 639);
    dv_inst_det d[64]; int32_t pl[64];
    int n = dv_stack_build_dets(boxes.data(), 64, 8, d, pl, 64);
    EXPECT(n == 3);
    EXPECT(pl[0] == 0 && d[0].track_id == 0 && d[0].x == 0 && d[0].y == 0 && d[0].w == 639 && d[0].h == 359);          // cv::Rect(min_pt, max_pt): max row / column excluded
    EXPECT(pl[1] == 4 && d[1].track_id == 4 && d[1].x == 10 && d[1].y == 10 && d[1].w == 8 && d[1].h == 8);
    EXPECT(pl[2] == 63 && d[2].x == 600 && d[2].w == 39 && d[2].y == 100 && d[2].h == 30 && d[2].mask == nullptr && d[2].points == nullptr && d[2].class_id == 0);
    EXPECT(dv_stack_build_dets(boxes.data(), 64, 8, d, pl, 2) == -1);          // cap too small
    EXPECT(dv_stack_build_dets(boxes.data(), 65, 8, d, pl, 64) == -1);
    EXPECT(dv_stack_build_dets(boxes.data(), 64, 0, d, nullptr, 64) == 4);     // floor 1: the single pixel (0 x 0) still drops, plane 3 comes in; planes[] is optional
    EXPECT(dv_stack_build_dets(boxes.data(), 3, 1, d, pl, 1) == 1 && pl[0] == 0);
}

static void descriptors() {
    static float buf[16];
    DvStackLayout L{};
    dv_mask_stack s{}; s.data = buf; s.n_planes = 3; s.kind = DV_STACK_U8; s.mem = DV_MEM_DEVICE;
    EXPECT(dv_stack_check(&s, 67, 5, &L) == nullptr && L.es == 1 && L.row_stride == 67 && L.plane_stride == 335);
    s.row_stride = 71; s.plane_stride = 71 * 5 + 13;
    EXPECT(dv_stack_check(&s, 67, 5, &L) == nullptr && L.row_stride == 71 && L.plane_stride == 368);
    s.plane_stride = 71 * 4 + 67;          // the last row may be tight
    EXPECT(dv_stack_check(&s, 67, 5, &L) == nullptr);
    s.plane_stride = 71 * 4 + 66;
    EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr);
    s.plane_stride = 0; s.row_stride = 66;
    EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr);
    s.row_stride = 0;
    for (int bad : { 0, -1, 65 }) { s.n_planes = bad; EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr && std::strstr(dv_stack_check(&s, 67, 5, &L), "1..64 planes")); }
    s.n_planes = 64; EXPECT(dv_stack_check(&s, 67, 5, &L) == nullptr);
    s.kind = 2; EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr);
    s.kind = DV_STACK_F32; EXPECT(dv_stack_check(&s, 67, 5, &L) == nullptr && L.es == 4 && L.row_stride == 268 && L.plane_stride == 1340);
    s.row_stride = 270; EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr);          // float rows off a 4-byte boundary
    s.row_stride = 284; EXPECT(dv_stack_check(&s, 67, 5, &L) == nullptr);
    s.data = (const char*)buf + 2; EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr);
    s.data = buf; s.mem = 7; EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr);
    s.mem = DV_MEM_HOST; s.data = nullptr; EXPECT(dv_stack_check(&s, 67, 5, &L) != nullptr);
    EXPECT(dv_stack_check(nullptr, 67, 5, &L) != nullptr);
    // a plane stride beyond 2^31 is a legal layout (64 planes of a large image)
    s.data = buf; s.kind = DV_STACK_U8; s.row_stride = 0; s.plane_stride = (int64_t)3 << 30;
    EXPECT(dv_stack_check(&s, 67, 5, &L) == nullptr && L.plane_stride == ((long long)3 << 30));

    dv_inst_det d[3]{}; int32_t pl[3] = { 0, 2, 1 };
    d[0].track_id = 7; d[0].x = 0; d[0].y = 0; d[0].w = 67; d[0].h = 5;          // the whole image
    d[1].track_id = 8; d[1].x = 66; d[1].y = 4; d[1].w = 1; d[1].h = 1;          // flush with the corner
    d[2].track_id = 9; d[2].x = 10; d[2].y = 1; d[2].w = 20; d[2].h = 3;
    EXPECT(dv_stack_check_dets(d, pl, 3, 3, 67, 5, nullptr, 0) == nullptr);
    pl[1] = 3; EXPECT(std::strstr(dv_stack_check_dets(d, pl, 3, 3, 67, 5, nullptr, 0), "plane index out of range"));
    const uint32_t only[1] = { 9 };
    EXPECT(dv_stack_check_dets(d, pl, 3, 3, 67, 5, only, 1) == nullptr);          // a detection that is not in the list is not looked at
    pl[1] = -1; EXPECT(dv_stack_check_dets(d, pl, 3, 3, 67, 5, nullptr, 0) != nullptr);
    pl[1] = 2; d[2].x = 48; EXPECT(std::strstr(dv_stack_check_dets(d, pl, 3, 3, 67, 5, nullptr, 0), "detection rectangle outside the image"));
    d[2].x = 0x7ffffff0; EXPECT(dv_stack_check_dets(d, pl, 3, 3, 67, 5, nullptr, 0) != nullptr);          // no overflow in x + w
    d[2].x = 10; d[2].h = 0; EXPECT(dv_stack_check_dets(d, pl, 3, 3, 67, 5, nullptr, 0) != nullptr);
}

int main() {
    rule(); detections(); descriptors();
    std::vector<std::thread> th;
    for (int i = 0; i < 4; ++i) th.emplace_back([] { for (int r = 0; r < 50; ++r) { detections(); descriptors(); } });
    for (auto& t : th) t.join();
    if (failures.load()) { std::printf("inst_stack_host: %d check(s) BROKEN\n", failures.load()); return 1; }
    std::printf("inst_stack_host: ok\n");
    return 0;
}
