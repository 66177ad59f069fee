// The LBD stage's host rules (csrc/lbd_host.h) as a stand-alone program for the sanitizers: the weight tables, the band-pair rule, the blur weights, the pixel-count
// rule, the sample and end-point roundings, the tail of computeLBD on crafted band sums, the selection and every refusal.  Prints "lbd_host ok"; any failed check aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "lbd_host.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::abort(); } } while (0)

int main() {
    // tables: symmetric, 1 at the centre, the constructor's integer divisions (u = 10, sigma = 7; u = sigma = 31)
    DvLbdTabs t;
    dv_lbd_tables(&t);
    CHECK(t.g[31] == 1.0f && t.l[10] == 1.0f && t.g[0] == (float)std::exp(-0.5) && t.l[0] == (float)std::exp(-100.0 / 98.0));
    for (int i = 0; i < DV_LBD_ROWS; ++i) CHECK(t.g[i] == t.g[DV_LBD_ROWS - 1 - i]);
    for (int i = 0; i < 21; ++i) CHECK(t.l[i] == t.l[20 - i]);
    // pairs: 32 distinct ascending pairs, none of (0|1, 7|8)
    int seen[9][9] = {};
    for (int k = 0; k < 32; ++k) {
        int a, b;
        dv_lbd_pair(k, &a, &b);
        CHECK(a >= 0 && a < b && b < 9 && !(a <= 1 && b >= 7) && !seen[a][b]);
        seen[a][b] = 1;
    }
    int a, b;
    dv_lbd_pair(0, &a, &b); CHECK(a == 0 && b == 1);
    dv_lbd_pair(15, &a, &b); CHECK(a == 2 && b == 7);
    dv_lbd_pair(31, &a, &b); CHECK(a == 7 && b == 8);
    CHECK(dv_lbd_reflect101(-1, 5) == 1 && dv_lbd_reflect101(5, 5) == 3 && dv_lbd_reflect101(-3, 2) == 1 && dv_lbd_reflect101(7, 1) == 0);

    // the pixel count: ties to even; saturation instead of overflow
    CHECK(dv_lbd_npix(0, 0, 0, 0) == 1 && dv_lbd_npix(0.5f, 0, 1.5f, 0) == 3 && dv_lbd_npix(2.5f, 7, 3.5f, 1) == 7 && dv_lbd_npix(10.4f, 3, 2.6f, 5.5f) == 8);
    CHECK(dv_lbd_npix(-3.0e38f, 0, 3.0e38f, 0) == 1000000000);
    // (short) round(): half away from zero, 16-bit wrap, clamp
    CHECK(dv_lbd_coord(0.5f, 95) == 1 && dv_lbd_coord(-0.5f, 95) == 0 && dv_lbd_coord(2.5f, 95) == 3 && dv_lbd_coord(0.49999997f, 95) == 0 && dv_lbd_coord(95.5f, 95) == 95);
    CHECK(dv_lbd_coord(32768.0f, 95) == 0 && dv_lbd_coord(65536.0f + 7.0f, 95) == 7 && dv_lbd_coord(-65536.0f + 9.0f, 95) == 9);          // the low 16 bits
    CHECK(dv_lbd_coord(3.0e9f, 95) == 0 && dv_lbd_coord(-3.0e9f, 95) == 0 && dv_lbd_coord(std::numeric_limits<float>::infinity(), 95) == 0 && dv_lbd_coord(NAN, 95) == 0);
    // end points: ties to even, inside test before any conversion
    int x, y;
    CHECK(dv_lbd_mask_pixel(2.5f, 3.5f, 96, 40, &x, &y) && x == 2 && y == 4);
    CHECK(dv_lbd_mask_pixel(-0.5f, 39.4f, 96, 40, &x, &y) && x == 0 && y == 39);
    CHECK(!dv_lbd_mask_pixel(95.5f, 0, 96, 40, &x, &y) && !dv_lbd_mask_pixel(0, 39.5f, 96, 40, &x, &y) && !dv_lbd_mask_pixel(-0.6f, 0, 96, 40, &x, &y));
    CHECK(!dv_lbd_mask_pixel(3.0e38f, 0, 96, 40, &x, &y) && !dv_lbd_mask_pixel(NAN, 0, 96, 40, &x, &y));

    // the tail: all-zero band sums give NaN everywhere and a zero row; one dominant element is clamped at 0.4 before the renormalisation
    float band[8][DV_LBD_BANDS] = {}, des[DV_LBD_FLOATS];
    dv_lbd_finish(band, des);
    for (int i = 0; i < DV_LBD_FLOATS; ++i) CHECK(des[i] != des[i]);
    for (int k = 0; k < 32; ++k) CHECK(dv_lbd_byte(des, k) == 0);
    for (int bnd = 0; bnd < DV_LBD_BANDS; ++bnd) { band[0][bnd] = 1.0f + (float)bnd; band[2][bnd] = 40.0f * (1.0f + (float)bnd) * (1.0f + (float)bnd); band[5][bnd] = 2.0f; band[7][bnd] = 9.0f; }
    dv_lbd_finish(band, des);
    float ss = 0;
    for (int i = 0; i < DV_LBD_FLOATS; ++i) { CHECK(des[i] == des[i] && des[i] >= 0.0f); ss += des[i] * des[i]; }
    CHECK(std::fabs(ss - 1.0f) < 1e-5f && des[8] > des[0] && (dv_lbd_byte(des, 0) & 1) == 0 && des[2] == 0.0f);
    const float* first = des;
    const float* last = des + 8 * 8;
    CHECK(last[0] > first[0] && last[4] > first[4]);

    // the selection
    std::vector<uint8_t> mask(40 * 100, 255);
    mask[5 * 100 + 2] = 0; mask[10 * 100 + 20] = 1;
    dv_key_line k{ 20, 10, 40, 10, 0, 15.0f };
    CHECK(dv_lbd_keep(k, 15.0f, mask.data(), 100, 96, 40) && dv_lbd_keep(k, 15.0f, nullptr, 0, 96, 40) && !dv_lbd_keep(k, std::nextafter(15.0f, 16.0f), nullptr, 0, 96, 40));
    k.sx = 2.5f; k.sy = 5; CHECK(!dv_lbd_keep(k, 15.0f, mask.data(), 100, 96, 40));
    k.sx = 3.5f; CHECK(dv_lbd_keep(k, 15.0f, mask.data(), 100, 96, 40));
    k.ex = 95.5f; CHECK(!dv_lbd_keep(k, 15.0f, mask.data(), 100, 96, 40) && dv_lbd_keep(k, 15.0f, nullptr, 0, 96, 40));
    k.length = NAN; CHECK(!dv_lbd_keep(k, 15.0f, nullptr, 0, 96, 40));

    // a line as the kernels read it
    const DvLbdLine L = dv_lbd_line(dv_key_line{ 1, 2, 3, 4, 0.0f, 9 }, 5);
    CHECK(L.c == 1.0f && L.s == 0.0f && L.npix == 5 && L.k.ex == 3);
    const float hp = (float)1.57079632679489661923;
    CHECK(dv_lbd_line(dv_key_line{ 0, 0, 0, 1, hp, 1 }, 2).s == 1.0f && std::fabs(dv_lbd_line(dv_key_line{ 0, 0, 0, 1, hp, 1 }, 2).c) < 1e-7f);

    // every refusal
    std::vector<dv_key_line> lines(DV_LINE_MAX + 1, dv_key_line{ 3, 4, 30, 9, 0.18f, 27.5f });
    std::vector<int32_t> np(DV_LINE_MAX + 1, 28);
    CHECK(dv_lbd_check_host(96, 40, 120, lines.data(), nullptr, 512, DV_MEM_HOST, nullptr, 0) == nullptr);
    CHECK(dv_lbd_check_host(96, 40, 96, lines.data(), np.data(), 512, DV_MEM_PINNED, mask.data(), 100) == nullptr);
    CHECK(dv_lbd_check_host(96, 40, 96, nullptr, nullptr, 0, DV_MEM_HOST, nullptr, 0) == nullptr);
    CHECK(dv_lbd_check_host(96, 40, 96, lines.data(), nullptr, 513, DV_MEM_HOST, nullptr, 0) && dv_lbd_check_host(96, 40, 96, lines.data(), nullptr, -1, DV_MEM_HOST, nullptr, 0));
    CHECK(dv_lbd_check_host(96, 40, 96, nullptr, nullptr, 3, DV_MEM_HOST, nullptr, 0) && dv_lbd_check_host(96, 40, 96, lines.data(), nullptr, 3, 3, nullptr, 0));
    CHECK(dv_lbd_check_host(96, 40, 95, lines.data(), nullptr, 3, DV_MEM_HOST, nullptr, 0) && dv_lbd_check_host(96, 40, 96, lines.data(), nullptr, 3, DV_MEM_HOST, mask.data(), 95));
    CHECK(dv_lbd_check_host(32768, 40, 32768, lines.data(), nullptr, 3, DV_MEM_HOST, nullptr, 0) && dv_lbd_check_host(96, 32768, 96, lines.data(), nullptr, 3, DV_MEM_HOST, nullptr, 0));
    CHECK(dv_lbd_check_host(0, 40, 96, lines.data(), nullptr, 3, DV_MEM_HOST, nullptr, 0));
    CHECK(dv_lbd_check_host(96, 40, 96, (const dv_key_line*)((const char*)lines.data() + 2), nullptr, 3, DV_MEM_HOST, nullptr, 0));
    CHECK(dv_lbd_check_host(96, 40, 96, (const dv_key_line*)16, nullptr, 3, DV_MEM_DEVICE, nullptr, 0) == nullptr);          // device lines are not read here
    np[2] = 0; CHECK(dv_lbd_check_host(96, 40, 96, lines.data(), np.data(), 3, DV_MEM_HOST, nullptr, 0));
    np[2] = 137; CHECK(dv_lbd_check_host(96, 40, 96, lines.data(), np.data(), 3, DV_MEM_HOST, nullptr, 0));
    np[2] = 136; CHECK(!dv_lbd_check_host(96, 40, 96, lines.data(), np.data(), 3, DV_MEM_HOST, nullptr, 0));
    lines[1].angle = NAN; CHECK(dv_lbd_check_host(96, 40, 96, lines.data(), nullptr, 3, DV_MEM_HOST, nullptr, 0));
    lines[1].angle = 0; lines[1].ex = std::numeric_limits<float>::infinity(); CHECK(dv_lbd_values_check_host(96, 40, lines.data(), nullptr, 3));
    lines[1].ex = 30; lines[1].length = std::numeric_limits<float>::infinity(); CHECK(!dv_lbd_values_check_host(96, 40, lines.data(), nullptr, 3));          // a length is not refused
    lines[1].length = NAN; CHECK(!dv_lbd_values_check_host(96, 40, lines.data(), nullptr, 3));
    lines[1].ex = 500; CHECK(dv_lbd_values_check_host(96, 40, lines.data(), nullptr, 3));          // the rule gives 498 > w + h
    std::printf("lbd_host ok\n");
    return 0;
}
