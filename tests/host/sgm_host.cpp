// The stereo matcher's host rules (csrc/stereo_sgm_host.h) as a stand-alone program for the sanitizers: the census at clamped borders, the cost rule, the path step,
// the uniqueness test, the floored subpixel division and every refusal, the census and the cost also on the smallest frames (narrower than n_disp, 1 x 1).  Prints "sgm_host ok"; any failed check aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "stereo_sgm_host.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::abort(); } } while (0)

static dv_sgm_params params(int n_disp = 64, int p1 = 10, int p2 = 120, int uniq = 5, int lr = 1) { return dv_sgm_params{n_disp, p1, p2, uniq, lr, {0, 0, 0}}; }
static bool refused(int w, int h, int stride, const dv_sgm_params& p, const char* why) {
    const char* r = dv_sgm_check_host(w, h, stride, &p);
    return r && std::strstr(r, why);
}
// floor(a / b) by repeated subtraction: no division involved
static int slow_floor(int a, int b) { int q = 0; while (a < 0) { a += b; --q; } while (a >= b) { a -= b; ++q; } return q; }

int main() {
    // clamp
    CHECK(dv_sgm_clamp(-4, 5) == 0 && dv_sgm_clamp(0, 5) == 0 && dv_sgm_clamp(4, 5) == 4 && dv_sgm_clamp(9, 5) == 4 && dv_sgm_clamp(3, 1) == 0);
    // census on exactly sized heap images (an index outside is the sanitizer's to report): 5 x 3 with a stride of 7 — lower than the window in both directions
    {
        const int w = 5, h = 3, stride = 7;
        std::vector<uint8_t> img((size_t)(h - 1) * stride + w);
        for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) img[(size_t)y * stride + x] = (uint8_t)(10 * y + x);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                uint64_t want = 0; int bits = 0;
                for (int dy = -3; dy <= 3; ++dy)
                    for (int dx = -4; dx <= 4; ++dx) {
                        if (!dx && !dy) continue;
                        const int yy = y + dy < 0 ? 0 : (y + dy > h - 1 ? h - 1 : y + dy), xx = x + dx < 0 ? 0 : (x + dx > w - 1 ? w - 1 : x + dx);
                        want = (want << 1) | (uint64_t)(10 * yy + xx < 10 * y + x); ++bits;
                    }
                CHECK(bits == 62 && dv_sgm_census(img.data(), stride, w, h, x, y) == want && (want >> 62) == 0);
            }
        CHECK(dv_sgm_census(img.data(), stride, w, h, 0, 0) == 0);                                   // the smallest pixel: no neighbour is below it
        CHECK(dv_sgm_popcount(dv_sgm_census(img.data(), stride, w, h, w - 1, h - 1)) > 0);
        std::vector<uint8_t> one(1, 200);                                                            // a 1 x 1 image: every neighbour is the centre
        CHECK(dv_sgm_census(one.data(), 1, 1, 1, 0, 0) == 0);
    }
    // the matcher's smallest frames (tests/sgm_hostile.py: narrower than n_disp, one row, one column, 1 x 1), tight rows and rows of w + 5 bytes, on exactly sized heap
    // blocks: the census against the clamp written out; the cost of every (x, d) with the right code fetched only where x - d >= 0, as the path kernel fetches it; the
    // right winner's range x + d < w; the frame accepted for every n_disp
    {
        const int shapes[][2] = {{37, 6}, {5, 3}, {63, 2}, {70, 1}, {130, 1}, {1, 9}, {1, 1}, {2, 2}};
        for (const auto& sh : shapes) for (int extra : {0, 5}) {
            const int w = sh[0], h = sh[1], stride = w + extra;
            std::vector<uint8_t> img((size_t)(h - 1) * stride + w);
            for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) img[(size_t)y * stride + x] = (uint8_t)((37 * x + 101 * y + (x * y) % 7) & 255);
            std::vector<uint64_t> code((size_t)w * h);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    uint64_t want = 0;
                    const int c = img[(size_t)y * stride + x];
                    for (int dy = -3; dy <= 3; ++dy)
                        for (int dx = -4; dx <= 4; ++dx) {
                            if (!dx && !dy) continue;
                            const int yy = y + dy < 0 ? 0 : (y + dy > h - 1 ? h - 1 : y + dy), xx = x + dx < 0 ? 0 : (x + dx > w - 1 ? w - 1 : x + dx);
                            want = (want << 1) | (uint64_t)(img[(size_t)yy * stride + xx] < c);
                        }
                    CHECK((code[(size_t)y * w + x] = dv_sgm_census(img.data(), stride, w, h, x, y)) == want);
                }
            if (w == 1 && h == 1) CHECK(code[0] == 0);
            for (int D : {64, 128, 256}) {
                const dv_sgm_params p = params(D);
                CHECK(!dv_sgm_check_host(w, h, stride, &p) && (extra == 0 || refused(w, h, w - 1, p, "row stride below width")));
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        int outside = 0, reach = 0;
                        for (int d = 0; d < D; ++d) {
                            const int xr = x - d;
                            const int c = dv_sgm_cost(code[(size_t)y * w + x], xr >= 0 ? code[(size_t)y * w + xr] : 0, x, d);
                            CHECK(xr >= 0 ? (c >= 0 && c <= 62) : c == DV_SGM_OOB_COST);
                            outside += xr < 0; reach += x + d < w;
                        }
                        CHECK(outside == (D - 1 - x > 0 ? D - 1 - x : 0) && reach == (w - x < D ? w - x : D) && reach >= 1);      // d = 0 always has a pixel on both sides
                    }
            }
        }
        for (int D : {64, 128, 256}) CHECK(dv_sgm_subpixel(D - 1, D, 7, 1, 0) == 16 * (D - 1) && dv_sgm_subpixel(D - 2, D, 9, 1, 9) == 16 * (D - 2) && dv_sgm_subpixel(0, D, 0, 1, 7) == 0);
    }
    // cost
    CHECK(dv_sgm_cost(0, ~0ull, 5, 6) == 64 && dv_sgm_cost(0x3ull, 0x1ull, 5, 5) == 1 && dv_sgm_cost(~0ull >> 2, 0, 9, 0) == 62 && dv_sgm_cost(7, 7, 0, 0) == 0);
    CHECK(dv_sgm_popcount(0) == 0 && dv_sgm_popcount(~0ull) == 64);
    // path step: each of the four terms wins once; left-out neighbours never win; the bound 64 + p2
    CHECK(dv_sgm_path_step(5, 20, 30, 30, 10, 10, 120) == 5 + 20 - 10);
    CHECK(dv_sgm_path_step(5, 40, 12, 30, 10, 10, 120) == 5 + 22 - 10);
    CHECK(dv_sgm_path_step(5, 40, 30, 11, 10, 10, 120) == 5 + 21 - 10);
    CHECK(dv_sgm_path_step(5, 400, 300, 300, 10, 10, 120) == 5 + 120);
    CHECK(dv_sgm_path_step(64, 10, DV_SGM_NO_TERM, DV_SGM_NO_TERM, 10, 255, 255) == 64);
    CHECK(dv_sgm_path_step(64, 319, DV_SGM_NO_TERM, 319, 0, 255, 255) == 64 + 255);
    // uniqueness: strict, integer
    CHECK(dv_sgm_not_unique(104, 100, 5) && !dv_sgm_not_unique(106, 100, 5) && !dv_sgm_not_unique(100, 100, 0) && dv_sgm_not_unique(99, 100, 0));
    CHECK(dv_sgm_not_unique(2552, 26, 99) && !dv_sgm_not_unique(2600, 26, 99) && !dv_sgm_not_unique(0, 0, 5));
    // the floor
    for (int a = -600; a <= 600; ++a) for (int b = 1; b <= 40; ++b) CHECK(dv_sgm_floor_div(a, b) == slow_floor(a, b));
    CHECK(dv_sgm_floor_div(-1, 2) == -1 && -1 / 2 == 0);
    for (int sm = 0; sm <= 60; sm += 3) for (int sp = 0; sp <= 60; sp += 4) for (int s0 = 0; s0 <= (sm < sp ? sm : sp); s0 += 5) {
        int den = sm + sp - 2 * s0; if (den < 1) den = 1;
        const int v = dv_sgm_subpixel(7, 64, sm, s0, sp);
        CHECK(v == 16 * 7 + slow_floor(16 * (sm - sp) + den, 2 * den) && v >= 16 * 7 - 8 && v <= 16 * 7 + 8);
    }
    CHECK(dv_sgm_subpixel(7, 64, 10, 5, 30) == 16 * 7 - 5);                                          // (16 (10 - 30) + 30) / 60 = -4.83..: the floor is -5, truncation gives -4
    CHECK(dv_sgm_subpixel(0, 64, 99, 1, 7) == 0 && dv_sgm_subpixel(63, 64, 7, 1, 99) == 16 * 63 && dv_sgm_subpixel(255, 256, 7, 1, 99) == 16 * 255);
    // refusals, by their texts
    CHECK(dv_sgm_check_host(70, 23, 70, nullptr));
    const dv_sgm_params ok = params();
    CHECK(!dv_sgm_check_host(70, 23, 70, &ok) && !dv_sgm_check_host(70, 23, 71, &ok) && !dv_sgm_check_host(1, 1, 1, &ok));
    for (int d : {64, 128, 256}) { const dv_sgm_params p = params(d); CHECK(!dv_sgm_check_host(70, 23, 70, &p)); }
    for (int d : {0, 32, 63, 96, 512, -64}) CHECK(refused(70, 23, 70, params(d), "n_disp"));
    CHECK(refused(70, 23, 70, params(64, -1), "p1 must not be negative") && !refused(70, 23, 70, params(64, 0, 0), "p"));
    CHECK(refused(70, 23, 70, params(64, 30, 29), "p2 must not be below p1") && refused(70, 23, 70, params(64, 10, 256), "p2 above 255"));
    { const dv_sgm_params top = params(64, 255, 255); CHECK(!dv_sgm_check_host(70, 23, 70, &top)); }
    CHECK(refused(70, 23, 70, params(64, 10, 120, -1), "uniqueness") && refused(70, 23, 70, params(64, 10, 120, 100), "uniqueness") && !refused(70, 23, 70, params(64, 10, 120, 99), "uniqueness"));
    for (int i = 0; i < 3; ++i) { dv_sgm_params p = params(); p.reserved[i] = 1; CHECK(refused(70, 23, 70, p, "reserved")); }
    CHECK(refused(70, 23, 69, ok, "row stride below width") && refused(0, 23, 70, ok, "positive") && refused(70, 0, 70, ok, "positive") && refused(16385, 2, 16385, ok, "16384"));
    std::printf("sgm_host ok\n");
    return 0;
}
