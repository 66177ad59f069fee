// The detector input stage's host rules (csrc/solo_input_host.h) as a stand-alone program for the sanitizers: every refusal, the rectangle the check hands back, and the
// per-axis index and weight rule over whole axes (indices inside the source, weights in [0, 1), identity at equal sizes).  Prints "solo_input_host ok"; any failed check
// aborts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "solo_input_host.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::abort(); } } while (0)

static dv_solo_input_params params(int mw, int mh) { return dv_solo_input_params{mw, mh, {123.675f, 116.28f, 103.53f}, {58.395f, 57.12f, 57.375f}}; }
static bool refused(int w, int h, int stride, const dv_solo_input_params& p, const char* why) {
    const char* r = dv_solo_input_check_host(w, h, stride, &p, nullptr, nullptr, nullptr, nullptr);
    return r && std::strstr(r, why);
}

int main() {
    // accepted, with the rectangles of the device test's table
    const int cases[5][8] = {{70, 23, 64, 32, 0, 5, 64, 22}, {23, 70, 64, 32, 27, 0, 10, 32}, {71, 23, 66, 34, 0, 6, 66, 22}, {30, 30, 64, 32, 16, 0, 32, 32}, {64, 32, 64, 32, 0, 0, 64, 32}};
    for (const auto& c : cases) {
        const dv_solo_input_params p = params(c[2], c[3]);
        int x = -1, y = -1, w = -1, h = -1;
        CHECK(dv_solo_input_check_host(c[0], c[1], 3 * c[0], &p, &x, &y, &w, &h) == nullptr);
        CHECK(x == c[4] && y == c[5] && w == c[6] && h == c[7]);
        CHECK(dv_solo_input_check_host(c[0], c[1], 3 * c[0] + 7, &p, nullptr, nullptr, nullptr, nullptr) == nullptr);
    }
    const dv_solo_input_params kitti = params(1152, 384);
    int x, y, w, h;
    CHECK(!dv_solo_input_check_host(1242, 375, 3 * 1242, &kitti, &x, &y, &w, &h) && x == 0 && y == 18 && w == 1152 && h == 348);

    // every refusal, by its text
    const dv_solo_input_params p = params(64, 32);
    CHECK(dv_solo_input_check_host(70, 23, 210, nullptr, nullptr, nullptr, nullptr, nullptr));
    CHECK(refused(0, 23, 210, p, "positive") && refused(70, -3, 210, p, "positive") && refused(70, 23, 210, params(0, 32), "positive") && refused(70, 23, 210, params(64, -1), "positive"));
    CHECK(refused(16385, 23, 3 * 16385, p, "16384") && refused(70, 23, 210, params(64, 16385), "16384"));
    CHECK(refused(1, 23, 3, p, "image sides under 2") && refused(70, 1, 210, p, "image sides under 2"));
    CHECK(refused(2000, 2, 6000, p, "rectangle sides under 2"));
    CHECK(refused(70, 23, 209, p, "stride") && !refused(70, 23, 210, p, "stride"));
    CHECK(refused(70, 23, 210, params(64, 33), "odd") && refused(23, 70, 69, params(65, 32), "odd"));
    dv_solo_input_params q = p;
    q.std[1] = 0.0f; CHECK(refused(70, 23, 210, q, "zero"));
    q.std[1] = -0.0f; CHECK(refused(70, 23, 210, q, "zero"));
    q.std[1] = std::numeric_limits<float>::infinity(); CHECK(refused(70, 23, 210, q, "finite"));
    q = p; q.mean[2] = NAN; CHECK(refused(70, 23, 210, q, "finite"));
    q = p; q.std[0] = -57.0f; CHECK(dv_solo_input_check_host(70, 23, 210, &q, nullptr, nullptr, nullptr, nullptr) == nullptr);      // a negative deviation is arithmetic, not an error

    // the axis rule over whole axes, at every size pair up to 40 and at the reference's own sizes
    auto walk = [](int in, int out) {
        const float scale = dv_solo_scale(in, out);
        std::vector<unsigned char> src((size_t)in, 1);
        int prev = 0;
        for (int d = 0; d < out; ++d) {
            int i0, i1; float l0, l1;
            dv_solo_input_axis(scale, d, in, &i0, &i1, &l0, &l1);
            CHECK(i0 >= 0 && i0 < in && i1 >= i0 && i1 <= i0 + 1 && i1 < in && i0 >= prev);
            CHECK(src[(size_t)i0] + src[(size_t)i1] == 2);                        // (an index outside the axis is the sanitizer's to report)
            CHECK(l1 >= 0.0f && l1 < 1.0f && l0 == 1.0f - l1);
            if (d == 0) CHECK(i0 == 0 && l1 == 0.0f);
            if (in == out) CHECK(i0 == d && l1 == 0.0f);
            prev = i0;
        }
        int i0, i1; float l0, l1;
        dv_solo_input_axis(scale, out - 1, in, &i0, &i1, &l0, &l1);
        CHECK(i1 == in - 1 && (i0 == in - 1 ? l1 < 1e-3f : l1 > 0.999f));          // the last sample lands on the last source sample, to rounding
    };
    for (int in = 2; in <= 40; ++in) for (int out = 2; out <= 40; ++out) walk(in, out);
    walk(1242, 1152); walk(375, 348); walk(16384, 2); walk(2, 16384); walk(16384, 16384); walk(16383, 16384);

    // the bilinear value: four equal sources give the source's bits at every weight the axis rule produces; upper weights of 0 give the sample; the corners
    const float vals[5] = {dv_solo_input_norm(0, 103.53f, 57.375f), dv_solo_input_norm(255, 116.28f, 57.12f), dv_solo_input_norm(17, 123.675f, 58.395f), 0.0f, 2.64f};
    for (int in = 2; in <= 40; ++in) for (int out = 2; out <= 40; ++out) {
        const float scale = dv_solo_scale(in, out);
        for (int d = 0; d < out; ++d) {
            int i0, i1; float l0, l1;
            dv_solo_input_axis(scale, d, in, &i0, &i1, &l0, &l1);
            for (float c : vals) CHECK(dv_solo_input_value(c, c, c, c, l1, l0) == c && dv_solo_input_value(c, c, c, c, l1, l1) == c);
            const float v = dv_solo_input_value(-2.1f, 1.7f, 0.3f, 2.6f, l1, l0);
            CHECK(v >= -2.1f - 1e-6f && v <= 2.6f + 1e-6f);
        }
    }
    CHECK(dv_solo_input_value(1.5f, -2.0f, 0.25f, 2.5f, 0.0f, 0.0f) == 1.5f && dv_solo_input_value(1.5f, -2.0f, 0.25f, 2.5f, 0.0f, 0.5f) == 0.875f);
    CHECK(dv_solo_input_value(1.5f, -2.0f, 0.25f, 2.5f, 0.5f, 0.0f) == -0.25f && dv_solo_input_value(1.0f, 3.0f, 5.0f, 7.0f, 0.5f, 0.5f) == 4.0f);

    // the normalisation: the expression of the tensor library, IEEE division
    CHECK(dv_solo_input_norm(255, 103.53f, 57.375f) == (255.0f - 103.53f) / 57.375f && dv_solo_input_norm(0, 123.675f, 58.395f) == (0.0f - 123.675f) / 58.395f);
    std::printf("solo_input_host ok\n");
    return 0;
}
