// The ReID extractor's host rules (csrc/reid_host.h) as a stand-alone program for the sanitizers: the layer list and its offsets into the weight file, the accepted
// sizes, the refusals, the fold, the weight layouts, cvRound of rectangles, and the resize rule on small crops whose every read must stay inside the crop.
// Then the rectangles of tests/reid_hostile.py on frames of a camera's size, each printed as it is walked.
// Prints "reid_host ok"; tests/test_reid_ref.py and tests/test_reid_hostile_ref.py build it through reid.mk and run it.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "reid_host.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    // the float count, recounted tensor by tensor, and the offsets in file order without gap or overlap
    constexpr DvReidPlan P = dv_reid_plan();
    size_t off = 64 * 27 + 64 + 4 * 64, n = 0;
    EXPECT(P.c1_w == 0 && P.c1_b == 1728 && P.c1_bn == 1792);
    for (int b = 0; b < DV_REID_BLOCKS; ++b) {
        const DvReidBlock B = DV_REID_BLOCK[b];
        const int shapes[3][4] = {{B.c_in, B.c_out, 3, B.down ? 2 : 1}, {B.c_out, B.c_out, 3, 1}, {B.c_in, B.c_out, 1, 2}};
        for (int r = 0; r < (B.down ? 3 : 2); ++r, ++n) {
            const DvReidConv& c = P.conv[n];
            EXPECT(c.c_in == shapes[r][0] && c.c_out == shapes[r][1] && c.k == shapes[r][2] && c.stride == shapes[r][3] && c.role == r && c.block == b);
            EXPECT(c.w_off == off); off += (size_t)c.c_out * c.c_in * c.k * c.k;
            EXPECT(c.bn_off == off); off += 4 * (size_t)c.c_out;
            EXPECT(!dv_reid_layer_check_host(1, c.c_in, 8, 4, c.c_out, c.k, c.stride));
        }
    }
    EXPECT(n == (size_t)DV_REID_CONVS && off == P.n_floats && off == (size_t)DV_REID_N_FLOATS && off == 11178496u);

    // sizes: the ceil chain
    for (int w = 1; w <= 80; ++w) for (int h = 1; h <= 140; ++h) EXPECT(dv_reid_size_ok(w, h) == (w >= 49 && w <= 64 && h >= 113 && h <= 128));
    EXPECT(!dv_reid_check_host(DV_REID_N_FLOATS, 64, 128) && !dv_reid_check_host(DV_REID_N_FLOATS, 57, 121));
    EXPECT(dv_reid_check_host(DV_REID_N_FLOATS - 1, 64, 128) && dv_reid_check_host(DV_REID_N_FLOATS + 1, 64, 128) && dv_reid_check_host(0, 64, 128));
    EXPECT(dv_reid_check_host(DV_REID_N_FLOATS, 48, 128) && dv_reid_check_host(DV_REID_N_FLOATS, 64, 129) && dv_reid_check_host(DV_REID_N_FLOATS, 0, 0) && dv_reid_check_host(DV_REID_N_FLOATS, -64, 128));
    EXPECT(dv_reid_out_size(9, 3, 1) == 9 && dv_reid_out_size(9, 3, 2) == 5 && dv_reid_out_size(9, 1, 2) == 5 && dv_reid_out_size(1, 3, 2) == 1 && dv_reid_out_size(8, 1, 2) == 4);
    EXPECT(dv_reid_layer_check_host(1, 64, 8, 4, 64, 1, 1) && dv_reid_layer_check_host(1, 3, 8, 4, 64, 3, 1) && dv_reid_layer_check_host(1, 64, 8, 4, 96, 3, 1));
    EXPECT(dv_reid_layer_check_host(65, 64, 8, 4, 64, 3, 1) && dv_reid_layer_check_host(1, 64, 129, 4, 64, 3, 1) && dv_reid_layer_check_host(0, 64, 8, 4, 64, 3, 1));

    EXPECT(!dv_reid_layer_check_host(64, 64, 64, 32, 64, 3, 1) && !dv_reid_layer_check_host(4, 512, 128, 64, 512, 3, 1) && dv_reid_layer_check_host(5, 512, 128, 64, 512, 3, 1));
    EXPECT(dv_reid_layer_check_host(64, 512, 128, 128, 512, 3, 1) && dv_reid_layer_check_host(3, 64, 128, 128, 512, 3, 1));

    // frame refusals
    std::vector<uint8_t> img(41 * 256);
    std::vector<float> rc(64 * 4, 1.0f);
    EXPECT(!dv_reid_frame_check_host(img.data(), 70, 256, rc.data(), 64, DV_MEM_HOST) && !dv_reid_frame_check_host(nullptr, 70, 0, nullptr, 0, DV_MEM_DEVICE));
    EXPECT(dv_reid_frame_check_host(img.data(), 70, 256, rc.data(), 65, DV_MEM_HOST) && dv_reid_frame_check_host(img.data(), 70, 209, rc.data(), 1, DV_MEM_HOST));
    EXPECT(dv_reid_frame_check_host(nullptr, 70, 256, rc.data(), 1, DV_MEM_HOST) && dv_reid_frame_check_host(img.data(), 70, 256, rc.data(), 1, 9));
    EXPECT(dv_reid_frame_check_host(img.data(), 70, 256, (const float*)((const char*)rc.data() + 2), 1, DV_MEM_HOST));

    // the fold and the layouts
    { const float bn[8] = {2.0f, 1.0f, 0.5f, -0.25f, 3.0f, 1.0f, 4.0f - 1e-5f, 1.0f - 1e-5f}, bias[2] = {1.0f, 0.0f}; float sc[2], sh[2];
      dv_reid_fold(bn, bias, 2, sc, sh);
      EXPECT(std::fabs(sc[0] - 1.0f) < 1e-6f && std::fabs(sc[1] - 1.0f) < 1e-6f && std::fabs(sh[0] - (0.5f - 3.0f + 1.0f)) < 1e-6f && std::fabs(sh[1] - (-0.25f - 1.0f)) < 1e-6f); }
    { const int ci = 8, co = 3, k = 3; std::vector<float> w((size_t)co * ci * k * k), o(w.size(), -1.0f);
      for (size_t i = 0; i < w.size(); ++i) w[i] = (float)i;
      dv_reid_pack(w.data(), ci, co, k, o.data());
      for (int tap = 0; tap < 9; ++tap) for (int c = 0; c < ci; ++c) for (int d = 0; d < co; ++d)
          EXPECT(o[(((size_t)tap * 2 + c / 4) * co + d) * 4 + (c & 3)] == w[((size_t)d * ci + c) * 9 + tap]); }
    { std::vector<float> w(64 * 27), o(64 * 27); for (size_t i = 0; i < w.size(); ++i) w[i] = (float)i; dv_reid_pack_c1(w.data(), o.data()); EXPECT(o[5 * 64 + 7] == w[7 * 27 + 5]); }
    { std::vector<float> lut(768); dv_reid_lut(lut.data()); EXPECT(lut[0] == (0.0f - 0.485f) / 0.229f && lut[2 * 256 + 255] == (255.0f * (1 / 255.f) - 0.406f) / 0.225f); }

    // cvRound: half to even; what cannot be a coordinate
    int q[4];
    EXPECT(dv_reid_round(0.5f, q) && q[0] == 0); EXPECT(dv_reid_round(1.5f, q) && q[0] == 2); EXPECT(dv_reid_round(2.5f, q) && q[0] == 2); EXPECT(dv_reid_round(-0.5f, q) && q[0] == 0);
    EXPECT(!dv_reid_round(std::numeric_limits<float>::quiet_NaN(), q) && !dv_reid_round(std::numeric_limits<float>::infinity(), q) && !dv_reid_round(3e9f, q) && !dv_reid_round(-3e9f, q));
    { const float r[4] = {0.5f, 1.5f, 69.5f, 38.5f}; EXPECT(dv_reid_rect(r, 70, 41, q) && q[0] == 0 && q[1] == 2 && q[2] == 70 && q[3] == 38); }
    { const float r[4] = {0.5f, 1.5f, 70.5f, 38.5f}; EXPECT(dv_reid_rect(r, 70, 41, q)); const float s[4] = {1.5f, 1.5f, 69.5f, 38.5f}; EXPECT(!dv_reid_rect(s, 70, 41, q)); }
    { const float r[4] = {3, 3, 0.4f, 5}; EXPECT(!dv_reid_rect(r, 70, 41, q)); const float s[4] = {-0.6f, 3, 4, 5}; EXPECT(!dv_reid_rect(s, 70, 41, q)); const float t[4] = {3, 3, 4, 39}; EXPECT(!dv_reid_rect(t, 70, 41, q)); }

    // the resize on crops held in allocations of EXACTLY their size (the sanitizer sees any read past the crop), stride = 3 w
    static const int SZ[5][2] = {{1, 1}, {2, 3}, {33, 17}, {128, 256}, {7, 5}};
    for (const auto& sz : SZ) {
        const int cw = sz[0], ch = sz[1];
        std::vector<uint8_t> crop((size_t)cw * ch * 3);
        for (size_t i = 0; i < crop.size(); ++i) crop[i] = (uint8_t)(i * 37 + 11);
        const int rq[4] = {0, 0, cw, ch};
        long long sum = 0;
        for (int dy = 0; dy < 128; ++dy) for (int dx = 0; dx < 64; ++dx) for (int c = 0; c < 3; ++c) { const int v = dv_reid_pixel(crop.data(), 3 * cw, rq, 64, 128, dx, dy, c); EXPECT(v >= 0 && v <= 255); sum += v; }
        EXPECT(sum > 0);
        if (cw == 1) EXPECT(dv_reid_pixel(crop.data(), 3, rq, 64, 128, 63, 127, 1) == crop[1]);
        if (cw == 128) EXPECT(dv_reid_pixel(crop.data(), 384, rq, 64, 128, 1, 1, 0) == (crop[2 * 384 + 6] + crop[2 * 384 + 9] + crop[3 * 384 + 6] + crop[3 * 384 + 9] + 2) >> 2);
    }
    // coefficients: an identity-sized crop copies, the halves of an upscale by 2
    { int i0, i1, c0, c1; dv_reid_coef(5, 64, 64, false, &i0, &i1, &c0, &c1); EXPECT(i0 == 5 && c0 == 2048 && c1 == 0);
      dv_reid_coef(0, 32, 64, false, &i0, &i1, &c0, &c1); EXPECT(i0 == 0 && c0 == 2048 && c1 == 0);            // sx = -1 -> 0, f = 0
      dv_reid_coef(0, 32, 64, true, &i0, &i1, &c0, &c1); EXPECT(i0 == 0 && i1 == 0 && c0 == 512 && c1 == 1536);      // f kept, both rows clamped
      dv_reid_coef(1, 32, 64, false, &i0, &i1, &c0, &c1); EXPECT(i0 == 0 && i1 == 1 && c0 == 1536 && c1 == 512);
      dv_reid_coef(63, 32, 64, false, &i0, &i1, &c0, &c1); EXPECT(i0 == 31 && i1 == 31 && c0 == 2048 && c1 == 0); }
    EXPECT(dv_reid_area2(128, 256, 64, 128) && !dv_reid_area2(128, 255, 64, 128));

    // the stem operator's refusals, and the limit shapes of tests/reid_hostile.py within the layer operator's 2^24 elements
    EXPECT(!dv_reid_stem_check_host(1, 1, 1) && !dv_reid_stem_check_host(64, 128, 128) && !dv_reid_stem_check_host(3, 121, 57));
    EXPECT(dv_reid_stem_check_host(0, 8, 8) && dv_reid_stem_check_host(65, 8, 8) && dv_reid_stem_check_host(1, 0, 8) && dv_reid_stem_check_host(1, 8, 0) && dv_reid_stem_check_host(1, 129, 8) &&
           dv_reid_stem_check_host(1, 8, 129) && dv_reid_stem_check_host(-1, 8, 8));
    { static const int PAIRS[4][2] = {{32, 64}, {96, 192}, {160, 320}, {512, 192}}, KS[3][2] = {{3, 1}, {3, 2}, {1, 2}}, MAPS[2][2] = {{9, 7}, {17, 13}};
      for (const auto& p : PAIRS) for (const auto& ks : KS) for (const auto& m : MAPS) EXPECT(!dv_reid_layer_check_host(3, p[0], m[0], m[1], p[1], ks[0], ks[1]));
      static const int NET[7][7] = {{1, 64, 128, 128, 64, 3, 1}, {2, 64, 61, 29, 64, 3, 1}, {2, 64, 61, 29, 128, 3, 2}, {2, 64, 64, 32, 128, 3, 2}, {2, 128, 31, 15, 256, 3, 2}, {2, 256, 16, 8, 512, 3, 2}, {64, 512, 8, 4, 512, 3, 1}};
      for (const auto& c : NET) { EXPECT(!dv_reid_layer_check_host(c[0], c[1], c[2], c[3], c[4], c[5], c[6])); EXPECT((long long)c[0] * c[2] * c[3] * (c[1] > c[4] ? c[1] : c[4]) <= (1LL << 24)); }
      EXPECT(!dv_reid_layer_check_host(24, 64, 17, 13, 64, 3, 1)); }      // the impulse cases' batch

    // crops at camera geometry: the rectangles of tests/reid_hostile.py (camera_rects; tests/test_reid_hostile_ref.py compares the lines printed here with its list) on
    // images of exactly H rows of 3 W + 5 bytes.  Every prepared byte is computed twice: from the frame, and from a copy of the crop in an allocation of exactly its size
    // with packed rows, where a read past the crop's edge is either a different byte or the sanitizer's business
    static const int CTX[3][2] = {{752, 480}, {1242, 375}, {480, 752}}, INSZ[2][2] = {{64, 128}, {57, 121}};
    for (const auto& cx : CTX) {
        const int W = cx[0], H = cx[1], stride = 3 * W + 5;
        std::vector<uint8_t> frame((size_t)stride * H);
        for (size_t i = 0; i < frame.size(); ++i) frame[i] = (uint8_t)((i * 2654435761u) >> 13);
        for (const auto& is : INSZ) {
            const int iw = is[0], ih = is[1];
            const float gx = 37, gy = 11;
            const float R[24][4] = {{gx, gy, 3.f * iw, 3.f * ih}, {gx, gy, 4.f * iw, 4.f * ih}, {gx, gy, 4.f * iw, 3.f * ih}, {gx, gy, 2.f * iw, 1.f * ih}, {gx, gy, 1.f * iw, 2.f * ih},
                                    {gx, gy, 2.f * iw, 2.f * ih}, {gx, gy, 2.f * iw - 1, 2.f * ih}, {gx, gy, 2.f * iw + 1, 2.f * ih}, {gx, gy, 2.f * iw, 2.f * ih - 1}, {gx, gy, 2.f * iw, 2.f * ih + 1},
                                    {gx, gy, (float)((3 * iw + 1) / 2), (float)((3 * ih + 1) / 2)}, {gx, gy, 200, 333}, {gx, gy, (float)iw, (float)ih}, {0, 0, (float)W, (float)H},
                                    {0, 0, 150, 290}, {W - 150.f, 0, 150, 290}, {0, H - 290.f, 150, 290}, {W - 150.f, H - 290.f, 150, 290},
                                    {W - 1.f, 0, 1, (float)H}, {0, H - 1.f, (float)W, 1}, {W - 1.f, H - 1.f, 1, 1},
                                    {W - 100.5f, H - 200.5f, 100.5f, H % 2 == 0 ? 200.5f : 201.f}, {0.5f, 0.5f, 2.5f, 3.5f}, {0.5f, 0.5f, W - 0.5f, H - 0.5f}};
            for (const auto& r : R) {
                if (!dv_reid_rect(r, W, H, q)) continue;
                std::printf("rect %d %d %d %d %d %d %d %d\n", W, H, iw, ih, q[0], q[1], q[2], q[3]);
                std::vector<uint8_t> crop((size_t)q[2] * q[3] * 3);
                for (int y = 0; y < q[3]; ++y) std::memcpy(crop.data() + (size_t)y * q[2] * 3, frame.data() + (size_t)(q[1] + y) * stride + (size_t)q[0] * 3, (size_t)q[2] * 3);
                const int rq[4] = {0, 0, q[2], q[3]};
                int differ = 0;
                for (int dy = 0; dy < ih; ++dy) for (int dx = 0; dx < iw; ++dx) for (int c = 0; c < 3; ++c)
                    differ += dv_reid_pixel(frame.data(), stride, q, iw, ih, dx, dy, c) != dv_reid_pixel(crop.data(), 3 * q[2], rq, iw, ih, dx, dy, c);
                EXPECT(differ == 0);
            }
        }
    }

    std::printf(fails ? "reid_host: %d FAILED\n" : "reid_host ok\n", fails);
    return fails ? 1 : 0;
}
