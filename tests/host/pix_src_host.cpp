// pix_src_host.cpp — stand-alone check of the host side of dv_pix_has (csrc/pix_src.h), the one place the dynamic front end's four membership rules are written: all
// 256 byte values of both byte kinds, the float cases around a threshold, key comparison above 2^31, and the addressing (origin, row stride) of every kind against
// literal expectations.  No GPU, no library: tests/test_pix_src_host.py builds it under AddressSanitizer + UBSan and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "pix_src.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("BROKEN %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    // ---- bytes: a 16 x 16 "image" holding every value once; ROI_U8 takes value >= 1, PLANE_U8 everything but 0 and 128 ----
    std::vector<uint8_t> all(256);
    for (int b = 0; b < 256; ++b) all[b] = (uint8_t)b;
    const DvPixSrc roi{ all.data(), 16, DV_PIX_ROI_U8, 0u, 0.f, 5, 7 };          // rectangle-local: element (0, 0) is image pixel (5, 7)
    const DvPixSrc pl8{ all.data(), 16, DV_PIX_PLANE_U8, 0u, 0.f, 0, 0 };
    int n_roi = 0, n_pl8 = 0;
    for (int y = 0; y < 16; ++y)
        for (int x = 0; x < 16; ++x) {
            const int b = 16 * y + x;
            const bool r = dv_pix_has(roi, x + 5, y + 7), p = dv_pix_has(pl8, x, y);
            EXPECT(r == (b != 0));
            EXPECT(p == (b != 0 && b != 128));
            EXPECT(p == dv_pix_u8_has((unsigned)b));
            n_roi += r; n_pl8 += p;
        }
    EXPECT(n_roi == 255 && n_pl8 == 254);
    EXPECT(!dv_pix_has(pl8, 0, 0) && dv_pix_has(pl8, 1, 0) && dv_pix_has(pl8, 15, 7) && !dv_pix_has(pl8, 0, 8) && dv_pix_has(pl8, 1, 8) && dv_pix_has(pl8, 15, 15));      // 0, 1, 127, 128, 129, 255
    EXPECT(dv_pix_has(roi, 5 + 0, 7 + 8));                                         // 128 is an ROI-mask pixel
    // a row stride above the row: rows of 3 bytes, 5 apart
    const uint8_t padded[10] = { 0, 0, 0, 9, 9, 0, 1, 0, 9, 9 };
    const DvPixSrc pp{ padded, 5, DV_PIX_PLANE_U8, 0u, 0.f, 0, 0 };
    EXPECT(!dv_pix_has(pp, 0, 1) && dv_pix_has(pp, 1, 1) && !dv_pix_has(pp, 2, 1) && !dv_pix_has(pp, 2, 0));
    // ---- floats: strictly above the threshold; NaN never, on either side ----
    const float thr = 0.5f, inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    const float f[2][4] = { { thr, std::nextafterf(thr, inf), nan, inf }, { -inf, std::nextafterf(thr, -inf), 0.f, 1e30f } };
    const DvPixSrc pf{ reinterpret_cast<const uint8_t*>(f), (int)sizeof(f[0]), DV_PIX_PLANE_F32, 0u, thr, 0, 0 };
    const bool want_f[2][4] = { { false, true, false, true }, { false, false, false, true } };
    for (int y = 0; y < 2; ++y) for (int x = 0; x < 4; ++x) EXPECT(dv_pix_has(pf, x, y) == want_f[y][x]);
    DvPixSrc pn = pf; pn.thr = nan;
    for (int x = 0; x < 4; ++x) EXPECT(!dv_pix_has(pn, x, 0));
    EXPECT(dv_pix_f32_has(0.50001f, 0.5f) && !dv_pix_f32_has(0.5f, 0.5f) && !dv_pix_f32_has(nan, 0.5f));
    // ---- keys: equality of unsigned dwords, id 0 and ids above 2^31 included; rows of 3 dwords, 4 apart ----
    const uint32_t k[8] = { 0u, 7u, 3000000001u, 7u, 0x80000000u, 0u, 0x7fffffffu, 7u };
    DvPixSrc pk{ reinterpret_cast<const uint8_t*>(k), 16, DV_PIX_KEY_U32, 0u, 0.f, 0, 0 };
    EXPECT(dv_pix_has(pk, 0, 0) && !dv_pix_has(pk, 1, 0) && !dv_pix_has(pk, 0, 1) && dv_pix_has(pk, 1, 1));
    pk.id = 3000000001u; EXPECT(dv_pix_has(pk, 2, 0) && !dv_pix_has(pk, 0, 0));
    pk.id = 0x80000000u; EXPECT(dv_pix_has(pk, 0, 1) && !dv_pix_has(pk, 2, 1));
    pk.id = 7u; EXPECT(dv_pix_has(pk, 1, 0) && !dv_pix_has(pk, 2, 1));            // (the filler column beyond the row is never asked)
    std::printf(failures ? "pix_src_host: %d BROKEN\n" : "pix_src_host: ok\n", failures);
    return failures ? 1 : 0;
}
