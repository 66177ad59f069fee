// pix_src.h — "does this pixel belong to the instance?": the one description of where the answer is read and the one place its four rules are written.  Plain C++ on
// the host (tests/host compiles it under the sanitizers), __host__ __device__ under hipcc: the unmask kernel (copy.hip), the ROI-mask kernel (inst_track.hip) and the
// element paths of inst_stack_kernel all answer through it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __HIPCC__
#define DV_PIX_HD __host__ __device__ __forceinline__
#else
#define DV_PIX_HD inline
#endif

enum DvPixKind {
    DV_PIX_ROI_U8 = 0,      // byte >= 1 (FeatureTrack's roi_mask, system/main.cpp:217-245); tight rows of a rectangle whose corner is the origin
    DV_PIX_KEY_U32,         // dword == id (VIODE::PixelToKey), image-wide
    DV_PIX_PLANE_U8,        // byte not 0 and not 128 (include/dvins.h, dv_mask_stack), image-wide
    DV_PIX_PLANE_F32        // float > thr, false for NaN, image-wide
};
// base: device-addressable; stride: bytes per row; (ox, oy): the image position of the source's element (0, 0)
struct DvPixSrc { const uint8_t* base; int stride, kind; uint32_t id; float thr; int ox, oy; };

// The reference's rule on one stack byte, mask_tensor.to(kInt8).abs().clamp(0, 1) (basic/semantic_image.cpp:20-93), as CPU torch 2.10 evaluates it — checked over all
// 256 byte values, in a 6-element tensor (scalar loop) and in a 10240-element one (vectorised loop), with the same answer: bytes 1..127 -> 1; bytes 129..255 -> int8
// -127..-1 -> abs 127..1 -> 1; byte 128 -> int8 -128, whose abs WRAPS to -128 and clamps to 0.  So 1, 127, 129 and 255 are object pixels and 128 is not.  sum(0) widens
// to int64, so 64 planes cannot wrap the merged mask.  tests/test_inst_stack_host.py re-establishes it against the installed torch.
DV_PIX_HD bool dv_pix_u8_has(unsigned b) { return b != 0u && b != 128u; }
DV_PIX_HD bool dv_pix_f32_has(float v, float thr) { return v > thr; }          // strict; false for NaN

// (x, y): image coordinates inside what the source covers — the caller's check, made once per rectangle by the entry that staged it
DV_PIX_HD bool dv_pix_has(const DvPixSrc& s, int x, int y) {
    const uint8_t* row = s.base + (size_t)(y - s.oy) * (size_t)s.stride;
    const int c = x - s.ox;
    switch (s.kind) {
    case DV_PIX_ROI_U8:   return row[c] >= 1;
    case DV_PIX_KEY_U32:  return reinterpret_cast<const uint32_t*>(row)[c] == s.id;
    case DV_PIX_PLANE_U8: return dv_pix_u8_has(row[c]);
    default:              return dv_pix_f32_has(reinterpret_cast<const float*>(row)[c], s.thr);
    }
}
