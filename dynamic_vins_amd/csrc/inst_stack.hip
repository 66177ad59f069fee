// inst_stack.hip — the detector branch of thread T1 on gfx950: a frame's instances arrive as a STACK of N mask planes (the segmentation network's output tensor, left in
// HBM) instead of a label image.  Reference: Detector2D::Launch's `seg_label > kSoloMaskThr` (det2d/detector2d.cpp:441), BuildBoxes2D (det2d/detector2d.cpp:58-97),
// SemanticImage::SetMaskAndRoi / SetBackgroundMask (basic/semantic_image.cpp:20-93).  Two kernels:
//   inst_stack_kernel            one pass over the stack -> merged mask, its inverse, per-plane bounding boxes (dv_inst_stack_frame_enqueue)
//   stack_finish_remap_kernel    the tail of the naive form: the remapped merged mask made tight, and its inverse
// The objects' ROI masks and the static-instance unmasking read single planes of the stack as a DvPixSrc (dv_plane_src): inst_track.hip, copy.hip.
// The membership rule (include/dvins.h, dv_mask_stack) is pix_src.h's: a byte belongs unless it is 0 or 128, a float belongs when it is > threshold (false for NaN).
#include "dv_internal.h"

namespace {

__device__ __forceinline__ unsigned u8_hits(uint32_t v) {          // bit i: byte i belongs
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { m |= (unsigned)dv_pix_u8_has((v >> (8 * i)) & 255u) << i; }
    return m;
}

// the 4 pixels x0 .. x0 + 3 of one row of one plane -> hit bits.  nv = how many of them lie inside the row (0 .. 4).  The wide load is taken when the lane has all
// four pixels AND the row's address allows it (wave-uniform: a wave works on one row of one plane); otherwise element by element, inside the row.  A tight byte stack whose
// width is no multiple of 4 (1242: every odd row starts 2 bytes off a dword) therefore takes the element path on the rows that start off a dword, loads and stores alike
template <int KIND>
__device__ __forceinline__ unsigned plane_hits(const uint8_t* __restrict__ row, int x0, int nv, float thr) {
    unsigned m = 0;
    if (KIND == DV_STACK_U8) {
        if (nv == 4 && ((uintptr_t)row & 3) == 0) return u8_hits(*reinterpret_cast<const uint32_t*>(row + x0));
        for (int i = 0; i < nv; ++i) m |= (unsigned)dv_pix_u8_has(row[x0 + i]) << i;
    } else {
        const float* rf = reinterpret_cast<const float*>(row);
        if (nv == 4 && ((uintptr_t)row & 15) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(rf + x0);
            return (unsigned)dv_pix_f32_has(v.x, thr) | ((unsigned)dv_pix_f32_has(v.y, thr) << 1) | ((unsigned)dv_pix_f32_has(v.z, thr) << 2) | ((unsigned)dv_pix_f32_has(v.w, thr) << 3);
        }
        for (int i = 0; i < nv; ++i) m |= (unsigned)dv_pix_f32_has(rf[x0 + i], thr) << i;
    }
    return m;
}

// Workgroup = 4 waves, each on one image row; a lane owns 4 consecutive pixels of that row (a wave: 256 pixels = 256 contiguous bytes, or 1 KiB of floats, per plane)
// and walks the planes four at a time (the four planes' hit bits are formed before the first box is folded, so their loads do not wait for a ballot; how many are in
// flight at once is the compiler's schedule and has not been measured), keeping the OR of its pixels in a register.  The two masks are written
// once, a dword per lane where the output row allows it.  Boxes: per plane the wave finds its first and last hit lane with one ballot (the row is the wave's), one lane
// folds them into the workgroup's LDS box with integer min / max, and the workgroup's boxes go to the global ones with integer atomics: order independent, deterministic.
// merge / inv: w x h bytes, tightly packed.
constexpr int IS_CHUNK = 4;
template <int KIND>
__global__ __launch_bounds__(256) void inst_stack_kernel(DvStackSrc S, int w, int h, uint8_t* __restrict__ merge, uint8_t* __restrict__ inv, int32_t* __restrict__ boxes) {
    __shared__ int s_box[DV_STACK_MAX_PLANES][4];
    const int t = threadIdx.y * 64 + threadIdx.x;
    if (t < S.n_planes) { s_box[t][0] = 0x7fffffff; s_box[t][1] = -1; s_box[t][2] = 0x7fffffff; s_box[t][3] = -1; }
    __syncthreads();
    const int xb = blockIdx.x * 256, x0 = xb + threadIdx.x * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (y < h) {          // wave-uniform: all 64 lanes of the wave take part in the ballots below (a lane beyond the row has nv = 0 and never hits)
        const int nv = min(max(w - x0, 0), 4);
        unsigned acc = 0;
        for (int p0 = 0; p0 < S.n_planes; p0 += IS_CHUNK) {
            unsigned m[IS_CHUNK];
#pragma unroll
            for (int k = 0; k < IS_CHUNK; ++k) {
                const int p = p0 + k;
                m[k] = p < S.n_planes ? plane_hits<KIND>(S.base + (size_t)p * S.plane_stride + (size_t)y * S.row_stride, x0, nv, S.thr) : 0u;
            }
#pragma unroll
            for (int k = 0; k < IS_CHUNK; ++k) {
                acc |= m[k];
                const unsigned long long b = __ballot(m[k] != 0u);
                if (b) {
                    const int lo = __ffsll((long long)b) - 1, hi = 63 - __clzll((long long)b);
                    const unsigned mlo = (unsigned)__shfl((int)m[k], lo), mhi = (unsigned)__shfl((int)m[k], hi);
                    if (threadIdx.x == 0) {
                        const int p = p0 + k, cmin = xb + lo * 4 + (__ffs((int)mlo) - 1), cmax = xb + hi * 4 + (31 - __clz((int)mhi));
                        atomicMin(&s_box[p][0], y); atomicMax(&s_box[p][1], y); atomicMin(&s_box[p][2], cmin); atomicMax(&s_box[p][3], cmax);
                    }
                }
            }
        }
        if (nv > 0) {
            const uint32_t mv = ((acc & 1u) ? 0xffu : 0u) | ((acc & 2u) ? 0xff00u : 0u) | ((acc & 4u) ? 0xff0000u : 0u) | ((acc & 8u) ? 0xff000000u : 0u);
            const size_t o = (size_t)y * w + x0;
            if (nv == 4 && (o & 3) == 0) {
                *reinterpret_cast<uint32_t*>(merge + o) = mv; *reinterpret_cast<uint32_t*>(inv + o) = ~mv;
            } else {
                for (int i = 0; i < nv; ++i) { const uint8_t v = (uint8_t)(mv >> (8 * i)); merge[o + i] = v; inv[o + i] = (uint8_t)~v; }
            }
        }
    }
    __syncthreads();
    if (t < S.n_planes && s_box[t][1] >= 0) {
        atomicMin(&boxes[4 * t + 0], s_box[t][0]); atomicMax(&boxes[4 * t + 1], s_box[t][1]);
        atomicMin(&boxes[4 * t + 2], s_box[t][2]); atomicMax(&boxes[4 * t + 3], s_box[t][3]);
    }
}

// SetBackgroundMask's tail (basic/semantic_image.cpp:85-92): the remapped merged mask (rows of spitch bytes) -> tightly packed merged mask and inv = ~merged
__global__ __launch_bounds__(256) void stack_finish_remap_kernel(const uint8_t* __restrict__ src, int spitch, int w, int h, uint8_t* __restrict__ merge, uint8_t* __restrict__ inv) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    const uint8_t v = src[(size_t)y * spitch + x];
    merge[(size_t)y * w + x] = v; inv[(size_t)y * w + x] = (uint8_t)~v;
}

}  // namespace

void dv_launch_inst_stack(const DvStackSrc& S, int w, int h, uint8_t* merge, uint8_t* inv, int32_t* boxes, hipStream_t s) {
    const dim3 grid((w + 255) / 256, (h + 3) / 4), block(64, 4);
    if (S.kind == DV_STACK_F32) hipLaunchKernelGGL((inst_stack_kernel<DV_STACK_F32>), grid, block, 0, s, S, w, h, merge, inv, boxes);
    else hipLaunchKernelGGL((inst_stack_kernel<DV_STACK_U8>), grid, block, 0, s, S, w, h, merge, inv, boxes);
}
void dv_launch_stack_finish_remap(const uint8_t* src, int spitch, int w, int h, uint8_t* merge, uint8_t* inv, hipStream_t s) {
    hipLaunchKernelGGL(stack_finish_remap_kernel, dim3((w + 255) / 256, h), dim3(256), 0, s, src, spitch, w, h, merge, inv);
}
