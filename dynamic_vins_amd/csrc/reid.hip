// reid.hip — the ReID extractor on gfx950: a frame's colour image and detection rectangles -> one L2-normalised 512-float embedding per detection.  Reference:
// Extractor::extract (mot/extractor.cpp:31-52) and ReIdNetImpl (mot/reid_net.cpp:17-135), restated as the reference evaluates them (include/dvins.h has the rule; the
// rules shared with the host are in reid_host.h).  float32 throughout.  Activations are NHWC so that the K dimension of the implicit GEMM is contiguous.  Kernels, in
// stream order:
//   reid_crop_kernel     a thread per prepared pixel: cvRound of the rectangle, cv::resize's 8-bit INTER_LINEAR (or the fast area path at exactly 2 x), the channel swap
//                        and the normalisation through a 3 x 256 table the host computed -> [n, 3, in_h, in_w].  A bad rectangle raises its crop's flag.
//   reid_stem_kernel     conv1 (K = 27) + scale / shift + ReLU + max_pool2d(3, 2, 1): a wave per pooled pixel, a lane per output channel, the 5 x 5 x 3 inputs wave-uniform.
//                        The pool skips positions outside the map (padding -inf), the convolution reads zero there.
//   reid_conv_kernel     every other convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32: M = output pixels, N = c_out, K = k^2 c_in.  A workgroup owns an 8 x 4
//                        pixel tile of ONE image (M = 32: at the last stage a whole map, so n = 1 fills the tile and no row belongs to another crop) and 32 output
//                        channels per wave.  The input patch with its halo and zero padding is staged through LDS in chunks of 32 input channels; no im2col matrix
//                        exists anywhere.  K is summed in two levels (per chunk on the matrix cores, the chunks on the vector unit).  Epilogue: scale, shift,
//                        residual, ReLU, a full store.  No atomics, no split-K.
//   reid_tail_kernel     the mean over the 8 x 4 map in a fixed order, the row 2-norm by a fixed tree, the division -> [n, 512].
#include "dv_ctx.h"
#include "dv_internal.h"
#include "reid_host.h"
#include <cstring>
#include <string>
#include <vector>

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
constexpr int MC = DV_REID_MAX_CROPS, FD = DV_REID_FEAT_DIM;
constexpr int TILE_H = 8, TILE_W = 4;                       // the M tile: 32 output pixels of one image
constexpr int CK = 32;                                      // input channels staged per chunk
constexpr int MAX_POS = (7 * 2 + 3) * (3 * 2 + 3);          // the largest patch: 3 x 3 at stride 2 -> 17 x 9 positions

struct CropArgs { const uint8_t* bgr; int stride, img_w, img_h; const float* rects; const float* lut; float* out; int* flags; int in_w, in_h; };

__global__ __launch_bounds__(256) void reid_crop_kernel(CropArgs a) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, npx = a.in_w * a.in_h;
    int q[4];
    const bool ok = dv_reid_rect(a.rects + 4 * b, a.img_w, a.img_h, q);
    if (p == 0) a.flags[b] = ok ? 0 : 1;
    if (p >= npx) return;
    const int dy = p / a.in_w, dx = p - dy * a.in_w;
    float* o = a.out + (size_t)b * 3 * npx + p;
#pragma unroll
    for (int c = 0; c < 3; ++c)                             // tensor channel c = the image's byte 2 - c; a refused crop is all zero so that nothing downstream is uninitialised
        o[(size_t)c * npx] = ok ? a.lut[c * 256 + dv_reid_pixel(a.bgr, a.stride, q, a.in_w, a.in_h, dx, dy, 2 - c)] : 0.0f;
}

struct StemArgs { const float* x /* [n, 3, H, W] */; const float* w /* [27][64] */; const float* scale; const float* shift; float* y /* [n, Hp, Wp, 64] */; int H, W, Hp, Wp; };

__global__ __launch_bounds__(256) void reid_stem_kernel(StemArgs a) {
    const int co = threadIdx.x & 63, b = blockIdx.y;
    const int pp = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (pp >= a.Hp * a.Wp) return;                          // wave-uniform
    const int py = pp / a.Wp, px = pp - py * a.Wp;
    float w[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) w[t] = a.w[t * 64 + co];
    const float sc = a.scale[co], sh = a.shift[co];
    const float* xb = a.x + (size_t)b * 3 * a.H * a.W;
    float in[3][5][5];                                      // rows 2 py - 2 .. 2 py + 2, zero outside the image
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const int iy = 2 * py - 2 + r, ix = 2 * px - 2 + s;
                in[c][r][s] = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? xb[((size_t)c * a.H + iy) * a.W + ix] : 0.0f;
            }
    float m = -__builtin_huge_valf();
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int cy = 2 * py - 1 + i, cx = 2 * px - 1 + j;
            if (cy < 0 || cy >= a.H || cx < 0 || cx >= a.W) continue;      // the pool's padding: not a candidate
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) acc += in[c][i + ky][j + kx] * w[(c * 3 + ky) * 3 + kx];
            float v = acc * sc + sh;
            v = v < 0.0f ? 0.0f : v;
            m = (v > m || v != v) ? v : m;
        }
    a.y[(((size_t)b * a.Hp + py) * a.Wp + px) * 64 + co] = m;
}

struct ConvArgs {
    const float* x /* [n, H, W, Cin] */; const float4* w /* [k k][Cin / 4][Cout] x 4 */; const float* scale; const float* shift; const float* res; float* y /* [n, Ho, Wo, Cout] */;
    int H, W, Cin, Cout, Ho, Wo, k, s, pad, relu, tiles_x;
};

// NW waves, each 32 output channels of the same 32 pixels.  Grid: x = pixel tiles of one image, y = Cout / (32 NW), z = image.
template <int NW>
__global__ __launch_bounds__(64 * NW) void reid_conv_kernel(ConvArgs a) {
    __shared__ float4 patch[(CK / 4) * MAX_POS];            // [channel quad of the chunk][patch position]: 19 584 B
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, kh = lane >> 5;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x, b = blockIdx.z;
    const int oy0 = ty * TILE_H, ox0 = tx * TILE_W, iy0 = oy0 * a.s - a.pad, ix0 = ox0 * a.s - a.pad;
    const int PH = (TILE_H - 1) * a.s + a.k, PW = (TILE_W - 1) * a.s + a.k, NPOS = PH * PW, Cq = a.Cin >> 2;
    const int co = (blockIdx.y * NW + wv) * 32 + li;
    const int ppos = ((li >> 2) * a.s) * PW + (li & 3) * a.s;      // A row li = pixel (li / 4, li % 4) of the tile: its patch position at tap (0, 0)
    // two levels of summation: a chunk's 32 k^2 products per output run through two matrix-core accumulators, the chunks' sums are added on the vector unit.  One chain
    // over all of K (up to 4608 products) measured up to 5 x the rounding error of a blocked CPU float32 product; chains of at most 144 stay beside it
    floatx16 tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.0f;
    const float* xb = a.x + (size_t)b * a.H * a.W * a.Cin;
    for (int c0 = 0; c0 < a.Cin; c0 += CK) {
        __syncthreads();
        for (int idx = tid; idx < NPOS * (CK / 4); idx += 64 * NW) {
            const int pos = idx >> 3, cq = idx & 7, r = pos / PW, c = pos - r * PW, iy = iy0 + r, ix = ix0 + c;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // the zero padding, and everything of a partial tile past the map
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = *reinterpret_cast<const float4*>(xb + ((size_t)iy * a.W + ix) * a.Cin + c0 + 4 * cq);
            patch[cq * NPOS + pos] = v;
        }
        __syncthreads();
        floatx16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
        // a lane brings 4 consecutive channels per step (its half of 8): instruction e multiplies channel e of the low half wave's quad and of the high one's
        for (int tap = 0; tap < a.k * a.k; ++tap) {
            const int ky = tap / a.k, kx = tap - ky * a.k;
            const float4* ap = patch + kh * NPOS + ppos + ky * PW + kx;
            const float4* wp = a.w + ((size_t)tap * Cq + (c0 >> 2) + kh) * a.Cout + co;
#pragma unroll
            for (int g = 0; g < CK / 8; g += 2) {
                const float4 a0 = ap[(2 * g) * NPOS], a1 = ap[(2 * g + 2) * NPOS];
                const float4 b0 = wp[(size_t)(2 * g) * a.Cout], b1 = wp[(size_t)(2 * g + 2) * a.Cout];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] += acc0[r] + acc1[r];
    }
    const float sc = a.scale[co], sh = a.shift[co];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * kh, oy = oy0 + (row >> 2), ox = ox0 + (row & 3);
        if (oy < a.Ho && ox < a.Wo) {
            const size_t o = (((size_t)b * a.Ho + oy) * a.Wo + ox) * a.Cout + co;
            float v = tot[r] * sc + sh;
            if (a.res) v += a.res[o];
            if (a.relu) v = v < 0.0f ? 0.0f : v;
            a.y[o] = v;
        }
    }
}

// x [n, 32, 512] (the 8 x 4 map, NHWC) -> out [n, 512]
__global__ __launch_bounds__(FD) void reid_tail_kernel(const float* x, float* out) {
    __shared__ float sq[FD];
    const int c = threadIdx.x, b = blockIdx.x;
    const float* xb = x + (size_t)b * 32 * FD;
    float s = 0.0f;
    for (int p = 0; p < 32; ++p) s += xb[p * FD + c];
    const float mean = s / 32.0f;
    sq[c] = mean * mean;
    __syncthreads();
    for (int h = FD / 2; h >= 1; h >>= 1) {
        if (c < h) sq[c] += sq[c + h];
        __syncthreads();
    }
    out[(size_t)b * FD + c] = mean / sqrtf(sq[0]);
}

static void launch_conv(const ConvArgs& a, int n, hipStream_t s) {
    const int tiles_y = (a.Ho + TILE_H - 1) / TILE_H;
    if (a.Cout % 128 == 0) hipLaunchKernelGGL(reid_conv_kernel<4>, dim3(a.tiles_x * tiles_y, a.Cout / 128, n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(reid_conv_kernel<2>, dim3(a.tiles_x * tiles_y, a.Cout / 64, n), dim3(128), 0, s, a);
}
static ConvArgs conv_args(const float* x, const float* w, const float* scale, const float* shift, const float* res, float* y, int H, int W, int Cin, int Cout, int k, int stride, int relu) {
    ConvArgs a{};
    a.x = x; a.w = reinterpret_cast<const float4*>(w); a.scale = scale; a.shift = shift; a.res = res; a.y = y;
    a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.k = k; a.s = stride; a.pad = k == 3 ? 1 : 0; a.relu = relu;
    a.Ho = dv_reid_out_size(H, k, stride); a.Wo = dv_reid_out_size(W, k, stride); a.tiles_x = (a.Wo + TILE_W - 1) / TILE_W;
    return a;
}

}  // namespace

struct ReidNet {
    int in_w = 0, in_h = 0;
    bool loaded = false, failed = false; int pend_n = 0, last_n = 0;
    DevBuf weights /* conv1 [27][64], then the packed convolutions in file order */, bn /* scale, shift per layer */, lut, act[3], input, feats, flags, img, rects, op;
    size_t w_off[DV_REID_CONVS]{}, s_off[DV_REID_CONVS]{};      // floats into weights / bn; conv1: weights 0, bn 0
    PinBuf pinned;      // MC flags
    StageSlot slot;
};

void dv_stage_delete(ReidNet* p) { delete p; }

extern "C" {

int dv_reid_check(size_t n_floats, int in_w, int in_h) {
    dv_ctx* ctx = nullptr;
    if (const char* why = dv_reid_check_host(n_floats, in_w, in_h)) DV_FAIL(std::string("dv_reid_check: ") + why);
    return 0;
}

int dv_reid_load(dv_ctx* ctx, const float* weights, size_t n_floats, int in_w, int in_h) {
    if (!ctx) return -1;
    if (const char* why = dv_reid_check_host(n_floats, in_w, in_h)) DV_FAIL(std::string("dv_reid_load: ") + why);
    if (!weights) DV_FAIL("dv_reid_load: null weights");
    if (ctx->reid && ctx->reid->slot.pending) DV_FAIL("dv_reid_load: a frame is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    if (!ctx->reid) ctx->reid = new ReidNet();
    ReidNet& R = *ctx->reid;
    R.loaded = false;
    DV_CHECK(R.pinned.ensure(MC * 4));
    // the device layout: conv1's [27][64] then every convolution packed for the kernel's B operand (same float counts as the file's); scale / shift pairs per layer
    constexpr DvReidPlan P = dv_reid_plan();
    size_t wn = 27 * DV_REID_C1, sn = 2 * DV_REID_C1;
    for (int i = 0; i < DV_REID_CONVS; ++i) {
        const DvReidConv& c = P.conv[i];
        R.w_off[i] = wn; wn += (size_t)c.c_out * c.c_in * c.k * c.k;
        R.s_off[i] = sn; sn += 2 * (size_t)c.c_out;
    }
    std::vector<float> hw(wn), hs(sn), hl(3 * 256);
    dv_reid_pack_c1(weights + P.c1_w, hw.data());
    dv_reid_fold(weights + P.c1_bn, weights + P.c1_b, DV_REID_C1, hs.data(), hs.data() + DV_REID_C1);
    for (int i = 0; i < DV_REID_CONVS; ++i) {
        const DvReidConv& c = P.conv[i];
        dv_reid_pack(weights + c.w_off, c.c_in, c.c_out, c.k, hw.data() + R.w_off[i]);
        dv_reid_fold(weights + c.bn_off, nullptr, c.c_out, hs.data() + R.s_off[i], hs.data() + R.s_off[i] + c.c_out);
    }
    dv_reid_lut(hl.data());
    const size_t act_bytes = (size_t)MC * dv_reid_half(128) * dv_reid_half(64) * 64 * 4;      // the widest map behind the fused stem: 64 x 32 x 64 per crop
    DV_CHECK(R.weights.ensure(wn * 4)); DV_CHECK(R.bn.ensure(sn * 4)); DV_CHECK(R.lut.ensure(hl.size() * 4));
    for (DevBuf& b : R.act) DV_CHECK(b.ensure(act_bytes));
    DV_CHECK(R.input.ensure((size_t)MC * 3 * 128 * 64 * 4)); DV_CHECK(R.feats.ensure((size_t)MC * FD * 4)); DV_CHECK(R.flags.ensure(MC * 4));
    DV_CHECK(hipMemcpy(R.weights.p, hw.data(), wn * 4, hipMemcpyHostToDevice));
    DV_CHECK(hipMemcpy(R.bn.p, hs.data(), sn * 4, hipMemcpyHostToDevice));
    DV_CHECK(hipMemcpy(R.lut.p, hl.data(), hl.size() * 4, hipMemcpyHostToDevice));
    R.in_w = in_w; R.in_h = in_h; R.loaded = true; R.last_n = 0; R.failed = false;
    return 0;
}

int dv_reid_extract_enqueue(dv_ctx* ctx, const uint8_t* bgr, int stride, const float* rects_xywh, int n, int mem) {
    if (!ctx) return -1;
    if (!ctx->reid || !ctx->reid->loaded) DV_FAIL("dv_reid_extract_enqueue: dv_reid_load first");
    ReidNet& R = *ctx->reid;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    if (const char* why = dv_reid_frame_check_host(bgr, W, stride, rects_xywh, n, mem)) DV_FAIL(std::string("dv_reid_extract_enqueue: ") + why);
    if (R.slot.open(ctx, "dv_reid_extract_enqueue: previous frame not collected")) return -1;
    if (n == 0) { R.slot.close_empty(); R.pend_n = 0; return 0; }
    hipStream_t s = ctx->stream;
    CropArgs ca{};
    DvRows im;          // the rectangles travel with the image: both in place, or both copied
    if (dv_stage_rows(ctx, R.img, bgr, (size_t)3 * W, H, stride, dv_in_place_device_or_pinned(mem), s, &im)) return -1;
    ca.bgr = im.p; ca.stride = im.pitch; ca.rects = rects_xywh;
    if (!dv_in_place_device_or_pinned(mem)) {
        DV_CHECK(R.rects.ensure(MC * 16));
        DV_CHECK(hipMemcpyAsync(R.rects.p, rects_xywh, (size_t)n * 16, hipMemcpyHostToDevice, s));
        ca.rects = (const float*)R.rects.p;
    }
    ca.img_w = W; ca.img_h = H; ca.lut = (const float*)R.lut.p; ca.out = (float*)R.input.p; ca.flags = (int*)R.flags.p; ca.in_w = R.in_w; ca.in_h = R.in_h;
    const float* wts = (const float*)R.weights.p; const float* bn = (const float*)R.bn.p;
    float* A = (float*)R.act[0].p; float* B = (float*)R.act[1].p; float* C = (float*)R.act[2].p;
    {
        StageScope sc_t(ctx, "reid");
        hipLaunchKernelGGL(reid_crop_kernel, dim3((R.in_w * R.in_h + 255) / 256, n), dim3(256), 0, s, ca);
        StemArgs sa{(const float*)R.input.p, wts, bn, bn + DV_REID_C1, A, R.in_h, R.in_w, dv_reid_half(R.in_h), dv_reid_half(R.in_w)};
        hipLaunchKernelGGL(reid_stem_kernel, dim3((sa.Hp * sa.Wp + 3) / 4, n), dim3(256), 0, s, sa);
        // a block: x in A -> conv.0 -> B; a down block's branch x -> C; conv.3 on B, residual C or A (read and written at the same element by the same lane) -> A
        constexpr DvReidPlan P = dv_reid_plan();
        int h = sa.Hp, w = sa.Wp;
        for (int i = 0; i < DV_REID_CONVS;) {
            const DvReidConv& c0 = P.conv[i]; const DvReidConv& c3 = P.conv[i + 1];
            const bool down = DV_REID_BLOCK[c0.block].down != 0;
            const ConvArgs a0 = conv_args(A, wts + R.w_off[i], bn + R.s_off[i], bn + R.s_off[i] + c0.c_out, nullptr, B, h, w, c0.c_in, c0.c_out, 3, c0.stride, 1);
            launch_conv(a0, n, s);
            if (down) {
                const DvReidConv& cd = P.conv[i + 2];
                launch_conv(conv_args(A, wts + R.w_off[i + 2], bn + R.s_off[i + 2], bn + R.s_off[i + 2] + cd.c_out, nullptr, C, h, w, cd.c_in, cd.c_out, 1, 2, 0), n, s);
            }
            h = a0.Ho; w = a0.Wo;
            launch_conv(conv_args(B, wts + R.w_off[i + 1], bn + R.s_off[i + 1], bn + R.s_off[i + 1] + c3.c_out, down ? C : A, A, h, w, c3.c_in, c3.c_out, 3, 1, 1), n, s);
            i += down ? 3 : 2;
        }
        hipLaunchKernelGGL(reid_tail_kernel, dim3(n), dim3(FD), 0, s, A, (float*)R.feats.p);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = dv_copy_async(R.pinned.p, R.flags.p, MC * 4, s);
    if (R.slot.close(ctx, e, s)) return -1;
    R.pend_n = n;
    return 0;
}

int dv_reid_extract_collect(dv_ctx* ctx, const float** feats_dev) {
    if (!ctx) return -1;
    if (!ctx->reid || !ctx->reid->slot.pending) DV_FAIL("dv_reid_extract_collect: nothing enqueued");
    ReidNet& R = *ctx->reid;
    if (R.slot.wait(ctx)) return -1;
    if (R.pend_n > 0 && ctx->timing) dv_harvest_timers(ctx, ctx->stream);
    R.last_n = R.pend_n; R.failed = false;
    if (feats_dev) *feats_dev = R.pend_n > 0 ? (const float*)R.feats.p : nullptr;
    for (int j = 0; j < R.pend_n; ++j)
        if (((const int32_t*)R.pinned.p)[j]) {
            R.failed = true;
            DV_FAIL("dv_reid_extract_collect: rectangle " + std::to_string(j) + " is empty or leaves the " + std::to_string(ctx->cfg.width) + " x " + std::to_string(ctx->cfg.height) +
                    " image after rounding (the reference's ori_img(rect) throws): the frame has no embeddings");
        }
    return 0;
}

int dv_reid_get_feats(dv_ctx* ctx, float* out, int n) {
    if (!ctx) return -1;
    if (!ctx->reid || !ctx->reid->loaded) DV_FAIL("dv_reid_get_feats: dv_reid_load first");
    ReidNet& R = *ctx->reid;
    if (R.slot.pending) DV_FAIL("dv_reid_get_feats: a frame is in flight");
    if (R.failed) DV_FAIL("dv_reid_get_feats: the last frame failed");
    if (n < 0 || n > R.last_n || (n > 0 && !out)) DV_FAIL("dv_reid_get_feats: n exceeds the last frame's crops, or null output");
    if (n == 0) return 0;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    DV_CHECK(hipMemcpy(out, R.feats.p, (size_t)n * FD * 4, hipMemcpyDeviceToHost));
    return 0;
}

int dv_reid_input(dv_ctx* ctx, float* out) {
    if (!ctx) return -1;
    if (!ctx->reid || !ctx->reid->loaded) DV_FAIL("dv_reid_input: dv_reid_load first");
    ReidNet& R = *ctx->reid;
    if (R.slot.pending) DV_FAIL("dv_reid_input: a frame is in flight");
    if (R.last_n == 0) return 0;
    if (!out) DV_FAIL("dv_reid_input: null output");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    DV_CHECK(hipMemcpy(out, R.input.p, (size_t)R.last_n * 3 * R.in_w * R.in_h * 4, hipMemcpyDeviceToHost));
    return 0;
}

int dv_reid_layer(dv_ctx* ctx, const float* x, int n, int c_in, int h, int w, const float* weight, int c_out, int k, int stride, const float* scale, const float* shift,
                  const float* residual_or_null, int relu, float* out) {
    if (!ctx) return -1;
    if (const char* why = dv_reid_layer_check_host(n, c_in, h, w, c_out, k, stride)) DV_FAIL(std::string("dv_reid_layer: ") + why);
    if (!x || !weight || !scale || !shift || !out) DV_FAIL("dv_reid_layer: null argument");
    if (ctx->reid && ctx->reid->slot.pending) DV_FAIL("dv_reid_layer: a frame is in flight");
    if (!ctx->reid) ctx->reid = new ReidNet();
    ReidNet& R = *ctx->reid;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const int ho = dv_reid_out_size(h, k, stride), wo = dv_reid_out_size(w, k, stride);
    const size_t nx = (size_t)n * c_in * h * w, nw = (size_t)c_out * c_in * k * k, ny = (size_t)n * c_out * ho * wo;
    // host side: NCHW -> NHWC, the weight into the kernel's layout; one device buffer x | w | scale | shift | residual | y
    std::vector<float> hb(nx + nw + 2 * (size_t)c_out + 2 * ny);
    float* hx = hb.data(); float* hw = hx + nx; float* hs = hw + nw; float* hr = hs + 2 * c_out; float* hy = hr + ny;
    for (int b = 0; b < n; ++b) for (int c = 0; c < c_in; ++c) for (int p = 0; p < h * w; ++p) hx[((size_t)b * h * w + p) * c_in + c] = x[((size_t)b * c_in + c) * h * w + p];
    dv_reid_pack(weight, c_in, c_out, k, hw);
    std::memcpy(hs, scale, (size_t)c_out * 4); std::memcpy(hs + c_out, shift, (size_t)c_out * 4);
    if (residual_or_null)
        for (int b = 0; b < n; ++b) for (int c = 0; c < c_out; ++c) for (int p = 0; p < ho * wo; ++p) hr[((size_t)b * ho * wo + p) * c_out + c] = residual_or_null[((size_t)b * c_out + c) * ho * wo + p];
    DV_CHECK(R.op.ensure(hb.size() * 4));
    float* d = (float*)R.op.p;
    DV_CHECK(hipMemcpy(d, hb.data(), (hb.size() - ny) * 4, hipMemcpyHostToDevice));      // blocking both ways: hb never outlives a copy in flight, whatever returns early
    float* dw = d + nx; float* ds = dw + nw; float* dr = ds + 2 * c_out; float* dy = dr + ny;
    launch_conv(conv_args(d, dw, ds, ds + c_out, residual_or_null ? dr : nullptr, dy, h, w, c_in, c_out, k, stride, relu ? 1 : 0), n, ctx->stream);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    DV_CHECK(hipMemcpy(hy, dy, ny * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < n; ++b) for (int c = 0; c < c_out; ++c) for (int p = 0; p < ho * wo; ++p) out[((size_t)b * c_out + c) * ho * wo + p] = hy[((size_t)b * ho * wo + p) * c_out + c];
    return 0;
}

int dv_reid_stem(dv_ctx* ctx, const float* x, int n, int h, int w, const float* weight, const float* scale, const float* shift, float* out) {
    if (!ctx) return -1;
    if (const char* why = dv_reid_stem_check_host(n, h, w)) DV_FAIL(std::string("dv_reid_stem: ") + why);
    if (!x || !weight || !scale || !shift || !out) DV_FAIL("dv_reid_stem: null argument");
    if (ctx->reid && ctx->reid->slot.pending) DV_FAIL("dv_reid_stem: a frame is in flight");
    if (!ctx->reid) ctx->reid = new ReidNet();
    ReidNet& R = *ctx->reid;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const int hp = dv_reid_half(h), wp = dv_reid_half(w);
    const size_t nx = (size_t)n * 3 * h * w, nw = 27 * (size_t)DV_REID_C1, ny = (size_t)n * hp * wp * DV_REID_C1;
    // host side: the input as it is (the kernel reads NCHW), conv1's weight into the kernel's layout; one device buffer x | w | scale | shift | y
    std::vector<float> hb(nx + nw + 2 * (size_t)DV_REID_C1 + ny);
    float* hx = hb.data(); float* hw = hx + nx; float* hs = hw + nw; float* hy = hs + 2 * DV_REID_C1;
    std::memcpy(hx, x, nx * 4);
    dv_reid_pack_c1(weight, hw);
    std::memcpy(hs, scale, (size_t)DV_REID_C1 * 4); std::memcpy(hs + DV_REID_C1, shift, (size_t)DV_REID_C1 * 4);
    DV_CHECK(R.op.ensure(hb.size() * 4));
    float* d = (float*)R.op.p;
    DV_CHECK(hipMemcpy(d, hb.data(), (hb.size() - ny) * 4, hipMemcpyHostToDevice));      // blocking both ways, as in dv_reid_layer
    float* dw = d + nx; float* ds = dw + nw; float* dy = ds + 2 * DV_REID_C1;
    StemArgs sa{d, dw, ds, ds + DV_REID_C1, dy, h, w, hp, wp};
    hipLaunchKernelGGL(reid_stem_kernel, dim3((hp * wp + 3) / 4, n), dim3(256), 0, ctx->stream, sa);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    DV_CHECK(hipMemcpy(hy, dy, ny * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < n; ++b) for (int c = 0; c < DV_REID_C1; ++c) for (int p = 0; p < hp * wp; ++p) out[((size_t)b * DV_REID_C1 + c) * hp * wp + p] = hy[((size_t)b * hp * wp + p) * DV_REID_C1 + c];
    return 0;
}

}  // extern "C"
