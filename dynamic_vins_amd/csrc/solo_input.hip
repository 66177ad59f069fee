// solo_input.hip — the detector's input on gfx950: the frame's 8-bit BGR image -> the network's normalised, resized, zero-padded [3, model_h, model_w] float32 tensor.
// Reference: Pipeline::ImageToTensor (det2d/pipeline.cpp:370-387) and Pipeline::ProcessInput (det2d/pipeline.cpp:204-232), restated in the reference's order (include/dvins.h
// has the rule; the refusals and the per-axis index and weight rule are solo_input_host.h).  One kernel:
//   solo_input_kernel   a workgroup = 4 waves on 4 consecutive output rows x 256 columns; a wave works inside ONE output row, so the source row pair and its two weights are
//                       wave-uniform; a lane owns 4 consecutive output columns and produces all three planes from the same source pixels.  The 3 x 256 normalised
//                       values (v - mean[c]) / std[c] are computed once per workgroup into LDS (3 KB, the bits of the per-pixel division), so the inner loop has no
//                       division.  The bilinear value is dv_solo_input_value's nested differences (solo_input_host.h): a constant image gives the constant's bits.
//                       Columns and rows outside the rectangle are stored as +0.0 in the same pass: every element is written every frame.  A plane row whose first
//                       float is 16-byte aligned (a wave-uniform fact) takes one 16-byte store per lane and plane; the others — model widths off a multiple of 4, a
//                       caller's buffer off 16 bytes — and the last columns of a row take element stores.  Loads are plain: per output column a lane reads the three
//                       bytes of each of its four source pixels one by one (up to 48 byte loads and 48 LDS reads per lane), not one wide read per corner pair.
#include "dv_ctx.h"
#include "solo_input_host.h"
#include <string>

namespace {

struct SoloInputArgs {
    const uint8_t* bgr; int stride, iw, ih;
    float* out; int mw, mh, rx, ry, rw, rh;
    float sx, sy, mean[3], sd[3];
};

__global__ __launch_bounds__(256) void solo_input_kernel(SoloInputArgs a) {
    __shared__ float lut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) lut[i] = dv_solo_input_norm(i & 255, a.mean[i >> 8], a.sd[i >> 8]);
    __syncthreads();
    const int y = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6));
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    if (y >= a.mh || x0 >= a.mw) return;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = 0.0f;
    const int yr = y - a.ry;
    if (yr >= 0 && yr < a.rh) {          // wave-uniform: the row crosses the rectangle
        int y0, y1; float h0, h1;
        dv_solo_input_axis(a.sy, yr, a.ih, &y0, &y1, &h0, &h1);
        const uint8_t* r0 = a.bgr + (size_t)y0 * a.stride; const uint8_t* r1 = a.bgr + (size_t)y1 * a.stride;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xr = x0 + i - a.rx;
            if (xr < 0 || xr >= a.rw) continue;
            int c0, c1; float w0, w1;
            dv_solo_input_axis(a.sx, xr, a.iw, &c0, &c1, &w0, &w1);
            const uint8_t* p00 = r0 + 3 * c0; const uint8_t* p01 = r0 + 3 * c1; const uint8_t* p10 = r1 + 3 * c0; const uint8_t* p11 = r1 + 3 * c1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {          // tensor plane c = the pixel's byte 2 - c
                const float* t = lut + c * 256;
                v[c][i] = dv_solo_input_value(t[p00[2 - c]], t[p01[2 - c]], t[p10[2 - c]], t[p11[2 - c]], w1, h1);
            }
        }
    }
    const bool full = x0 + 4 <= a.mw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* row = a.out + ((size_t)c * a.mh + y) * a.mw;
        if ((((uintptr_t)row & 15) == 0) && full) {          // the alignment is wave-uniform, the tail is the row's last lane
            *reinterpret_cast<float4*>(row + x0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (x0 + i < a.mw) row[x0 + i] = v[c][i];
        }
    }
}

}  // namespace

// Two output tensors used alternately (out[cur] belongs to the frame enqueued last into a library-owned buffer); `staged` holds a DV_MEM_HOST frame.
struct SoloInputFrame {
    DevBuf out[2], staged;
    int cur = 1;
    StageSlot slot;
    const float* last = nullptr; int rect[4] = {0, 0, 0, 0};
};

void dv_stage_delete(SoloInputFrame* p) { delete p; }

extern "C" {

int dv_solo_input_check(int img_w, int img_h, int stride, const dv_solo_input_params* par) {
    dv_ctx* ctx = nullptr;
    if (const char* why = dv_solo_input_check_host(img_w, img_h, stride, par, nullptr, nullptr, nullptr, nullptr)) DV_FAIL(std::string("dv_solo_input_check: ") + why);
    return 0;
}

int dv_solo_input_enqueue(dv_ctx* ctx, const uint8_t* bgr, int stride, int mem, const dv_solo_input_params* par, float* dst_dev) {
    if (!ctx) return -1;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    SoloInputArgs a{};
    if (const char* why = dv_solo_input_check_host(W, H, stride, par, &a.rx, &a.ry, &a.rw, &a.rh)) DV_FAIL(std::string("dv_solo_input_enqueue: ") + why);
    if (!bgr) DV_FAIL("dv_solo_input_enqueue: null image");
    if (!dv_mem_known(mem)) DV_FAIL("dv_solo_input_enqueue: unknown memory kind");
    if ((uintptr_t)dst_dev & 3) DV_FAIL("dv_solo_input_enqueue: dst_dev must be 4-byte aligned");
    if (!ctx->solo_in) ctx->solo_in = new SoloInputFrame();
    SoloInputFrame& V = *ctx->solo_in;
    if (V.slot.open(ctx, "dv_solo_input_enqueue: previous frame not collected")) return -1;
    hipStream_t s = ctx->stream;

    DvRows im;
    if (dv_stage_rows(ctx, V.staged, bgr, (size_t)3 * W, H, stride, dv_in_place_device_or_pinned(mem), s, &im)) return -1;
    a.bgr = im.p; a.stride = im.pitch;
    a.iw = W; a.ih = H; a.mw = par->model_w; a.mh = par->model_h;
    a.sx = dv_solo_scale(W, a.rw); a.sy = dv_solo_scale(H, a.rh);
    for (int c = 0; c < 3; ++c) { a.mean[c] = par->mean[c]; a.sd[c] = par->std[c]; }
    if (dst_dev) a.out = dst_dev;
    else {
        DevBuf& B = V.out[V.cur ^ 1];
        DV_CHECK(B.ensure((size_t)3 * a.mh * a.mw * 4));
        a.out = (float*)B.p;
    }
    {
        StageScope sc_t(ctx, "solo_input");
        hipLaunchKernelGGL(solo_input_kernel, dim3((a.mw + 255) / 256, (a.mh + 3) / 4), dim3(256), 0, s, a);
    }
    if (V.slot.close(ctx, hipGetLastError(), s)) return -1;
    if (!dst_dev) V.cur ^= 1;
    V.last = a.out; V.rect[0] = a.rx; V.rect[1] = a.ry; V.rect[2] = a.rw; V.rect[3] = a.rh;
    return 0;
}

int dv_solo_input_collect(dv_ctx* ctx, const float** input_dev, int* rect_x, int* rect_y, int* rect_w, int* rect_h) {
    if (!ctx) return -1;
    if (!ctx->solo_in || !ctx->solo_in->slot.pending) DV_FAIL("dv_solo_input_collect: nothing enqueued");
    SoloInputFrame& V = *ctx->solo_in;
    if (V.slot.wait(ctx)) return -1;
    if (input_dev) *input_dev = V.last;
    if (rect_x) *rect_x = V.rect[0];
    if (rect_y) *rect_y = V.rect[1];
    if (rect_w) *rect_w = V.rect[2];
    if (rect_h) *rect_h = V.rect[3];
    return 0;
}

}  // extern "C"
