// lbd.hip — the LBD line descriptor on gfx950: a gray image and the key lines LSD left -> the selected key lines and their 32-byte rows, in device buffers of the
// layout dv_line_track_enqueue(..., DV_MEM_DEVICE) takes.  Reference: LineDetector::Detect from lbd_descriptor->compute on (line_detector/line_detector.cpp:78-97) over
// BinaryDescriptor::computeImpl / computeSobel / computeLBD (thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:350-398,539-687,1026-1372) at octave 0.
// include/dvins.h has the rule; everything the host shares with the kernels (tables, roundings, the tail of computeLBD, the selection) is in lbd_host.h.
//   lbd_grad_kernel      one 256-thread workgroup per 64 x 16 tile: u8 tile + 3 px halo in LDS -> 5 x 5 blur to u8 (the tile + 1 px, BORDER_REFLECT_101 of the image)
//                        -> Sobel dx, dy as int16 (BORDER_REFLECT_101 of the BLURRED image: a halo pixel outside the image is the blur AT its mirror position).
//   lbd_describe_kernel  one wave per line, one lane per row of the 63-row support region.  A lane steps its row start serially (x0 -= dL[1], y0 += dL[0], once per
//                        row above it), walks its row pixel by pixel with the reference's running float sums, and leaves 8 row values in LDS.  The 72 band sums are
//                        each ONE lane's fold over at most 21 consecutive rows in row order — the order in which the reference's row loop adds into a band, since a
//                        row feeds its own band and the two beside it.  Lane 0 runs the tail (dv_lbd_finish), 32 lanes make the bytes.  No tree, no atomics.
//   lbd_select_kernel    ONE workgroup, a thread per line: Detect's length and mask test, survivors ranked in line order by ballot + per-wave counts, then lines, rows
//                        and src written at their ranks.
#include "dv_ctx.h"
#include "lbd_host.h"
#include <string>
#include <vector>

namespace {

constexpr int LM = DV_LINE_MAX, GT_W = 64, GT_H = 16, RAW_W = GT_W + 6, RAW_H = GT_H + 6, RAW_P = 72, BL_W = GT_W + 2, BL_H = GT_H + 2;
constexpr int SEL_THREADS = 512, SEL_WAVES = SEL_THREADS / 64;
static_assert(SEL_THREADS == LM, "a thread per line");

__global__ __launch_bounds__(256) void lbd_grad_kernel(const uint8_t* __restrict__ img, int pitch, int w, int h, int16_t* __restrict__ dx, int16_t* __restrict__ dy) {
    __shared__ uint8_t s_raw[RAW_H * RAW_P];
    __shared__ uint8_t s_bl[BL_H][BL_W];
    const int tid = threadIdx.x, x0 = blockIdx.x * GT_W, y0 = blockIdx.y * GT_H;
    for (int i = tid; i < RAW_H * RAW_P; i += 256) {
        const int r = i / RAW_P, c = i - r * RAW_P;
        if (c < RAW_W) s_raw[i] = img[(size_t)dv_lbd_reflect101(y0 - 3 + r, h) * pitch + dv_lbd_reflect101(x0 - 3 + c, w)];
    }
    __syncthreads();
    for (int i = tid; i < BL_H * BL_W; i += 256) {
        const int r = i / BL_W, c = i - r * BL_W;
        const int lx = x0 - 1 + c, ly = y0 - 1 + r;
        int v = 0;
        if (lx >= -1 && lx <= w && ly >= -1 && ly <= h) {
            const int rx = dv_lbd_reflect101(lx, w), ry = dv_lbd_reflect101(ly, h);      // Sobel's border: blurred(-1) = blurred(1)
            const uint8_t* p = &s_raw[(ry - (y0 - 3)) * RAW_P + (rx - (x0 - 3))];
            int acc = 0;
            for (int j = -2; j <= 2; ++j) {
                int row = 0;
                for (int k = -2; k <= 2; ++k) row += DV_LBD_BLUR_W[k + 2] * (int)p[j * RAW_P + k];
                acc += DV_LBD_BLUR_W[j + 2] * row;
            }
            v = (acc + 32768) >> 16;
        }
        s_bl[r][c] = (uint8_t)v;
    }
    __syncthreads();
    for (int i = tid; i < GT_H * GT_W; i += 256) {
        const int r = i / GT_W, c = i - r * GT_W;
        const int x = x0 + c, y = y0 + r;
        if (x >= w || y >= h) continue;
        const int a0 = s_bl[r][c], b0 = s_bl[r][c + 1], c0 = s_bl[r][c + 2];
        const int a1 = s_bl[r + 1][c], c1 = s_bl[r + 1][c + 2];
        const int a2 = s_bl[r + 2][c], b2 = s_bl[r + 2][c + 1], c2 = s_bl[r + 2][c + 2];
        dx[(size_t)y * w + x] = (int16_t)((c0 - a0) + 2 * (c1 - a1) + (c2 - a2));
        dy[(size_t)y * w + x] = (int16_t)((a2 + 2 * b2 + c2) - (a0 + 2 * b0 + c0));
    }
}

__global__ __launch_bounds__(64) void lbd_describe_kernel(const int16_t* __restrict__ dxi, const int16_t* __restrict__ dyi, int w, int h, const DvLbdLine* __restrict__ lines, int n,
                                                          DvLbdTabs T, float* __restrict__ fdesc, uint8_t* __restrict__ desc) {
    __shared__ float s_row[DV_LBD_ROWS][8];
    __shared__ float s_band[8][DV_LBD_BANDS];
    __shared__ float s_des[DV_LBD_FLOATS];
    const int li = blockIdx.x, lane = threadIdx.x;
    if (li >= n) return;
    const DvLbdLine L = lines[li];
    if (lane < DV_LBD_ROWS) {
        const float c = L.c, s = L.s, o0 = -s, o1 = c;                     // dL, dO (:1130-1135)
        const int len = (int16_t)L.npix, half_w = (int16_t)((len - 1) / 2), half_h = (DV_LBD_ROWS - 1) / 2, wmax = w - 1, hmax = h - 1;
        const float mx = (float)(0.5 * (double)(L.k.sx + L.k.ex)), my = (float)(0.5 * (double)(L.k.sy + L.k.ey));
        float x0 = -c * (float)half_w + s * (float)half_h + mx;            // (:1138-1139)
        float y0 = -s * (float)half_w - c * (float)half_h + my;
        for (int r = 0; r < lane; ++r) { x0 -= s; y0 += c; }               // (:1186-1187), once per row above this one
        float x = x0, y = y0, pl = 0, nl = 0, po = 0, no = 0;
        for (int k = 0; k < len; ++k) {
            const int xc = dv_lbd_coord(x, wmax), yc = dv_lbd_coord(y, hmax);
            const size_t at = (size_t)yc * w + xc;
            const float gx = (float)dxi[at], gy = (float)dyi[at];
            const float gl = gx * c + gy * s, go = gx * o0 + gy * o1;
            if (gl > 0) pl += gl; else nl -= gl;
            if (go > 0) po += go; else no -= go;
            x += c; y += s;
        }
        const float g = T.g[lane];
        pl = g * pl; nl = g * nl; po = g * po; no = g * no;
        float* o = s_row[lane];
        o[0] = pl; o[1] = nl; o[2] = pl * pl; o[3] = nl * nl; o[4] = po; o[5] = no; o[6] = po * po; o[7] = no * no;
    }
    __syncthreads();
    for (int idx = lane; idx < DV_LBD_FLOATS; idx += 64) {
        const int q = idx / DV_LBD_BANDS, b = idx - q * DV_LBD_BANDS;
        const bool sq = (q & 2) != 0;
        const int lo = b > 0 ? DV_LBD_BAND_W * (b - 1) : 0, hi = b + 2 < DV_LBD_BANDS ? DV_LBD_BAND_W * (b + 2) : DV_LBD_ROWS;
        float acc = 0;
        for (int r = lo; r < hi; ++r) {
            const float cf = T.l[r - DV_LBD_BAND_W * b + DV_LBD_BAND_W], v = s_row[r][q];      // own band: l[r % 7 + 7]; the band below feeds up with l[r % 7], the band above down with l[r % 7 + 14]
            acc += sq ? cf * cf * v : cf * v;
        }
        s_band[q][b] = acc;
    }
    __syncthreads();
    if (lane == 0) dv_lbd_finish(s_band, s_des);
    __syncthreads();
    for (int i = lane; i < DV_LBD_FLOATS; i += 64) fdesc[(size_t)li * DV_LBD_FLOATS + i] = s_des[i];
    if (lane < DV_LINE_DESC_BYTES) desc[(size_t)li * DV_LINE_DESC_BYTES + lane] = dv_lbd_byte(s_des, lane);
}

__global__ __launch_bounds__(SEL_THREADS) void lbd_select_kernel(const DvLbdLine* __restrict__ lines, const uint32_t* __restrict__ desc, int n, float min_length,
                                                                 const uint8_t* __restrict__ mask, int mask_pitch, int w, int h,
                                                                 dv_key_line* __restrict__ o_line, uint32_t* __restrict__ o_desc, int* __restrict__ o_hdr) {
    __shared__ int s_w[SEL_WAVES];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    dv_key_line k{};
    bool keep = false;
    if (t < n) { k = lines[t].k; keep = dv_lbd_keep(k, min_length, mask, mask_pitch, w, h); }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) s_w[wv] = __popcll(b);
    __syncthreads();
    int off = 0, total = 0;
    for (int i = 0; i < SEL_WAVES; ++i) { const int c = s_w[i]; if (i < wv) off += c; total += c; }
    if (keep) {
        const int pos = off + __popcll(b & ((1ull << lane) - 1));
        o_line[pos] = k;
        for (int i = 0; i < DV_LINE_DESC_BYTES / 4; ++i) o_desc[(size_t)pos * (DV_LINE_DESC_BYTES / 4) + i] = desc[(size_t)t * (DV_LINE_DESC_BYTES / 4) + i];
        o_hdr[DV_LBD_O_WORDS + pos] = t;
    }
    if (t == 0) o_hdr[DV_LBD_O_NKEPT] = total;
}

}  // namespace

struct LbdSet {      // one image's buffers: cam 0 / 1
    DevBuf img, mask, grad, lines, fdesc, desc, o_line, o_desc, o_hdr;
    PinBuf pinned_in;       // DvLbdLine[DV_LINE_MAX], then the fetched key lines and num_pixels of a DV_MEM_DEVICE frame
    PinBuf pinned_out;      // DV_LBD_OUT_BYTES
    StageSlot slot;
    int w = 0, h = 0, n = 0;
    bool have = false;
};
static constexpr size_t PIN_LINES = (size_t)LM * sizeof(DvLbdLine), PIN_KEYS = (size_t)LM * sizeof(dv_key_line), PIN_IN = PIN_LINES + PIN_KEYS + (size_t)LM * 4;

struct LbdStage { LbdSet set[2]; DvLbdTabs tabs{}; bool tabs_ready = false; };

void dv_stage_delete(LbdStage* p) { delete p; }

static int lbd_ensure(dv_ctx* ctx, LbdSet& b, int w, int h) {
    DV_CHECK(b.pinned_in.ensure(PIN_IN));
    DV_CHECK(b.pinned_out.ensure(DV_LBD_OUT_BYTES));
    DV_CHECK(b.grad.ensure((size_t)w * h * 4));                     // dx | dy, int16, rows of w
    DV_CHECK(b.lines.ensure(PIN_LINES));
    DV_CHECK(b.fdesc.ensure((size_t)LM * DV_LBD_FLOATS * 4));
    DV_CHECK(b.desc.ensure((size_t)LM * DV_LINE_DESC_BYTES));
    DV_CHECK(b.o_line.ensure(PIN_KEYS));
    DV_CHECK(b.o_desc.ensure((size_t)LM * DV_LINE_DESC_BYTES));
    DV_CHECK(b.o_hdr.ensure(DV_LBD_OUT_BYTES));
    return 0;
}

extern "C" {

int dv_lbd_check(int w, int h, int stride, const dv_key_line* lines, const int32_t* num_pixels, int n, int lines_mem, const uint8_t* mask, int mask_stride) {
    dv_ctx* ctx = nullptr;
    if (const char* why = dv_lbd_check_host(w, h, stride, lines, num_pixels, n, lines_mem, mask, mask_stride)) DV_FAIL(std::string("dv_lbd_check: ") + why);
    return 0;
}

int dv_lbd_num_pixels(const dv_key_line* lines, int n, int32_t* out) {
    dv_ctx* ctx = nullptr;
    if (n < 0 || (n > 0 && (!lines || !out))) DV_FAIL("dv_lbd_num_pixels: bad arguments");
    for (int i = 0; i < n; ++i) out[i] = dv_lbd_npix(lines[i].sx, lines[i].sy, lines[i].ex, lines[i].ey);
    return 0;
}

int dv_lbd_describe_enqueue(dv_ctx* ctx, int cam, const uint8_t* image, int stride, int w, int h, int image_mem, const dv_key_line* lines, const int32_t* num_pixels, int n,
                            int lines_mem, const uint8_t* mask, int mask_stride, float min_length) {
    if (!ctx) return -1;
    if (cam != 0 && cam != 1) DV_FAIL("dv_lbd_describe_enqueue: cam must be 0 or 1");
    if (!image) DV_FAIL("dv_lbd_describe_enqueue: null image");
    if (!dv_mem_known(image_mem)) DV_FAIL("dv_lbd_describe_enqueue: unknown memory kind");
    if (const char* why = dv_lbd_check_host(w, h, stride, lines, num_pixels, n, lines_mem, mask, mask_stride)) DV_FAIL(std::string("dv_lbd_describe_enqueue: ") + why);
    if (!(min_length == min_length)) DV_FAIL("dv_lbd_describe_enqueue: min_length is NaN");
    if (!ctx->lbd) ctx->lbd = new LbdStage();
    LbdStage& S = *ctx->lbd;
    LbdSet& b = S.set[cam];
    if (b.slot.open(ctx, "dv_lbd_describe_enqueue: previous frame of this cam not collected")) return -1;
    if (!S.tabs_ready) { dv_lbd_tables(&S.tabs); S.tabs_ready = true; }
    if (lbd_ensure(ctx, b, w, h)) return -1;
    hipStream_t s = ctx->stream;
    // the lines: dL is computed on the host, so a frame whose lines are in device memory is fetched first (<= 14 KB); its values are checked here
    const dv_key_line* hk = lines; const int32_t* hn = num_pixels;
    if (n > 0 && lines_mem == DV_MEM_DEVICE) {
        dv_key_line* fk = (dv_key_line*)(b.pinned_in.p + PIN_LINES); int32_t* fn = (int32_t*)(b.pinned_in.p + PIN_LINES + PIN_KEYS);
        DV_CHECK(hipMemcpyAsync(fk, lines, (size_t)n * sizeof(dv_key_line), hipMemcpyDeviceToHost, s));
        if (num_pixels) DV_CHECK(hipMemcpyAsync(fn, num_pixels, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        DV_CHECK(hipStreamSynchronize(s));
        hk = fk; hn = num_pixels ? fn : nullptr;
        if (const char* why = dv_lbd_values_check_host(w, h, hk, hn, n)) DV_FAIL(std::string("dv_lbd_describe_enqueue: ") + why);
    }
    DvLbdLine* pl = (DvLbdLine*)b.pinned_in.p;
    for (int i = 0; i < n; ++i) pl[i] = dv_lbd_line(hk[i], hn ? hn[i] : dv_lbd_npix(hk[i].sx, hk[i].sy, hk[i].ex, hk[i].ey));
    DvRows im, mk{};          // device and pinned memory in place, pageable memory through the set's own buffers
    if (dv_stage_rows(ctx, b.img, image, w, h, stride, dv_in_place_device_or_pinned(image_mem), s, &im)) return -1;
    if (mask && dv_stage_rows(ctx, b.mask, mask, w, h, mask_stride, dv_in_place_device_or_pinned(image_mem), s, &mk)) return -1;
    int16_t* dx = (int16_t*)b.grad.p; int16_t* dy = dx + (size_t)w * h;
    hipError_t e;
    {
        StageScope sc_t(ctx, "lbd_describe");
        e = n > 0 ? dv_copy_async(b.lines.p, b.pinned_in.p, (size_t)n * sizeof(DvLbdLine), s) : hipSuccess;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(lbd_grad_kernel, dim3((w + GT_W - 1) / GT_W, (h + GT_H - 1) / GT_H), dim3(256), 0, s, im.p, im.pitch, w, h, dx, dy);
            if (n > 0) hipLaunchKernelGGL(lbd_describe_kernel, dim3(n), dim3(64), 0, s, dx, dy, w, h, (const DvLbdLine*)b.lines.p, n, S.tabs, (float*)b.fdesc.p, (uint8_t*)b.desc.p);
            hipLaunchKernelGGL(lbd_select_kernel, dim3(1), dim3(SEL_THREADS), 0, s, (const DvLbdLine*)b.lines.p, (const uint32_t*)b.desc.p, n, min_length, mk.p, mk.pitch, w, h,
                               (dv_key_line*)b.o_line.p, (uint32_t*)b.o_desc.p, (int*)b.o_hdr.p);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = dv_copy_async(b.pinned_out.p, b.o_hdr.p, (size_t)(DV_LBD_O_WORDS + n) * 4, s);      // the count and at most n indices
    }
    if (b.slot.close(ctx, e, s)) return -1;          // (kernels read the caller's arrays in place)
    b.w = w; b.h = h; b.n = n; b.have = true;
    return 0;
}

int dv_lbd_describe_collect(dv_ctx* ctx, int cam, int* n_kept, int32_t* src, const dv_key_line** dev_lines, const uint8_t** dev_desc, dv_key_line* host_lines, uint8_t* host_desc) {
    if (!ctx) return -1;
    if (cam != 0 && cam != 1) DV_FAIL("dv_lbd_describe_collect: cam must be 0 or 1");
    if (!n_kept) DV_FAIL("dv_lbd_describe_collect: null n_kept");
    if (!ctx->lbd || !ctx->lbd->set[cam].slot.pending) DV_FAIL("dv_lbd_describe_collect: nothing enqueued on this cam");
    LbdSet& b = ctx->lbd->set[cam];
    if (b.slot.wait(ctx)) return -1;
    const int32_t* o = (const int32_t*)b.pinned_out.p;
    const int nk = o[DV_LBD_O_NKEPT];
    if (nk < 0 || nk > b.n) DV_FAIL("dv_lbd_describe_collect: corrupt counter");
    *n_kept = nk;
    if (src && nk > 0) std::memcpy(src, o + DV_LBD_O_WORDS, (size_t)nk * 4);
    if (dev_lines) *dev_lines = (const dv_key_line*)b.o_line.p;
    if (dev_desc) *dev_desc = (const uint8_t*)b.o_desc.p;
    if (nk > 0 && (host_lines || host_desc)) {
        DV_CHECK(hipSetDevice(ctx->cfg.device));
        if (host_lines) DV_CHECK(hipMemcpyAsync(host_lines, b.o_line.p, (size_t)nk * sizeof(dv_key_line), hipMemcpyDeviceToHost, ctx->stream));
        if (host_desc) DV_CHECK(hipMemcpyAsync(host_desc, b.o_desc.p, (size_t)nk * DV_LINE_DESC_BYTES, hipMemcpyDeviceToHost, ctx->stream));
        DV_CHECK(hipStreamSynchronize(ctx->stream));
    }
    if (ctx->timing && !ctx->lbd->set[cam ^ 1].slot.pending) dv_harvest_timers(ctx, ctx->stream);      // (the stream is idle only when the other cam has nothing in flight)
    return 0;
}

int dv_lbd_debug(dv_ctx* ctx, int cam, int16_t* dx_out, int16_t* dy_out, float* float_desc_out) {
    if (!ctx) return -1;
    if (cam != 0 && cam != 1) DV_FAIL("dv_lbd_debug: cam must be 0 or 1");
    if (!ctx->lbd || !ctx->lbd->set[cam].have) DV_FAIL("dv_lbd_debug: no frame was enqueued on this cam");
    LbdSet& b = ctx->lbd->set[cam];
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const size_t px = (size_t)b.w * b.h;
    if (dx_out) DV_CHECK(hipMemcpyAsync(dx_out, b.grad.p, px * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (dy_out) DV_CHECK(hipMemcpyAsync(dy_out, (int16_t*)b.grad.p + px, px * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (float_desc_out && b.n > 0) DV_CHECK(hipMemcpyAsync(float_desc_out, b.fdesc.p, (size_t)b.n * DV_LBD_FLOATS * 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
