// dv_ops.hip — the operator-level entries of the C ABI (include/dvins.h): one reference operator per call on the ctx's scratch buffers (s0 .. s4, opA / opB), synchronous.
// The parity tests drive the kernels through them.  Images come in through the staging rule (dv_stage_rows, dv_ctx.h) under the "device only" policy: pinned memory is
// copied like pageable memory.
#include "dv_ctx.h"
#include "viode_host.h"
#include <optional>

// copies `bytes` from user memory (host or device) into a ctx scratch buffer on the device
static int stage_in(dv_ctx* ctx, DevBuf& b, const void* src, size_t bytes, int mem) {
    DV_CHECK(b.ensure(bytes ? bytes : 1));
    if (bytes) DV_CHECK(hipMemcpyAsync(b.p, src, bytes, mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
static int stage_out(dv_ctx* ctx, void* dst, const void* src, size_t bytes, int mem) {
    if (bytes) DV_CHECK(hipMemcpyAsync(dst, src, bytes, mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

// The four LK operators in one body: prepare() builds the two images' pyramids (non-zero: failed); the points of image A go to s0, the initial points of image B (use_initial)
// to s1, the status bytes to s2; launch(pts_a, pts_b, status) enqueues the tracker on the ctx's stream; both results go back and the stream is drained.  timer: the
// stage timer that starts in front of the launch (nullptr: none)
template <class Prepare, class Launch>
static int lk_op(dv_ctx* ctx, Prepare prepare, Launch launch, const char* timer, const float* pts_a, int n, int use_initial, float* pts_b, uint8_t* status, int mem) {
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (prepare()) return -1;
    if (stage_in(ctx, ctx->s0, pts_a, (size_t)n * 8, mem)) return -1;
    if (use_initial) { if (stage_in(ctx, ctx->s1, pts_b, (size_t)n * 8, mem)) return -1; }
    else DV_CHECK(ctx->s1.ensure((size_t)n * 8));
    DV_CHECK(ctx->s2.ensure(n));
    std::optional<StageScope> sc;
    if (timer) sc.emplace(ctx, timer);
    launch((const float2*)ctx->s0.p, (float2*)ctx->s1.p, (uint8_t*)ctx->s2.p);
    DV_CHECK(hipGetLastError());
    if (stage_out(ctx, pts_b, ctx->s1.p, (size_t)n * 8, mem)) return -1;
    if (stage_out(ctx, status, ctx->s2.p, n, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" {

int dv_lk(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride, const float* pts_a, int n, int max_level,
          int iters, double eps, int use_initial, float* pts_b, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img_a || !img_b || !pts_a || n <= 0) DV_FAIL("dv_lk: empty input (reference throws std::runtime_error, feature_utils.cpp:39-41)");
    if (max_level < 0 || max_level > 3) DV_FAIL("dv_lk: max_level must be in [0,3]");
    iters = std::min(std::max(iters, 0), 100);
    eps = std::min(std::max(eps, 0.), 10.);
    return lk_op(ctx,
        [&] { return dv_build_pyramids(ctx, ctx->opA, nullptr, img_a, nullptr, w, h, stride, mem, max_level) || dv_build_pyramids(ctx, ctx->opB, nullptr, img_b, nullptr, w, h, stride, mem, max_level); },
        [&](const float2* a, float2* b, uint8_t* st) {
            const int ml = std::min(ctx->opA.pyr.levels, ctx->opB.pyr.levels) - 1;
            dv_launch_lk_generic(ctx->opA.pyr, ctx->opB.pyr, a, n, ml, iters, eps * eps, use_initial, b, st, ctx->stream);
        }, nullptr, pts_a, n, use_initial, pts_b, status, mem);
}

int dv_track_by_lk(dv_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride, const float* pts1, int n,
                   int flow_back, float dist_thresh, float* pts2, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img1 || !img2 || !pts1 || n <= 0) DV_FAIL("dv_track_by_lk: FeatureTrackByLK() input wrong, received at least one of parameter are empty");
    return lk_op(ctx,
        [&] { return dv_build_pyramids(ctx, ctx->opA, &ctx->opB, img1, img2, w, h, stride, mem, 3); },
        [&](const float2* a, float2* b, uint8_t* st) { dv_launch_lk_track(ctx->opA.pyr, ctx->opB.pyr, a, nullptr, n, flow_back, dist_thresh, b, st, ctx->stream); },
        "op_lk_track", pts1, n, 0, pts2, status, mem);
}

// cv::cuda::SparsePyrLKOpticalFlow::calc (use_initial: pts_b holds the initial flow) and FeatureTrackByLKGpu, operator forms for the parity tests
static int lk_cuda_prepare(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride, int mem, int max_level) {
    if (dv_build_pyramids(ctx, ctx->opA, &ctx->opB, img_a, img_b, w, h, stride, mem, 0)) return -1;          // level 0 only (pitched copies)
    return dv_build_cuda_pyramids(ctx, ctx->leftc[0], &ctx->leftc[1], ctx->opA.pyr, &ctx->opB.pyr, w, h, max_level);
}
int dv_lk_cuda(dv_ctx* ctx, const uint8_t* img_a, const uint8_t* img_b, int w, int h, int stride, const float* pts_a, int n, int max_level, int iters, int use_initial,
               float* pts_b, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img_a || !img_b || !pts_a || n <= 0) DV_FAIL("dv_lk_cuda: empty input");
    if (max_level < 0 || max_level > 3 || iters < 0 || iters > 100) DV_FAIL("dv_lk_cuda: max_level must be in [0,3], iters in [0,100]");
    if (ctx->pending || ctx->have_prev) DV_FAIL("dv_lk_cuda: operator calls need a ctx that is not tracking a sequence (its pyramids are used as scratch)");
    return lk_op(ctx,
        [&] { return lk_cuda_prepare(ctx, img_a, img_b, w, h, stride, mem, max_level); },
        [&](const float2* a, float2* b, uint8_t* st) {
            const int ml = std::min(ctx->leftc[0].pyr.levels, ctx->leftc[1].pyr.levels) - 1;
            dv_launch_lk_cuda_generic(ctx->leftc[0].pyr, ctx->leftc[1].pyr, a, n, ml, iters, use_initial, b, st, ctx->stream);
        }, nullptr, pts_a, n, use_initial, pts_b, status, mem);
}
int dv_track_by_lk_gpu(dv_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride, const float* pts1, int n, int flow_back, float* pts2, uint8_t* status, int mem) {
    if (!ctx) return -1;
    if (!img1 || !img2 || !pts1 || n <= 0) DV_FAIL("dv_track_by_lk_gpu: flowTrack() input wrong, received at least one of parameter are empty");
    if (ctx->pending || ctx->have_prev) DV_FAIL("dv_track_by_lk_gpu: operator calls need a ctx that is not tracking a sequence (its pyramids are used as scratch)");
    return lk_op(ctx,
        [&] { return lk_cuda_prepare(ctx, img1, img2, w, h, stride, mem, 3); },
        [&](const float2* a, float2* b, uint8_t* st) { dv_launch_lk_cuda_track(ctx->leftc[0].pyr, ctx->leftc[1].pyr, a, nullptr, n, flow_back, 1.0f, b, st, ctx->stream); },
        nullptr, pts1, n, 0, pts2, status, mem);
}

// cv::pyrDown / cuda::pyrDown (rn_even: the level step of the GPU tracker's pyramid) on an 8-bit image; dst is ((w+1)/2) x ((h+1)/2), tightly packed
static int pyr_down_op(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, int mem, int rn_even) {
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DvRows im;
    if (dv_stage_rows(ctx, ctx->s0, src, w, h, stride, dv_in_place_device(mem), ctx->stream, &im, 64)) return -1;
    const int dw = (w + 1) / 2, dh = (h + 1) / 2, dp = align_up(dw, 16);
    DV_CHECK(ctx->s1.ensure((size_t)dp * dh + 64));
    dv_launch_pyr_down2(im.p, nullptr, w, h, im.pitch, (uint8_t*)ctx->s1.p, nullptr, dp, nullptr, nullptr, 0, ctx->stream, rn_even);
    DV_CHECK(hipGetLastError());
    if (dv_unstage_rows(ctx, dst, dw, ctx->s1.p, dp, dw, dh, mem, ctx->stream)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}
int dv_pyr_down(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst) DV_FAIL("dv_pyr_down: null argument");
    return pyr_down_op(ctx, src, w, h, stride, dst, mem, 0);
}
int dv_pyr_down_cuda(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst) DV_FAIL("dv_pyr_down_cuda: null argument");
    return pyr_down_op(ctx, src, w, h, stride, dst, mem, 1);
}

static int min_eigen_rule(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem, int rule) {
    if (!ctx) return -1;
    if (!img || !eig) DV_FAIL("dv_min_eigen: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DvRows im;
    if (dv_stage_rows(ctx, ctx->s0, img, w, h, stride, dv_in_place_device(mem), ctx->stream, &im, 64)) return -1;
    if (dv_ensure_cand(ctx, w, h)) return -1;
    float* d_eig = eig;
    if (mem != DV_MEM_DEVICE) { DV_CHECK(ctx->s1.ensure((size_t)w * h * 4)); d_eig = (float*)ctx->s1.p; }
    DV_CHECK(hipMemsetAsync(ctx->n_cand, 0, 8, ctx->stream));     // n_cand + max_ord
    GfttTileArgs a{};
    a.img = im.p; a.w = w; a.h = h; a.pitch = im.pitch; a.eig_out = d_eig; a.eig_pitch = w;
    a.cand = (DvCand*)ctx->cand_buf.p; a.cand_cap = ctx->cand_cap; a.n_cand = ctx->n_cand; a.max_ord = ctx->max_ord; a.rule = rule;
    dv_launch_gftt_tile(a, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (mem != DV_MEM_DEVICE) DV_CHECK(hipMemcpyAsync(eig, d_eig, (size_t)w * h * 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_min_eigen(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem) { return min_eigen_rule(ctx, img, w, h, stride, eig, mem, DV_GFTT_RULE_CPU); }
int dv_min_eigen_cuda(dv_ctx* ctx, const uint8_t* img, int w, int h, int stride, float* eig, int mem) { return min_eigen_rule(ctx, img, w, h, stride, eig, mem, DV_GFTT_RULE_CUDA); }

static int gftt_rule_op(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride, int max_n, double quality,
                        double min_dist, float* out_xy, int* n_out, int mem, int rule) {
    if (!ctx) return -1;
    if (!img || !out_xy || !n_out) DV_FAIL("dv_gftt: null argument");
    if (!(quality > 0)) DV_FAIL("dv_gftt: qualityLevel must be > 0");
    if (min_dist < 0) DV_FAIL("dv_gftt: minDistance must be >= 0");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DvRows im, mk{};
    if (dv_stage_rows(ctx, ctx->s0, img, w, h, stride, dv_in_place_device(mem), ctx->stream, &im, 64)) return -1;
    if (mask_or_null && dv_stage_rows(ctx, ctx->s3, mask_or_null, w, h, stride, dv_in_place_device(mem), ctx->stream, &mk, 64)) return -1;
    if (dv_ensure_cand(ctx, w, h)) return -1;
    DV_CHECK(ctx->s1.ensure((size_t)DV_MAX_FEATS * 8 + 16));
    float2* d_out = (float2*)ctx->s1.p; int* d_n = (int*)((uint8_t*)ctx->s1.p + (size_t)DV_MAX_FEATS * 8);
    DV_CHECK(hipMemsetAsync(ctx->n_cand, 0, 12, ctx->stream));    // n_cand, max_ord, err_flag
    GfttTileArgs a{};
    a.img = im.p; a.w = w; a.h = h; a.pitch = im.pitch; a.in_mask = mk.p; a.mask_pitch = mk.pitch;
    a.cand = (DvCand*)ctx->cand_buf.p; a.cand_cap = ctx->cand_cap; a.n_cand = ctx->n_cand; a.max_ord = ctx->max_ord; a.rule = rule;
    dv_launch_gftt_tile(a, ctx->stream);
    GfttSelectArgs sa{};
    sa.cand = (const DvCand*)ctx->cand_buf.p; sa.n_cand = ctx->n_cand; sa.cand_cap = ctx->cand_cap; sa.max_ord = ctx->max_ord;
    sa.w = w; sa.h = h; sa.quality = quality; sa.min_dist = min_dist; sa.max_n_host = max_n; sa.n_feat = nullptr;
    sa.out_xy = d_out; sa.n_out = d_n; sa.has_tr = 0; sa.err_flag = ctx->err_flag; sa.rule = rule;
    if (dv_launch_gftt_select(sa, ctx->stream)) DV_FAIL("gftt_select: cannot set dynamic LDS size");
    DV_CHECK(hipGetLastError());
    int n = 0, ef = 0;
    DV_CHECK(hipMemcpyAsync(&n, d_n, 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipMemcpyAsync(&ef, ctx->err_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    if (ef) { DV_CHECK(hipMemsetAsync(ctx->err_flag, 0, 4, ctx->stream)); DV_FAIL("dv_gftt: device error flags=" + std::to_string(ef)); }
    if (stage_out(ctx, out_xy, d_out, (size_t)n * 8, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    *n_out = n;
    return 0;
}

int dv_gftt(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride, int max_n, double quality,
            double min_dist, float* out_xy, int* n_out, int mem) {
    return gftt_rule_op(ctx, img, mask_or_null, w, h, stride, max_n, quality, min_dist, out_xy, n_out, mem, DV_GFTT_RULE_CPU);
}
int dv_gftt_cuda(dv_ctx* ctx, const uint8_t* img, const uint8_t* mask_or_null, int w, int h, int stride, int max_n, double quality,
                 double min_dist, float* out_xy, int* n_out, int mem) {
    return gftt_rule_op(ctx, img, mask_or_null, w, h, stride, max_n, quality, min_dist, out_xy, n_out, mem, DV_GFTT_RULE_CUDA);
}

// viode_mask_kernel on one label image in host memory; every output goes to host memory
int dv_viode_mask(dv_ctx* ctx, const uint8_t* seg_bgr, int w, int h, int stride, const uint32_t* dyn_keys, int nkeys, uint8_t* merge_mask, uint8_t* inv_merge_mask,
                  uint32_t* key_image, int32_t* boxes) {
    if (!ctx) return -1;
    if (!seg_bgr || !dyn_keys || !merge_mask || !inv_merge_mask || !boxes || w <= 0 || h <= 0 || stride < 3 * w) DV_FAIL("dv_viode_mask: bad argument");
    if (nkeys < 1 || nkeys > 64) DV_FAIL("dv_viode_mask: 1..64 dynamic keys");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    const int mp = align_up(w, 16);
    DV_CHECK(ctx->s1.ensure((size_t)mp * h)); DV_CHECK(ctx->s2.ensure((size_t)mp * h));      // merge, inverse
    DV_CHECK(ctx->s3.ensure((size_t)4 * w * h + 4096));                    // key image | keys | boxes
    DV_CHECK(ctx->s4.ensure(4096));
    uint32_t* d_keys = (uint32_t*)ctx->s4.p; int32_t* d_box = (int32_t*)((uint8_t*)ctx->s4.p + 1024);
    int32_t init[256];
    dv_boxes_init(init);
    DvRows seg;                                                            // label image
    if (dv_stage_rows(ctx, ctx->s0, seg_bgr, (size_t)3 * w, h, stride, false, s, &seg)) return -1;
    DV_CHECK(hipMemcpyAsync(d_keys, dyn_keys, 4 * (size_t)nkeys, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync(d_box, init, 16 * (size_t)nkeys, hipMemcpyHostToDevice, s));
    DV_CHECK(hipStreamSynchronize(s));                                     // init[] is a stack object
    dv_launch_viode_mask(seg.p, w, h, seg.pitch, d_keys, nkeys, (uint8_t*)ctx->s1.p, (uint8_t*)ctx->s2.p, mp, key_image ? (uint32_t*)ctx->s3.p : nullptr, d_box, s);
    DV_CHECK(hipGetLastError());
    if (dv_unstage_rows(ctx, merge_mask, w, ctx->s1.p, mp, w, h, DV_MEM_HOST, s)) return -1;
    if (dv_unstage_rows(ctx, inv_merge_mask, w, ctx->s2.p, mp, w, h, DV_MEM_HOST, s)) return -1;
    if (key_image) DV_CHECK(hipMemcpyAsync(key_image, ctx->s3.p, (size_t)4 * w * h, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipMemcpyAsync(boxes, d_box, 16 * (size_t)nkeys, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < nkeys; ++k) if (boxes[4 * k + 1] < 0) { boxes[4 * k] = boxes[4 * k + 2] = -1; boxes[4 * k + 3] = -1; }      // key not present
    return 0;
}

int dv_bgr2gray(dv_ctx* ctx, const uint8_t* bgr, int w, int h, int stride, uint8_t* gray, int mem) {
    if (!ctx) return -1;
    if (!bgr || !gray || w <= 0 || h <= 0 || stride < 3 * w) DV_FAIL("dv_bgr2gray: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    DvRows src;
    if (dv_stage_rows(ctx, ctx->s3, bgr, (size_t)3 * w, h, stride, dv_in_place_device(mem), s, &src)) return -1;
    const int dp = align_up(w, 16);
    DV_CHECK(ctx->s4.ensure((size_t)dp * h));
    dv_launch_bgr2gray(src.p, nullptr, w, h, src.pitch, (uint8_t*)ctx->s4.p, nullptr, dp, s);
    DV_CHECK(hipGetLastError());
    if (dv_unstage_rows(ctx, gray, w, ctx->s4.p, dp, w, h, mem, s)) return -1;
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

int dv_remap(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, int channels, const int16_t* map1_xy, const uint16_t* map2, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst || !map1_xy || !map2 || w <= 0 || h <= 0 || (channels != 1 && channels != 3) || stride < channels * w) DV_FAIL("dv_remap: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    DvRows im;
    if (dv_stage_rows(ctx, ctx->s3, src, (size_t)channels * w, h, stride, dv_in_place_device(mem), s, &im)) return -1;
    const size_t npx = (size_t)w * h;
    DV_CHECK(ctx->s2.ensure(6 * npx));
    DV_CHECK(hipMemcpyAsync(ctx->s2.p, map1_xy, 4 * npx, hipMemcpyHostToDevice, s));
    DV_CHECK(hipMemcpyAsync((uint8_t*)ctx->s2.p + 4 * npx, map2, 2 * npx, hipMemcpyHostToDevice, s));
    const int dp = align_up(channels * w, 16);
    DV_CHECK(ctx->s4.ensure((size_t)dp * h));
    dv_launch_remap(im.p, nullptr, w, h, im.pitch, channels, 0, (const int16_t*)ctx->s2.p, (const uint16_t*)((uint8_t*)ctx->s2.p + 4 * npx), nullptr, nullptr,
                    (uint8_t*)ctx->s4.p, nullptr, dp, s);
    DV_CHECK(hipGetLastError());
    if (dv_unstage_rows(ctx, dst, (size_t)channels * w, ctx->s4.p, dp, (size_t)channels * w, h, mem, s)) return -1;
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

// the discs are drawn into the caller's mask: a host mask travels to s0 and back
int dv_circle_mask(dv_ctx* ctx, uint8_t* mask, int w, int h, int stride, const float* pts_xy, int n, int radius, int mem) {
    if (!ctx) return -1;
    if (!mask || (n > 0 && !pts_xy)) DV_FAIL("dv_circle_mask: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (dv_ensure_hw(ctx, radius)) return -1;
    DvRows m;
    if (dv_stage_rows(ctx, ctx->s0, mask, w, h, stride, dv_in_place_device(mem), ctx->stream, &m)) return -1;
    if (stage_in(ctx, ctx->s1, pts_xy, (size_t)n * 8, mem)) return -1;
    dv_launch_circle_mask((uint8_t*)m.p, w, h, m.pitch, (const float2*)ctx->s1.p, n, radius, (const uint8_t*)ctx->hw_buf.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (!dv_in_place_device(mem) && dv_unstage_rows(ctx, mask, stride, m.p, m.pitch, w, h, mem, ctx->stream)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_erode(dv_ctx* ctx, const uint8_t* src, int w, int h, int stride, int k, uint8_t* dst, int mem) {
    if (!ctx) return -1;
    if (!src || !dst || k < 1) DV_FAIL("dv_erode: bad argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DvRows im;
    if (dv_stage_rows(ctx, ctx->s0, src, w, h, stride, dv_in_place_device(mem), ctx->stream, &im, 64)) return -1;
    const int p = align_up(w, 16);
    DV_CHECK(ctx->s1.ensure((size_t)p * h)); DV_CHECK(ctx->s2.ensure((size_t)p * h));
    dv_launch_erode(im.p, w, h, im.pitch, k, (uint8_t*)ctx->s1.p, p, (uint8_t*)ctx->s2.p, p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (dv_unstage_rows(ctx, dst, mem == DV_MEM_DEVICE ? stride : w, ctx->s2.p, p, w, h, mem, ctx->stream)) return -1;      // a device destination has the source's stride, a host one is tightly packed
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_lift_projective(dv_ctx* ctx, const dv_cam* cam, const float* pts_xy, int n, float* out_xy, int mem) {
    return dv_lift_projective_offset(ctx, cam, pts_xy, n, 0.0, 0.0, out_xy, mem);
}

int dv_lift_projective_offset(dv_ctx* ctx, const dv_cam* cam, const float* pts_xy, int n, double off_x, double off_y, float* out_xy, int mem) {
    if (!ctx) return -1;
    if (!cam || (n > 0 && (!pts_xy || !out_xy))) DV_FAIL("dv_lift_projective: null argument");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (stage_in(ctx, ctx->s0, pts_xy, (size_t)n * 8, mem)) return -1;
    DV_CHECK(ctx->s1.ensure((size_t)std::max(n, 1) * 8));
    dv_launch_lift(*cam, (const float2*)ctx->s0.p, n, off_x, off_y, (float2*)ctx->s1.p, ctx->stream);
    DV_CHECK(hipGetLastError());
    if (stage_out(ctx, out_xy, ctx->s1.p, (size_t)n * 8, mem)) return -1;
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// FrameLines::UndistortedLineEndPoints (line_detector, front end of TrackImageLine): both end points through PinholeCamera::liftProjective; the Line keeps
// them as cv::Point2f, LineFeature widens to double (basic/line_feature.h:31-33)
int dv_undistort_lines(dv_ctx* ctx, const dv_cam* cam, const float* lines_xyxy, int n, double* out_xyxy) {
    if (!ctx) return -1;
    if (!cam || n < 0 || (n > 0 && (!lines_xyxy || !out_xyxy))) DV_FAIL("dv_undistort_lines: bad argument");
    if (n == 0) return 0;
    std::vector<float> un((size_t)4 * n);
    if (dv_lift_projective(ctx, cam, lines_xyxy, 2 * n, un.data(), DV_MEM_HOST)) return -1;
    for (size_t i = 0; i < (size_t)4 * n; ++i) out_xyxy[i] = (double)un[i];
    return 0;
}

} // extern "C"
