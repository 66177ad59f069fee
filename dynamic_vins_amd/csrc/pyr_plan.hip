// pyr_plan.hip — a frame's way into the image pyramids: the plans (copies enqueued, launches described in the job types of the table kernels) and their launches by value.
#include "dv_ctx.h"

// How a frame becomes pyramid level 0, decided here and nowhere else.  Maps and / or BGR frames: a level-0 job (cv::remap, with cvtColor for colour frames, or
// cvtColor alone, straight into level 0; host frames are staged in s3 / s4 first, in rows of align_up(channels * w, 16) bytes).  Gray host frames, and pyramids of
// one level: a pitched copy.  Gray device frames: the level-1 step reads the frame itself and writes the pitched level-0 copy beside level 1 (frame read once).
// The copies are enqueued on s, the launches left to dv_launch_pyramids or a dv_batch round's tables.  undistort: the caller has checked the maps.
int dv_plan_pyramids(dv_ctx* ctx, const DvPyr& a, const DvPyr* b, const uint8_t* img0, const uint8_t* img1, int stride, int mem, bool undistort, hipStream_t s, PyrPlan& P) {
    const int w = a.L[0].w, h = a.L[0].h;
    const bool bgr = (mem & DV_FMT_BGR) != 0, dev = dv_in_place_device(mem & ~DV_FMT_BGR);
    if (!b) img1 = nullptr;
    P.has_l0 = undistort || bgr; P.pair = b != nullptr; P.levels = a.levels;
    if (P.has_l0) {
        const int cn = bgr ? 3 : 1;
        DvLevel0Job& z = P.l0; z = DvLevel0Job{};
        DvRows r0, r1{};
        if (dv_stage_rows(ctx, ctx->s3, img0, (size_t)cn * w, h, stride, dev, s, &r0)) return -1;
        if (b && dv_stage_rows(ctx, ctx->s4, img1, (size_t)cn * w, h, stride, dev, s, &r1)) return -1;
        z.src0 = r0.p; z.src1 = r1.p; z.spitch = r0.pitch;
        z.map0 = undistort ? (const uint8_t*)ctx->undist_buf[0].p : nullptr; z.map1 = (undistort && b) ? (const uint8_t*)ctx->undist_buf[1].p : nullptr;
        z.dst0 = a.L[0].p; z.dst1 = b ? b->L[0].p : nullptr; z.dpitch = a.L[0].pitch;
        z.kind = undistort ? (bgr ? DV_L0_REMAP_BGR : DV_L0_REMAP_GRAY) : DV_L0_BGR;
    } else if (!dev || a.levels == 1) {
        const hipMemcpyKind k = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        DV_CHECK(hipMemcpy2DAsync(a.L[0].p, a.L[0].pitch, img0, stride, w, h, k, s));
        if (b) DV_CHECK(hipMemcpy2DAsync(b->L[0].p, b->L[0].pitch, img1, stride, w, h, k, s));
    }
    for (int l = 1; l < a.levels; ++l) {
        const bool fuse = dev && l == 1 && !P.has_l0;
        DvPyrJob& pj = P.down[l - 1]; pj = DvPyrJob{};
        pj.src0 = fuse ? img0 : a.L[l - 1].p; pj.src1 = b ? (fuse ? img1 : b->L[l - 1].p) : nullptr;
        pj.dst0 = a.L[l].p; pj.dst1 = b ? b->L[l].p : nullptr;
        pj.sw = a.L[l - 1].w; pj.sh = a.L[l - 1].h; pj.spitch = fuse ? stride : a.L[l - 1].pitch; pj.dw = a.L[l].w; pj.dh = a.L[l].h; pj.dpitch = a.L[l].pitch;
        pj.cpy0 = fuse ? a.L[0].p : nullptr; pj.cpy1 = (fuse && b) ? b->L[0].p : nullptr; pj.cpitch = a.L[0].pitch;
    }
    P.apron[0] = a; P.apron[1] = b ? *b : a;      // (one image: the second entry repeats the first — idempotent in a table, not launched by value)
    return 0;
}

// the plan's launches with the single-sequence kernels, every argument by value
void dv_launch_pyramids(const PyrPlan& P, hipStream_t s) {
    const DvLevel0Job& z = P.l0;
    const int w = P.apron[0].L[0].w, h = P.apron[0].L[0].h;
    if (P.has_l0 && z.kind == DV_L0_BGR) dv_launch_bgr2gray(z.src0, z.src1, w, h, z.spitch, z.dst0, z.dst1, z.dpitch, s);
    else if (P.has_l0) {
        const size_t m2off = (size_t)4 * w * h;      // a camera's map block: w * h short2 of map1, then map2
        const int bgr = z.kind == DV_L0_REMAP_BGR;
        dv_launch_remap(z.src0, z.src1, w, h, z.spitch, bgr ? 3 : 1, bgr, (const int16_t*)z.map0, (const uint16_t*)(z.map0 + m2off),
                        (const int16_t*)z.map1, z.map1 ? (const uint16_t*)(z.map1 + m2off) : nullptr, z.dst0, z.dst1, z.dpitch, s);
    }
    for (int l = 1; l < P.levels; ++l) { const DvPyrJob& j = P.down[l - 1]; dv_launch_pyr_down2(j.src0, j.src1, j.sw, j.sh, j.spitch, j.dst0, j.dst1, j.dpitch, j.cpy0, j.cpy1, j.cpitch, s); }
    dv_launch_pyr_apron(P.apron[0], P.pair ? &P.apron[1] : nullptr, s);
}

int dv_build_pyramids(dv_ctx* ctx, PyrSet& P0, PyrSet* P1, const uint8_t* img0, const uint8_t* img1, int w, int h, int stride, int mem, int max_level) {
    DV_CHECK(P0.alloc(w, h, max_level));
    if (P1) DV_CHECK(P1->alloc(w, h, max_level));
    PyrPlan P;
    if (dv_plan_pyramids(ctx, P0.pyr, P1 ? &P1->pyr : nullptr, img0, img1, stride, mem, false, ctx->stream, P)) return -1;
    dv_launch_pyramids(P, ctx->stream);
    DV_CHECK(hipGetLastError());
    return 0;
}

// the pyramid cv::cuda::SparsePyrLKOpticalFlow builds (cuda::pyrDown: round half to even) on top of an existing level 0 (a0 / b0: level 0 of the regular pyramids)
int dv_plan_cuda_pyramids(dv_ctx* ctx, PyrSet& C0, PyrSet* C1, const DvPyr& a0, const DvPyr* b0, int w, int h, int max_level, CudaPyrPlan& P) {
    DV_CHECK(C0.alloc(w, h, max_level, true));
    if (C1) DV_CHECK(C1->alloc(w, h, max_level, true));
    C0.pyr.L[0] = a0.L[0];
    if (C1) C1->pyr.L[0] = b0->L[0];
    P.levels = C0.pyr.levels;
    for (int l = 1; l < P.levels; ++l) {
        const DvLevel& f = C0.pyr.L[l - 1]; const DvLevel& t = C0.pyr.L[l];
        DvPyrJob& pj = P.down[l - 1]; pj = DvPyrJob{};
        pj.src0 = f.p; pj.src1 = C1 ? C1->pyr.L[l - 1].p : nullptr; pj.dst0 = t.p; pj.dst1 = C1 ? C1->pyr.L[l].p : nullptr;
        pj.sw = f.w; pj.sh = f.h; pj.spitch = f.pitch; pj.dw = t.w; pj.dh = t.h; pj.dpitch = t.pitch;
    }
    return 0;
}
void dv_launch_cuda_pyramids(const CudaPyrPlan& P, hipStream_t s) {
    for (int l = 1; l < P.levels; ++l) { const DvPyrJob& j = P.down[l - 1]; dv_launch_pyr_down2(j.src0, j.src1, j.sw, j.sh, j.spitch, j.dst0, j.dst1, j.dpitch, nullptr, nullptr, 0, s, 1); }
}
int dv_build_cuda_pyramids(dv_ctx* ctx, PyrSet& C0, PyrSet* C1, const DvPyr& a0, const DvPyr* b0, int w, int h, int max_level) {
    CudaPyrPlan P;
    if (dv_plan_cuda_pyramids(ctx, C0, C1, a0, b0, w, h, max_level, P)) return -1;
    dv_launch_cuda_pyramids(P, ctx->stream);
    DV_CHECK(hipGetLastError());
    return 0;
}
