// undistort_map.hip — cv::initUndistortRectifyMap(K, D, Mat(), newK, size, CV_16SC2, map1, map2) for the pinhole + radtan(k1, k2, p1, p2)
// cameras of the reference (utils/camera_model.cpp:484,494), and cv::getOptimalNewCameraMatrix in front of it (:483,493).
// OpenCV 3.4 imgproc undistort.cpp / calib3d calibration.cpp, restated (un-vendored: PARITY UNPINNED, DESIGN.md 2 choice U1).
//
// The library walks every row with running sums: _x = i ir[1] + ir[2], _y = i ir[4] + ir[5], _w = i ir[7] + ir[8] at the row's start and
// _x += ir[0], _y += ir[3], _w += ir[6] per pixel, ir = (newK R)^-1.  With R = I: ir[1] = ir[3] = ir[6] = ir[7] = 0, ir[8] = 1, so
//   * _x of pixel (i, j) is ir[2] followed by j ROUNDED additions of ir[0] — not ir[2] + j ir[0] — and is the same in every row: the chain is
//     walked once, by one lane, into a table of w doubles (undistort_xcol_kernel: w dependent additions, ~5 us at 1280 columns);
//   * _y is i ir[4] + ir[5] (+ 0.0 from the second pixel on: only the sign of a zero can change), _w is 1.
// Everything behind the running sums is independent per pixel: undistort_map_kernel evaluates the distortion polynomial in the library's
// expression order (the Makefile's -ffp-contract=off keeps every product and sum separately rounded) and rounds as it does:
// lrint(u 32), >> 5 for the integer part, & 31 for the 5 fractional bits.
// Stores: one lane owns two CONSECUTIVE pixels of the row-major image (the pair may straddle a row end), so it writes one 8-byte (x, y, x, y)
// record of map1 and one dword of map2, both naturally aligned whatever the width: a wave writes 512 + 256 contiguous bytes.
#include "dv_ctx.h"

__global__ __launch_bounds__(64) void undistort_xcol_kernel(double ir0, double ir1, double ir2, int w, double* __restrict__ xcol) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double _x = 0 * ir1 + ir2;
    for (int j = 0; j < w; ++j, _x += ir0) xcol[j] = _x;
}

struct UmapPixel { int16_t x, y; uint16_t f; };

__device__ __forceinline__ UmapPixel umap_pixel(const dv_cam& cam, double _x, int i, int j, double ir4, double ir5) {
    double _y = i * ir4 + ir5, _w = i * 0.0 + 1.0;
    if (j > 0) { _y += 0.0; _w += 0.0; }
    const double k1 = cam.k1, k2 = cam.k2, p1 = cam.p1, p2 = cam.p2;
    const double iw = 1. / _w, x = _x * iw, y = _y * iw;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = (1 + ((0 * r2 + k2) * r2 + k1) * r2) / (1 + ((0 * r2 + 0) * r2 + 0) * r2);
    const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2), yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
    const double u = cam.fx * xd + cam.cx, v = cam.fy * yd + cam.cy;
    const int iu = (int)llrint(u * 32), iv = (int)llrint(v * 32);
    return UmapPixel{ (int16_t)(iu >> 5), (int16_t)(iv >> 5), (uint16_t)((iv & 31) * 32 + (iu & 31)) };
}

__global__ __launch_bounds__(256) void undistort_map_kernel(dv_cam cam, double ir4, double ir5, int w, int npx, const double* __restrict__ xcol,
                                                            int16_t* __restrict__ map1, uint16_t* __restrict__ map2) {
    const int p = (blockIdx.x * 256 + threadIdx.x) * 2;      // npx <= 2^30 (dv_init_undistort_map)
    if (p >= npx) return;
    const int i = p / w, j = p - i * w;
    const UmapPixel a = umap_pixel(cam, xcol[j], i, j, ir4, ir5);
    if (p + 1 < npx) {
        const int j1 = (j + 1 < w) ? j + 1 : 0, i1 = (j + 1 < w) ? i : i + 1;
        const UmapPixel b = umap_pixel(cam, xcol[j1], i1, j1, ir4, ir5);
        *reinterpret_cast<short4*>(map1 + (size_t)p * 2) = make_short4(a.x, a.y, b.x, b.y);
        *reinterpret_cast<uint32_t*>(map2 + p) = (uint32_t)a.f | ((uint32_t)b.f << 16);
    } else {
        map1[(size_t)p * 2] = a.x; map1[(size_t)p * 2 + 1] = a.y; map2[p] = a.f;
    }
}

void dv_launch_undistort_map(const dv_cam& cam, const double* newK4, int w, int h, double* xcol, int16_t* map1_xy, uint16_t* map2, hipStream_t s) {
    const double ir[9] = { 1.0 / newK4[0], 0, -newK4[2] / newK4[0], 0, 1.0 / newK4[1], -newK4[3] / newK4[1], 0, 0, 1 };      // (newK I)^-1
    const int npx = w * h;
    hipLaunchKernelGGL(undistort_xcol_kernel, dim3(1), dim3(64), 0, s, ir[0], ir[1], ir[2], w, xcol);
    hipLaunchKernelGGL(undistort_map_kernel, dim3((npx + DV_UMAP_TILE - 1) / DV_UMAP_TILE), dim3(256), 0, s, cam, ir[4], ir[5], w, npx, xcol, map1_xy, map2);
}

// ---- cv::getOptimalNewCameraMatrix (host) ----
// cvUndistortPoints with R = P = I for one pixel: OpenCV 3.4 undistort.cpp, iters = 5
static void undistort_point(const dv_cam& c, double px, double py, double& xo, double& yo) {
    double x = (px - c.cx) * (1. / c.fx), y = (py - c.cy) * (1. / c.fy);
    const double x0 = x, y0 = y;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1. / (1 + (c.k2 * r2 + c.k1) * r2);
        const double dx = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x), dy = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
        x = (x0 - dx) * icdist; y = (y0 - dy) * icdist;
    }
    xo = x; yo = y;
}

extern "C" {

int dv_optimal_new_camera(const dv_cam* cam, int w, int h, double alpha, double newK4[4]) {
    auto fail = [](const char* m) { dv_set_error(nullptr, m); return -1; };
    if (!cam || !newK4 || w <= 1 || h <= 1 || !(alpha >= 0.0 && alpha <= 1.0) || !(cam->fx > 0) || !(cam->fy > 0)) return fail("dv_optimal_new_camera: bad argument");
    const int N = 9;                                    // icvGetRectangles
    double iX0 = -HUGE_VAL, iX1 = HUGE_VAL, iY0 = -HUGE_VAL, iY1 = HUGE_VAL, oX0 = HUGE_VAL, oX1 = -HUGE_VAL, oY0 = HUGE_VAL, oY1 = -HUGE_VAL;
    for (int y = 0; y < N; ++y) for (int x = 0; x < N; ++x) {
        double px, py;
        undistort_point(*cam, (double)x * w / (N - 1), (double)y * h / (N - 1), px, py);
        oX0 = std::min(oX0, px); oX1 = std::max(oX1, px); oY0 = std::min(oY0, py); oY1 = std::max(oY1, py);
        if (x == 0) iX0 = std::max(iX0, px);
        if (x == N - 1) iX1 = std::min(iX1, px);
        if (y == 0) iY0 = std::max(iY0, py);
        if (y == N - 1) iY1 = std::min(iY1, py);
    }
    const double iw = iX1 - iX0, ih = iY1 - iY0, ow = oX1 - oX0, oh = oY1 - oY0;
    if (!(iw > 0) || !(ih > 0) || !std::isfinite(ow) || !std::isfinite(oh)) return fail("dv_optimal_new_camera: the undistorted grid has no inner rectangle");
    const double fx0 = (w - 1) / iw, fy0 = (h - 1) / ih, cx0 = -fx0 * iX0, cy0 = -fy0 * iY0;      // inner rectangle -> viewport
    const double fx1 = (w - 1) / ow, fy1 = (h - 1) / oh, cx1 = -fx1 * oX0, cy1 = -fy1 * oY0;      // outer rectangle -> viewport
    newK4[0] = fx0 * (1 - alpha) + fx1 * alpha; newK4[1] = fy0 * (1 - alpha) + fy1 * alpha;
    newK4[2] = cx0 * (1 - alpha) + cx1 * alpha; newK4[3] = cy0 * (1 - alpha) + cy1 * alpha;
    return 0;
}

static int umap_check(dv_ctx* ctx, const dv_cam* cam, const double* newK4, int w, int h, const char* who) {
    if (!cam || !newK4 || w <= 0 || h <= 0 || w > 32767 || h > 32767 || (long long)w * h > (1ll << 30)) DV_FAIL(std::string(who) + ": bad argument");
    if (!(newK4[0] > 0) || !(newK4[1] > 0) || !std::isfinite(newK4[0]) || !std::isfinite(newK4[1]) || !std::isfinite(newK4[2]) || !std::isfinite(newK4[3]))
        DV_FAIL(std::string(who) + ": newK must be finite with positive focal lengths");
    return 0;
}

int dv_init_undistort_map(dv_ctx* ctx, const dv_cam* cam, const double newK4[4], int w, int h, int16_t* map1_xy, uint16_t* map2, int mem) {
    if (!ctx) return -1;
    if (!map1_xy || !map2 || (mem != DV_MEM_HOST && mem != DV_MEM_DEVICE)) DV_FAIL("dv_init_undistort_map: bad argument");
    if (umap_check(ctx, cam, newK4, w, h, "dv_init_undistort_map")) return -1;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    const size_t npx = (size_t)w * h;
    DV_CHECK(ctx->s0.ensure((size_t)w * 8));
    // a device destination is written in place when it is aligned for the kernel's 8- and 4-byte stores, otherwise through scratch like a host destination
    const bool direct = mem == DV_MEM_DEVICE && ((uintptr_t)map1_xy & 7) == 0 && ((uintptr_t)map2 & 3) == 0;
    int16_t* d1 = map1_xy; uint16_t* d2 = map2;
    if (!direct) { DV_CHECK(ctx->s2.ensure(6 * npx)); d1 = (int16_t*)ctx->s2.p; d2 = (uint16_t*)((uint8_t*)ctx->s2.p + 4 * npx); }
    dv_launch_undistort_map(*cam, newK4, w, h, (double*)ctx->s0.p, d1, d2, s);
    DV_CHECK(hipGetLastError());
    if (!direct) {
        const hipMemcpyKind k = mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        DV_CHECK(hipMemcpyAsync(map1_xy, d1, 4 * npx, k, s));
        DV_CHECK(hipMemcpyAsync(map2, d2, 2 * npx, k, s));
    }
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

int dv_undistort_setup(dv_ctx* ctx, double alpha, dv_cam* new_cam0, dv_cam* new_cam1) {
    if (!ctx) return -1;
    if (ctx->pending) DV_FAIL("dv_undistort_setup: a frame is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const int w = ctx->cfg.width, h = ctx->cfg.height, ncam = ctx->cfg.stereo ? 2 : 1;
    const dv_cam src[2] = { ctx->cam_switched ? ctx->cam_orig[0] : ctx->cfg.cam0, ctx->cam_switched ? ctx->cam_orig[1] : ctx->cfg.cam1 };
    double nk[2][4];
    for (int c = 0; c < ncam; ++c) {
        if (dv_optimal_new_camera(&src[c], w, h, alpha, nk[c])) DV_FAIL(std::string("dv_undistort_setup: ") + dv_last_error(nullptr));
        if (umap_check(ctx, &src[c], nk[c], w, h, "dv_undistort_setup")) return -1;
    }
    const size_t npx = (size_t)w * h;
    // from here on the buffers of earlier maps may be reallocated or overwritten: until the new maps stand, none are installed and the original cameras hold
    ctx->undist[0] = ctx->undist[1] = false;
    ctx->cfg.cam0 = src[0]; ctx->cfg.cam1 = src[1]; ctx->cam_orig[0] = src[0]; ctx->cam_orig[1] = src[1]; ctx->cam_switched = false;
    DV_CHECK(ctx->s0.ensure((size_t)w * 8));
    for (int c = 0; c < ncam; ++c) DV_CHECK(ctx->undist_buf[c].ensure(6 * npx));
    for (int c = 0; c < ncam; ++c) {      // the column table is rewritten per camera: both launches are ordered on the ctx's stream
        uint8_t* b = (uint8_t*)ctx->undist_buf[c].p;
        dv_launch_undistort_map(src[c], nk[c], w, h, (double*)ctx->s0.p, (int16_t*)b, (uint16_t*)(b + 4 * npx), ctx->stream);
    }
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->cam_switched = true;
    ctx->cfg.cam0 = dv_cam{ nk[0][0], nk[0][1], nk[0][2], nk[0][3], 0, 0, 0, 0 };
    if (ncam == 2) ctx->cfg.cam1 = dv_cam{ nk[1][0], nk[1][1], nk[1][2], nk[1][3], 0, 0, 0, 0 };
    ctx->undist[0] = true; ctx->undist[1] = ncam == 2; ctx->undist_w = w; ctx->undist_h = h;
    if (new_cam0) *new_cam0 = ctx->cfg.cam0;
    if (new_cam1) *new_cam1 = ctx->cfg.cam1;
    return 0;
}

int dv_set_undistort_maps(dv_ctx* ctx, int cam, const int16_t* map1_xy, const uint16_t* map2, int w, int h) {
    if (!ctx) return -1;
    if (cam < 0 || cam > 1) DV_FAIL("dv_set_undistort_maps: cam must be 0 or 1");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (ctx->pending) DV_FAIL("dv_set_undistort_maps: a frame is in flight");
    if (!map1_xy) {
        ctx->undist[cam] = false; if (cam == 0) ctx->undist[1] = false;
        if (ctx->cam_switched) {      // dv_undistort_setup re-parameterised the cameras for the undistorted frames: without the maps the original ones hold again
            ctx->cfg.cam1 = ctx->cam_orig[1];
            if (cam == 0) { ctx->cfg.cam0 = ctx->cam_orig[0]; ctx->cam_switched = false; }
        }
        return 0;
    }
    if (!map2 || w != ctx->cfg.width || h != ctx->cfg.height) DV_FAIL("dv_set_undistort_maps: maps must be width x height of the config");
    if (cam == 1 && !ctx->undist[0]) DV_FAIL("dv_set_undistort_maps: install camera 0 first");
    const size_t npx = (size_t)w * h;
    DV_CHECK(ctx->undist_buf[cam].ensure(6 * npx));
    DV_CHECK(hipMemcpyAsync(ctx->undist_buf[cam].p, map1_xy, 4 * npx, hipMemcpyHostToDevice, ctx->stream));
    DV_CHECK(hipMemcpyAsync((uint8_t*)ctx->undist_buf[cam].p + 4 * npx, map2, 2 * npx, hipMemcpyHostToDevice, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->undist[cam] = true; ctx->undist_w = w; ctx->undist_h = h;
    if (ctx->cam_switched) {      // the caller's own maps replace those of dv_undistort_setup: its (newK, 0) no longer describes this camera's frames — the camera the ctx was created with holds again
        if (cam == 0) ctx->cfg.cam0 = ctx->cam_orig[0]; else ctx->cfg.cam1 = ctx->cam_orig[1];
    }
    return 0;
}

int dv_get_undistort_maps(dv_ctx* ctx, int cam, int16_t* map1_xy, uint16_t* map2, int mem) {
    if (!ctx) return -1;
    if (cam < 0 || cam > 1 || !map1_xy || !map2 || (mem != DV_MEM_HOST && mem != DV_MEM_DEVICE)) DV_FAIL("dv_get_undistort_maps: bad argument");
    if (!ctx->undist[cam]) DV_FAIL("dv_get_undistort_maps: no maps installed for this camera");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const size_t npx = (size_t)ctx->undist_w * ctx->undist_h;
    const hipMemcpyKind k = mem == DV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const uint8_t* b = (const uint8_t*)ctx->undist_buf[cam].p;
    DV_CHECK(hipMemcpyAsync(map1_xy, b, 4 * npx, k, ctx->stream));
    DV_CHECK(hipMemcpyAsync(map2, b + 4 * npx, 2 * npx, k, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

int dv_get_cameras(dv_ctx* ctx, dv_cam* cam0, dv_cam* cam1) {
    if (!ctx) return -1;
    if (cam0) *cam0 = ctx->cfg.cam0;
    if (cam1) *cam1 = ctx->cfg.cam1;
    return 0;
}

}      // extern "C"
