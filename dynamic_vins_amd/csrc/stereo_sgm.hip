// stereo_sgm.hip — the stereo matcher on gfx950: the frame's rectified gray pair -> the float disparity map of the left image (SemanticImage::disp), in device memory.
// Reference: MyStereoMatcher::Launch / WaitResult (stereo/stereo.cpp) — an empty StereoMatch() and a PNG read; there is no matcher to restate, so the algorithm is this
// project's own, specified in integers in include/dvins.h (census 9 x 7 + eight-path SGM + OpenCV's uniqueness rule + left-right check + floored subpixel), and
// tests/sgm_ref.py restates it bit for bit.  The rules that exist once (clamp, bit order, cost, path step, uniqueness, floor, refusals) are stereo_sgm_host.h.  Kernels:
//   sgm_census_kernel   both images in one launch (blockIdx.z).  A workgroup = 4 waves on 4 rows x 256 columns; the (4 + 6) x (256 + 8) source bytes go through LDS once,
//                       clamped on the way in; a lane owns 4 consecutive columns, reads three dwords per window row and forms its four codes in registers (uint64 out).
//   sgm_path_kernel     <K, DX, DY, FIRST>: ONE WAVE WALKS ONE PATH CHAIN, its lanes are the disparities (lane l holds d = l K .. l K + K - 1; K = n_disp / 64).  The
//                       predecessor's L_r stays in registers; d - 1 / d + 1 cross lanes by DPP wave shifts, the minimum over d is a DPP row scan + row broadcasts +
//                       v_readlane (no LDS).  C is computed on the fly: the left code is wave-uniform, the lanes read the right codes at x - d as one run.  The next
//                       pixel's right codes and S are requested before this pixel's step, so the memory latency lies beside the chain.  Horizontal: a wave per row;
//                       vertical: a wave per column; diagonal: a wave per start pixel on the two entry borders (w + h - 1 chains).
//   sgm_decide_kernel   <K>: one wave per pixel — winner by (S, d) key (ties cannot depend on the reduction order), uniqueness on the smallest other S, dR of the
//                       pixel the winner points at (a gather down S's diagonal), left-right check, subpixel, the float store.  Every element is written.
// S: ONE uint16 volume [h][w][n_disp]; the eight directions add into it in place, one launch each, in stream order (no atomics, never cleared: the first direction
// stores).  Bytes moved per pixel: 2 n_disp written by the first direction, 4 n_disp (read + write) by each of the other seven, 2 n_disp read by the decision and up
// to 2 n_disp gathered for dR: 34 n_disp bytes, plus 8 (n_disp + 1) of codes per direction.  (Per-direction uint8 volumes would halve that but only hold 64 + p2 <= 255.)
#include "dv_ctx.h"
#include "stereo_sgm_host.h"
#include <string>

namespace {

// DPP with the old value kept where the source lane does not exist (bound_ctrl off).  row_shr:n = 0x110 + n, row_bcast:15 / 31 = 0x142 / 0x143 (wave_dpp.h);
// wave_shl:1 = 0x130 (lane i reads lane i + 1), wave_shr:1 = 0x138 (lane i reads lane i - 1).  All 64 lanes must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_keep(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int wave_min_i32(int v) {          // the wave's minimum, lane-uniform
    v = imin(v, dpp_keep<0x111, 0xf>(v, v)); v = imin(v, dpp_keep<0x112, 0xf>(v, v)); v = imin(v, dpp_keep<0x114, 0xf>(v, v)); v = imin(v, dpp_keep<0x118, 0xf>(v, v));
    v = imin(v, dpp_keep<0x142, 0xa>(v, v));
    v = imin(v, dpp_keep<0x143, 0xc>(v, v));
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int from_lane_below(int v, int none) { return dpp_keep<0x138, 0xf>(none, v); }      // lane 0 gets `none`
__device__ __forceinline__ int from_lane_above(int v, int none) { return dpp_keep<0x130, 0xf>(none, v); }      // lane 63 gets `none`

constexpr int CENSUS_TW = 256, CENSUS_TH = 4, CENSUS_PW = CENSUS_TW + 2 * DV_SGM_CENSUS_RX, CENSUS_PH = CENSUS_TH + 2 * DV_SGM_CENSUS_RY;

struct CensusArgs { const uint8_t* img[2]; int stride[2]; int w, h; uint64_t* out[2]; };

__global__ __launch_bounds__(256) void sgm_census_kernel(CensusArgs a) {
    __shared__ uint32_t tile[CENSUS_PH][CENSUS_PW / 4];
    const int im = blockIdx.z, xb = blockIdx.x * CENSUS_TW, yb = blockIdx.y * CENSUS_TH;
    const uint8_t* img = a.img[im]; const int stride = a.stride[im];
    uint8_t* tb = reinterpret_cast<uint8_t*>(&tile[0][0]);
    for (int i = threadIdx.x; i < CENSUS_PH * CENSUS_PW; i += 256) {
        const int r = i / CENSUS_PW, c = i - r * CENSUS_PW;
        tb[i] = img[(size_t)dv_sgm_clamp(yb + r - DV_SGM_CENSUS_RY, a.h) * stride + dv_sgm_clamp(xb + c - DV_SGM_CENSUS_RX, a.w)];
    }
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = yb + wv, x0 = xb + lane * 4;
    if (y >= a.h || x0 >= a.w) return;
    // tile column lane * 4 + k (k = 0..11) is image column x0 - 4 + k: pixel i's window is bytes i .. i + 8, its centre byte i + 4 of window row 3
    const uint32_t cw = tile[wv + DV_SGM_CENSUS_RY][lane + 1];
    int centre[4]; uint64_t code[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { centre[i] = (cw >> (8 * i)) & 255; code[i] = 0; }
#pragma unroll
    for (int dy = 0; dy < 2 * DV_SGM_CENSUS_RY + 1; ++dy) {
        const uint32_t q[3] = { tile[wv + dy][lane], tile[wv + dy][lane + 1], tile[wv + dy][lane + 2] };
#pragma unroll
        for (int dx = 0; dx < 2 * DV_SGM_CENSUS_RX + 1; ++dx) {
            if (dy == DV_SGM_CENSUS_RY && dx == DV_SGM_CENSUS_RX) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) { const int k = i + dx; code[i] = dv_sgm_census_push(code[i], (q[k >> 2] >> (8 * (k & 3))) & 255, centre[i]); }
        }
    }
    uint64_t* o = a.out[im] + (size_t)y * a.w + x0;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (x0 + i < a.w) o[i] = code[i];
}

template <int K> struct alignas(2 * K) SPack { uint16_t v[K]; };

struct PathArgs { const uint64_t* cl; const uint64_t* cr; uint16_t* S; int w, h, p1, p2; };

template <int K, int DX, int DY, bool FIRST>
__global__ __launch_bounds__(256) void sgm_path_kernel(PathArgs a) {
    constexpr int D = 64 * K;
    const int chain = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int w = a.w, h = a.h;
    const int nchains = DY == 0 ? h : (DX == 0 ? w : w + h - 1);
    if (chain >= nchains) return;
    int x, y;
    if (DY == 0) { x = DX > 0 ? 0 : w - 1; y = chain; }
    else if (DX == 0) { x = chain; y = DY > 0 ? 0 : h - 1; }
    else if (chain < w) { x = chain; y = DY > 0 ? 0 : h - 1; }
    else { const int t = chain - w + 1; x = DX > 0 ? 0 : w - 1; y = DY > 0 ? t : h - 1 - t; }
    const int d0 = lane * K;

    // what the step of pixel (x, y) reads from memory: the left code (uniform), the right codes at x - d, and S (unless this direction is the first)
    uint64_t cl, cr[K]; SPack<K> so;
    auto fetch = [&](int px, int py, uint64_t& l, uint64_t (&r)[K], SPack<K>& s) {
        const size_t row = (size_t)py * w;
        l = a.cl[row + px];
#pragma unroll
        for (int j = 0; j < K; ++j) { const int xr = px - d0 - j; r[j] = xr >= 0 ? a.cr[row + xr] : 0; }
        if (!FIRST) s = *reinterpret_cast<const SPack<K>*>(a.S + (row + px) * D + d0);
    };
    fetch(x, y, cl, cr, so);
    int Lp[K];
    bool first = true;
    while (true) {
        const int nx = x + DX, ny = y + DY;
        const bool more = nx >= 0 && nx < w && ny >= 0 && ny < h;      // wave-uniform
        uint64_t ncl = 0, ncr[K]; SPack<K> nso;
        if (more) fetch(nx, ny, ncl, ncr, nso);
        int L[K];
        if (first) {
#pragma unroll
            for (int j = 0; j < K; ++j) L[j] = dv_sgm_cost(cl, cr[j], x, d0 + j);
        } else {
            int mine = Lp[0];
#pragma unroll
            for (int j = 1; j < K; ++j) mine = imin(mine, Lp[j]);
            const int m = wave_min_i32(mine);
            const int below = from_lane_below(Lp[K - 1], DV_SGM_NO_TERM), above = from_lane_above(Lp[0], DV_SGM_NO_TERM);
#pragma unroll
            for (int j = 0; j < K; ++j)
                L[j] = dv_sgm_path_step(dv_sgm_cost(cl, cr[j], x, d0 + j), Lp[j], j > 0 ? Lp[j - 1] : below, j < K - 1 ? Lp[j + 1] : above, m, a.p1, a.p2);
        }
        SPack<K> sn;
#pragma unroll
        for (int j = 0; j < K; ++j) { sn.v[j] = (uint16_t)((FIRST ? 0 : so.v[j]) + L[j]); Lp[j] = L[j]; }
        *reinterpret_cast<SPack<K>*>(a.S + ((size_t)y * w + x) * D + d0) = sn;
        if (!more) break;
        first = false; x = nx; y = ny; cl = ncl; so = nso;
#pragma unroll
        for (int j = 0; j < K; ++j) cr[j] = ncr[j];
    }
}

struct DecideArgs { const uint16_t* S; float* out; int16_t* dbg_dstar; int16_t* dbg_dr; int w, h, uniqueness, lr_max_diff; };

constexpr int SGM_NO_KEY = 0x7fffffff;

// dR(x, y) = argmin_d S((x + d, y), d) over x + d < w, ties to the lowest d: the (S, d) key makes the order of the reduction irrelevant
template <int K>
__device__ __forceinline__ int sgm_right_winner(const uint16_t* S, int w, int x, int y, int lane) {
    constexpr int D = 64 * K;
    int key = SGM_NO_KEY;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int d = lane * K + j, xx = x + d;
        if (xx < w) key = imin(key, ((int)S[((size_t)y * w + xx) * D + d] << 8) | d);
    }
    return wave_min_i32(key) & 255;
}

// S(d) of this wave's pixel for a wave-uniform d
template <int K>
__device__ __forceinline__ int sgm_pick(const int (&Sv)[K], int d) {
    const int src = d / K, jj = d % K;
    int v = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) if (jj == j) v = __builtin_amdgcn_readlane(Sv[j], src);
    return v;
}

template <int K>
__global__ __launch_bounds__(256) void sgm_decide_kernel(DecideArgs a) {
    constexpr int D = 64 * K;
    const long long pix = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, w = a.w;
    if (pix >= (long long)w * a.h) return;
    const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
    const SPack<K> sp = *reinterpret_cast<const SPack<K>*>(a.S + (size_t)pix * D + lane * K);
    int Sv[K], key = SGM_NO_KEY;
#pragma unroll
    for (int j = 0; j < K; ++j) { Sv[j] = sp.v[j]; key = imin(key, (Sv[j] << 8) | (lane * K + j)); }
    key = wave_min_i32(key);
    const int ds = key & 255, s0 = key >> 8;
    // uniqueness: the smallest S among the d with |d - d*| > 1 decides (n_disp >= 64: there always is one)
    int other = 0xffff;
#pragma unroll
    for (int j = 0; j < K; ++j) { const int d = lane * K + j; if (d < ds - 1 || d > ds + 1) other = imin(other, Sv[j]); }
    other = wave_min_i32(other);
    bool valid = !dv_sgm_not_unique(other, s0, a.uniqueness) && ds <= x;
    if (valid && a.lr_max_diff >= 0) {          // wave-uniform
        const int dr = sgm_right_winner<K>(a.S, w, x - ds, y, lane);
        const int diff = dr > ds ? dr - ds : ds - dr;
        if (diff > a.lr_max_diff) valid = false;
    }
    if (a.out) {
        const int sm = ds > 0 ? sgm_pick<K>(Sv, ds - 1) : 0, sq = ds < D - 1 ? sgm_pick<K>(Sv, ds + 1) : 0;
        const int d16 = dv_sgm_subpixel(ds, D, sm, s0, sq);
        if (lane == 0) a.out[pix] = valid ? (float)d16 / 16.0f : 0.0f;
    }
    if (a.dbg_dstar) {          // dv_stereo_sgm_debug: the two winners of every pixel, before any validity test
        const int dr = sgm_right_winner<K>(a.S, w, x, y, lane);
        if (lane == 0) { a.dbg_dstar[pix] = (int16_t)ds; a.dbg_dr[pix] = (int16_t)dr; }
    }
}

template <int K>
void sgm_launch_paths(const PathArgs& a, hipStream_t s) {
    const int w = a.w, h = a.h, nd = w + h - 1;
    auto blocks = [](int n) { return dim3((unsigned)((n + 3) / 4)); };
    // in-place accumulation: the order of these launches on ONE stream is what keeps S race-free
    hipLaunchKernelGGL((sgm_path_kernel<K, 1, 0, true>), blocks(h), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sgm_path_kernel<K, -1, 0, false>), blocks(h), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sgm_path_kernel<K, 0, 1, false>), blocks(w), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sgm_path_kernel<K, 0, -1, false>), blocks(w), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sgm_path_kernel<K, 1, 1, false>), blocks(nd), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sgm_path_kernel<K, -1, 1, false>), blocks(nd), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sgm_path_kernel<K, 1, -1, false>), blocks(nd), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sgm_path_kernel<K, -1, -1, false>), blocks(nd), dim3(256), 0, s, a);
}

void sgm_launch_decide(int n_disp, const DecideArgs& a, hipStream_t s) {
    const dim3 g((unsigned)(((long long)a.w * a.h + 3) / 4));
    if (n_disp == 64) hipLaunchKernelGGL(sgm_decide_kernel<1>, g, dim3(256), 0, s, a);
    else if (n_disp == 128) hipLaunchKernelGGL(sgm_decide_kernel<2>, g, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sgm_decide_kernel<4>, g, dim3(256), 0, s, a);
}

}  // namespace

// Two disparity maps used alternately (out[cur] belongs to the frame enqueued last); the census codes (left | right) and S are the last frame's and are what
// dv_stereo_sgm_debug reads; staged[] hold a DV_MEM_HOST pair.
struct StereoSgmStage {
    DevBuf out[2], staged[2], census, S, dbg;
    int cur = 1;
    StageSlot slot;
    const float* last = nullptr; bool have = false;
    int w = 0, h = 0; dv_sgm_params par{};
};

void dv_stage_delete(StereoSgmStage* p) { delete p; }

extern "C" {

int dv_stereo_sgm_check(int w, int h, int stride, const dv_sgm_params* par) {
    dv_ctx* ctx = nullptr;
    if (const char* why = dv_sgm_check_host(w, h, stride, par)) DV_FAIL(std::string("dv_stereo_sgm_check: ") + why);
    return 0;
}

int dv_stereo_sgm_enqueue(dv_ctx* ctx, const uint8_t* gray0, const uint8_t* gray1, int stride, int mem, const dv_sgm_params* par) {
    if (!ctx) return -1;
    const int W = ctx->cfg.width, H = ctx->cfg.height;
    if (const char* why = dv_sgm_check_host(W, H, stride, par)) DV_FAIL(std::string("dv_stereo_sgm_enqueue: ") + why);
    if (!gray0 || !gray1) DV_FAIL("dv_stereo_sgm_enqueue: null image");
    if (!dv_mem_known(mem)) DV_FAIL("dv_stereo_sgm_enqueue: unknown memory kind");
    if (!ctx->sgm) ctx->sgm = new StereoSgmStage();
    StereoSgmStage& V = *ctx->sgm;
    if (V.slot.open(ctx, "dv_stereo_sgm_enqueue: previous frame not collected")) return -1;
    hipStream_t s = ctx->stream;
    const size_t npix = (size_t)W * H;
    V.have = false;
    DV_CHECK(V.census.ensure(2 * npix * sizeof(uint64_t)));
    DV_CHECK(V.S.ensure(npix * par->n_disp * sizeof(uint16_t)));
    DevBuf& B = V.out[V.cur ^ 1];
    DV_CHECK(B.ensure(npix * sizeof(float)));

    CensusArgs ca{};
    const uint8_t* src[2] = { gray0, gray1 };
    for (int i = 0; i < 2; ++i) {
        DvRows im;
        if (dv_stage_rows(ctx, V.staged[i], src[i], (size_t)W, H, stride, dv_in_place_device_or_pinned(mem), s, &im)) return -1;
        ca.img[i] = im.p; ca.stride[i] = im.pitch;
        ca.out[i] = (uint64_t*)V.census.p + i * npix;
    }
    ca.w = W; ca.h = H;
    PathArgs pa{ ca.out[0], ca.out[1], (uint16_t*)V.S.p, W, H, par->p1, par->p2 };
    DecideArgs da{ (const uint16_t*)V.S.p, (float*)B.p, nullptr, nullptr, W, H, par->uniqueness, par->lr_max_diff };
    {
        StageScope sc_t(ctx, "stereo_sgm");
        hipLaunchKernelGGL(sgm_census_kernel, dim3((W + CENSUS_TW - 1) / CENSUS_TW, (H + CENSUS_TH - 1) / CENSUS_TH, 2), dim3(256), 0, s, ca);
        if (par->n_disp == 64) sgm_launch_paths<1>(pa, s);
        else if (par->n_disp == 128) sgm_launch_paths<2>(pa, s);
        else sgm_launch_paths<4>(pa, s);
        sgm_launch_decide(par->n_disp, da, s);
    }
    if (V.slot.close(ctx, hipGetLastError(), s)) return -1;
    V.cur ^= 1;
    V.last = (const float*)B.p; V.w = W; V.h = H; V.par = *par;
    return 0;
}

int dv_stereo_sgm_collect(dv_ctx* ctx, const float** disp_dev, int* stride_bytes) {
    if (!ctx) return -1;
    if (!ctx->sgm || !ctx->sgm->slot.pending) DV_FAIL("dv_stereo_sgm_collect: nothing enqueued");
    StereoSgmStage& V = *ctx->sgm;
    if (V.slot.wait(ctx)) return -1;
    V.have = true;
    if (disp_dev) *disp_dev = V.last;
    if (stride_bytes) *stride_bytes = V.w * (int)sizeof(float);
    return 0;
}

int dv_stereo_sgm_debug(dv_ctx* ctx, int what, void* host, long long cap_bytes) {
    if (!ctx) return -1;
    if (!ctx->sgm || !ctx->sgm->have || ctx->sgm->slot.pending) DV_FAIL("dv_stereo_sgm_debug: no collected frame");
    if (!host) DV_FAIL("dv_stereo_sgm_debug: null buffer");
    StereoSgmStage& V = *ctx->sgm;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipStream_t s = ctx->stream;
    const size_t npix = (size_t)V.w * V.h;
    const void* src = nullptr; size_t n = 0;
    if (what == DV_SGM_DEBUG_CENSUS_L || what == DV_SGM_DEBUG_CENSUS_R) { n = npix * sizeof(uint64_t); src = (const uint64_t*)V.census.p + (what == DV_SGM_DEBUG_CENSUS_R ? npix : 0); }
    else if (what == DV_SGM_DEBUG_S) { n = npix * V.par.n_disp * sizeof(uint16_t); src = V.S.p; }
    else if (what == DV_SGM_DEBUG_DSTAR || what == DV_SGM_DEBUG_DR) {
        n = npix * sizeof(int16_t);
        DV_CHECK(V.dbg.ensure(2 * n));
        DecideArgs da{ (const uint16_t*)V.S.p, nullptr, (int16_t*)V.dbg.p, (int16_t*)V.dbg.p + npix, V.w, V.h, V.par.uniqueness, V.par.lr_max_diff };
        sgm_launch_decide(V.par.n_disp, da, s);
        DV_CHECK(hipGetLastError());
        src = (const int16_t*)V.dbg.p + (what == DV_SGM_DEBUG_DR ? npix : 0);
    } else DV_FAIL("dv_stereo_sgm_debug: unknown item");
    if (cap_bytes < (long long)n) DV_FAIL("dv_stereo_sgm_debug: buffer too small");
    DV_CHECK(hipMemcpyAsync(host, src, n, hipMemcpyDeviceToHost, s));
    DV_CHECK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
