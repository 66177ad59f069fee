// solo_head.hip — the detector's head on gfx950: the SOLOv2 network's output tensors -> the instance-mask stack inst_stack.hip reads.  Reference: Solov2::GetSegTensor
// (det2d/solo_head.cpp:410-559) and Solov2::MatrixNMS (det2d/solo_head.cpp:31-71), restated step by step as the reference evaluates them (include/dvins.h has the rule;
// the host half — refusals, cell tables, pixel floor — is solo_head_host.h).  The pixel floor of a candidate comes from the cumulative sums of num_grids[]^2 applied to the
// CONCATENATED cell index, never from the levels' own g: the reference's tables disagree in order (solo_head.cpp:24-28,454-465) and that is kept.  Kernels, in stream order:
//   solo_count_kernel     a lane per cell counts its classes over score_thr (reads coalesced along the cells of a category map)
//   solo_scan_kernel      one workgroup: exclusive scan of the counts over the cells -> where each cell's candidates go; total, over-capacity flag
//   solo_emit_kernel      a lane per cell writes its candidates, ascending class: together nonzero() order, no atomics
//   solo_product_kernel   seg = sigmoid(kernel . feature) on v_mfma_f32_32x32x2_f32, rows = candidates (their kernel rows gathered in the A-operand load), columns = pixels.
//                         <false>: epilogue = test, ballot into bit-packed masks (a 32-bit word per candidate and 32 pixels), per-word sums of seg * mask
//                         <true>:  the same main loop over the survivors, epilogue stores seg — the only float planes that ever exist (<= 128)
//   solo_sums_kernel      a wave per candidate: popcount and the float sums of its words -> sum_mask, pixel floor, score
//   solo_sort_kernel      one workgroup: rank sort (descending, ties by candidate order), the first nms_pre
//   solo_inter_kernel     the masks' inner products as popcount(a & b) over the packed words, upper-triangle tiles of 16 x 16 pairs
//   solo_nms_kernel       one workgroup: column maximum, decay, minimum over all rows, second filter and rank sort -> survivors, labels, scores
//   solo_resample_kernel  both bilinear resamplings and the crop in one pass from the survivors' seg to the 0 / 1 byte planes; a lane owns 4 pixels and writes a dword
// Counts (candidates, sorted, survivors) stay in a device header between the kernels; the grids are sized for the capacities and leave early.
#include "dv_ctx.h"
#include "solo_head_host.h"
#include <string>

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

enum { H_NCAND = 0, H_OVER = 1, H_NSORT = 2, H_NSURV = 3, H_NFLOOR = 4, H_NPASS = 5, H_WORDS = 8 };

struct SoloDev {
    const float* kern[DV_SOLO_MAX_LEVELS]; const float* cate[DV_SOLO_MAX_LEVELS]; const float* feat;
    int cell_off[DV_SOLO_MAX_LEVELS + 1], floor_end[DV_SOLO_MAX_LEVELS]; float floor_val[DV_SOLO_MAX_LEVELS];
    int n_levels, channels, n_classes, n_cells, P, fh, fw, Wn;      // P = fh * fw pixels, Wn = ceil(P / 32) words per mask
    float score_thr, mask_thr, update_thr, sigma; int nms_pre, max_per_img, nms_kernel, max_cand;
    // work buffers
    int* hdr; int* cell_cnt; int* cell_pos;
    int* cand_cell; int* cand_label; float* cand_cate; float* cand_floor; float* cand_sum; float* cand_score;
    uint32_t* masks; float* psum;
    int* order; int* inter;
    int* out_i /* n, n_cand, over, pad | labels[128] | survivor's candidate [128] */; float* out_score /* [128] */;
    float* seg;
};

__device__ __forceinline__ int level_of(const SoloDev& D, int cell) {
    int l = 0;
    while (l + 1 < D.n_levels && cell >= D.cell_off[l + 1]) ++l;
    return l;
}

__global__ __launch_bounds__(256) void solo_count_kernel(SoloDev D) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= D.n_cells) return;
    const int l = level_of(D, cell), g2 = D.cell_off[l + 1] - D.cell_off[l];
    const float* c = D.cate[l] + (cell - D.cell_off[l]);
    int n = 0;
    for (int k = 0; k < D.n_classes; ++k) n += c[(size_t)k * g2] > D.score_thr;
    D.cell_cnt[cell] = n;
}

// block-wide inclusive scan of one int per thread (1024 threads), through LDS
__device__ __forceinline__ int block_scan_1024(int v, int* s_wave) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
    if (lane == 63) s_wave[wv] = x;
    __syncthreads();
    if (wv == 0) {
        int w = lane < 16 ? s_wave[lane] : 0;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) { const int y = __shfl_up(w, d); if (lane >= d) w += y; }
        if (lane < 16) s_wave[lane] = w;
    }
    __syncthreads();
    const int r = x + (wv ? s_wave[wv - 1] : 0);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(1024) void solo_scan_kernel(SoloDev D) {
    __shared__ int s_wave[16];
    int carry = 0;
    for (int base = 0; base < D.n_cells; base += 1024) {
        const int cell = base + threadIdx.x;
        const int v = cell < D.n_cells ? D.cell_cnt[cell] : 0;
        const int inc = block_scan_1024(v, s_wave);
        if (cell < D.n_cells) D.cell_pos[cell] = carry + inc - v;
        __shared__ int s_tot;
        if (threadIdx.x == 1023) s_tot = inc;
        __syncthreads();
        carry += s_tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool over = carry > D.max_cand;
        D.hdr[H_NPASS] = carry; D.hdr[H_OVER] = over; D.hdr[H_NCAND] = over ? 0 : carry;
        D.hdr[H_NSORT] = 0; D.hdr[H_NSURV] = 0; D.hdr[H_NFLOOR] = 0;
    }
}

__global__ __launch_bounds__(256) void solo_emit_kernel(SoloDev D) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= D.n_cells || D.hdr[H_OVER]) return;
    int pos = D.cell_pos[cell];
    const int n = D.cell_cnt[cell];
    if (!n) return;
    const int l = level_of(D, cell), g2 = D.cell_off[l + 1] - D.cell_off[l];
    const float* c = D.cate[l] + (cell - D.cell_off[l]);
    const float fl = dv_solo_floor_of(cell, D.n_levels, D.floor_end, D.floor_val);
    for (int k = 0; k < D.n_classes; ++k) {
        const float v = c[(size_t)k * g2];
        if (v > D.score_thr && pos < D.max_cand) { D.cand_cell[pos] = cell; D.cand_label[pos] = k; D.cand_cate[pos] = v; D.cand_floor[pos] = fl; ++pos; }
    }
}

// A wave: 32 rows (candidates / survivors) x 64 pixels, two accumulator tiles; a workgroup: four waves on four neighbouring pixel tiles of the same rows.  Operands come
// straight from memory: lane l gives A[row l & 31][k + (l >> 5)] — the kernel map is [channels, g, g], so a candidate's row is a walk of stride g^2 from its cell — and
// B[k + (l >> 5)][pixel l & 31] of each tile (128 contiguous bytes per half wave).  The accumulation is the k-ordered float fma chain of the instruction.
constexpr int SP_NT = 2, SP_COLS = 32 * SP_NT;
template <bool STORE>
__global__ __launch_bounds__(256) void solo_product_kernel(SoloDev D) {
    const int n_rows = STORE ? D.hdr[H_NSURV] : D.hdr[H_NCAND];
    const int row0 = blockIdx.y * 32;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
    const int p0 = (blockIdx.x * 4 + wv) * SP_COLS;
    if (row0 >= n_rows || p0 >= D.P) return;          // wave-uniform
    const float* arow = nullptr; int astride = 0;
    if (row0 + li < n_rows) {
        const int cand = STORE ? D.out_i[4 + DV_SOLO_MAX_PER_IMG + row0 + li] : row0 + li;
        const int cell = D.cand_cell[cand], l = level_of(D, cell);
        astride = D.cell_off[l + 1] - D.cell_off[l];
        arow = D.kern[l] + (cell - D.cell_off[l]);
    }
    floatx16 acc[SP_NT];
#pragma unroll
    for (int t = 0; t < SP_NT; ++t) for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const int C = D.channels;
    // (the operands of step k + 2 are requested before the two instructions of step k are issued: one step of loads in flight behind the matrix pipe)
    auto load = [&](int k0, float& a, float (&b)[SP_NT]) {
        const int k = k0 + kh;
        const bool kin = k < C;
        a = (arow && kin) ? arow[(size_t)k * astride] : 0.0f;
#pragma unroll
        for (int t = 0; t < SP_NT; ++t) { const int p = p0 + 32 * t + li; b[t] = (kin && p < D.P) ? D.feat[(size_t)k * D.P + p] : 0.0f; }
    };
    float a_nx, b_nx[SP_NT];
    load(0, a_nx, b_nx);
    for (int k0 = 0; k0 < C; k0 += 2) {
        const float a = a_nx; float b[SP_NT];
#pragma unroll
        for (int t = 0; t < SP_NT; ++t) b[t] = b_nx[t];
        if (k0 + 2 < C) load(k0 + 2, a_nx, b_nx);
#pragma unroll
        for (int t = 0; t < SP_NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < SP_NT; ++t) {
        const int p = p0 + 32 * t + li;
        if (p0 + 32 * t >= D.P) break;                // wave-uniform: the tile lies beyond the last word
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            const float seg = 1.0f / (1.0f + expf(-acc[t][r]));      // torch's sigmoid; expf is the accurate one
            const bool in = p < D.P && row < n_rows;
            if (STORE) {
                if (in) D.seg[(size_t)row * D.P + p] = seg;
            } else {
                const bool hit = in && seg > D.mask_thr;
                const unsigned long long b = __ballot(hit);
                float s = hit ? seg : 0.0f;
#pragma unroll
                for (int d = 16; d >= 1; d >>= 1) s += __shfl_xor(s, d);      // a fixed tree over the 32 lanes of the row
                if (li == 0 && row < n_rows) {
                    const size_t o = (size_t)row * D.Wn + (size_t)((p0 >> 5) + t);
                    D.masks[o] = (uint32_t)(b >> (32 * kh)); D.psum[o] = s;
                }
            }
        }
    }
}

// a wave per candidate: sum_mask (an exact integer as float), the float sum of seg * mask in a fixed order, the pixel floor and the score
__global__ __launch_bounds__(256) void solo_sums_kernel(SoloDev D) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= D.hdr[H_NCAND]) return;
    int cnt = 0; float s = 0.0f;
    for (int w = lane; w < D.Wn; w += 64) { cnt += __popc(D.masks[(size_t)c * D.Wn + w]); s += D.psum[(size_t)c * D.Wn + w]; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { cnt += __shfl_xor(cnt, d); s += __shfl_xor(s, d); }
    if (lane == 0) {
        const float sum = (float)cnt;
        const bool keep = sum > D.cand_floor[c];
        D.cand_sum[c] = sum;
        D.cand_score[c] = keep ? D.cand_cate[c] * (s / sum) : -INFINITY;
    }
}

// one workgroup: rank of every kept candidate among the kept ones, descending score, equal scores in candidate order; the first nms_pre are written in that order
__global__ __launch_bounds__(1024) void solo_sort_kernel(SoloDev D) {
    __shared__ float s_sc[DV_SOLO_MAX_CANDIDATES];
    __shared__ int s_kept;
    const int n = D.hdr[H_NCAND];
    if (threadIdx.x == 0) s_kept = 0;
    for (int i = threadIdx.x; i < n; i += 1024) s_sc[i] = D.cand_score[i];
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += 1024) {
        const float v = s_sc[c];
        if (!(v > -INFINITY)) continue;
        int rank = 0;
        for (int d = 0; d < n; ++d) { const float u = s_sc[d]; rank += (u > v) || (u == v && d < c); }
        if (rank < D.nms_pre) D.order[rank] = c;
        atomicAdd(&s_kept, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) { D.hdr[H_NFLOOR] = s_kept; D.hdr[H_NSORT] = min(s_kept, D.nms_pre); }
}

// inter[i][j] = |mask_i & mask_j| for the sorted candidates, tiles of 16 x 16 pairs with bj >= bi (the upper triangle is all Matrix NMS reads); exact integers
__global__ __launch_bounds__(256) void solo_inter_kernel(SoloDev D) {
    const int n = D.hdr[H_NSORT], bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi || bi * 16 >= n || bj * 16 >= n) return;
    __shared__ uint32_t sa[16][65], sb[16][65];
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    int acc = 0;
    for (int w0 = 0; w0 < D.Wn; w0 += 64) {
        for (int e = threadIdx.x; e < 1024; e += 256) {
            const int r = e >> 6, w = w0 + (e & 63);
            const int ia = bi * 16 + r, ib = bj * 16 + r;
            sa[r][e & 63] = (ia < n && w < D.Wn) ? D.masks[(size_t)D.order[ia] * D.Wn + w] : 0u;
            sb[r][e & 63] = (ib < n && w < D.Wn) ? D.masks[(size_t)D.order[ib] * D.Wn + w] : 0u;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 64; ++k) acc += __popc(sa[ti][k] & sb[tj][k]);
        __syncthreads();
    }
    const int i = bi * 16 + ti, j = bj * 16 + tj;
    if (i < n && j < n) D.inter[i * DV_SOLO_MAX_NMS_PRE + j] = acc;
}

// Matrix NMS on one workgroup, a thread per column j (n <= 512), then the second filter and sort.  decay_iou[i][j] = iou[i][j] for i < j with equal labels, else 0;
// comp[j] = max over i of decay_iou[i][j]; coefficient[j] = min over ALL i of f(decay_iou[i][j]) / f(comp[i]) — rows i >= j contribute f(0) / f(comp[i]) as in the
// reference — with a NaN carried as the tensor library's min carries it
__global__ __launch_bounds__(512) void solo_nms_kernel(SoloDev D) {
    __shared__ float s_sum[DV_SOLO_MAX_NMS_PRE], s_comp[DV_SOLO_MAX_NMS_PRE], s_new[DV_SOLO_MAX_NMS_PRE];
    __shared__ int s_lab[DV_SOLO_MAX_NMS_PRE], s_kept;
    const int n = D.hdr[H_NSORT], j = threadIdx.x;
    const bool gauss = D.nms_kernel == DV_SOLO_NMS_GAUSSIAN;
    if (j == 0) s_kept = 0;
    int cand = 0; float score = 0.0f;
    if (j < n) { cand = D.order[j]; s_sum[j] = D.cand_sum[cand]; s_lab[j] = D.cand_label[cand]; score = D.cand_score[cand]; }
    __syncthreads();
    if (j < n) {
        float comp = 0.0f;
        for (int i = 0; i < j; ++i) {
            const float in = (float)D.inter[i * DV_SOLO_MAX_NMS_PRE + j];
            const float iou = in / (s_sum[j] + s_sum[i] - in);
            const float d = iou * (s_lab[i] == s_lab[j] ? 1.0f : 0.0f);
            if (d > comp || d != d) comp = d;
        }
        s_comp[j] = comp;
    }
    __syncthreads();
    if (j < n) {
        float coef = INFINITY;
        for (int i = 0; i < n; ++i) {
            float d = 0.0f;
            if (i < j) {
                const float in = (float)D.inter[i * DV_SOLO_MAX_NMS_PRE + j];
                d = (in / (s_sum[j] + s_sum[i] - in)) * (s_lab[i] == s_lab[j] ? 1.0f : 0.0f);
            }
            const float ci = s_comp[i];
            const float v = gauss ? expf(-D.sigma * (d * d)) / expf(-D.sigma * (ci * ci)) : (1.0f - d) / (1.0f - ci);
            if (coef == coef && (v < coef || v != v)) coef = v;
        }
        const float upd = score * coef;
        s_new[j] = upd >= D.update_thr ? upd : -INFINITY;      // (a NaN fails the test, as in the reference)
    }
    __syncthreads();
    if (j < n && s_new[j] > -INFINITY) {
        const float v = s_new[j];
        int rank = 0;
        for (int d = 0; d < n; ++d) { const float u = s_new[d]; rank += (u > v) || (u == v && d < j); }
        if (rank < D.max_per_img) { D.out_i[4 + rank] = s_lab[j]; D.out_i[4 + DV_SOLO_MAX_PER_IMG + rank] = cand; D.out_score[rank] = v; }
        atomicAdd(&s_kept, 1);
    }
    __syncthreads();
    if (j == 0) {
        const int ns = min(s_kept, D.max_per_img);
        D.hdr[H_NSURV] = ns;
        D.out_i[0] = ns; D.out_i[1] = D.hdr[H_NPASS]; D.out_i[2] = D.hdr[H_OVER]; D.out_i[3] = D.hdr[H_NFLOOR];
    }
}

// upsample_bilinear2d's source index and weights, align_corners = true, float32 (guard_index_and_lambda)
__device__ __forceinline__ void lin_src(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
    const float src = scale * (float)dst;
    i0 = min((int)src, in - 1); i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f); l0 = 1.0f - l1;
}
struct SoloResample { int rect_x, rect_y, rect_w, rect_h, ow, oh, pitch; float s1y, s1x, s2y, s2x; uint8_t* planes; };
// the 4 x intermediate at (y, x), from the survivor's seg plane: h0 (w0 a + w1 b) + h1 (w0 c + w1 d)
__device__ __forceinline__ float solo_mid(const float* __restrict__ seg, int fh, int fw, float s1y, float s1x, int y, int x) {
    int y0, y1, x0, x1; float hy0, hy1, wx0, wx1;
    lin_src(s1y, y, fh, y0, y1, hy0, hy1); lin_src(s1x, x, fw, x0, x1, wx0, wx1);
    const float* r0 = seg + (size_t)y0 * fw; const float* r1 = seg + (size_t)y1 * fw;
    return hy0 * (wx0 * r0[x0] + wx1 * r0[x1]) + hy1 * (wx0 * r1[x0] + wx1 * r1[x1]);
}
// blockIdx.z = survivor.  A lane owns the 4 output pixels c .. c + 3 of one row and writes them as one dword (rows are `pitch` bytes, a multiple of 4; the bytes beyond
// the image width are written as zero).  Each output pixel reads its four intermediate pixels' four sources: the intermediate is never stored.
__global__ __launch_bounds__(256) void solo_resample_kernel(SoloDev D, SoloResample R) {
    const int s = blockIdx.z;
    if (s >= D.hdr[H_NSURV]) return;
    const int c = (blockIdx.x * 64 + threadIdx.x) * 4, Y = blockIdx.y * 4 + threadIdx.y;
    if (c >= R.pitch || Y >= R.oh) return;
    const float* seg = D.seg + (size_t)s * D.P;
    int y0, y1; float hy0, hy1;
    lin_src(R.s2y, Y, R.rect_h, y0, y1, hy0, hy1);
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int X = c + i;
        if (X >= R.ow) break;
        int x0, x1; float wx0, wx1;
        lin_src(R.s2x, X, R.rect_w, x0, x1, wx0, wx1);
        const float a = solo_mid(seg, D.fh, D.fw, R.s1y, R.s1x, R.rect_y + y0, R.rect_x + x0), b = solo_mid(seg, D.fh, D.fw, R.s1y, R.s1x, R.rect_y + y0, R.rect_x + x1);
        const float e = solo_mid(seg, D.fh, D.fw, R.s1y, R.s1x, R.rect_y + y1, R.rect_x + x0), f = solo_mid(seg, D.fh, D.fw, R.s1y, R.s1x, R.rect_y + y1, R.rect_x + x1);
        const float v = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * e + wx1 * f);
        if (v > D.mask_thr) out |= 1u << (8 * i);
    }
    *reinterpret_cast<uint32_t*>(R.planes + ((size_t)s * R.oh + Y) * R.pitch + c) = out;
}

}  // namespace

// Two plane sets used alternately (set[cur] belongs to the frame enqueued last); everything else is work memory of the stage in flight.
struct SoloHeadFrame {
    DevBuf planes[2], work, staged;
    int cur = 1;
    PinBuf pinned;      // out_i (4 + 128 + 128 ints) | scores (128 floats)
    StageSlot slot;
    int ow = 0, oh = 0, pitch = 0;
};
constexpr size_t SOLO_OUT_INTS = 4 + 2 * DV_SOLO_MAX_PER_IMG, SOLO_OUT_BYTES = SOLO_OUT_INTS * 4 + DV_SOLO_MAX_PER_IMG * 4;

void dv_stage_delete(SoloHeadFrame* p) { delete p; }

extern "C" {

int dv_solo_rect(int model_w, int model_h, int img_w, int img_h, int* rect_x, int* rect_y, int* rect_w, int* rect_h) {
    dv_ctx* ctx = nullptr;
    if (dv_solo_rect_host(model_w, model_h, img_w, img_h, rect_x, rect_y, rect_w, rect_h)) DV_FAIL("dv_solo_rect: bad argument");
    return 0;
}

int dv_solo_check(const dv_solo_outputs* out, const dv_solo_params* par) {
    dv_ctx* ctx = nullptr;
    if (const char* why = dv_solo_check_host(out, par)) DV_FAIL(std::string("dv_solo_check: ") + why);
    return 0;
}

int dv_solo_head_enqueue(dv_ctx* ctx, const dv_solo_outputs* out, const dv_solo_params* par) {
    if (!ctx) return -1;
    if (const char* why = dv_solo_check_host(out, par)) DV_FAIL(std::string("dv_solo_head_enqueue: ") + why);
    if (!ctx->solo) ctx->solo = new SoloHeadFrame();
    SoloHeadFrame& V = *ctx->solo;
    if (V.slot.open(ctx, "dv_solo_head_enqueue: previous frame not collected")) return -1;
    hipStream_t s = ctx->stream;
    DV_CHECK(V.pinned.ensure(SOLO_OUT_BYTES));

    DvSoloTables T;
    dv_solo_tables(out, par, &T);
    SoloDev D{};
    D.n_levels = out->n_levels; D.channels = out->channels; D.n_classes = out->n_classes; D.n_cells = T.cell_off[out->n_levels];
    D.fh = out->fh; D.fw = out->fw; D.P = out->fh * out->fw; D.Wn = (D.P + 31) / 32;
    D.score_thr = par->score_thr; D.mask_thr = par->mask_thr; D.update_thr = par->update_thr; D.sigma = par->nms_sigma;
    D.nms_pre = par->nms_pre; D.max_per_img = par->max_per_img; D.nms_kernel = par->nms_kernel; D.max_cand = par->max_candidates;
    for (int l = 0; l <= DV_SOLO_MAX_LEVELS; ++l) D.cell_off[l] = T.cell_off[l];
    for (int l = 0; l < DV_SOLO_MAX_LEVELS; ++l) { D.floor_end[l] = T.floor_end[l]; D.floor_val[l] = par->strides[l]; }

    // the tensors: read in place, or staged (a DV_MEM_HOST set) one behind the other
    if (out->mem == DV_MEM_HOST) {
        size_t total = (size_t)D.channels * D.P;
        for (int l = 0; l < D.n_levels; ++l) total += (size_t)(D.channels + D.n_classes) * out->grid[l] * out->grid[l];
        DV_CHECK(V.staged.ensure(total * 4));
        float* d = (float*)V.staged.p;
        auto put = [&](const float* src, size_t n, const float** dst) -> hipError_t { *dst = d; hipError_t e = hipMemcpyAsync(d, src, n * 4, hipMemcpyHostToDevice, s); d += n; return e; };
        for (int l = 0; l < D.n_levels; ++l) {
            const size_t g2 = (size_t)out->grid[l] * out->grid[l];
            DV_CHECK(put(out->kernel[l], D.channels * g2, &D.kern[l]));
            DV_CHECK(put(out->cate[l], D.n_classes * g2, &D.cate[l]));
        }
        DV_CHECK(put(out->feature, (size_t)D.channels * D.P, &D.feat));
    } else {
        for (int l = 0; l < D.n_levels; ++l) { D.kern[l] = out->kernel[l]; D.cate[l] = out->cate[l]; }
        D.feat = out->feature;
    }

    // work memory, carved once per size
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const size_t mc = (size_t)D.max_cand;
    const size_t o_hdr = take(64), o_cnt = take((size_t)D.n_cells * 4), o_pos = take((size_t)D.n_cells * 4), o_cell = take(mc * 4), o_lab = take(mc * 4), o_cate = take(mc * 4),
                 o_floor = take(mc * 4), o_sum = take(mc * 4), o_score = take(mc * 4), o_masks = take(mc * D.Wn * 4), o_psum = take(mc * D.Wn * 4),
                 o_order = take(DV_SOLO_MAX_NMS_PRE * 4), o_inter = take((size_t)DV_SOLO_MAX_NMS_PRE * DV_SOLO_MAX_NMS_PRE * 4), o_out = take(SOLO_OUT_BYTES),
                 o_seg = take((size_t)D.max_per_img * D.P * 4);
    DV_CHECK(V.work.ensure(off));
    uint8_t* wb = (uint8_t*)V.work.p;
    D.hdr = (int*)(wb + o_hdr); D.cell_cnt = (int*)(wb + o_cnt); D.cell_pos = (int*)(wb + o_pos); D.cand_cell = (int*)(wb + o_cell); D.cand_label = (int*)(wb + o_lab);
    D.cand_cate = (float*)(wb + o_cate); D.cand_floor = (float*)(wb + o_floor); D.cand_sum = (float*)(wb + o_sum); D.cand_score = (float*)(wb + o_score);
    D.masks = (uint32_t*)(wb + o_masks); D.psum = (float*)(wb + o_psum); D.order = (int*)(wb + o_order); D.inter = (int*)(wb + o_inter);
    D.out_i = (int*)(wb + o_out); D.out_score = (float*)(wb + o_out + SOLO_OUT_INTS * 4); D.seg = (float*)(wb + o_seg);

    SoloResample R{};
    R.rect_x = par->rect_x; R.rect_y = par->rect_y; R.rect_w = par->rect_w; R.rect_h = par->rect_h; R.ow = par->origin_w; R.oh = par->origin_h; R.pitch = align_up(par->origin_w, 4);
    R.s1y = dv_solo_scale(D.fh, 4 * D.fh); R.s1x = dv_solo_scale(D.fw, 4 * D.fw); R.s2y = dv_solo_scale(R.rect_h, R.oh); R.s2x = dv_solo_scale(R.rect_w, R.ow);
    DevBuf& PB = V.planes[V.cur ^ 1];
    DV_CHECK(PB.ensure((size_t)D.max_per_img * R.oh * R.pitch));
    R.planes = (uint8_t*)PB.p;

    {
        StageScope sc_t(ctx, "solo_head");
        const int cell_blocks = (D.n_cells + 255) / 256, row_tiles = (D.max_cand + 31) / 32, col_blocks = (D.P + 4 * SP_COLS - 1) / (4 * SP_COLS);
        const int pair_tiles = (D.nms_pre + 15) / 16;
        hipLaunchKernelGGL(solo_count_kernel, dim3(cell_blocks), dim3(256), 0, s, D);
        hipLaunchKernelGGL(solo_scan_kernel, dim3(1), dim3(1024), 0, s, D);
        hipLaunchKernelGGL(solo_emit_kernel, dim3(cell_blocks), dim3(256), 0, s, D);
        hipLaunchKernelGGL(solo_product_kernel<false>, dim3(col_blocks, row_tiles), dim3(256), 0, s, D);
        hipLaunchKernelGGL(solo_sums_kernel, dim3((D.max_cand + 3) / 4), dim3(256), 0, s, D);
        hipLaunchKernelGGL(solo_sort_kernel, dim3(1), dim3(1024), 0, s, D);
        hipLaunchKernelGGL(solo_inter_kernel, dim3(pair_tiles, pair_tiles), dim3(256), 0, s, D);
        hipLaunchKernelGGL(solo_nms_kernel, dim3(1), dim3(512), 0, s, D);
        hipLaunchKernelGGL((solo_product_kernel<true>), dim3(col_blocks, (D.max_per_img + 31) / 32), dim3(256), 0, s, D);
        hipLaunchKernelGGL(solo_resample_kernel, dim3((R.pitch / 4 + 63) / 64, (R.oh + 3) / 4, D.max_per_img), dim3(64, 4), 0, s, D, R);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = dv_copy_async(V.pinned.p, D.out_i, SOLO_OUT_BYTES, s);
    if (V.slot.close(ctx, e, s)) return -1;
    V.cur ^= 1; V.ow = R.ow; V.oh = R.oh; V.pitch = R.pitch;
    return 0;
}

int dv_solo_head_collect(dv_ctx* ctx, int32_t* labels, float* scores, int cap, int* n, int* n_candidates, dv_mask_stack* stack) {
    if (!ctx) return -1;
    if (!ctx->solo || !ctx->solo->slot.pending) DV_FAIL("dv_solo_head_collect: nothing enqueued");
    if (!n || cap < 0 || (cap > 0 && (!labels || !scores))) DV_FAIL("dv_solo_head_collect: bad argument");
    SoloHeadFrame& V = *ctx->solo;
    if (V.slot.wait(ctx)) return -1;
    const int32_t* oi = (const int32_t*)V.pinned.p;
    const float* os = (const float*)(V.pinned.p + SOLO_OUT_INTS * 4);
    if (n_candidates) *n_candidates = oi[1];
    *n = 0;
    if (stack) *stack = dv_mask_stack{};
    if (oi[2]) DV_FAIL("dv_solo_head_collect: " + std::to_string(oi[1]) + " cells pass score_thr, more than max_candidates: the frame is dropped (no planes)");
    const int ns = oi[0];
    if (ns < 0 || ns > DV_SOLO_MAX_PER_IMG) DV_FAIL("dv_solo_head_collect: corrupt survivor count");
    *n = ns;
    for (int i = 0; i < ns && i < cap; ++i) { labels[i] = oi[4 + i]; scores[i] = os[i]; }
    if (stack) {
        stack->data = V.planes[V.cur].p; stack->n_planes = ns < DV_STACK_MAX_PLANES ? ns : DV_STACK_MAX_PLANES; stack->kind = DV_STACK_U8; stack->mem = DV_MEM_DEVICE;
        stack->row_stride = V.pitch; stack->plane_stride = (int64_t)V.pitch * V.oh; stack->threshold = 0.0f;
    }
    return 0;
}

}  // extern "C"
