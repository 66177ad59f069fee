// mot.hip — the multi-object tracker on gfx950: a frame's detection rectangles and appearance embeddings -> a track id per detection.  Reference: DeepSORT::update
// (mot/deep_sort.cpp:72-139) over TrackerManager (mot/tracker_manager.h:40-156, mot/tracker_manager.cpp:20-69), KalmanTracker (mot/kalman_tracker.cpp:20-96),
// FeatureBundle / FeatureMetric (mot/feature_bundle.h:40-50, mot/feature_metric.h:32-61) and HungarianAlgorithm (mot/hungarian.cpp), restated step by step as the
// reference evaluates them (include/dvins.h has the rule; the rules shared with the host are in mot_host.h).  Track table and galleries are resident; kernels, in stream order:
//   mot_feat_kernel    a workgroup per gallery slot in use: (stored rows) x (detections) over feat_dim on v_mfma_f32_32x32x2_f32, a wave per 32 rows, and the minimum of
//                      1 - g . f over the slot's VALID rows in the epilogue.  Rows at or past the ring's count are excluded by index: their A operand is never loaded.
//                      The minimum carries a NaN as torch::min does (feature_metric.h:59-61): a NaN in ONE valid row makes the slot's distance a NaN, which is gated.
//   mot_assoc_kernel   ONE workgroup: predict, remove_nan, both cost matrices and Munkres solves, miss / update with the filter's correct, births, the stable compaction of
//                      the table, the ring writes and the answer.  Everything is decided in LDS and registers first; the table is written only when the frame fits
//                      max_tracks, so a refused frame leaves it as it was.
//   mot_assign_kernel  the operator form of the Munkres solve alone (dv_mot_assign).
// Munkres runs in wave 0 with the reference's decisions in the reference's order: the cost matrix is column-major in LDS as hungarian.cpp holds it, a lane owns rows
// lane and lane + 64, "the first uncovered row with a zero in this column" is a ballot, and the covers are three 64-bit masks.  min and subtraction in double are exact
// whatever the order, so only the decisions need the order.  One star per row and column and one prime per row (a primed row is covered at once or ends the pass) let
// rowstar / colstar / rowprime stand for the three bool matrices.
#include "dv_ctx.h"
#include "mot_host.h"
#include <string>
#include <vector>

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
constexpr int MT = DV_MOT_MAX_TRACKS, MD = DV_STACK_MAX_PLANES;
constexpr int MUNKRES_MAX_ROUNDS = 1 << 17;      // a finite non-negative matrix ends after <= min(R, C) augmentations with O(R + C) reductions each; a bound so that nothing can spin
enum { O_FAIL = 0, O_NTRACKS = 1, O_NCONF = 2, O_WOULD = 3, O_IDS = 16, O_WORDS = O_IDS + MD };      // the frame's device -> host words
enum { FAIL_CAPACITY = 1, FAIL_MUNKRES = 2 };

struct MotDev {
    int n_init, max_age, budget, F, max_tracks;
    int* hdr; float* x; float* P; int* state; int* id; int* hits; int* tsu; int* slot; int* next; int* full; int* slot_rows;
    float* gallery; float* featmin /* [max_tracks][MD] by slot */; int* out;
    const float* rects; const float* feats; int n;
};

__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// min that carries a NaN from either side (a plain `<` would skip one)
__device__ __forceinline__ float nan_min(float c, float m) { return (c < m || c != c) ? c : m; }

__global__ __launch_bounds__(256) void mot_feat_kernel(MotDev D) {
    __shared__ float smin[4][MD];
    const int slot = blockIdx.x, cnt = D.slot_rows[slot], n = D.n, F = D.F;
    if (cnt <= 0) return;                                   // workgroup-uniform: a free slot
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 31, kh = lane >> 5;
    const int row0 = 32 * wv;
    const float INF = __builtin_huge_valf();
    float m0 = INF, m1 = INF;
    if (row0 < cnt) {                                       // wave-uniform
        const float* arow = row0 + li < cnt ? D.gallery + ((size_t)slot * D.budget + row0 + li) * F : nullptr;
        const float* b0 = li < n ? D.feats + (size_t)li * F : nullptr;
        const float* b1 = li + 32 < n ? D.feats + (size_t)(li + 32) * F : nullptr;
        const bool two = n > 32;
        floatx16 acc0, acc1;
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
        // a lane brings 4 consecutive k per step (its half of 8): instruction e multiplies k0 + e of the low half wave and k0 + 4 + e of the high one
        for (int k0 = 0; k0 < F; k0 += 8) {
            float a[4], u[4], v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + 4 * kh + e;
                const bool in = k < F;                      // the K tail
                a[e] = (arow && in) ? arow[k] : 0.0f;
                u[e] = (b0 && in) ? b0[k] : 0.0f;
                v[e] = (b1 && in) ? b1[k] : 0.0f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], u[e], acc0, 0, 0, 0);
                if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], v[e], acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (row < cnt) {
                const float c0 = 1.0f - acc0[r], c1 = 1.0f - acc1[r];
                m0 = nan_min(c0, m0); m1 = nan_min(c1, m1);
            }
        }
        const float o0 = __shfl_xor(m0, 32), o1 = __shfl_xor(m1, 32);
        m0 = nan_min(o0, m0); m1 = nan_min(o1, m1);
    }
    if (kh == 0) { smin[wv][li] = m0; smin[wv][32 + li] = m1; }
    __syncthreads();
    if (threadIdx.x < MD) {
        float m = smin[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) { m = nan_min(smin[w][threadIdx.x], m); }
        D.featmin[(size_t)slot * MD + threadIdx.x] = m;
    }
}

// HungarianAlgorithm::assignmentoptimal for ONE wave (all 64 lanes, wave-uniform control flow).  d: R x C, column-major (d[row + R * col]), modified in place.
// rowstar[row] = the assigned column or -1 on return.  Returns false when MUNKRES_MAX_ROUNDS ran out.
__device__ bool munkres_wave(double* d, int* rowstar, int* rowprime, int* colstar, const int R, const int C, const int lane) {
    for (int r = lane; r < R; r += 64) { rowstar[r] = -1; rowprime[r] = -1; }
    if (lane < C) colstar[lane] = -1;
    wave_sync();
    if (R == 0 || C == 0) return true;
    unsigned long long covC = 0, covR0 = 0, covR1 = 0;
    const int r0 = lane, r1 = lane + 64;
    const bool has0 = r0 < R, has1 = r1 < R;
    const double INF = __builtin_huge_val();
    auto wave_min = [&](double v) { for (int s = 32; s >= 1; s >>= 1) { const double o = __shfl_xor(v, s); v = o < v ? o : v; } return v; };
    // the first row, not covered, with a zero in column col (-1: none)
    auto first_zero_row = [&](int col) -> int {
        const bool z0 = has0 && !((covR0 >> lane) & 1) && fabs(d[r0 + R * col]) < DBL_EPSILON;
        unsigned long long b = __ballot(z0);
        if (b) return __ffsll((long long)b) - 1;
        if (R > 64) {
            const bool z1 = has1 && !((covR1 >> lane) & 1) && fabs(d[r1 + R * col]) < DBL_EPSILON;
            b = __ballot(z1);
            if (b) return 64 + __ffsll((long long)b) - 1;
        }
        return -1;
    };
    auto cover_row = [&](int row) { if (row < 64) covR0 |= 1ull << row; else covR1 |= 1ull << (row - 64); };
    int minDim;
    if (R <= C) {
        minDim = R;
        if (has0) {                                          // R <= 64: a lane per row
            double m = d[r0];
            for (int c = 1; c < C; ++c) { const double v = d[r0 + R * c]; if (v < m) m = v; }
            for (int c = 0; c < C; ++c) d[r0 + R * c] -= m;
        }
        wave_sync();
        for (int row = 0; row < R; ++row) {                  // steps 1 and 2a: by row, the first zero in a column not covered yet (a lane per column)
            const bool z = lane < C && fabs(d[row + R * lane]) < DBL_EPSILON;
            const unsigned long long b = __ballot(z) & ~covC;
            if (b) { const int c = __ffsll((long long)b) - 1; rowstar[row] = c; colstar[c] = row; covC |= 1ull << c; }
        }
    } else {
        minDim = C;
        for (int c = 0; c < C; ++c) {
            const double v0 = has0 ? d[r0 + R * c] : INF, v1 = has1 ? d[r1 + R * c] : INF;
            const double m = wave_min(v1 < v0 ? v1 : v0);
            if (has0) d[r0 + R * c] = v0 - m;
            if (has1) d[r1 + R * c] = v1 - m;
        }
        wave_sync();
        for (int c = 0; c < C; ++c) {                        // by column, the first zero in a row not covered yet
            const int row = first_zero_row(c);
            if (row >= 0) { rowstar[row] = c; colstar[c] = row; covC |= 1ull << c; cover_row(row); }
        }
        covR0 = covR1 = 0;
    }
    wave_sync();
    for (int round = 0; round < MUNKRES_MAX_ROUNDS; ++round) {
        if (__popcll(covC) == minDim) return true;            // step 2b
        // step 3: passes over the columns in order; a primed zero whose row has a star covers the row and uncovers the star's column, the scan goes on with the NEXT column
        int prow = -1, pcol = -1;
        bool zeros = true;
        while (zeros && prow < 0) {
            zeros = false;
            for (int c = 0; c < C; ++c) {
                if ((covC >> c) & 1) continue;
                const int row = first_zero_row(c);
                if (row < 0) continue;
                rowprime[row] = c;
                wave_sync();
                const int sc = rowstar[row];
                if (sc < 0) { prow = row; pcol = c; break; }
                cover_row(row); covC &= ~(1ull << sc); zeros = true;
            }
        }
        if (prow >= 0) {
            // step 4: the alternating path from the primed zero; a column is met once, so the stars move in place
            int r = prow, c = pcol;
            for (int guard = 0; guard <= C; ++guard) {
                const int prev = colstar[c];
                wave_sync();
                colstar[c] = r; rowstar[r] = c;
                wave_sync();
                if (prev < 0) break;
                r = prev; c = rowprime[r];
                if (c < 0) break;
            }
            for (int q = lane; q < R; q += 64) rowprime[q] = -1;
            covR0 = covR1 = 0;
            wave_sync();
            covC |= __ballot(lane < C && colstar[lane] >= 0);      // step 2a
        } else {
            // step 5: h = the smallest element not covered; + h on covered rows, then - h on uncovered columns, in that order as the reference rounds it
            double h = DBL_MAX;
            const bool u0 = has0 && !((covR0 >> lane) & 1), u1 = has1 && !((covR1 >> lane) & 1);
            for (int c = 0; c < C; ++c) {
                if ((covC >> c) & 1) continue;
                if (u0) { const double v = d[r0 + R * c]; if (v < h) h = v; }
                if (u1) { const double v = d[r1 + R * c]; if (v < h) h = v; }
            }
            h = wave_min(h);
            for (int c = 0; c < C; ++c) {
                const bool cc = (covC >> c) & 1;
                if (has0) { double v = d[r0 + R * c]; if (!u0) v += h; if (!cc) v -= h; d[r0 + R * c] = v; }
                if (has1) { double v = d[r1 + R * c]; if (!u1) v += h; if (!cc) v -= h; d[r1 + R * c] = v; }
            }
            wave_sync();
        }
    }
    return false;
}

// rank of a flagged thread among the flagged threads of the workgroup (256 threads), and their number
__device__ __forceinline__ int block_rank(bool f, int* s_cnt, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    __syncthreads();
    if (lane == 0) s_cnt[wv] = __popcll(b);
    __syncthreads();
    int off = 0, sum = 0;
    for (int w = 0; w < 4; ++w) { const int c = s_cnt[w]; if (w < wv) off += c; sum += c; }
    *total = sum;
    return off + __popcll(b & ((1ull << lane) - 1));
}

struct MunkresLds { double d[MT * MD]; int rowstar[MT], rowprime[MT], colstar[MD]; int ok; };

__global__ __launch_bounds__(64) void mot_assign_kernel(const float* cost, int R, int C, int* assignment, int* status) {
    __shared__ MunkresLds M;
    const int lane = threadIdx.x;
    for (int e = lane; e < R * C; e += 64) { const int i = e / C, j = e % C; M.d[i + R * j] = (double)cost[e]; }
    wave_sync();
    const bool ok = munkres_wave(M.d, M.rowstar, M.rowprime, M.colstar, R, C, lane);
    wave_sync();
    for (int r = lane; r < R; r += 64) assignment[r] = M.rowstar[r];
    if (lane == 0) *status = ok ? 0 : FAIL_MUNKRES;
}

__global__ __launch_bounds__(256) void mot_assoc_kernel(MotDev D) {
    __shared__ MunkresLds M;
    __shared__ float s_ioud[MT * MD];                       // 1 - IoU, [track position after remove_nan][detection]
    __shared__ float s_trect[MT][4], s_drect[MD][4];
    __shared__ int s_tstate[MT], s_thits[MT], s_tslot[MT], s_tdet[MT], s_tnewid[MT], s_rows[MT];
    __shared__ int s_cols[MD], s_detm[MD], s_colidx[MD], s_free[MT];
    __shared__ int s_pslot[MT + MD], s_prow[MT + MD], s_pdet[MT + MD];      // the ring writes: a matched track by position, then a birth by column
    __shared__ int s_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int nT = D.hdr[DV_MOT_H_NTRACKS], next_id = D.hdr[DV_MOT_H_NEXT_ID], n = D.n;

    // predict, rect(), remove_nan: thread t owns the track at table position t for the whole frame
    float x[7], P[49];
    int st = DV_MOT_DELETED, id = -1, hits = 0, tsu = 0, slot = -1, nxt = 0, full = 0;
    bool alive = false;
    if (t < nT) {
        for (int i = 0; i < 7; ++i) x[i] = D.x[t * 7 + i];
        for (int i = 0; i < 49; ++i) P[i] = D.P[t * 49 + i];
        st = D.state[t]; id = D.id[t]; hits = D.hits[t]; tsu = D.tsu[t] + 1; slot = D.slot[t]; nxt = D.next[t]; full = D.full[t];
        // x' = A x, P' = A P A^T + Q: A = I plus ones at (0,4), (1,5), (2,6); its zero products are left out (exact for finite values)
        for (int i = 0; i < 3; ++i) x[i] = x[i] + x[i + 4];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 7; ++j) P[i * 7 + j] = P[i * 7 + j] + P[(i + 4) * 7 + j];
        for (int i = 0; i < 7; ++i) for (int j = 0; j < 3; ++j) P[i * 7 + j] = P[i * 7 + j] + P[i * 7 + j + 4];
        for (int i = 0; i < 7; ++i) P[i * 7 + i] += 1e-2f;
        float r[4];
        dv_mot_rect_of(x, r);
        alive = !dv_mot_rect_nan(r);
    }
    int n1;
    const int p = block_rank(alive, s_cnt, &n1);
    if (alive) {
        float r[4];
        dv_mot_rect_of(x, r);
        for (int i = 0; i < 4; ++i) s_trect[p][i] = r[i];
        s_tstate[p] = st; s_thits[p] = hits; s_tslot[p] = slot; s_tdet[p] = -1; s_tnewid[p] = -1;
    }
    if (t < MD) {
        s_detm[t] = 0; s_colidx[t] = 0;
        if (t < n) { for (int i = 0; i < 4; ++i) s_drect[t][i] = D.rects[t * 4 + i]; D.out[O_IDS + t] = -1; }
    }
    for (int e = t; e < MT + MD; e += 256) s_pdet[e] = -1;
    __syncthreads();
    for (int e = t; e < n1 * n; e += 256) { const int pp = e / n, j = e % n; s_ioud[pp * MD + j] = dv_mot_iou_dist(s_trect[pp], s_drect[j]); }

    // stage 1: the Confirmed tracks against all detections, appearance cost
    int R1;
    const int k1 = block_rank(alive && st == DV_MOT_CONFIRMED, s_cnt, &R1);
    if (alive && st == DV_MOT_CONFIRMED) s_rows[k1] = p;
    __syncthreads();
    auto cost1 = [&](int pp, int j) { return dv_mot_cost1(s_ioud[pp * MD + j], D.featmin[(size_t)s_tslot[pp] * MD + j]); };
    for (int e = t; e < R1 * n; e += 256) { const int i = e % R1, j = e / R1; M.d[e] = (double)cost1(s_rows[i], j); }
    if (t == 0) M.ok = 1;
    __syncthreads();
    if (wv == 0 && R1 > 0) { if (!munkres_wave(M.d, M.rowstar, M.rowprime, M.colstar, R1, n, lane) && lane == 0) M.ok = 0; }
    __syncthreads();
    if (t < R1) {
        const int pp = s_rows[t], c = M.rowstar[t];
        if (c >= 0 && !(cost1(pp, c) > DV_MOT_INVALID_DIST / 10)) { s_tdet[pp] = c; s_detm[c] = 1; }
    }
    __syncthreads();

    // stage 2: what stage 1 left, then the Tentative tracks, against the detections still unmatched; IoU cost
    int RA, RB, C2;
    const bool inA = alive && st == DV_MOT_CONFIRMED && s_tdet[p] < 0, inB = alive && st == DV_MOT_TENTATIVE;
    const int kA = block_rank(inA, s_cnt, &RA);
    const int kB = block_rank(inB, s_cnt, &RB);
    const int kC = block_rank(t < n && !s_detm[t], s_cnt, &C2);
    __syncthreads();                                         // (s_rows of stage 1 has been read by everyone)
    if (inA) s_rows[kA] = p;
    if (inB) s_rows[RA + kB] = p;
    if (t < n && !s_detm[t]) s_cols[kC] = t;
    const int R2 = RA + RB;
    __syncthreads();
    auto cost2 = [&](int pp, int j) { return dv_mot_cost2(s_ioud[pp * MD + j]); };
    for (int e = t; e < R2 * C2; e += 256) { const int i = e % R2, k = e / R2; M.d[e] = (double)cost2(s_rows[i], s_cols[k]); }
    __syncthreads();
    if (wv == 0 && R2 > 0) { if (!munkres_wave(M.d, M.rowstar, M.rowprime, M.colstar, R2, C2, lane) && lane == 0) M.ok = 0; }
    __syncthreads();
    bool newconf = false;
    if (t < R2) {
        const int pp = s_rows[t], c = M.rowstar[t];
        if (c >= 0 && !(cost2(pp, s_cols[c]) > DV_MOT_INVALID_DIST / 10)) {
            s_tdet[pp] = s_cols[c];
            s_colidx[c] = 1;                                 // the column INDEX: what the reference subtracts from the detection ids (tracker_manager.cpp:62-68)
            newconf = s_tstate[pp] == DV_MOT_TENTATIVE && s_thits[pp] + 1 > D.n_init;
        }
    }
    // ids in the order of `matched`: stage-1 pairs are Confirmed already, so the new ones are stage-2 rows in row order
    int n_new;
    const int knew = block_rank(newconf, s_cnt, &n_new);
    if (newconf) s_tnewid[s_rows[t]] = next_id + knew;
    __syncthreads();
    // births: the detections of stage 2's columns that no assigned column index names
    const bool born = t < C2 && !s_colidx[s_cols[t]];
    int nb;
    const int kb = block_rank(born, s_cnt, &nb);

    // miss / update with correct, by the track's owner
    int ring_row = -1, md = -1;
    if (alive) {
        md = s_tdet[p];
        if (md < 0) st = dv_mot_miss(st, tsu, D.max_age);
        else {
            tsu = 0; ++hits;
            if (s_tnewid[p] >= 0) { st = DV_MOT_CONFIRMED; id = s_tnewid[p]; }
            float z[4];
            dv_mot_measure(s_drect[md], z);
            // S = H P' H^T + R; Kt = S^-1 (H P') by Gaussian elimination with partial pivoting; x += K (z - H x'); P = P' - K (H P')
            float S[4][4], B[4][7], HP[4][7];
            for (int i = 0; i < 4; ++i) { for (int j = 0; j < 4; ++j) S[i][j] = P[i * 7 + j] + (i == j ? 1e-1f : 0.0f); for (int j = 0; j < 7; ++j) { HP[i][j] = P[i * 7 + j]; B[i][j] = HP[i][j]; } }
            for (int c = 0; c < 4; ++c) {
                int piv = c;
                for (int i = c + 1; i < 4; ++i) if (fabsf(S[i][c]) > fabsf(S[piv][c])) piv = i;
                for (int j = 0; j < 4; ++j) { const float a = S[c][j]; S[c][j] = S[piv][j]; S[piv][j] = a; }
                for (int j = 0; j < 7; ++j) { const float a = B[c][j]; B[c][j] = B[piv][j]; B[piv][j] = a; }
                for (int i = c + 1; i < 4; ++i) {
                    const float f = S[i][c] / S[c][c];
                    for (int j = c; j < 4; ++j) S[i][j] -= f * S[c][j];
                    for (int j = 0; j < 7; ++j) B[i][j] -= f * B[c][j];
                }
            }
            for (int c = 3; c >= 0; --c)
                for (int j = 0; j < 7; ++j) {
                    float s = B[c][j];
                    for (int k = c + 1; k < 4; ++k) s -= S[c][k] * B[k][j];
                    B[c][j] = s / S[c][c];
                }
            float y[4];
            for (int i = 0; i < 4; ++i) y[i] = z[i] - x[i];
            for (int i = 0; i < 7; ++i) { float s = 0.0f; for (int k = 0; k < 4; ++k) s += B[k][i] * y[k]; x[i] = x[i] + s; }
            for (int i = 0; i < 7; ++i) for (int j = 0; j < 7; ++j) { float s = 0.0f; for (int k = 0; k < 4; ++k) s += B[k][i] * HP[k][j]; P[i * 7 + j] = P[i * 7 + j] - s; }
            ring_row = dv_mot_ring_add(&nxt, &full, D.budget);
        }
    }
    const bool keep = alive && st != DV_MOT_DELETED;
    int nsurv, nconf;
    const int q = block_rank(keep, s_cnt, &nsurv);
    (void)block_rank(keep && st == DV_MOT_CONFIRMED, s_cnt, &nconf);
    const int total = nsurv + nb;
    if (total > D.max_tracks || !M.ok) {                     // workgroup-uniform: nothing of the table has been written
        if (t == 0) { D.out[O_FAIL] = M.ok ? FAIL_CAPACITY : FAIL_MUNKRES; D.out[O_WOULD] = total; D.out[O_NTRACKS] = nT; D.out[O_NCONF] = -1; }
        return;
    }

    // commit.  Slots of the tracks that leave are free before the births take theirs, lowest first
    if (t < nT && !keep) D.slot_rows[slot] = 0;
    __syncthreads();
    int nfree;
    const bool isfree = t < D.max_tracks && D.slot_rows[t] == 0;
    const int kf = block_rank(isfree, s_cnt, &nfree);
    if (isfree) s_free[kf] = t;
    __syncthreads();
    if (keep) {
        for (int i = 0; i < 7; ++i) D.x[q * 7 + i] = x[i];
        for (int i = 0; i < 49; ++i) D.P[q * 49 + i] = P[i];
        D.state[q] = st; D.id[q] = id; D.hits[q] = hits; D.tsu[q] = tsu; D.slot[q] = slot; D.next[q] = nxt; D.full[q] = full;
        if (md >= 0) {
            D.slot_rows[slot] = dv_mot_ring_rows(nxt, full, D.budget);
            s_pslot[p] = slot; s_prow[p] = ring_row; s_pdet[p] = md;
            if (st == DV_MOT_CONFIRMED) D.out[O_IDS + md] = id;
        }
    }
    if (born) {                                              // nsurv + nb <= max_tracks and every kept track holds a slot: kb < nfree
        const int pos = nsurv + kb, dj = s_cols[t], bs = s_free[kb];
        float z[4];
        dv_mot_measure(s_drect[dj], z);
        for (int i = 0; i < 7; ++i) D.x[pos * 7 + i] = i < 4 ? z[i] : 0.0f;
        for (int i = 0; i < 49; ++i) D.P[pos * 49 + i] = (i / 7 == i % 7) ? 1.0f : 0.0f;
        int bn = 0, bf = 0;
        const int brow = dv_mot_ring_add(&bn, &bf, D.budget);
        D.state[pos] = DV_MOT_TENTATIVE; D.id[pos] = -1; D.hits[pos] = 0; D.tsu[pos] = 0; D.slot[pos] = bs; D.next[pos] = bn; D.full[pos] = bf;
        D.slot_rows[bs] = dv_mot_ring_rows(bn, bf, D.budget);
        s_pslot[MT + t] = bs; s_prow[MT + t] = brow; s_pdet[MT + t] = dj;
    }
    if (t == 0) {
        D.hdr[DV_MOT_H_NTRACKS] = total; D.hdr[DV_MOT_H_NEXT_ID] = next_id + n_new;
        D.out[O_FAIL] = 0; D.out[O_NTRACKS] = total; D.out[O_NCONF] = nconf; D.out[O_WOULD] = total;
    }
    __syncthreads();
    // gallery: a wave per pair copies the detection's embedding into the track's ring row
    for (int e = wv; e < MT + MD; e += 4) {
        const int dj = s_pdet[e];
        if (dj < 0) continue;
        float* dst = D.gallery + ((size_t)s_pslot[e] * D.budget + s_prow[e]) * D.F;
        const float* src = D.feats + (size_t)dj * D.F;
        for (int k = lane; k < D.F; k += 64) dst[k] = src[k];
    }
}

__global__ void mot_reset_kernel(MotDev D) {
    const int t = threadIdx.x;
    if (t < DV_MOT_H_WORDS) D.hdr[t] = t == DV_MOT_H_NEXT_ID ? 1 : 0;
    if (t < D.max_tracks) D.slot_rows[t] = 0;
}

}  // namespace

struct MotTracker {
    dv_mot_params par{};
    DvMotLayout L{};
    DevBuf table, gallery, featmin, out, staged, op;
    MotDev D{};
    PinBuf pinned;      // O_WORDS ints
    StageSlot slot;
    bool configured = false; int pend_n = 0;
    int n_tracks = 0, n_confirmed = 0;
};

void dv_stage_delete(MotTracker* p) { delete p; }

static int mot_reset(dv_ctx* ctx, MotTracker& T) {
    hipLaunchKernelGGL(mot_reset_kernel, dim3(1), dim3(256), 0, ctx->stream, T.D);
    DV_CHECK(hipGetLastError());
    T.n_tracks = 0; T.n_confirmed = 0;
    return 0;
}

extern "C" {

int dv_mot_check(const dv_mot_params* par) {
    dv_ctx* ctx = nullptr;
    if (const char* why = dv_mot_check_host(par)) DV_FAIL(std::string("dv_mot_check: ") + why);
    return 0;
}

int dv_mot_config(dv_ctx* ctx, const dv_mot_params* par) {
    if (!ctx) return -1;
    if (const char* why = dv_mot_check_host(par)) DV_FAIL(std::string("dv_mot_config: ") + why);
    if (ctx->mot && ctx->mot->slot.pending) DV_FAIL("dv_mot_config: a frame is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    if (!ctx->mot) ctx->mot = new MotTracker();
    MotTracker& T = *ctx->mot;
    DV_CHECK(T.pinned.ensure(O_WORDS * 4));
    T.par = *par; T.L = dv_mot_layout(par->max_tracks);
    const size_t gbytes = (size_t)par->max_tracks * par->budget * par->feat_dim * 4;
    DV_CHECK(T.table.ensure(T.L.bytes));
    DV_CHECK(T.gallery.ensure(gbytes));
    DV_CHECK(T.featmin.ensure((size_t)par->max_tracks * MD * 4));
    DV_CHECK(T.out.ensure(O_WORDS * 4));
    DV_CHECK(hipMemsetAsync(T.table.p, 0, T.L.bytes, ctx->stream));
    DV_CHECK(hipMemsetAsync(T.gallery.p, 0xFF, gbytes, ctx->stream));      // every float a NaN: a ring row read before it was written shows
    uint8_t* tb = (uint8_t*)T.table.p;
    MotDev& D = T.D;
    D = MotDev{};
    D.n_init = par->n_init; D.max_age = par->max_age; D.budget = par->budget; D.F = par->feat_dim; D.max_tracks = par->max_tracks;
    D.hdr = (int*)(tb + T.L.hdr); D.x = (float*)(tb + T.L.x); D.P = (float*)(tb + T.L.P); D.state = (int*)(tb + T.L.state); D.id = (int*)(tb + T.L.id);
    D.hits = (int*)(tb + T.L.hits); D.tsu = (int*)(tb + T.L.tsu); D.slot = (int*)(tb + T.L.slot); D.next = (int*)(tb + T.L.next); D.full = (int*)(tb + T.L.full);
    D.slot_rows = (int*)(tb + T.L.slot_rows);
    D.gallery = (float*)T.gallery.p; D.featmin = (float*)T.featmin.p; D.out = (int*)T.out.p;
    T.configured = true;
    return mot_reset(ctx, T);
}

int dv_mot_reset(dv_ctx* ctx) {
    if (!ctx) return -1;
    if (!ctx->mot || !ctx->mot->configured) DV_FAIL("dv_mot_reset: dv_mot_config first");
    if (ctx->mot->slot.pending) DV_FAIL("dv_mot_reset: a frame is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    return mot_reset(ctx, *ctx->mot);
}

int dv_mot_update_enqueue(dv_ctx* ctx, const float* rects_xywh, const float* feats, int n, int mem) {
    if (!ctx) return -1;
    if (!ctx->mot || !ctx->mot->configured) DV_FAIL("dv_mot_update_enqueue: dv_mot_config first");
    MotTracker& T = *ctx->mot;
    if (const char* why = dv_mot_frame_check_host(rects_xywh, feats, n, mem)) DV_FAIL(std::string("dv_mot_update_enqueue: ") + why);
    if (T.slot.open(ctx, "dv_mot_update_enqueue: previous frame not collected")) return -1;
    if (n == 0) { T.slot.close_empty(); T.pend_n = 0; return 0; }      // the reference's tracker is not called: nothing predicts, nothing ages
    hipStream_t s = ctx->stream;
    MotDev D = T.D;
    D.n = n;
    if (mem == DV_MEM_HOST) {
        const size_t nr = (size_t)n * 4, nf = (size_t)n * T.par.feat_dim;
        DV_CHECK(T.staged.ensure((size_t)MD * (4 + DV_MOT_MAX_FEAT_DIM) * 4));
        float* d = (float*)T.staged.p;
        DV_CHECK(hipMemcpyAsync(d, rects_xywh, nr * 4, hipMemcpyHostToDevice, s));
        DV_CHECK(hipMemcpyAsync(d + MD * 4, feats, nf * 4, hipMemcpyHostToDevice, s));
        D.rects = d; D.feats = d + MD * 4;
    } else { D.rects = rects_xywh; D.feats = feats; }
    {
        StageScope sc_t(ctx, "mot");
        hipLaunchKernelGGL(mot_feat_kernel, dim3(T.par.max_tracks), dim3(256), 0, s, D);
        hipLaunchKernelGGL(mot_assoc_kernel, dim3(1), dim3(256), 0, s, D);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = dv_copy_async(T.pinned.p, D.out, O_WORDS * 4, s);
    if (T.slot.close(ctx, e, s)) return -1;
    T.pend_n = n;
    return 0;
}

int dv_mot_update_collect(dv_ctx* ctx, int32_t* track_id, int* n_tracks, int* n_confirmed) {
    if (!ctx) return -1;
    if (!ctx->mot || !ctx->mot->slot.pending) DV_FAIL("dv_mot_update_collect: nothing enqueued");
    MotTracker& T = *ctx->mot;
    if (T.pend_n > 0 && !track_id) DV_FAIL("dv_mot_update_collect: null track_id");
    if (T.slot.wait(ctx)) return -1;
    if (T.pend_n > 0) {
        if (ctx->timing) dv_harvest_timers(ctx, ctx->stream);
        const int32_t* o = (const int32_t*)T.pinned.p;
        if (o[O_FAIL] == FAIL_CAPACITY)
            DV_FAIL("dv_mot_update_collect: the frame would leave " + std::to_string(o[O_WOULD]) + " tracks, more than max_tracks " + std::to_string(T.par.max_tracks) +
                    ": the frame is dropped and the tracker is as it was before it");
        if (o[O_FAIL]) DV_FAIL("dv_mot_update_collect: the assignment did not end (costs not finite?): the frame is dropped and the tracker is as it was before it");
        if (o[O_NTRACKS] < 0 || o[O_NTRACKS] > T.par.max_tracks) DV_FAIL("dv_mot_update_collect: corrupt track count");
        for (int j = 0; j < T.pend_n; ++j) track_id[j] = o[O_IDS + j];
        T.n_tracks = o[O_NTRACKS]; T.n_confirmed = o[O_NCONF];
    }
    if (n_tracks) *n_tracks = T.n_tracks;
    if (n_confirmed) *n_confirmed = T.n_confirmed;
    return 0;
}

int dv_mot_get_tracks(dv_ctx* ctx, dv_mot_track* out, int cap, int* n) {
    if (!ctx) return -1;
    if (!ctx->mot || !ctx->mot->configured) DV_FAIL("dv_mot_get_tracks: dv_mot_config first");
    MotTracker& T = *ctx->mot;
    if (!n || cap < 0 || (cap > 0 && !out)) DV_FAIL("dv_mot_get_tracks: bad argument");
    if (T.slot.pending) DV_FAIL("dv_mot_get_tracks: a frame is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<uint8_t> h(T.L.bytes);
    DV_CHECK(hipMemcpy(h.data(), T.table.p, T.L.bytes, hipMemcpyDeviceToHost));
    const int32_t* hdr = (const int32_t*)(h.data() + T.L.hdr);
    const int nt = hdr[DV_MOT_H_NTRACKS];
    if (nt < 0 || nt > T.par.max_tracks) DV_FAIL("dv_mot_get_tracks: corrupt track count");
    *n = nt;
    auto I = [&](size_t off, int i) { return ((const int32_t*)(h.data() + off))[i]; };
    for (int i = 0; i < nt && i < cap; ++i) {
        dv_mot_track& o = out[i];
        const float* x = (const float*)(h.data() + T.L.x) + i * 7;
        const float* P = (const float*)(h.data() + T.L.P) + i * 49;
        for (int k = 0; k < 7; ++k) { o.x[k] = x[k]; o.p_diag[k] = P[k * 7 + k]; }
        dv_mot_rect_of(x, o.rect);
        o.state = I(T.L.state, i); o.id = I(T.L.id, i); o.hits = I(T.L.hits, i); o.time_since_update = I(T.L.tsu, i);
        o.n_feats = dv_mot_ring_rows(I(T.L.next, i), I(T.L.full, i), T.par.budget); o.reserved = 0;
    }
    return 0;
}

int dv_mot_assign(dv_ctx* ctx, const float* cost, int rows, int cols, int32_t* assignment) {
    if (!ctx) return -1;
    if (const char* why = dv_mot_assign_check_host(cost, rows, cols, assignment)) DV_FAIL(std::string("dv_mot_assign: ") + why);
    if (rows == 0) return 0;
    if (!ctx->mot) ctx->mot = new MotTracker();
    MotTracker& T = *ctx->mot;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    const size_t cbytes = ((size_t)rows * cols * 4 + 255) / 256 * 256;
    DV_CHECK(T.op.ensure(cbytes + (MT + 1) * 4));
    float* dc = (float*)T.op.p; int* da = (int*)((uint8_t*)T.op.p + cbytes);
    if (cols > 0) DV_CHECK(hipMemcpyAsync(dc, cost, (size_t)rows * cols * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(mot_assign_kernel, dim3(1), dim3(64), 0, ctx->stream, dc, rows, cols, da, da + MT);
    DV_CHECK(hipGetLastError());
    int32_t res[MT + 1];
    DV_CHECK(hipMemcpyAsync(res, da, (MT + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    if (res[MT]) DV_FAIL("dv_mot_assign: the assignment did not end");
    for (int r = 0; r < rows; ++r) assignment[r] = res[r];
    return 0;
}

}  // extern "C"
