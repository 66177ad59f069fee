// line_track.hip — the line tracker on gfx950: a frame's key lines and 32-byte LBD descriptors -> line ids, track counts and the frame's dv_line_rows.  Reference:
// LineDetector::TrackLeftLine / TrackLine / TrackRightLine (line_detector/line_detector.cpp:101-297) over BinaryDescriptorMatcher::match
// (thirdparty/line_descriptor/src/binary_descriptor_matcher.cpp:197-254, Mihasher::query :635-753), then FrameLines::SetLines / UndistortedLineEndPoints
// (basic/frame_lines.cpp:15-45) and SetOutputFeats' `lines` map (front_end/background_tracker.cpp:373-389).  include/dvins.h has the rule; the rules shared with the host
// (distance, first-equal-byte key, gate, h / v, quota) are in line_track_host.h.  The previous left frame and the id counter are resident.
//   line_track_kernel  ONE workgroup of 512 threads, a thread per line, one launch per frame:
//                      left   the previous frame's descriptors, lines, ids and counts go to LDS; a thread scans the 16 KB of train rows (every lane reads the same
//                             address: a broadcast) and keeps the least (distance, first equal byte, index) below 30; gate; matched / new h / new v are ranked by
//                             ballot + per-wave counts, always in line order, and the frame's left set is written in output order into the SAME LDS arrays (the next
//                             train set) and into the resident table.
//                      right  the same scan against the left set just written; matched right lines compacted in right order.
//                      rows   first left line of an id, rank by id among the firsts, first right line of the id; both end points through lift_dev.h.
//                      No atomics: every position is a rank in line order, so the result does not depend on scheduling.
//   line_match_kernel  the operator form of the scan alone (dv_line_match).
#include "dv_ctx.h"
#include "lift_dev.h"
#include "line_track_host.h"
#include <string>

namespace {

constexpr int LM = DV_LINE_MAX, LT_THREADS = 512, LT_WAVES = LT_THREADS / 64, DW = DV_LT_DESC_WORDS;
static_assert(LT_THREADS == LM, "a thread per line");

struct LineDev {
    int* hdr; dv_key_line* p_line; uint32_t* p_id; int* p_cnt; uint32_t* p_desc;      // the resident previous left frame
    uint8_t* out;                                                                     // DvLineOut
    const dv_key_line* l_line; const uint32_t* l_desc; int n_left;
    const dv_key_line* r_line; const uint32_t* r_desc; int n_right;
    dv_cam cam0, cam1;
};

// rank of a flagged thread among the flagged threads of the workgroup in thread order, and their number.  Called by ALL threads
__device__ __forceinline__ int block_rank(bool f, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    __syncthreads();
    if (lane == 0) s_w[wv] = __popcll(b);
    __syncthreads();
    int off = 0, sum = 0;
    for (int w = 0; w < LT_WAVES; ++w) { const int c = s_w[w]; if (w < wv) off += c; sum += c; }
    *total = sum;
    return off + __popcll(b & ((1ull << lane) - 1));
}

__device__ __forceinline__ void load_desc(uint32_t* d, const uint32_t* src, int row) { for (int w = 0; w < DW; ++w) d[w] = src[(size_t)row * DW + w]; }

__global__ __launch_bounds__(LT_THREADS) void line_track_kernel(LineDev D) {
    __shared__ uint32_t s_desc[LM * DW];            // the train set: the previous left frame, then this frame's left set
    __shared__ dv_key_line s_line[LM];
    __shared__ uint32_t s_id[LM];
    __shared__ int s_cnt[LM];
    __shared__ uint32_t s_rid[LM];                  // the kept right lines
    __shared__ float s_rpx[LM][4];
    __shared__ int s_first[LM];
    __shared__ int s_w[LT_WAVES];
    const int t = threadIdx.x;
    const DvLineOut O = dv_line_out_layout();
    int* o_cnt = (int*)D.out;
    uint32_t* o_lid = (uint32_t*)(D.out + O.left_ids); int* o_lsrc = (int*)(D.out + O.left_src); int* o_lcnt = (int*)(D.out + O.left_cnt);
    uint32_t* o_rid = (uint32_t*)(D.out + O.right_ids); int* o_rsrc = (int*)(D.out + O.right_src);
    dv_line_row* o_rows = (dv_line_row*)(D.out + O.rows);

    const bool have_prev = D.hdr[DV_LT_H_HAVE_PREV] != 0;
    int nP = D.hdr[DV_LT_H_NPREV];
    nP = nP < 0 ? 0 : (nP > LM ? LM : nP);
    const uint32_t next_id = (uint32_t)D.hdr[DV_LT_H_NEXT_ID];
    const int n = D.n_left < 0 ? 0 : (D.n_left > LM ? LM : D.n_left);
    const int nR = (D.r_line && D.r_desc) ? (D.n_right < 0 ? 0 : (D.n_right > LM ? LM : D.n_right)) : 0;

    // ---- left: TrackLeftLine ----
    if (have_prev && t < nP) { load_desc(s_desc + t * DW, D.p_desc, t); s_line[t] = D.p_line[t]; s_id[t] = D.p_id[t]; s_cnt[t] = D.p_cnt[t]; }
    dv_key_line q{};
    uint32_t qd[DW] = {};
    const bool live = t < n;
    if (live) { q = D.l_line[t]; load_desc(qd, D.l_desc, t); }
    __syncthreads();
    bool m = false;
    uint32_t id = DV_LT_NO_ID;
    int cnt = 0;
    if (have_prev && live && nP > 0) {
        int dist;
        const int j = dv_lt_nearest(qd, s_desc, nP, &dist);
        if (j >= 0 && dv_lt_gate(q, s_line[j]) && s_id[j] != DV_LT_NO_ID) { m = true; id = s_id[j]; cnt = s_cnt[j] + 1; }      // an id of "-1" reads as unmatched (:147)
    }
    const bool u = live && !m, h = dv_lt_is_h(q.angle);
    int T, U, hT, NH, NV;
    const int rt = block_rank(m, s_w, &T);
    const int ru = block_rank(u, s_w, &U);
    (void)block_rank(m && h, s_w, &hT);
    const int rh = block_rank(u && h, s_w, &NH);
    const int rv = block_rank(u && !h, s_w, &NV);
    int pos = -1, n_out;
    uint32_t new_next;
    if (!have_prev) {                                // first frame (:229-234): fresh ids, no quota, no counts
        if (live) { id = next_id + (uint32_t)t; pos = t; cnt = 0; }
        n_out = n; new_next = next_id + (uint32_t)n;
    } else {
        const int takeH = dv_lt_take(hT, NH), takeV = dv_lt_take(T - hT, NV);
        if (u) id = next_id + (uint32_t)ru;          // every unmatched line consumes an id, kept or not (:146-152)
        if (m) pos = rt;
        else if (u && h) { if (rh < takeH) { pos = T + rh; cnt = 0; } }               // no entry in curr_track_cnt (:200-204)
        else if (u) { if (rv < takeV) { pos = T + takeH + rv; cnt = 1; } }            // curr_track_cnt.insert({id, 1}) (:218)
        n_out = T + takeH + takeV; new_next = next_id + (uint32_t)U;
    }
    __syncthreads();                                 // everyone has read the previous frame
    if (pos >= 0 && pos < LM) {
        for (int w = 0; w < DW; ++w) { s_desc[pos * DW + w] = qd[w]; D.p_desc[(size_t)pos * DW + w] = qd[w]; }
        s_line[pos] = q; s_id[pos] = id; s_cnt[pos] = cnt;
        D.p_line[pos] = q; D.p_id[pos] = id; D.p_cnt[pos] = cnt;
        o_lid[pos] = id; o_lsrc[pos] = t; o_lcnt[pos] = cnt;
    }
    if (t == 0) { D.hdr[DV_LT_H_HAVE_PREV] = 1; D.hdr[DV_LT_H_NPREV] = n_out; D.hdr[DV_LT_H_NEXT_ID] = (int)new_next; }
    __syncthreads();

    // ---- right: TrackRightLine against the left set ----
    dv_key_line rq{};
    uint32_t rd[DW] = {};
    if (t < nR) { rq = D.r_line[t]; load_desc(rd, D.r_desc, t); }
    bool rm = false;
    uint32_t rid = DV_LT_NO_ID;
    if (t < nR && n_out > 0) {
        int dist;
        const int j = dv_lt_nearest(rd, s_desc, n_out, &dist);
        if (j >= 0 && dv_lt_gate(rq, s_line[j]) && s_id[j] != DV_LT_NO_ID) { rm = true; rid = s_id[j]; }
    }
    int NR;
    const int rr = block_rank(rm, s_w, &NR);
    if (rm) { s_rid[rr] = rid; s_rpx[rr][0] = rq.sx; s_rpx[rr][1] = rq.sy; s_rpx[rr][2] = rq.ex; s_rpx[rr][3] = rq.ey; o_rid[rr] = rid; o_rsrc[rr] = t; }

    // ---- rows: SetOutputFeats' map ----
    bool first = false;
    uint32_t myid = 0;
    if (t < n_out) {
        myid = s_id[t]; first = true;
        for (int j = 0; j < t; ++j) if (s_id[j] == myid) { first = false; break; }
    }
    s_first[t] = first ? 1 : 0;
    int NROWS;
    (void)block_rank(first, s_w, &NROWS);            // (its barriers publish s_first, s_rid and s_rpx)
    if (first) {
        int r = 0;
        for (int j = 0; j < n_out; ++j) r += (s_first[j] && s_id[j] < myid) ? 1 : 0;
        dv_line_row row;
        row.id = myid; row.has_right = 0;
        const dv_key_line l = s_line[t];
        double x, y;
        dv_lift_projective_d(D.cam0, (double)l.sx, (double)l.sy, x, y); row.left[0] = (double)(float)x; row.left[1] = (double)(float)y;      // Line keeps cv::Point2f
        dv_lift_projective_d(D.cam0, (double)l.ex, (double)l.ey, x, y); row.left[2] = (double)(float)x; row.left[3] = (double)(float)y;
        for (int c = 0; c < 4; ++c) row.right[c] = 0.0;
        for (int k = 0; k < NR; ++k)
            if (s_rid[k] == myid) {                  // the first right line of the id: the one feature_manager.cpp:127-128 reads
                row.has_right = 1;
                dv_lift_projective_d(D.cam1, (double)s_rpx[k][0], (double)s_rpx[k][1], x, y); row.right[0] = (double)(float)x; row.right[1] = (double)(float)y;
                dv_lift_projective_d(D.cam1, (double)s_rpx[k][2], (double)s_rpx[k][3], x, y); row.right[2] = (double)(float)x; row.right[3] = (double)(float)y;
                break;
            }
        if (r < LM) o_rows[r] = row;
    }
    if (t == 0) { o_cnt[DV_LT_O_NROWS] = NROWS; o_cnt[DV_LT_O_NLEFT] = n_out; o_cnt[DV_LT_O_NRIGHT] = NR; o_cnt[DV_LT_O_NEXT_ID] = (int)new_next; }
}

__global__ __launch_bounds__(LT_THREADS) void line_match_kernel(const uint32_t* query, int nq, const uint32_t* train, int nt, int* idx, int* dist) {
    __shared__ uint32_t s_desc[LM * DW];
    const int t = threadIdx.x;
    nt = nt > LM ? LM : nt;
    if (t < nt) load_desc(s_desc + t * DW, train, t);
    __syncthreads();
    if (t >= nq || t >= LM) return;
    uint32_t qd[DW];
    load_desc(qd, query, t);
    int d = 0;
    idx[t] = nt > 0 ? dv_lt_nearest(qd, s_desc, nt, &d) : -1;
    dist[t] = d;
}

__global__ void line_reset_kernel(int* hdr) { if (threadIdx.x < DV_LT_H_WORDS) hdr[threadIdx.x] = 0; }

constexpr size_t IN_LINES = (size_t)LM * sizeof(dv_key_line), IN_DESC = (size_t)LM * DV_LINE_DESC_BYTES, IN_BYTES = 2 * (IN_LINES + IN_DESC);

}  // namespace

struct LineTracker {
    DvLineLayout L{}; DvLineOut O{};
    DevBuf table, out, op;
    PinBuf pinned_out;      // O.bytes
    PinBuf pinned_in;       // DV_MEM_HOST frames: left lines | left descriptors | right lines | right descriptors, read in place by the kernel
    StageSlot slot;
    bool ready = false;
};

void dv_stage_delete(LineTracker* p) { delete p; }

// the tracker's buffers, once; the resident table starts as dv_line_track_reset leaves it
static int line_ensure(dv_ctx* ctx) {
    if (!ctx->line_track) ctx->line_track = new LineTracker();
    LineTracker& T = *ctx->line_track;
    if (T.ready) return 0;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    T.L = dv_line_layout(); T.O = dv_line_out_layout();
    DV_CHECK(T.pinned_out.ensure(T.O.bytes));
    DV_CHECK(T.pinned_in.ensure(IN_BYTES));
    DV_CHECK(T.table.ensure(T.L.bytes));
    DV_CHECK(T.out.ensure(T.O.bytes));
    DV_CHECK(hipMemsetAsync(T.table.p, 0, T.L.bytes, ctx->stream));
    DV_CHECK(hipMemsetAsync(T.out.p, 0, T.O.bytes, ctx->stream));
    T.ready = true;
    return 0;
}

extern "C" {

int dv_line_track_check(const dv_key_line* left_lines, const uint8_t* left_desc, int n_left, const dv_key_line* right_lines, const uint8_t* right_desc, int n_right, int mem) {
    dv_ctx* ctx = nullptr;
    if (const char* why = dv_line_frame_check_host(left_lines, left_desc, n_left, right_lines, right_desc, n_right, mem)) DV_FAIL(std::string("dv_line_track_check: ") + why);
    return 0;
}

int dv_line_track_reset(dv_ctx* ctx) {
    if (!ctx) return -1;
    if (ctx->line_track && ctx->line_track->slot.pending) DV_FAIL("dv_line_track_reset: a frame is in flight");
    if (line_ensure(ctx)) return -1;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    hipLaunchKernelGGL(line_reset_kernel, dim3(1), dim3(64), 0, ctx->stream, (int*)((uint8_t*)ctx->line_track->table.p + ctx->line_track->L.hdr));
    DV_CHECK(hipGetLastError());
    return 0;
}

int dv_line_track_enqueue(dv_ctx* ctx, const dv_key_line* left_lines, const uint8_t* left_desc, int n_left, const dv_key_line* right_lines, const uint8_t* right_desc, int n_right, int mem) {
    if (!ctx) return -1;
    if (const char* why = dv_line_frame_check_host(left_lines, left_desc, n_left, right_lines, right_desc, n_right, mem)) DV_FAIL(std::string("dv_line_track_enqueue: ") + why);
    if (!ctx->line_track) ctx->line_track = new LineTracker();
    LineTracker& T = *ctx->line_track;
    if (T.slot.open(ctx, "dv_line_track_enqueue: previous frame not collected")) return -1;
    if (line_ensure(ctx)) return -1;
    hipStream_t s = ctx->stream;
    uint8_t* tb = (uint8_t*)T.table.p;
    LineDev D{};
    D.hdr = (int*)(tb + T.L.hdr); D.p_line = (dv_key_line*)(tb + T.L.line); D.p_id = (uint32_t*)(tb + T.L.id); D.p_cnt = (int*)(tb + T.L.cnt); D.p_desc = (uint32_t*)(tb + T.L.desc);
    D.out = (uint8_t*)T.out.p;
    D.n_left = n_left; D.n_right = (right_lines && right_desc) ? n_right : 0;
    D.cam0 = ctx->cfg.cam0; D.cam1 = ctx->cfg.cam1;
    if (mem == DV_MEM_HOST) {                        // the caller's memory may be pageable: into the library's pinned block, which the kernel reads in place
        uint8_t* p = T.pinned_in.p;
        if (n_left > 0) { std::memcpy(p, left_lines, (size_t)n_left * sizeof(dv_key_line)); std::memcpy(p + IN_LINES, left_desc, (size_t)n_left * DV_LINE_DESC_BYTES); }
        if (D.n_right > 0) { std::memcpy(p + IN_LINES + IN_DESC, right_lines, (size_t)n_right * sizeof(dv_key_line)); std::memcpy(p + 2 * IN_LINES + IN_DESC, right_desc, (size_t)n_right * DV_LINE_DESC_BYTES); }
        D.l_line = (const dv_key_line*)p; D.l_desc = (const uint32_t*)(p + IN_LINES);
        D.r_line = (const dv_key_line*)(p + IN_LINES + IN_DESC); D.r_desc = (const uint32_t*)(p + 2 * IN_LINES + IN_DESC);
    } else {
        D.l_line = left_lines; D.l_desc = (const uint32_t*)left_desc; D.r_line = right_lines; D.r_desc = (const uint32_t*)right_desc;
    }
    hipError_t e;
    {
        StageScope sc_t(ctx, "line_track");
        hipLaunchKernelGGL(line_track_kernel, dim3(1), dim3(LT_THREADS), 0, s, D);
        e = hipGetLastError();
        if (e == hipSuccess) e = dv_copy_async(T.pinned_out.p, T.out.p, T.O.rows + (size_t)n_left * sizeof(dv_line_row), s);      // counters, per-line words and at most n_left rows
    }
    return T.slot.close(ctx, e, s);                  // (the kernel reads pinned_in / the caller's arrays in place)
}

int dv_line_track_collect(dv_ctx* ctx, dv_line_row* rows, int cap, int* n_rows, uint32_t* left_ids, int32_t* left_src, int32_t* left_cnt, int* n_left_out,
                          uint32_t* right_ids, int32_t* right_src, int* n_right_out) {
    if (!ctx) return -1;
    if (!ctx->line_track || !ctx->line_track->slot.pending) DV_FAIL("dv_line_track_collect: nothing enqueued");
    if (const char* why = dv_line_collect_check_host(rows, cap, n_rows)) DV_FAIL(std::string("dv_line_track_collect: ") + why);
    LineTracker& T = *ctx->line_track;
    if (T.slot.wait(ctx)) return -1;
    if (ctx->timing) dv_harvest_timers(ctx, ctx->stream);
    const uint8_t* po = T.pinned_out.p;
    const int32_t* o = (const int32_t*)po;
    const int nr = o[DV_LT_O_NROWS], nl = o[DV_LT_O_NLEFT], nrt = o[DV_LT_O_NRIGHT];
    if (nr < 0 || nl < 0 || nrt < 0 || nl > DV_LINE_MAX || nrt > DV_LINE_MAX || nr > nl) DV_FAIL("dv_line_track_collect: corrupt counters");
    *n_rows = nr;
    if (rows && cap > 0 && nr > 0) std::memcpy(rows, po + T.O.rows, (size_t)(nr < cap ? nr : cap) * sizeof(dv_line_row));
    if (left_ids) std::memcpy(left_ids, po + T.O.left_ids, (size_t)nl * 4);
    if (left_src) std::memcpy(left_src, po + T.O.left_src, (size_t)nl * 4);
    if (left_cnt) std::memcpy(left_cnt, po + T.O.left_cnt, (size_t)nl * 4);
    if (n_left_out) *n_left_out = nl;
    if (right_ids) std::memcpy(right_ids, po + T.O.right_ids, (size_t)nrt * 4);
    if (right_src) std::memcpy(right_src, po + T.O.right_src, (size_t)nrt * 4);
    if (n_right_out) *n_right_out = nrt;
    return 0;
}

int dv_line_match(dv_ctx* ctx, const uint8_t* query_desc, int nq, const uint8_t* train_desc, int nt, int32_t* train_idx, int32_t* distance) {
    if (!ctx) return -1;
    if (const char* why = dv_line_match_check_host(query_desc, nq, train_desc, nt, train_idx, distance)) DV_FAIL(std::string("dv_line_match: ") + why);
    if (nq == 0) return 0;
    if (nt == 0) { for (int i = 0; i < nq; ++i) { train_idx[i] = -1; distance[i] = 0; } return 0; }      // "descriptors matrices cannot be void": no matches
    if (!ctx->line_track) ctx->line_track = new LineTracker();
    LineTracker& T = *ctx->line_track;
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    DV_CHECK(T.op.ensure(2 * IN_DESC + 2 * (size_t)LM * 4));
    uint8_t* d = (uint8_t*)T.op.p;
    uint32_t* dq = (uint32_t*)d; uint32_t* dt = (uint32_t*)(d + IN_DESC); int* di = (int*)(d + 2 * IN_DESC); int* dd = di + LM;
    DV_CHECK(hipMemcpyAsync(dq, query_desc, (size_t)nq * DV_LINE_DESC_BYTES, hipMemcpyHostToDevice, ctx->stream));
    DV_CHECK(hipMemcpyAsync(dt, train_desc, (size_t)nt * DV_LINE_DESC_BYTES, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(line_match_kernel, dim3(1), dim3(LT_THREADS), 0, ctx->stream, dq, nq, dt, nt, di, dd);
    DV_CHECK(hipGetLastError());
    DV_CHECK(hipMemcpyAsync(train_idx, di, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipMemcpyAsync(distance, dd, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    DV_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
