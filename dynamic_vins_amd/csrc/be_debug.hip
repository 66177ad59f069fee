// be_debug.hip — diagnostics of the window solve: hashes of what the device holds (dv_debug_set "hash_log"), their logs, and the debug switches of dv_debug_set.
#include <algorithm>
#include "be_host.h"

// diagnostics (dv_debug_set "hash_log"): a deterministic hash of a device byte range — 256 threads hash interleaved 8-byte words with FNV-1a, thread 0 folds the 256 results in order
__global__ __launch_bounds__(256) void be_dbg_hash_kernel(const unsigned long long* __restrict__ p, size_t words, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sh[256];
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = threadIdx.x; i < words; i += 256) { h ^= p[i]; h *= 1099511628211ull; }
    sh[threadIdx.x] = h;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long t = 1469598103934665603ull; for (int k = 0; k < 256; ++k) { t ^= sh[k]; t *= 1099511628211ull; } *out = t; }
}
struct BeDbgJob { const unsigned long long* p[BeWork::DBG_RANGES]; unsigned long long words[BeWork::DBG_RANGES]; unsigned long long* out; };
__global__ __launch_bounds__(256) void be_dbg_hash_multi_kernel(BeDbgJob j) {      // blockIdx.x = range
    __shared__ unsigned long long sh[256];
    const unsigned long long* p = j.p[blockIdx.x]; const unsigned long long words = j.words[blockIdx.x];
    unsigned long long h = 1469598103934665603ull;
    for (unsigned long long i = threadIdx.x; i < words; i += 256) { h ^= p[i]; h *= 1099511628211ull; }
    sh[threadIdx.x] = h;
    __syncthreads();
    if (threadIdx.x == 0) { unsigned long long t = 1469598103934665603ull; for (int k = 0; k < 256; ++k) { t ^= sh[k]; t *= 1099511628211ull; } j.out[blockIdx.x] = t; }
}
// everything a launch of the round may write, hashed behind it on the same stream: 0 packets[0] 1 packets[1] 2 imu_out[0] 3 imu_out[1] 4 prior_out[0] 5 prior_out[1] 6 cand_cost
// 7 Hd[0] 8 Hd[1] 9 Sc[0] 10 Sc[1] 11 gvec[0] 12 gvec[1] 13 x 14 cand 15 ctl
void be_dbg_stage(dv_ctx* c, int it, int kind, hipStream_t s) {
    BeWork& w = c->be;
    if (!w.debug_hash_log || it >= BeWork::DBG_SLOTS) return;
    const bool light = w.debug_hash_light;      // "hash_light": only the small buffers (a few KB: microsecond kernels), and only behind solve / candidate evaluation — the full form changes the timing so much that the defect does not occur
    if (light && kind != 2 && kind != 3) return;
    if (!w.dbg_slots) { if (hipHostMalloc((void**)&w.dbg_slots, sizeof(unsigned long long) * BeWork::DBG_SLOTS * 5 * BeWork::DBG_RANGES, hipHostMallocDefault) != hipSuccess) return; std::memset(w.dbg_slots, 0, sizeof(unsigned long long) * BeWork::DBG_SLOTS * 5 * BeWork::DBG_RANGES); }
    const size_t n = BE_MAX_STATE, pk = (size_t)BE_PK_SIZE * BE_PK_STRIDE, sb = w.pend->state_bytes / 8;
    BeDbgJob j{};
    const void* ptr[BeWork::DBG_RANGES] = { w.packets[0], w.packets[1], w.imu_out[0], w.imu_out[1], w.prior_out[0], w.prior_out[1], w.cand_cost, w.Hd[0], w.Hd[1], w.Sc[0], w.Sc[1], w.gvec[0], w.gvec[1], w.x, w.cand, w.ctl };
    const size_t io = (size_t)BE_WIN * IMU_OUT_STRIDE, po = (size_t)BE_MAX_PRIOR + 1;
    const size_t words[BeWork::DBG_RANGES] = { pk, pk, io, io, po, po, (size_t)BE_MAX_LM + BE_WIN + 1, n * n, n * n, n * n, n * n, 2 * n, 2 * n, sb, sb, sizeof(BeCtl) / 8 };
    for (int r = 0; r < BeWork::DBG_RANGES; ++r) { j.p[r] = (const unsigned long long*)ptr[r]; j.words[r] = (light && !(r == 6 || r == 11 || r == 12 || r >= 13)) ? 0 : words[r]; }
    j.out = w.dbg_slots + (size_t)(it * 5 + kind) * BeWork::DBG_RANGES;
    hipLaunchKernelGGL(be_dbg_hash_multi_kernel, dim3(BeWork::DBG_RANGES), dim3(256), 0, s, j);
}

void be_dbg_hash(const void* dev, size_t bytes, unsigned long long* out_pinned, hipStream_t s) {
    if (!dev || bytes < 8) { *out_pinned = 0; return; }
    hipLaunchKernelGGL(be_dbg_hash_kernel, dim3(1), dim3(256), 0, s, (const unsigned long long*)dev, bytes / 8, out_pinned);
}

extern "C" {

// diagnostics (dv_debug_set "hash_log"): rows of seven uint64 per fused window solve: [counter, uploaded block on the device, prior A, prior b, x after the round, candidate buffer, control block]
int dv_ba_debug_dev_log(dv_ctx* ctx, unsigned long long* rows7, int cap, int* n_rows) {
    if (!ctx) return -1;
    const int n = (int)(ctx->be.dbg_dev_log.size() / 7);
    if (n_rows) *n_rows = n;
    if (rows7) std::memcpy(rows7, ctx->be.dbg_dev_log.data(), sizeof(unsigned long long) * 7 * (size_t)std::min(n, std::max(cap, 0)));
    return 0;
}

// the same per launch of the round: per fused solve DBG_SLOTS x 5 launch kinds x DBG_RANGES hashes (0 = launch not issued); *row_len = values per solve
int dv_ba_debug_slot_log(dv_ctx* ctx, unsigned long long* vals, long long cap_vals, long long* n_vals, int* row_len) {
    if (!ctx) return -1;
    const long long n = (long long)ctx->be.dbg_slot_log.size();
    if (n_vals) *n_vals = n;
    if (row_len) *row_len = BeWork::DBG_SLOTS * 5 * BeWork::DBG_RANGES;
    if (vals) std::memcpy(vals, ctx->be.dbg_slot_log.data(), sizeof(unsigned long long) * (size_t)std::min(n, std::max(cap_vals, 0ll)));
    return 0;
}

// the linearisation buffers as the device holds them (include/dvins.h; tests/test_eval_chain.py and tests/test_reduce_chain.py compare them bit for bit with records of an earlier library)
int dv_ba_debug_buffer(dv_ctx* ctx, int which, int set, void* host, long long bytes) {
    if (!ctx) return -1;
    if (which < 0 || which > 8 || set < 0 || set > 1) DV_FAIL("dv_ba_debug_buffer: bad buffer");
    if (ctx->be.pend->active) DV_FAIL("dv_ba_debug_buffer: a solve is in flight");
    DV_CHECK(hipSetDevice(ctx->cfg.device));
    if (be_ensure(ctx, 0)) return -1;
    BeWork& w = ctx->be;
    const size_t n = BE_MAX_STATE;
    void* const ptr[9] = { w.packets[set], w.imu_out[set], w.prior_out[set], w.cand_cost, w.lm_obs, w.Hd[set], w.Sc[set], w.gvec[set], w.scale_l };
    const size_t cap[9] = { 8 * (size_t)BE_PK_SIZE * BE_PK_STRIDE, 8 * (size_t)BE_WIN * IMU_OUT_STRIDE, 8 * (BE_MAX_PRIOR + 1), 8 * (BE_MAX_LM + BE_WIN + 1), 4 * BE_MAX_LM, 8 * n * n, 8 * n * n, 8 * 2 * n, 8 * (size_t)BE_MAX_LM };
    DV_CHECK(hipStreamSynchronize(ctx->be_stream));
    if (!host) { DV_CHECK(hipMemset(ptr[which], 0xFF, cap[which])); return 0; }
    if (bytes < 0 || (size_t)bytes > cap[which]) DV_FAIL("dv_ba_debug_buffer: more bytes than the buffer holds");
    DV_CHECK(hipMemcpy(host, ptr[which], (size_t)bytes, hipMemcpyDeviceToHost));
    return 0;
}

// debug-only switches (not read from the environment): "short_first_pass" = enqueue max_iters - 2 slots first so that the spare-slot
// continuation of be_solve_fused_end runs on every frame (tests/test_estimator_parity.py::test_spare_slot_path_is_equivalent)
int dv_debug_set(dv_ctx* ctx, const char* key, int value) {
    if (!ctx || !key) return -1;
    if (std::strcmp(key, "short_first_pass") == 0) { ctx->be.debug_short_first_pass = value != 0; return 0; }
    if (std::strcmp(key, "peer_timeout_ms") == 0) { ctx->dist.peer_timeout_ticks = 100000ll * std::max(value, 1); return 0; }      // transport peer: how long a wait kernel spins for a peer's flag (default 2000)
    if (std::strcmp(key, "batch_single_eval") == 0) { ctx->be.debug_batch_single = (ctx->be.debug_batch_single & ~1) | (value ? 1 : 0); return 0; }
    if (std::strcmp(key, "batch_single_reduce") == 0) { ctx->be.debug_batch_single = (ctx->be.debug_batch_single & ~2) | (value ? 2 : 0); return 0; }
    if (std::strcmp(key, "batch_single_tail") == 0) { ctx->be.debug_batch_single = (ctx->be.debug_batch_single & ~8) | (value ? 8 : 0); return 0; }
    if (std::strcmp(key, "batch_single_solve") == 0) { ctx->be.debug_batch_single = (ctx->be.debug_batch_single & ~4) | (value ? 4 : 0); return 0; }
    if (std::strcmp(key, "hash_light") == 0) { ctx->be.debug_hash_light = value != 0; return 0; }
    if (std::strcmp(key, "hash_log") == 0) { ctx->be.debug_hash_log = value != 0; return 0; }      // the estimator keeps per-solve hashes of what it uploads / downloads (dv_est_debug_hash_log)
    if (std::strcmp(key, "wait_tail") == 0) { ctx->be.debug_wait_tail = value != 0; return 0; }
    if (std::strcmp(key, "gpu_reject") == 0) { ctx->be.gpu_reject = value != 0; return 0; }      // 0: OutliersRejection on the host (rounds 1-3 until be_reject_kernel)
    if (std::strcmp(key, "ldl_generic") == 0) { ctx->be.ldl_generic = value != 0; return 0; }      // the generic 4-wide panel LDL^T instead of the 16-wide MFMA form (A/B runs, agreement tests)
    if (std::strcmp(key, "ldl_barriers") == 0) { ctx->be.ldl_barriers = value != 0; return 0; }      // the MF16 loop on workgroup barriers instead of the LDS-flag hand-off (single-window kernel: A/B runs, bit comparison)
    DV_FAIL(std::string("dv_debug_set: unknown key ") + key);
}

}  // extern "C"
