// be_marg_eig.hip — the reference's form of the new prior (DV_MARG_EIGEN, include/dvins.h): MarginalizationInfo::marginalize's second
// eigen-decomposition (estimator/factor/marginalization_factor.cpp:297-308) on gfx950.
//
// be_marg_finish leaves A' = Arr - Arm Amm^-1 Amr and b' = brr - Arm Amm^-1 bmm in outA / outb (kept-block order, the reference's A, b after
// :291-292).  The reference then factors A' = Q S Q^T with SelfAdjointEigenSolver, zeroes the eigenvalues <= 1e-8 and stores J0 = S^1/2 Q^T,
// r0 = S^-1/2 Q^T b'.  Every consumer of the prior only ever forms J0^T J0, J0^T r0 and r0^T r0, so this kernel writes, in place,
//   A'_c = sum_{lambda_k > 1e-8} lambda_k q_k q_k^T,   b'_c = sum_{lambda_k > 1e-8} q_k (q_k^T b'),   c0 = sum_{lambda_k > 1e-8} (q_k^T b')^2 / lambda_k
// (c0 summed in ascending eigenvalue order, as r0^T r0), i.e. the information form of the clamped prior: be_eval / be_solve read it unchanged.
//
// ONE 1024-thread workgroup, A' and V resident in LDS (row stride N + 1 doubles, N = n rounded up to even; n <= 96 -> 146 KB).
// Parallel two-sided Jacobi, round-robin (Brent-Luk / circle) ordering: each step rotates N / 2 disjoint pairs.
//   phase A  lane i of the first N / 2 computes (c, s) of pair i with the classical formula (theta, t, cs, sn: the CPU checker's cyclic Jacobi) and updates its
//            own 2 x 2 diagonal block analytically (a_pp - t a_pq, a_qq + t a_pq, off-diagonal exactly 0);
//   phase B  every off-diagonal 2 x 2 block (pair i, pair j), i < j, becomes R_i^T B R_j (mirrored: A stays bitwise symmetric), V becomes V J.
// A sweep is N - 1 steps; before each sweep off = sum_{i<j} a_ij^2 and diag = sum a_ii^2 are reduced in a fixed order and the oracle's test
// off <= 1e-30 (diag + 1e-300) ends the iteration.  30 sweeps without convergence is a failure: out_scalars[3] (the rank) becomes -1 and the
// host refuses the result (be_marg_host.hip).  Schedule and reductions are fixed, so the result is bitwise reproducible.
//
// Out of scope: the reference's pseudo-inverse of a rank-deficient A_mm (a dense eigen-decomposition of 15 + L columns does not fit one
// workgroup).  be_marg_finish keeps eliminating A_mm with its LDL^T and reports the smallest pivot and the clamp flag (out_scalars[1], [2];
// dv_est_get_marg_health); on every sequence measured that pivot is ~1e4, where the pseudo-inverse IS the inverse.
#include <hip/hip_runtime.h>
#include <cfloat>
#include "be_kernels.h"
#include "dev_once.h"

#define EG_THREADS 1024
#define EG_MAXN 96
#define EG_SWEEPS 30
#define EG_EPS 1e-8

__device__ __forceinline__ double eg_wave_sum(double v) {      // fixed xor tree: the same bits on every run
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(EG_THREADS) void be_marg_eig_kernel(BeMargEigArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = a.n, N = (n + 1) & ~1, NP = N / 2, S = N + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* A = sm;                   // N x S
    double* V = sm + (size_t)N * S;   // N x S
    __shared__ double s_c[EG_MAXN / 2], s_s[EG_MAXN / 2];
    __shared__ int s_p[EG_MAXN / 2], s_q[EG_MAXN / 2];
    __shared__ double s_red[2][EG_THREADS / 64];
    __shared__ double s_ev[EG_MAXN], s_y[EG_MAXN];
    __shared__ int s_perm[EG_MAXN];
    __shared__ int s_done, s_sweeps;

    // A' from its lower triangle (SelfAdjointEigenSolver reads one triangle), zero padding; V = I
    for (int e = tid; e < N * N; e += EG_THREADS) {
        const int i = e / N, j = e - i * N;
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        A[i * S + j] = (i < n && j < n) ? a.A[(size_t)hi * n + lo] : 0.0;
        V[i * S + j] = i == j ? 1.0 : 0.0;
    }
    if (tid == 0) { s_done = 0; s_sweeps = 0; }
    __syncthreads();

    const int ntri = NP * (NP - 1) / 2;      // off-diagonal blocks (i < j)
    for (int sweep = 0; ; ++sweep) {
        // ---- convergence test (the CPU checker's), fixed-order reduction: thread-strided, wave xor tree, waves in order ----
        double off = 0.0, dg = 0.0;
        for (int e = tid; e < n * n; e += EG_THREADS) {
            const int i = e / n, j = e - i * n;
            const double v = A[i * S + j];
            if (j > i) off += v * v; else if (j == i) dg += v * v;
        }
        off = eg_wave_sum(off); dg = eg_wave_sum(dg);
        if (lane == 0) { s_red[0][wave] = off; s_red[1][wave] = dg; }
        __syncthreads();
        if (tid == 0) {
            double o = 0.0, d = 0.0;
            for (int w = 0; w < EG_THREADS / 64; ++w) { o += s_red[0][w]; d += s_red[1][w]; }
            s_done = (o <= 1e-30 * (d + 1e-300)) ? 1 : (sweep == EG_SWEEPS ? -1 : 0);
            s_sweeps = sweep;
        }
        __syncthreads();
        if (s_done != 0) break;
        // ---- one sweep: N - 1 steps of N / 2 disjoint rotations ----
        for (int r = 0; r < N - 1; ++r) {
            if (tid < NP) {           // phase A: pair tid of step r (circle method: N - 1 fixed, the rest rotate), its rotation, its diagonal block
                int p, q;
                if (tid == 0) { p = r; q = N - 1; }
                else { p = (r + tid) % (N - 1); q = (r - tid + N - 1) % (N - 1); if (p > q) { const int t = p; p = q; q = t; } }
                const double apq = A[p * S + q];
                double c = 1.0, s = 0.0;
                if (fabs(apq) >= 1e-300) {
                    const double app = A[p * S + p], aqq = A[q * S + q];
                    const double theta = (aqq - app) / (2 * apq);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                    c = 1 / sqrt(t * t + 1); s = t * c;
                    A[p * S + p] = app - t * apq; A[q * S + q] = aqq + t * apq;
                    A[p * S + q] = 0.0; A[q * S + p] = 0.0;
                }
                s_c[tid] = c; s_s[tid] = s; s_p[tid] = p; s_q[tid] = q;
            }
            __syncthreads();
            // phase B: off-diagonal blocks (i < j): B <- R_i^T B R_j, written to both triangles
            for (int e = tid; e < ntri; e += EG_THREADS) {
                int j = (int)((sqrtf(8.0f * (float)e + 1.0f) + 1.0f) * 0.5f);      // e = j (j - 1) / 2 + i, i < j
                while (j * (j - 1) / 2 > e) --j;
                while ((j + 1) * j / 2 <= e) ++j;
                const int i = e - j * (j - 1) / 2;
                const int pi = s_p[i], qi = s_q[i], pj = s_p[j], qj = s_q[j];
                const double ci = s_c[i], si = s_s[i], cj = s_c[j], sj = s_s[j];
                const double b00 = A[pi * S + pj], b01 = A[pi * S + qj], b10 = A[qi * S + pj], b11 = A[qi * S + qj];
                const double x00 = cj * b00 - sj * b01, x01 = sj * b00 + cj * b01;      // columns (A R_j)
                const double x10 = cj * b10 - sj * b11, x11 = sj * b10 + cj * b11;
                const double y00 = ci * x00 - si * x10, y10 = si * x00 + ci * x10;      // rows (R_i^T .)
                const double y01 = ci * x01 - si * x11, y11 = si * x01 + ci * x11;
                A[pi * S + pj] = y00; A[pj * S + pi] = y00;
                A[pi * S + qj] = y01; A[qj * S + pi] = y01;
                A[qi * S + pj] = y10; A[pj * S + qi] = y10;
                A[qi * S + qj] = y11; A[qj * S + qi] = y11;
            }
            // V <- V J: (row, pair) tasks; rows >= n of the real columns are zero and stay so
            for (int e = tid; e < n * NP; e += EG_THREADS) {
                const int row = e / NP, k = e - row * NP;
                const int p = s_p[k], q = s_q[k];
                const double c = s_c[k], s = s_s[k];
                const double vp = V[row * S + p], vq = V[row * S + q];
                V[row * S + p] = c * vp - s * vq; V[row * S + q] = s * vp + c * vq;
            }
            __syncthreads();
        }
    }
    const bool ok = s_done > 0;
    // ---- eigenvalues ascending (ties by index: a fixed permutation) ----
    if (tid < n) {
        const double d = A[tid * S + tid];
        int rk = 0;
        for (int j = 0; j < n; ++j) { const double dj = A[j * S + j]; rk += (dj < d || (dj == d && j < tid)) ? 1 : 0; }
        s_ev[rk] = d; s_perm[rk] = tid;
    }
    __syncthreads();
    // y_k = q_k^T b' (in the sorted order)
    if (tid < n) {
        const int k = s_perm[tid];
        double y = 0.0;
        for (int i = 0; i < n; ++i) y += V[i * S + k] * a.b[i];
        s_y[tid] = y;
    }
    __syncthreads();
    // A'_c (lower triangle computed, mirrored), b'_c: sums over the kept eigenpairs in ascending order
    for (int e = tid; e < n * (n + 1) / 2 + n; e += EG_THREADS) {
        if (e >= n * (n + 1) / 2) {
            const int i = e - n * (n + 1) / 2;
            double s = 0.0;
            for (int r = 0; r < n; ++r) if (s_ev[r] > EG_EPS) s += V[i * S + s_perm[r]] * s_y[r];
            a.b[i] = s;
            continue;
        }
        int i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);      // e = i (i + 1) / 2 + j, j <= i
        while (i * (i + 1) / 2 > e) --i;
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        const int j = e - i * (i + 1) / 2;
        double s = 0.0;
        for (int r = 0; r < n; ++r) if (s_ev[r] > EG_EPS) { const int k = s_perm[r]; s += s_ev[r] * V[i * S + k] * V[j * S + k]; }
        a.A[(size_t)i * n + j] = s; a.A[(size_t)j * n + i] = s;
    }
    if (tid == 0) {           // c0 = r0^T r0 with r0_k = S^-1/2 q_k^T b', ascending; rank of J0
        double c0 = 0.0; int rank = 0;
        for (int r = 0; r < n; ++r) if (s_ev[r] > EG_EPS) { const double rk = sqrt(1.0 / s_ev[r]) * s_y[r]; c0 += rk * rk; ++rank; }
        a.scal[0] = c0; a.scal[3] = ok ? (double)rank : -1.0;
        if (a.c0_out) a.c0_out[0] = c0;
        a.spec[EG_MAXN] = (double)s_sweeps; a.spec[EG_MAXN + 1] = (double)n; a.spec[EG_MAXN + 2] = ok ? 1.0 : 0.0;
    }
    for (int r = tid; r < n; r += EG_THREADS) a.spec[r] = s_ev[r];
}

size_t be_marg_eig_smem(int n) { const size_t N = (size_t)((n + 1) & ~1); return 2 * N * (N + 1) * sizeof(double); }

int be_launch_marg_eig(const BeMargEigArgs& a, hipStream_t s) {
    if (a.n < 1 || a.n > EG_MAXN) return -2;
    static DevOnce once;
    if (once.run([] { return hipFuncSetAttribute(reinterpret_cast<const void*>(be_marg_eig_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)be_marg_eig_smem(EG_MAXN)) != hipSuccess ? 1 : 0; })) return -1;
    hipLaunchKernelGGL(be_marg_eig_kernel, dim3(1), dim3(EG_THREADS), be_marg_eig_smem(a.n), s, a);
    return 0;
}
