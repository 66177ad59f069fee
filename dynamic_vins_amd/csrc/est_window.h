// est_window.h — the estimator's window bookkeeping and host arithmetic (product code, HIP-free: no dv_ctx, stream or HIP call; est_host.hip schedules the
// device around it, tests/host/est_window_host.cpp runs it under the sanitizers).  Mirrors, with flat arrays instead of std::list / Eigen / Ceres objects:
//   Estimator::{InputIMU (FastPredictIMU),ProcessMeasurements (GetIMUInterval, AddIMU, InitFirstIMUPose),SlideWindow,InitFramePoseByPnP,
//               UpdateLatestStates,ClearState}                                              estimator/estimator.cpp
//   BodyState::{SetOptimizeParameters,GetOptimizationParameters} and the residual-block tables of AddResidualBlock      estimator/body.cpp, estimator.cpp:130-178
//   FeatureManager::{AddFeatureCheckParallax,TriangulatePoints,RemoveBack*,RemoveFront,RemoveOutlier,RemoveFailures}    estimator/feature_manager.cpp
//   IntegrationBase (midpoint pre-integration)                                          estimator/imu/integration_base.h
//   OutliersRejection / TriangulatePoint / SolvePoseByPnP / SolveGyroscopeBias          estimator/vio_util.cpp, initial/
// Deviation from the reference that changes no result: feature lookup by merge join / hash map instead of the O(N*L) find_if (feature_manager.cpp:80-83).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <unordered_map>
#include <vector>
#include "be_math.h"
#include "inst_host.h"
#include "line_host.h"

namespace estw {
using namespace be;

constexpr int kWin = dvi::kW;
constexpr double kFocal = 460.0;

inline void put3(double* o, d3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }      // (the way back is be::P3)
inline void pack_pose(d3 P, quat q, double* o) { put3(o, P); o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w; }      // pose block [p, qx qy qz qw]
inline void pack_pose(d3 P, const m33& R, double* o) { pack_pose(P, qfromR(R), o); }

// the one Cholesky of the host side: A = L L^T in the left-looking column order, sums in ascending k, and the two substitutions (PnP seed 6x6, SolveGyroscopeBias 3x3, below 15x15)
template <int N> inline bool chol_factor(const double (&A)[N][N], double (&L)[N][N]) {      // lower triangle of L only; false on a non-positive pivot
    for (int j = 0; j < N; ++j) {
        double s = A[j][j]; for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0)) return false;
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < N; ++i) { double t = A[i][j]; for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k]; L[i][j] = t / L[j][j]; }
    }
    return true;
}
template <int N> inline bool chol_solve(const double (&A)[N][N], const double (&b)[N], double (&x)[N]) {      // A x = b; x untouched when A is not positive definite
    double L[N][N];
    if (!chol_factor(A, L)) return false;
    for (int i = 0; i < N; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s -= L[i][k] * x[k]; x[i] = s / L[i][i]; }
    for (int i = N - 1; i >= 0; --i) { double s = x[i]; for (int k = i + 1; k < N; ++k) s -= L[k][i] * x[k]; x[i] = s / L[i][i]; }
    return true;
}

// 15x15: U upper-triangular with U^T U = cov^-1   (LLT(cov^-1).matrixL().transpose(), imu_factor.h:74-75; cached, Q8)
inline bool imu_sqrt_info(const double* cov, double* U) {
    double a[15][30];
    for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) { a[i][j] = cov[i * 15 + j]; a[i][15 + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < 15; ++c) {
        int p = c; for (int i = c + 1; i < 15; ++i) if (std::fabs(a[i][c]) > std::fabs(a[p][c])) p = i;
        if (a[p][c] == 0.0) return false;
        if (p != c) for (int j = 0; j < 30; ++j) std::swap(a[c][j], a[p][j]);
        const double piv = a[c][c];
        for (int j = 0; j < 30; ++j) a[c][j] /= piv;
        for (int i = 0; i < 15; ++i) if (i != c) { const double f = a[i][c]; if (f != 0.0) for (int j = 0; j < 30; ++j) a[i][j] -= f * a[c][j]; }
    }
    double inv[15][15], L[15][15];
    for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) inv[i][j] = 0.5 * (a[i][15 + j] + a[j][15 + i]);
    if (!chol_factor(inv, L)) return false;
    for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) U[i * 15 + j] = j >= i ? L[j][i] : 0.0;
    return true;
}

struct Preint {       // IntegrationBase
    d3 acc_0, gyr_0, lin_acc, lin_gyr, lin_ba, lin_bg, dp, dv; quat dq;
    double J[225], P[225], noise[18], sum_dt = 0;
    mutable double U[225]; mutable bool U_ok = false;      // cached sqrt-information of P (IMUFactor recomputes it on every Evaluate, Q8)
    std::vector<double> dts; std::vector<d3> accs, gyrs;
    Preint(d3 a0, d3 g0, d3 ba, d3 bg, const double n4[4]) : acc_0(a0), gyr_0(g0), lin_acc(a0), lin_gyr(g0), lin_ba(ba), lin_bg(bg) {
        reset_state();
        const double v[6] = { n4[0] * n4[0], n4[1] * n4[1], n4[0] * n4[0], n4[1] * n4[1], n4[2] * n4[2], n4[3] * n4[3] };
        for (int b = 0; b < 6; ++b) for (int k = 0; k < 3; ++k) noise[3 * b + k] = v[b];
    }
    void reset_state() { dp = mk3(0, 0, 0); dv = mk3(0, 0, 0); dq = mkq(1, 0, 0, 0); sum_dt = 0; for (int i = 0; i < 225; ++i) { J[i] = (i % 16 == 0) ? 1.0 : 0.0; P[i] = 0.0; } }
    void push_back(double dt, d3 a, d3 g) { dts.push_back(dt); accs.push_back(a); gyrs.push_back(g); propagate(dt, a, g); }
    void repropagate(d3 ba, d3 bg) {
        acc_0 = lin_acc; gyr_0 = lin_gyr; lin_ba = ba; lin_bg = bg; reset_state();
        for (size_t i = 0; i < dts.size(); ++i) propagate(dts[i], accs[i], gyrs[i]);
    }
    static void blk(double* M, int ld, int r, int c, const m33& b) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[(r + i) * ld + c + j] = b.m[i * 3 + j]; }
    void propagate(double dt, d3 a1, d3 g1) {      // midPointIntegration + propagate (integration_base.h:70-173)
        const d3 un_acc_0 = qrot(dq, acc_0 - lin_ba);
        const d3 un_gyr = (gyr_0 + g1) * 0.5 - lin_bg;
        const quat rq = qmul(dq, mkq(1, un_gyr.x * dt / 2, un_gyr.y * dt / 2, un_gyr.z * dt / 2));
        const d3 un_acc_1 = qrot(rq, a1 - lin_ba);
        const d3 un_acc = (un_acc_0 + un_acc_1) * 0.5;
        const d3 rp = dp + dv * dt + un_acc * (0.5 * dt * dt), rv = dv + un_acc * dt;
        const m33 Rw = skew(un_gyr), Ra0 = skew(acc_0 - lin_ba), Ra1 = skew(a1 - lin_ba), I = eye3(), Rq = qR(dq), Rr = qR(rq);
        const m33 IRw = sub(I, scale(Rw, dt));
        static thread_local double F[225], V[270], T1[225];
        std::fill(F, F + 225, 0.0); std::fill(V, V + 270, 0.0);
        blk(F, 15, 0, 0, I);
        blk(F, 15, 0, 3, add(scale(mul(Rq, Ra0), -0.25 * dt * dt), scale(mul(mul(Rr, Ra1), IRw), -0.25 * dt * dt)));
        blk(F, 15, 0, 6, scale(I, dt));
        blk(F, 15, 0, 9, scale(add(Rq, Rr), -0.25 * dt * dt));
        blk(F, 15, 0, 12, scale(mul(Rr, Ra1), -0.25 * dt * dt * -dt));
        blk(F, 15, 3, 3, IRw); blk(F, 15, 3, 12, scale(I, -dt));
        blk(F, 15, 6, 3, add(scale(mul(Rq, Ra0), -0.5 * dt), scale(mul(mul(Rr, Ra1), IRw), -0.5 * dt)));
        blk(F, 15, 6, 6, I); blk(F, 15, 6, 9, scale(add(Rq, Rr), -0.5 * dt)); blk(F, 15, 6, 12, scale(mul(Rr, Ra1), -0.5 * dt * -dt));
        blk(F, 15, 9, 9, I); blk(F, 15, 12, 12, I);
        const m33 V03 = scale(mul(scale(Rr, -1.0), Ra1), 0.25 * dt * dt * 0.5 * dt), V63 = scale(mul(scale(Rr, -1.0), Ra1), 0.5 * dt * 0.5 * dt);
        blk(V, 18, 0, 0, scale(Rq, 0.25 * dt * dt)); blk(V, 18, 0, 3, V03); blk(V, 18, 0, 6, scale(Rr, 0.25 * dt * dt)); blk(V, 18, 0, 9, V03);
        blk(V, 18, 3, 3, scale(I, 0.5 * dt)); blk(V, 18, 3, 9, scale(I, 0.5 * dt));
        blk(V, 18, 6, 0, scale(Rq, 0.5 * dt)); blk(V, 18, 6, 3, V63); blk(V, 18, 6, 6, scale(Rr, 0.5 * dt)); blk(V, 18, 6, 9, V63);
        blk(V, 18, 9, 12, scale(I, dt)); blk(V, 18, 12, 15, scale(I, dt));
        // J <- F J, P <- F P F^T + V diag(noise) V^T over the STRUCTURAL non-zeros of F and V only (81 of 225 and 78 of 270 entries: identity / zero blocks).
        // The skipped products are exact zeros and the kept ones are added in the same (ascending k) order as the dense loops of
        // integration_base.h, so the sums are the same bits; a third of the multiply-adds (44 -> ~16 us per frame at 10 samples).
        static const struct Pattern {
            int fn[15], fk[15][11], vn[15], vk[15][12];
            Pattern() {
                for (int i = 0; i < 15; ++i) {
                    const int b = i / 3, r = i % 3; int n = 0;
                    auto blk3 = [&](int c0) { fk[i][n++] = c0; fk[i][n++] = c0 + 1; fk[i][n++] = c0 + 2; };
                    if (b == 0) { fk[i][n++] = r; blk3(3); fk[i][n++] = 6 + r; blk3(9); blk3(12); }
                    else if (b == 1) { blk3(3); fk[i][n++] = 12 + r; }
                    else if (b == 2) { blk3(3); fk[i][n++] = 6 + r; blk3(9); blk3(12); }
                    else fk[i][n++] = i;
                    fn[i] = n;
                    int m = 0;
                    if (b == 0 || b == 2) for (int k = 0; k < 12; ++k) vk[i][m++] = k;
                    else if (b == 1) { vk[i][m++] = 3 + r; vk[i][m++] = 9 + r; }
                    else if (b == 3) vk[i][m++] = 12 + r;
                    else vk[i][m++] = 15 + r;
                    vn[i] = m;
                }
            }
        } pat;
        // axpy form (row of the result += scalar * row of the right operand): every entry still receives its products in ascending k, one rounding each,
        // but the inner loop runs over 15 independent entries and vectorises
        auto fmul = [&](const double* B, double* C) {          // C = F B
            for (int i = 0; i < 15; ++i) {
                double acc[15] = { 0 };
                for (int q = 0; q < pat.fn[i]; ++q) { const int k = pat.fk[i][q]; const double f = F[i * 15 + k]; const double* b = B + k * 15; for (int j = 0; j < 15; ++j) acc[j] += f * b[j]; }
                for (int j = 0; j < 15; ++j) C[i * 15 + j] = acc[j];
            }
        };
        fmul(J, T1); std::copy(T1, T1 + 225, J);
        fmul(P, T1);                                          // F P
        double Ft[225], Vt[270], FPFt[225];
        for (int i = 0; i < 15; ++i) for (int k = 0; k < 15; ++k) Ft[k * 15 + i] = F[i * 15 + k];
        for (int i = 0; i < 15; ++i) for (int k = 0; k < 18; ++k) Vt[k * 15 + i] = V[i * 18 + k];
        for (int i = 0; i < 15; ++i) {                        // (F P) F^T: the structural zeros of F^T contribute exact zeros
            double acc[15] = { 0 };
            for (int k = 0; k < 15; ++k) { const double t = T1[i * 15 + k]; const double* b = Ft + k * 15; for (int j = 0; j < 15; ++j) acc[j] += t * b[j]; }
            for (int j = 0; j < 15; ++j) FPFt[i * 15 + j] = acc[j];
        }
        for (int i = 0; i < 15; ++i) {                        // + V diag(noise) V^T
            double acc[15] = { 0 };
            for (int q = 0; q < pat.vn[i]; ++q) { const int k = pat.vk[i][q]; const double t = V[i * 18 + k] * noise[k]; const double* b = Vt + k * 15; for (int j = 0; j < 15; ++j) acc[j] += t * b[j]; }
            for (int j = 0; j < 15; ++j) P[i * 15 + j] = FPFt[i * 15 + j] + acc[j];
        }
        dp = rp; dq = qnormalized(rq); dv = rv; sum_dt += dt; acc_0 = a1; gyr_0 = g1; U_ok = false;
    }
    const double* sqrt_info() const { if (!U_ok) U_ok = imu_sqrt_info(P, U); return U_ok ? U : nullptr; }
    m33 jb(int r, int c) const { m33 b; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) b.m[i * 3 + j] = J[(r + i) * 15 + c + j]; return b; }
    void fill(dv_ba_imu& o, int fi, int fj) const {
        o.sum_dt = sum_dt;
        put3(o.dp, dp); put3(o.dv, dv); put3(o.lin_ba, lin_ba); put3(o.lin_bg, lin_bg);
        o.dq[0] = dq.w; o.dq[1] = dq.x; o.dq[2] = dq.y; o.dq[3] = dq.z;
        std::memcpy(o.jacobian, J, sizeof(J)); std::memcpy(o.covariance, P, sizeof(P));
        o.fi = fi; o.fj = fj; o.pad0 = o.pad1 = 0;
    }
};

struct Obs { d3 pt, pt_r, vel, vel_r; double td; bool stereo; };
struct Lm { int id, start; std::vector<Obs> obs; double depth = -1.0; int solve_flag = 0; int end() const { return start + (int)obs.size() - 1; } };

// symmetric 4x4 eigen (cyclic Jacobi) -> eigenvector of the smallest eigenvalue
inline void smallest_eigvec4(double A[4][4], double v[4]) {
    double V[4][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } };
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0; for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j];
        if (off < 1e-300) break;
        for (int p = 0; p < 3; ++p) for (int q = p + 1; q < 4; ++q) {
            if (std::fabs(A[p][q]) < 1e-300) continue;
            const double th = (A[q][q] - A[p][p]) / (2 * A[p][q]);
            const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1)), c = 1 / std::sqrt(t * t + 1), s = t * c;
            for (int k = 0; k < 4; ++k) { const double a = A[k][p], b = A[k][q]; A[k][p] = c * a - s * b; A[k][q] = s * a + c * b; }
            for (int k = 0; k < 4; ++k) { const double a = A[p][k], b = A[q][k]; A[p][k] = c * a - s * b; A[q][k] = s * a + c * b; }
            for (int k = 0; k < 4; ++k) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
        }
    }
    int m = 0; for (int i = 1; i < 4; ++i) if (A[i][i] < A[m][m]) m = i;
    for (int i = 0; i < 4; ++i) v[i] = V[i][m];
}

inline quat from_two_vectors(d3 a, d3 b) {
    const d3 v0 = a / norm(a), v1 = b / norm(b);
    const double c = dot(v1, v0);
    if (c < -1.0 + 1e-12) { d3 ax = std::fabs(v0.x) < 0.9 ? cross(mk3(1, 0, 0), v0) : cross(mk3(0, 1, 0), v0); ax = ax / norm(ax); return mkq(0, ax.x, ax.y, ax.z); }
    const d3 ax = cross(v0, v1); const double s = sqrt((1.0 + c) * 2.0), inv = 1.0 / s;
    return mkq(s * 0.5, ax.x * inv, ax.y * inv, ax.z * inv);
}

struct EstWindow {
    dv_est_config cfg;
    m33 ric[2]; d3 tic[2]; d3 Ps[kWin + 1], Vs[kWin + 1], Bas[kWin + 1], Bgs[kWin + 1]; m33 Rs[kWin + 1];
    d3 g; double td = 0, headers[kWin + 1] = { 0 };
    int frame = 0;
    std::vector<Lm> lms; std::unordered_map<int, size_t> lm_index; bool index_dirty = true;
    std::deque<std::pair<double, std::pair<d3, d3>>> imu_buf;
    double prev_time = -1, cur_time = 0; bool first_imu = false, init_pose = false; d3 acc_0, gyr_0;
    std::unique_ptr<Preint> pre[kWin + 1], tmp_pre;          // each keeps its own samples (dts / accs / gyrs): the second-new slide and repropagate replay them
    std::vector<std::shared_ptr<Preint>> frame_pre;        // all_image_frame pre-integrations (initialisation only)
    bool nonlinear = false, margin_old = true;
    m33 back_R0; d3 back_P0;
    // line mode (cfg.use_line): FeatureManager::line_landmarks
    dvl::LineMgr lines; std::vector<dv_line_row> pending_lines;
    bool line_zero_w() const { return cfg.line_sqrt_info[0] == 0.0 && cfg.line_sqrt_info[1] == 0.0 && cfg.line_sqrt_info[2] == 0.0 && cfg.line_sqrt_info[3] == 0.0; }
    // Estimator::latest_* (estimator.h): the state of the newest frame propagated by every IMU sample that arrived since (FastPredictIMU, estimator.cpp:1376-1392)
    double latest_time = 0; d3 latest_P, latest_V, latest_Ba, latest_Bg, latest_acc_0, latest_gyr_0; quat latest_Q; bool latest_valid = false;
    void fast_predict_imu(double t, d3 la, d3 av) {
        const double dt = t - latest_time; latest_time = t;
        const d3 un_acc_0 = qrot(latest_Q, latest_acc_0 - latest_Ba) - g;
        const d3 un_gyr = (latest_gyr_0 + av) * 0.5 - latest_Bg;
        latest_Q = qmul(latest_Q, dq_half(un_gyr * dt));
        const d3 un_acc_1 = qrot(latest_Q, la - latest_Ba) - g;
        const d3 un_acc = (un_acc_0 + un_acc_1) * 0.5;
        latest_P = latest_P + latest_V * dt + un_acc * (0.5 * dt * dt);
        latest_V = latest_V + un_acc * dt;
        latest_acc_0 = la; latest_gyr_0 = av;
    }
    void update_latest_states() {          // UpdateLatestStates (estimator.cpp:1395-1418)
        latest_time = headers[frame] + td; latest_P = Ps[frame]; latest_Q = qfromR(Rs[frame]); latest_V = Vs[frame]; latest_Ba = Bas[frame]; latest_Bg = Bgs[frame];
        latest_acc_0 = acc_0; latest_gyr_0 = gyr_0; latest_valid = true;
        for (auto& smp : imu_buf) fast_predict_imu(smp.first, smp.second.first, smp.second.second);
    }
    // flat problem buffers
    std::vector<dv_ba_factor> fac; std::vector<dv_ba_lm> lmt; std::vector<dv_ba_imu> imu; std::vector<double> invd;
    double pose[kWin + 1][7], sb[kWin + 1][9], ex[2][7], tdv[1];

    explicit EstWindow(const dv_est_config& c) : cfg(c) { clear(); }
    void clear() {
        for (int i = 0; i <= kWin; ++i) { Rs[i] = eye3(); Ps[i] = Vs[i] = Bas[i] = Bgs[i] = mk3(0, 0, 0); pre[i].reset(); headers[i] = 0; }
        lms.clear(); lm_index.clear(); imu_buf.clear(); frame_pre.clear(); tmp_pre.reset();
        prev_time = -1; cur_time = 0; first_imu = false; init_pose = false; frame = 0; nonlinear = false; acc_0 = gyr_0 = mk3(0, 0, 0);
        for (int k = 0; k < 2; ++k) { for (int i = 0; i < 9; ++i) ric[k].m[i] = cfg.ric[k][i]; tic[k] = P3(cfg.tic[k]); }
        td = cfg.td; g = mk3(0, 0, cfg.g_norm);
        lines.clear(); lines.min_obs = cfg.line_min_obs > 0 ? cfg.line_min_obs : 5; pending_lines.clear();
        latest_valid = false; latest_time = 0; latest_P = latest_V = latest_Ba = latest_Bg = latest_acc_0 = latest_gyr_0 = mk3(0, 0, 0); latest_Q = mkq(1, 0, 0, 0);
    }
    dvi::BodyView body_view() const { return dvi::BodyView{ Rs, Ps, ric, tic, headers, td, frame }; }
    std::unique_ptr<Preint> new_preint(int i) const { const double n4[4] = { cfg.acc_n, cfg.gyr_n, cfg.acc_w, cfg.gyr_w }; return std::make_unique<Preint>(acc_0, gyr_0, Bas[i], Bgs[i], n4); }

    // ---------------- IMU ----------------
    void process_imu(double dt, d3 la, d3 av) {
        if (!first_imu) { first_imu = true; acc_0 = la; gyr_0 = av; }
        if (!pre[frame]) pre[frame] = new_preint(frame);
        if (frame != 0) {
            pre[frame]->push_back(dt, la, av); tmp_pre->push_back(dt, la, av);
            const int j = frame;
            const d3 un_acc_0 = mul(Rs[j], acc_0 - Bas[j]) - g;
            const d3 un_gyr = (gyr_0 + av) * 0.5 - Bgs[j];
            Rs[j] = mul(Rs[j], qR(dq_half(un_gyr * dt)));
            const d3 un_acc_1 = mul(Rs[j], la - Bas[j]) - g;
            const d3 un_acc = (un_acc_0 + un_acc_1) * 0.5;
            Ps[j] = Ps[j] + Vs[j] * dt + un_acc * (0.5 * dt * dt);
            Vs[j] = Vs[j] + un_acc * dt;
        }
        acc_0 = la; gyr_0 = av;
    }
    bool add_imu_until(double t1) {       // GetIMUInterval + AddIMU (estimator.cpp:752-778,1765-1779)
        if (imu_buf.empty() || !(t1 <= imu_buf.back().first)) return false;
        std::vector<std::pair<double, std::pair<d3, d3>>> v;
        while (imu_buf.front().first <= prev_time) imu_buf.pop_front();
        while (imu_buf.front().first < t1) { v.push_back(imu_buf.front()); imu_buf.pop_front(); }
        v.push_back(imu_buf.front());
        if (!init_pose) {                  // InitFirstIMUPose
            init_pose = true;
            d3 aver = mk3(0, 0, 0); for (auto& s : v) aver = aver + s.second.first; aver = aver / (double)v.size();
            m33 R0 = qR(from_two_vectors(aver, mk3(0, 0, 1)));
            R0 = mul(ypr2r(mk3(-r2ypr(R0).x, 0, 0)), R0);                 // Utility::g2R
            Rs[0] = mul(ypr2r(mk3(-r2ypr(R0).x, 0, 0)), R0);
        }
        for (size_t i = 0; i < v.size(); ++i) {
            double dt;
            if (i == 0) dt = v[i].first - prev_time; else if (i == v.size() - 1) dt = cur_time - v[i - 1].first; else dt = v[i].first - v[i - 1].first;
            process_imu(dt, v[i].second.first, v[i].second.second);
        }
        return true;
    }

    // ---------------- feature manager ----------------
    void reindex() { lm_index.clear(); for (size_t i = 0; i < lms.size(); ++i) lm_index[lms[i].id] = i; index_dirty = false; }
    int long_count() const { int c = 0; for (auto& l : lms) if (l.obs.size() >= 4) ++c; return c; }
    bool add_features(int fc, const dv_feat* feats, int n) {
        // feature ids are handed out by a monotone counter, and landmarks are appended in id order and only ever erased: `lms` stays sorted
        // by id, so matching the (sorted) frame against it is a merge join — no hash index to rebuild after every slide / rejection.
        // Should the invariant ever be broken by a caller (ids not monotone), fall back to the hash index.
        bool sorted_ids = true;
        for (size_t i = 1; i < lms.size(); ++i) if (lms[i - 1].id >= lms[i].id) { sorted_ids = false; break; }
        if (!sorted_ids && index_dirty) reindex();
        std::vector<const dv_feat*> order(n);
        for (int i = 0; i < n; ++i) order[i] = &feats[i];
        std::sort(order.begin(), order.end(), [](const dv_feat* a, const dv_feat* b) { return a->id < b->id; });     // the reference iterates a std::map keyed by id
        int last_track = 0, new_feat = 0, long_track = 0;
        const size_t n_old = lms.size(); size_t cur = 0;
        for (const dv_feat* f : order) {
            Obs o; o.pt = P3(f->left); o.vel = mk3(f->left[5], f->left[6], 0); o.td = td; o.stereo = f->has_right != 0;
            o.pt_r = o.stereo ? P3(f->right) : mk3(0, 0, 0); o.vel_r = o.stereo ? mk3(f->right[5], f->right[6], 0) : mk3(0, 0, 0);
            long found = -1;
            if (sorted_ids) {
                while (cur < n_old && lms[cur].id < (int)f->id) ++cur;
                if (cur < n_old && lms[cur].id == (int)f->id) found = (long)cur;
                else if (!lms.empty() && lms.back().id >= (int)f->id) {      // a new id below a known one: the order would break -> hash index from here on
                    sorted_ids = false; reindex();
                }
            }
            if (!sorted_ids) { auto it = lm_index.find((int)f->id); if (it != lm_index.end()) found = (long)it->second; }
            if (found < 0) { Lm l; l.id = (int)f->id; l.start = fc; l.obs.push_back(o); if (!sorted_ids) lm_index[l.id] = lms.size(); lms.push_back(std::move(l)); new_feat++; }
            else { Lm& l = lms[(size_t)found]; l.obs.push_back(o); last_track++; if (l.obs.size() >= 4) long_track++; }
        }
        if (fc < 2 || last_track < 20 || long_track < 40 || new_feat > 0.5 * last_track) return true;
        double psum = 0; int pnum = 0;
        for (auto& l : lms) if (l.start <= fc - 2 && l.end() >= fc - 1) {
            const Obs& a = l.obs[fc - 2 - l.start]; const Obs& b = l.obs[fc - 1 - l.start];
            const double du = a.pt.x / a.pt.z - b.pt.x, dv = a.pt.y / a.pt.z - b.pt.y;
            psum += sqrt(du * du + dv * dv); pnum++;
        }
        if (pnum == 0) return true;
        return psum / pnum >= cfg.keyframe_parallax / kFocal;
    }
    static double tri_depth(const double L[3][4], const double R[3][4], double x0, double y0, double x1, double y1) {
        double D[4][4], A[4][4], v[4];
        for (int c = 0; c < 4; ++c) { D[0][c] = x0 * L[2][c] - L[0][c]; D[1][c] = y0 * L[2][c] - L[1][c]; D[2][c] = x1 * R[2][c] - R[0][c]; D[3][c] = y1 * R[2][c] - R[1][c]; }
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += D[k][i] * D[k][j]; A[i][j] = s; }
        smallest_eigvec4(A, v);
        const double X = v[0] / v[3], Y = v[1] / v[3], Z = v[2] / v[3];
        return L[2][0] * X + L[2][1] * Y + L[2][2] * Z + L[2][3];
    }
    void triangulate() {
        for (auto& l : lms) {
            if (l.depth > 0) continue;
            double L[3][4], R[3][4]; const dvi::BodyView B = body_view();
            if (cfg.stereo && l.obs[0].stereo) { B.cam34(l.start, 0, L); B.cam34(l.start, 1, R); const double d = tri_depth(L, R, l.obs[0].pt.x, l.obs[0].pt.y, l.obs[0].pt_r.x, l.obs[0].pt_r.y); l.depth = d > 0 ? d : cfg.init_depth; }
            else if (l.obs.size() > 1) { B.cam34(l.start, 0, L); B.cam34(l.start + 1, 0, R); const double d = tri_depth(L, R, l.obs[0].pt.x, l.obs[0].pt.y, l.obs[1].pt.x, l.obs[1].pt.y); l.depth = d > 0 ? d : cfg.init_depth; }
        }
    }
    template <class Pred> void erase_if(Pred p) { lms.erase(std::remove_if(lms.begin(), lms.end(), p), lms.end()); index_dirty = true; }

    // ---------------- PnP seed (solvePnP iterative restated as LM on rvec/t) ----------------
    static m33 rodrigues(d3 r) { const double th = norm(r); if (th < 1e-12) return add(eye3(), skew(r)); const m33 K = skew(r / th); return add(add(eye3(), scale(K, sin(th))), scale(mul(K, K), 1 - cos(th))); }
    static d3 inv_rodrigues(const m33& R) {
        quat q = qnormalized(qfromR(R)); if (q.w < 0) q = mkq(-q.w, -q.x, -q.y, -q.z);
        const double s = norm(qvec(q)); if (s < 1e-12) return qvec(q) * 2.0;
        return qvec(q) / s * (2 * atan2(s, q.w));
    }
    void pnp_frame(int fc) {
        if (fc <= 0) return;
        std::vector<d3> p3; std::vector<std::pair<float, float>> p2;
        for (auto& l : lms) if (l.depth > 0) {
            const int idx = fc - l.start;
            if ((int)l.obs.size() >= idx + 1) {
                const d3 w = mul(Rs[l.start], mul(ric[0], l.obs[0].pt * l.depth) + tic[0]) + Ps[l.start];
                p3.push_back(mk3((float)w.x, (float)w.y, (float)w.z)); p2.push_back({ (float)l.obs[idx].pt.x, (float)l.obs[idx].pt.y });
            }
        }
        if ((int)p2.size() < 4) return;
        m33 RCam = mul(Rs[fc - 1], ric[0]); d3 PCam = mul(Rs[fc - 1], tic[0]) + Ps[fc - 1];
        const m33 Ri = tr(RCam); const d3 ti = -mul(Ri, PCam), rv = inv_rodrigues(Ri);
        double x[6] = { rv.x, rv.y, rv.z, ti.x, ti.y, ti.z };
        auto resid = [&](const double* p, std::vector<double>& r) {
            const m33 Rm = rodrigues(P3(p)); const d3 t = P3(p + 3); double c = 0; r.resize(p2.size() * 2);
            for (size_t i = 0; i < p2.size(); ++i) { const d3 q = mul(Rm, p3[i]) + t; r[2 * i] = q.x / q.z - p2[i].first; r[2 * i + 1] = q.y / q.z - p2[i].second; c += r[2 * i] * r[2 * i] + r[2 * i + 1] * r[2 * i + 1]; }
            return c;
        };
        std::vector<double> r0, r1; double lambda = 1e-3, c0 = resid(x, r0);
        for (int it = 0; it < 20; ++it) {
            double JtJ[6][6] = { { 0 } }, Jtr[6] = { 0 };
            std::vector<double> rp;
            std::vector<std::vector<double>> Jc(6);
            for (int k = 0; k < 6; ++k) { double xp[6]; std::memcpy(xp, x, sizeof(xp)); xp[k] += 1e-7; resid(xp, rp); Jc[k].resize(rp.size()); for (size_t q = 0; q < rp.size(); ++q) Jc[k][q] = (rp[q] - r0[q]) / 1e-7; }
            for (int a = 0; a < 6; ++a) { for (size_t q = 0; q < r0.size(); ++q) Jtr[a] += Jc[a][q] * r0[q]; for (int b = 0; b < 6; ++b) { double s = 0; for (size_t q = 0; q < r0.size(); ++q) s += Jc[a][q] * Jc[b][q]; JtJ[a][b] = s; } }
            bool improved = false;
            for (int tries = 0; tries < 10 && !improved; ++tries) {
                double A[6][6], d[6];
                for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) A[a][b] = JtJ[a][b] * (a == b ? 1 + lambda : 1.0);
                if (!chol_solve(A, Jtr, d)) { lambda *= 10; continue; }
                double xn[6]; for (int a = 0; a < 6; ++a) xn[a] = x[a] - d[a];
                const double c1 = resid(xn, r1);
                if (c1 < c0) { std::memcpy(x, xn, sizeof(xn)); r0 = r1; const double dc = c0 - c1; c0 = c1; lambda = std::max(lambda / 10, 1e-16); improved = true; if (dc < 1e-20) it = 100; }
                else lambda *= 10;
            }
            if (!improved) break;
        }
        const m33 Rp = rodrigues(P3(x));
        RCam = tr(Rp); PCam = mul(RCam, -P3(x + 3));
        Rs[fc] = mul(RCam, tr(ric[0])); Ps[fc] = -mul(mul(RCam, tr(ric[0])), tic[0]) + PCam;
        if (cfg.plane_constraint) { if (cfg.use_imu) Ps[fc].z = 0; else Ps[fc].y = 0; }
    }

    // ---------------- the solve's tables and parameter blocks ----------------
    void states_to_arrays() {        // BodyState::SetOptimizeParameters
        for (int i = 0; i <= kWin; ++i) { pack_pose(Ps[i], Rs[i], pose[i]); put3(sb[i], Vs[i]); put3(sb[i] + 3, Bas[i]); put3(sb[i] + 6, Bgs[i]); }
        for (int c = 0; c < 2; ++c) pack_pose(tic[c], ric[c], ex[c]);
        tdv[0] = td;
    }
    static dv_ba_factor mkfac(const Obs& o0, const Obs& o, bool right, int kind, int lm, int fi, int fj) {
        dv_ba_factor f{}; f.pix = o0.pt.x; f.piy = o0.pt.y; f.pjx = right ? o.pt_r.x : o.pt.x; f.pjy = right ? o.pt_r.y : o.pt.y;
        f.vix = o0.vel.x; f.viy = o0.vel.y; f.vjx = right ? o.vel_r.x : o.vel.x; f.vjy = right ? o.vel_r.y : o.vel.y; f.td_i = o0.td; f.td_j = o.td;
        f.kind = kind; f.lm = lm; f.fi = fi; f.fj = fj; return f;
    }
    // builds the residual blocks of AddResidualBlock (estimator.cpp:130-178); only_anchor0: the marginalization subset (:440-493)
    // out / cap: optional destination for the factor records — the caller's pinned staging mirror of the device's upload region
    // (be_staging_factors), so that the table is assembled where the upload reads it instead of being copied there (336 KB per frame)
    dv_ba_factor* fac_out = nullptr; int fac_cap = 0, nfac = 0;
    void put_factor(const dv_ba_factor& f) {
        if (fac_out && nfac < fac_cap) fac_out[nfac] = f;
        else { if (fac_out) { fac.assign(fac_out, fac_out + nfac); fac_out = nullptr; } fac.push_back(f); }      // over capacity: back to the vector
        ++nfac;
    }
    void build_factors(bool only_anchor0, dv_ba_factor* out, int cap) {
        fac_out = out; fac_cap = cap;
        fac.clear(); nfac = 0; lmt.clear(); if (!only_anchor0) invd.clear();
        int fi = -1;
        for (auto& l : lms) {
            if (l.obs.size() < 4) continue;
            ++fi;
            if (!only_anchor0) invd.push_back(1.0 / l.depth);
            if (only_anchor0 && l.start != 0) continue;
            dv_ba_lm t{}; t.first = nfac; t.anchor = l.start; t.mask = 0;
            int j = l.start - 1;
            for (auto& o : l.obs) {
                ++j; t.mask |= 1 << j;
                if (j != l.start) put_factor(mkfac(l.obs[0], o, false, 0, fi, l.start, j));
                if (cfg.stereo && o.stereo) put_factor(mkfac(l.obs[0], o, true, j != l.start ? 1 : 2, fi, l.start, j));
            }
            t.count = nfac - t.first;
            lmt.push_back(t);
        }
    }
    dv_ba_problem make_problem(int nframes) {          // everything but the prior
        dv_ba_problem P{};
        P.nframes = nframes; P.nlm = (int)lmt.size(); P.nfac = nfac; P.nimu = (int)imu.size(); P.use_imu = cfg.use_imu;
        P.plane_kind = cfg.plane_constraint ? (cfg.use_imu ? 1 : 2) : 0; P.max_iters = cfg.max_iters; P.g_norm = cfg.g_norm;
        P.pose = &pose[0][0]; P.speed_bias = &sb[0][0]; P.ex_pose = &ex[0][0]; P.td = tdv; P.inv_depth = invd.data();
        P.factors = fac_out ? fac_out : fac.data(); P.landmarks = lmt.data(); P.imu = imu.data();
        return P;
    }
    void arrays_to_states() {         // Double2vector + BodyState::GetOptimizationParameters (body.cpp:61-132); the yaw-gauge fix ran on the device
        for (int i = 0; i <= kWin; ++i) {
            Rs[i] = qR(qnormalized(Q4(pose[i]))); Ps[i] = P3(pose[i]);
            if (cfg.use_imu) { Vs[i] = P3(sb[i]); Bas[i] = P3(sb[i] + 3); Bgs[i] = P3(sb[i] + 6); }
        }
        if (cfg.use_imu) {
            for (int c = 0; c < 2; ++c) { tic[c] = P3(ex[c]); ric[c] = qR(qnormalized(Q4(ex[c]))); }
            td = tdv[0];
        }
        int k = -1;
        for (auto& l : lms) if (l.obs.size() >= 4) { l.depth = 1.0 / invd[++k]; l.solve_flag = l.depth < 0 ? 2 : 1; }
    }
    // OutliersRejection + RemoveOutlier (vio_util.cpp:381-430).  flags: decided on the device (same expressions, same order: be_reject_kernel), one flag per
    // landmark of the problem = per landmark with >= 4 observations, in order; null: the host rule
    void reject_outliers(const uint8_t* flags) {
        if (flags) { int k = -1; erase_if([&](const Lm& l) { if (l.obs.size() < 4) return false; return flags[++k] != 0; }); return; }
        m33 RsT[kWin + 1], ricT[2];          // the transposes, once per frame instead of twice per observation (same values, same products)
        for (int i = 0; i <= kWin; ++i) RsT[i] = tr(Rs[i]);
        ricT[0] = tr(ric[0]); ricT[1] = tr(ric[1]);
        erase_if([&](const Lm& l) {
            if (l.obs.size() < 4) return false;
            double err = 0; int cnt = 0; int j = l.start - 1;
            const d3 pw = mul(Rs[l.start], mul(ric[0], l.obs[0].pt * l.depth) + tic[0]) + Ps[l.start];
            auto rp = [&](int fj, int cam, d3 uv) { const d3 pc = mul(ricT[cam], mul(RsT[fj], pw - Ps[fj]) - tic[cam]); const double rx = pc.x / pc.z - uv.x, ry = pc.y / pc.z - uv.y; return sqrt(rx * rx + ry * ry); };
            for (auto& o : l.obs) { ++j; if (j != l.start) { err += rp(j, 0, o.pt); cnt++; } if (cfg.stereo && o.stereo) { err += rp(j, 1, o.pt_r); cnt++; } }
            return err / cnt * kFocal > 3;
        });
    }
    void fresh_tail_preint() { pre[kWin] = new_preint(kWin); }
    void slide_window() {             // Estimator::SlideWindow (estimator.cpp:1201-1312)
        if (margin_old) {
            back_R0 = Rs[0]; back_P0 = Ps[0];
            if (frame != kWin) return;
            for (int i = 0; i < kWin; ++i) {
                headers[i] = headers[i + 1]; std::swap(Rs[i], Rs[i + 1]); std::swap(Ps[i], Ps[i + 1]);
                if (cfg.use_imu) { std::swap(pre[i], pre[i + 1]); std::swap(Vs[i], Vs[i + 1]); std::swap(Bas[i], Bas[i + 1]); std::swap(Bgs[i], Bgs[i + 1]); }
            }
            headers[kWin] = headers[kWin - 1]; Ps[kWin] = Ps[kWin - 1]; Rs[kWin] = Rs[kWin - 1];
            if (cfg.use_imu) { Vs[kWin] = Vs[kWin - 1]; Bas[kWin] = Bas[kWin - 1]; Bgs[kWin] = Bgs[kWin - 1]; fresh_tail_preint(); }
            if (nonlinear) {          // SlideWindowOld + RemoveBackShiftDepth
                const m33 R0 = mul(back_R0, ric[0]), R1 = mul(Rs[0], ric[0]); const d3 P0 = back_P0 + mul(back_R0, tic[0]), P1 = Ps[0] + mul(Rs[0], tic[0]);
                for (auto& l : lms) {
                    if (l.start != 0) { l.start--; continue; }
                    const d3 uv = l.obs[0].pt; l.obs.erase(l.obs.begin());
                    if (l.obs.size() < 2) { l.id = -1; continue; }
                    const d3 pj = mul(tr(R1), mul(R0, uv * l.depth) + P0 - P1);
                    l.depth = pj.z > 0 ? pj.z : cfg.init_depth;
                }
                erase_if([](const Lm& l) { return l.id < 0; });
                if (cfg.use_line) lines.remove_back_shift(R0, P0, R1, P1);
            } else {                  // RemoveBack
                for (auto& l : lms) { if (l.start != 0) l.start--; else { l.obs.erase(l.obs.begin()); if (l.obs.empty()) l.id = -1; } }
                erase_if([](const Lm& l) { return l.id < 0; });
                if (cfg.use_line) lines.remove_back();
            }
        } else if (frame == kWin) {
            headers[frame - 1] = headers[frame]; Ps[frame - 1] = Ps[frame]; Rs[frame - 1] = Rs[frame];
            if (cfg.use_imu) {
                const Preint& tail = *pre[frame];      // the newest interval's samples, appended to the interval before it
                for (size_t i = 0; i < tail.dts.size(); ++i) pre[frame - 1]->push_back(tail.dts[i], tail.accs[i], tail.gyrs[i]);
                Vs[frame - 1] = Vs[frame]; Bas[frame - 1] = Bas[frame]; Bgs[frame - 1] = Bgs[frame];
                fresh_tail_preint();
            }
            for (auto& l : lms) {     // RemoveFront
                if (l.start == frame) { l.start--; continue; }
                if (l.end() < frame - 1) continue;
                l.obs.erase(l.obs.begin() + (kWin - 1 - l.start));
                if (l.obs.empty()) l.id = -1;
            }
            erase_if([](const Lm& l) { return l.id < 0; });
            if (cfg.use_line) lines.remove_front(frame);
        }
    }
    void solve_gyro_bias() {          // SolveGyroscopeBias (initial_aligment.cpp:29-61)
        double A[3][3] = { { 0 } }, b[3] = { 0 };
        for (size_t k = 0; k + 1 < frame_pre.size(); ++k) {
            const Preint& pj = *frame_pre[k + 1];
            const quat qij = qfromR(mul(tr(Rs[k]), Rs[k + 1]));
            const m33 tA = pj.jb(3, 12); const d3 tb = qvec(qmul(qinv(pj.dq), qij)) * 2.0;
            const m33 AtA = mul(tr(tA), tA); const d3 Atb = mul(tr(tA), tb);
            for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) A[i][j] += AtA.m[i * 3 + j]; b[i] += get(Atb, i); }
        }
        double d[3] = { 0, 0, 0 };
        chol_solve(A, b, d);          // not positive definite: no correction
        for (int i = 0; i <= kWin; ++i) Bgs[i] = Bgs[i] + P3(d);
    }
};

}  // namespace estw
