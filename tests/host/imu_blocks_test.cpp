// be_factor_dev.h compiled for the host: imu_raw_sel called once per block (and once for the residual) must reproduce imu_raw's residual and 15 x 30 Jacobian bit for bit,
// and a call must write its own block only.  Random factors from a fixed generator plus one with zero biases and identity rotations.  Prints "ok <n>" or the first difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "be_factor_dev.h"

using namespace be;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double rnd() {      // uniform in (-1, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(g_state >> 11) / (double)(1ull << 52) - 1.0;
}
static void unit_quat(double* q) {      // x y z w
    double n = 0;
    for (int k = 0; k < 4; ++k) { q[k] = rnd(); n += q[k] * q[k]; }
    n = sqrt(n);
    for (int k = 0; k < 4; ++k) q[k] /= n;
}

int main() {
    int checked = 0;
    for (int trial = 0; trial < 9; ++trial) {
        const bool zero = trial == 8;
        BeImu m;
        std::memset(&m, 0, sizeof(m));
        double pose_i[7] = { 0, 0, 0, 0, 0, 0, 1 }, pose_j[7] = { 0, 0, 0, 0, 0, 0, 1 }, sb_i[9] = { 0 }, sb_j[9] = { 0 };
        m.sum_dt = 0.1; m.dq[0] = 1.0;
        if (!zero) {
            m.sum_dt = 0.05 + 0.1 * (rnd() + 1.0);
            for (int k = 0; k < 3; ++k) { m.dp[k] = 0.1 * rnd(); m.dv[k] = rnd(); m.lin_ba[k] = 0.02 * rnd(); m.lin_bg[k] = 0.005 * rnd(); pose_i[k] = 3 * rnd(); pose_j[k] = pose_i[k] + 0.2 * rnd(); }
            double q[4]; unit_quat(q); m.dq[0] = q[3]; m.dq[1] = q[0]; m.dq[2] = q[1]; m.dq[3] = q[2];
            unit_quat(pose_i + 3); unit_quat(pose_j + 3);
            for (int k = 0; k < 9; ++k) { m.dp_dba[k] = 0.01 * rnd(); m.dp_dbg[k] = 0.01 * rnd(); m.dq_dbg[k] = 0.1 * rnd(); m.dv_dba[k] = 0.1 * rnd(); m.dv_dbg[k] = 0.1 * rnd(); sb_i[k] = (k < 3 ? 1.0 : 0.02) * rnd(); sb_j[k] = (k < 3 ? 1.0 : 0.02) * rnd(); }
        }
        double r0[15], J0[450] = { 0 }, r1[15], J1[450] = { 0 };
        for (int k = 0; k < 15; ++k) { r0[k] = -7.0; r1[k] = -7.0; }
        imu_raw<true>(m, 9.81, pose_i, sb_i, pose_j, sb_j, r0, J0);
        imu_raw_sel<true>(m, 9.81, pose_i, sb_i, pose_j, sb_j, BE_IMU_SEL_R, r1, J1);
        for (int e = 0; e < 450; ++e) if (J1[e] != 0.0) { std::printf("trial %d: the residual call wrote J[%d]\n", trial, e); return 1; }
        int written = 0;
        for (int b = 0; b < BE_IMU_BLOCKS; ++b) {
            double Jb[450] = { 0 }, rb[15];
            for (int k = 0; k < 15; ++k) rb[k] = -7.0;
            imu_raw_sel<true>(m, 9.81, pose_i, sb_i, pose_j, sb_j, BE_IMU_SEL_BLK(b), rb, Jb);
            for (int k = 0; k < 15; ++k) if (rb[k] != -7.0) { std::printf("trial %d: block %d wrote the residual\n", trial, b); return 1; }
            int r_lo = 15, r_hi = -1, c_lo = 30, c_hi = -1;
            for (int e = 0; e < 450; ++e) {
                uint64_t bits; std::memcpy(&bits, &Jb[e], 8);
                if (!bits) continue;
                const int r = e / 30, c = e % 30;
                r_lo = r < r_lo ? r : r_lo; r_hi = r > r_hi ? r : r_hi; c_lo = c < c_lo ? c : c_lo; c_hi = c > c_hi ? c : c_hi;
                if (J1[e] != 0.0) { std::printf("trial %d: block %d writes J[%d], which an earlier block wrote\n", trial, b, e); return 1; }
                J1[e] = Jb[e]; ++written;
            }
            if (r_hi - r_lo > 2 || c_hi - c_lo > 2) { std::printf("trial %d: block %d is not one 3 x 3 block\n", trial, b); return 1; }
        }
        if (std::memcmp(r0, r1, sizeof(r0)) != 0) { std::printf("trial %d: residual differs\n", trial); return 1; }
        for (int e = 0; e < 450; ++e)
            if (std::memcmp(&J0[e], &J1[e], 8) != 0) { std::printf("trial %d: J[%d][%d] %a against %a\n", trial, e / 30, e % 30, J1[e], J0[e]); return 1; }
        if (!zero && written < 100) { std::printf("trial %d: only %d entries written\n", trial, written); return 1; }
        ++checked;
    }
    std::printf("ok %d\n", checked);
    return 0;
}
