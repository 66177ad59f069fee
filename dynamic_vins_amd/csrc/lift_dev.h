// lift_dev.h — PinholeCamera::liftProjective (PinholeCamera.cc:450-508) on the device, in ONE copy for every kernel that lifts: the point rows (track.hip),
// the operator entries behind dv_lift_projective / dv_undistort_lines (lift_kernel) and the line tracker's rows (line_track.hip).
#pragma once
#include "dv_internal.h"

__device__ inline void dv_lift_projective_d(const dv_cam& c, double px, double py, double& ox, double& oy) {
    const double ik11 = 1.0 / c.fx, ik13 = -c.cx / c.fx, ik22 = 1.0 / c.fy, ik23 = -c.cy / c.fy;
    const double mx_d = ik11 * px + ik13, my_d = ik22 * py + ik23;
    if (c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0) { ox = mx_d; oy = my_d; return; }   // m_noDistortion
    double mx_u = mx_d, my_u = my_d;
    for (int i = 0; i < 8; ++i) {       // recursive distortion model, n = 8
        double mx2 = mx_u * mx_u, my2 = my_u * my_u, mxy = mx_u * my_u, rho2 = mx2 + my2;
        double rad = c.k1 * rho2 + c.k2 * rho2 * rho2;
        double dx = mx_u * rad + 2.0 * c.p1 * mxy + c.p2 * (rho2 + 2.0 * mx2);
        double dy = my_u * rad + 2.0 * c.p2 * mxy + c.p1 * (rho2 + 2.0 * my2);
        mx_u = mx_d - dx; my_u = my_d - dy;
    }
    ox = mx_u; oy = my_u;
}
