"""cv::getOptimalNewCameraMatrix(K, D, (w, h), alpha, (w, h), centerPrincipalPoint = false) restated in float64 numpy, independently of the library's C++
(tests/test_undistort_setup.py compares the two).  OpenCV 3.4 calib3d: cvGetOptimalNewCameraMatrix -> icvGetRectangles -> cvUndistortPoints, pinhole + radtan
(k1, k2, p1, p2; k3 = 0), R = P = I.  TEST INFRASTRUCTURE ONLY.

The three readings DESIGN.md 2 (choice U1) declares are parameters, so that the distance between them can be measured:
  spacing       "w"   : grid pixel x w / (N - 1)        (OpenCV 3.4; the declared choice)
                "w-1" : grid pixel x (w - 1) / (N - 1)  (OpenCV >= 4.5)
  iters         fixed-point iterations of cvUndistortPoints (3.4: 5)
  float_points  True: the grid and the undistorted points are rounded to float32, as the library's CV_32FC2 point matrix does; False (declared): double throughout
"""
import numpy as np

N = 9


def undistort_points(cam, px, py, iters=5):
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    x0 = (px - cx) / fx
    y0 = (py - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + (k2 * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return x, y


def rectangles(cam, w, h, spacing="w", iters=5, float_points=False):
    """-> (inner, outer) as (x, y, width, height) on the normalised plane"""
    sw, sh = (w, h) if spacing == "w" else (w - 1, h - 1)
    gx, gy = np.meshgrid(np.arange(N, dtype=np.float64) * sw / (N - 1), np.arange(N, dtype=np.float64) * sh / (N - 1))      # [row y, column x]
    if float_points:
        gx, gy = gx.astype(np.float32).astype(np.float64), gy.astype(np.float32).astype(np.float64)
    ux, uy = undistort_points(cam, gx, gy, iters)
    if float_points:
        ux, uy = ux.astype(np.float32).astype(np.float64), uy.astype(np.float32).astype(np.float64)
    ix0, ix1 = ux[:, 0].max(), ux[:, -1].min()
    iy0, iy1 = uy[0, :].max(), uy[-1, :].min()
    ox0, ox1, oy0, oy1 = ux.min(), ux.max(), uy.min(), uy.max()
    return (ix0, iy0, ix1 - ix0, iy1 - iy0), (ox0, oy0, ox1 - ox0, oy1 - oy0)


def optimal_new_camera(cam, w, h, alpha=0.0, spacing="w", iters=5, float_points=False):
    """-> np.array([fx, fy, cx, cy])"""
    inner, outer = rectangles(cam, w, h, spacing, iters, float_points)
    k = []
    for (rx, ry, rw, rh) in (inner, outer):
        f_x, f_y = (w - 1) / rw, (h - 1) / rh
        k.append(np.array([f_x, f_y, -f_x * rx, -f_y * ry]))
    return k[0] * (1.0 - alpha) + k[1] * alpha


def identity_closed_form(cam, w, h, spacing="w"):
    """newK of a camera WITHOUT distortion: the grid maps linearly, inner == outer.  Spacing "w": the grid spans [0, w] — one pixel more than the viewport [0, w - 1] —
    so K shrinks by (w - 1) / w; spacing "w-1": K itself."""
    fx, fy, cx, cy = cam[:4]
    if spacing == "w":
        return np.array([fx * (w - 1) / w, fy * (h - 1) / h, cx * (w - 1) / w, cy * (h - 1) / h])
    return np.array([fx, fy, cx, cy], np.float64)


def outside_share(map1, map2, w, h):
    """share of destination pixels whose source sample (map1 + map2 / 32) lies outside [0, w - 1] x [0, h - 1]"""
    sx = map1[..., 0].astype(np.float64) + (map2 & 31).astype(np.float64) / 32.0
    sy = map1[..., 1].astype(np.float64) + ((map2 >> 5) & 31).astype(np.float64) / 32.0
    out = (sx < 0) | (sx > w - 1) | (sy < 0) | (sy > h - 1)
    return float(out.mean())
