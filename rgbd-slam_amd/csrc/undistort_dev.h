// undistort_dev.h -- cv::undistortPoints(..., P = K) of one point, shared by k_undistort (every keypoint,
// Core/Frame.cpp:251-281) and k_proj_bounds (the four image corners, Core/Frame.cpp:283-315).
#pragma once
#include <hip/hip_runtime.h>

#include "rgbd_internal.h"

namespace rgbd {

// 5 iterations in double (Core/Frame.cpp:270), the result rounded to float once per coordinate
__device__ __forceinline__ void undistort_point(const ExtractCfg& cfg, float kx, float ky, float* ux, float* uy)
{
    const double fx = cfg.fx, fy = cfg.fy, cx = cfg.cx, cy = cfg.cy;
    const double k0 = cfg.k1, k1 = cfg.k2, k2 = cfg.p1, k3 = cfg.p2, k4 = cfg.k3;
    const double ifx = 1. / fx, ify = 1. / fy;
    double xx = kx, yy = ky;
    xx = (xx - cx) * ifx;
    yy = (yy - cy) * ify;
    const double x0 = xx, y0 = yy;
    for (int j = 0; j < 5; j++) {
        const double r2 = xx * xx + yy * yy;
        const double icdist = 1 / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        const double deltaX = 2 * k2 * xx * yy + k3 * (r2 + 2 * xx * xx);
        const double deltaY = k2 * (r2 + 2 * yy * yy) + 2 * k3 * xx * yy;
        xx = (x0 - deltaX) * icdist;
        yy = (y0 - deltaY) * icdist;
    }
    *ux = (float)(fx * xx + cx);
    *uy = (float)(fy * yy + cy);
}

}  // namespace rgbd
