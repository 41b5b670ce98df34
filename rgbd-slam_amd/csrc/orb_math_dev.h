// orb_math_dev.h -- the ORB orientation's scalar arithmetic, shared by k_describe (extract.hip) and k_cvorb_describe
// (cvorb.hip): cv::fastAtan2 in degrees and the f32 cos / sin pair of the oracle's definition.  Device code.
#pragma once
#include <hip/hip_runtime.h>

namespace rgbd {

__device__ __forceinline__ float fast_atan2_deg(float y, float x)
{
    const float p1 = 0.9997878412794807f * (float)(180 / M_PI);
    const float p3 = -0.3258083974640975f * (float)(180 / M_PI);
    const float p5 = 0.1555786518463281f * (float)(180 / M_PI);
    const float p7 = -0.04432655554792128f * (float)(180 / M_PI);
    const float ax = fabsf(x), ay = fabsf(y);
    // both branches of the reference as one division of selected operands (no divergent paths when the
    // two keypoints of a wave fall on different sides)
    const bool ge = ax >= ay;
    const float c = (ge ? ay : ax) / ((ge ? ax : ay) + (float)2.220446049250313080847e-16);
    const float c2 = c * c;
    const float t = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    float a = ge ? t : 90.f - t;
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// float cos/sin as the rounding of a double evaluation built from + - * only (same
// operation sequence as the oracle's definition; see DESIGN.md "Oracle definitions").
__device__ __forceinline__ void cos_sin_f(float xf, float* co, float* si)
{
    const double PIO2_1 = 1.57079632673412561417e+00;
    const double PIO2_1T = 6.07710050650619224932e-11;
    const double INV_PIO2 = 6.36619772367581382433e-01;
    const double x = (double)xf;
    const double kd = floor(x * INV_PIO2 + 0.5);
    const int k = (int)kd;
    const double r = (x - kd * PIO2_1) - kd * PIO2_1T;
    const double r2 = r * r;
    double s = -1.0 / 121645100408832000.0;
    s = s * r2 + 1.0 / 355687428096000.0;
    s = s * r2 - 1.0 / 1307674368000.0;
    s = s * r2 + 1.0 / 6227020800.0;
    s = s * r2 - 1.0 / 39916800.0;
    s = s * r2 + 1.0 / 362880.0;
    s = s * r2 - 1.0 / 5040.0;
    s = s * r2 + 1.0 / 120.0;
    s = s * r2 - 1.0 / 6.0;
    s = s * r2 + 1.0;
    const double sr = s * r;
    double c = -1.0 / 6402373705728000.0;
    c = c * r2 + 1.0 / 20922789888000.0;
    c = c * r2 - 1.0 / 87178291200.0;
    c = c * r2 + 1.0 / 479001600.0;
    c = c * r2 - 1.0 / 3628800.0;
    c = c * r2 + 1.0 / 40320.0;
    c = c * r2 - 1.0 / 720.0;
    c = c * r2 + 1.0 / 24.0;
    c = c * r2 - 0.5;
    c = c * r2 + 1.0;
    double cc, ss;
    switch (k & 3) {
    case 0: cc = c; ss = sr; break;
    case 1: cc = -sr; ss = c; break;
    case 2: cc = -c; ss = -sr; break;
    default: cc = sr; ss = -c; break;
    }
    *co = (float)cc;
    *si = (float)ss;
}

}  // namespace rgbd
