// fast_tile_dev.h -- what the packed-pair FAST kernels share (k_svo_detect in svo.hip, k_adp_score in adaptive.hip):
// the segment tests on the 16-pixel ring of two horizontally adjacent pixels at once (packed u16 lanes) over a pair
// image PI[r][c] = G[r][c] | G[r][c+1] << 16.  Each kernel stages its own tile and builds its own pair image: the
// same loops as a shared inline function compile to other code in k_adp_score, which knows its tile origin to be
// dword-aligned where k_svo_detect reads it from a table (profiles/front_refactor/README.md).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbd {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// the 16 ring pixels (radius 3) around pair-image entry p, row stride S, as pixel pairs
__device__ __forceinline__ void ring16_pairs(const uint32_t* p, int S, u16x2 (&x)[16])
{
    uint32_t raw[16];
    raw[0] = p[3 * S];       raw[1] = p[3 * S + 1];   raw[2] = p[2 * S + 2];   raw[3] = p[1 * S + 3];
    raw[4] = p[3];           raw[5] = p[-1 * S + 3];  raw[6] = p[-2 * S + 2];  raw[7] = p[-3 * S + 1];
    raw[8] = p[-3 * S];      raw[9] = p[-3 * S - 1];  raw[10] = p[-2 * S - 2]; raw[11] = p[-1 * S - 3];
    raw[12] = p[-3];         raw[13] = p[1 * S - 3];  raw[14] = p[2 * S - 2];  raw[15] = p[3 * S - 1];
#pragma unroll
    for (int k = 0; k < 16; k++) x[k] = __builtin_bit_cast(u16x2, raw[k]);
}

// FAST-9's M of two horizontally adjacent pixels at once: the largest, over the 16 nine-pixel arcs of the ring,
// of min(x - v) (brighter) or min(v - x) (darker), clamped at 0 by the saturating subtraction
__device__ __forceinline__ u16x2 fast9_m2(const uint32_t* P, int S, int r, int c)
{
    const uint32_t* p = P + r * S + c;
    u16x2 x[16], mn2[16], mx2[16], mn4[16], mx4[16];
    ring16_pairs(p, S, x);
    const u16x2 v = __builtin_bit_cast(u16x2, p[0]);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mn2[k] = __builtin_elementwise_min(x[k], x[(k + 1) & 15]);
        mx2[k] = __builtin_elementwise_max(x[k], x[(k + 1) & 15]);
    }
#pragma unroll
    for (int k = 0; k < 16; k++) {
        mn4[k] = __builtin_elementwise_min(mn2[k], mn2[(k + 2) & 15]);
        mx4[k] = __builtin_elementwise_max(mx2[k], mx2[(k + 2) & 15]);
    }
    u16x2 MM = {0xffff, 0xffff}, mm = {0, 0};
#pragma unroll
    for (int k = 0; k < 16; k++) {   // arc k .. k+8 = (k .. k+3), (k+4 .. k+7) and k+8
        const u16x2 amin = __builtin_elementwise_min(__builtin_elementwise_min(mn4[k], mn4[(k + 4) & 15]), x[(k + 8) & 15]);
        const u16x2 amax = __builtin_elementwise_max(__builtin_elementwise_max(mx4[k], mx4[(k + 4) & 15]), x[(k + 8) & 15]);
        mm = __builtin_elementwise_max(mm, amin);
        MM = __builtin_elementwise_min(MM, amax);
    }
    return __builtin_elementwise_max(__builtin_elementwise_sub_sat(v, MM), __builtin_elementwise_sub_sat(mm, v));
}

// FAST-10's m of two horizontally adjacent pixels at once: max over the 16 ten-pixel arcs of
// the ring of min(v - x) (darker) or min(x - v) (brighter), clamped to [0, 255] by saturation.  The
// darker side of arc A is v (-) max_A x, the brighter min_A x (-) v, so only the smallest arc maximum MM
// and the largest arc minimum mm are needed.  Arcs k and k+1 (k even) share the core k+1 .. k+9, so the
// pair contributes max(core max, min(x_k, x_k+10)) to MM (and dually to mm).
__device__ __forceinline__ u16x2 fast10_m2(const uint32_t* P, int S, int r, int c)
{
    const uint32_t* p = P + r * S + c;
    u16x2 x[16];
    ring16_pairs(p, S, x);
    const u16x2 v = __builtin_bit_cast(u16x2, p[0]);
    u16x2 mx2[16], mn2[16], mx4[16], mn4[16];
#pragma unroll
    for (int j = 1; j < 16; j += 2) {
        mx2[j] = __builtin_elementwise_max(x[j], x[(j + 1) & 15]);
        mn2[j] = __builtin_elementwise_min(x[j], x[(j + 1) & 15]);
    }
#pragma unroll
    for (int j = 1; j < 16; j += 2) {
        mx4[j] = __builtin_elementwise_max(mx2[j], mx2[(j + 2) & 15]);
        mn4[j] = __builtin_elementwise_min(mn2[j], mn2[(j + 2) & 15]);
    }
    u16x2 MM = {0xffff, 0xffff}, mm = {0, 0};
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        const int j = k + 1;   // core j .. j+8 = max over j..j+7 and x[j+8]
        const u16x2 cmax = __builtin_elementwise_max(__builtin_elementwise_max(mx4[j], mx4[(j + 4) & 15]), x[(j + 8) & 15]);
        const u16x2 cmin = __builtin_elementwise_min(__builtin_elementwise_min(mn4[j], mn4[(j + 4) & 15]), x[(j + 8) & 15]);
        const u16x2 lo = __builtin_elementwise_min(x[k], x[(k + 10) & 15]);
        const u16x2 hi = __builtin_elementwise_max(x[k], x[(k + 10) & 15]);
        MM = __builtin_elementwise_min(MM, __builtin_elementwise_max(cmax, lo));
        mm = __builtin_elementwise_max(mm, __builtin_elementwise_min(cmin, hi));
    }
    return __builtin_elementwise_max(__builtin_elementwise_sub_sat(v, MM), __builtin_elementwise_sub_sat(mm, v));
}

}  // namespace rgbd
