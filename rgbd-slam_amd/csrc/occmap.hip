// occmap.hip -- the coloured occupancy map on gfx950 (OctomapDrawer::insertCloud, Drawer/OctomapDrawer.cpp:38-79 over
// octomap::ColorOcTree; DESIGN.md "Occupancy map definition").  The map is an open-addressing table of depth-16 voxels;
// one scan is three launches on the context's stream, ordered by the kernel boundaries alone:
//   k_occ_mark    one ray per lane: the point to the world frame, computeRayKeys in f64, every cell's slot found or
//                 claimed with a 64-bit compare-and-swap, its stamp raised to 2 * scan_seq + occupied (atomicMax: occupied
//                 beats free, and the lane that first raises it this scan appends the slot to the touched list; the
//                 list counter is bumped once per wave and step)
//   k_occ_apply   one lane per touched slot: the clamped f32 add (or, for a scan that did not fit, the claimed slots
//                 freed again)
//   k_occ_colour  one workgroup: (slot, point index) keys sorted in LDS, one lane per voxel folds its points' colours
//                 in cloud order
// No float atomics and no barrier across workgroups: every voxel's float and colour is written by one lane per scan.
#include <hip/hip_runtime.h>

#include "dispatch.h"

#include <algorithm>
#include <cfloat>
#include <cstdint>

#include "occmap_dev.h"

namespace rgbd {

__device__ __forceinline__ bool occ_key(double rf, float c, int* k)
{
    const double f = floor(rf * (double)c);
    if (!(f >= -(double)kOccTmax && f < (double)kOccTmax)) return false;
    *k = (int)f + kOccTmax;
    return true;
}

__device__ __forceinline__ bool occ_key3(double rf, const float* p, int* k)
{
    const bool a = occ_key(rf, p[0], &k[0]), b = occ_key(rf, p[1], &k[1]), c = occ_key(rf, p[2], &k[2]);
    return a && b && c;
}

__device__ __forceinline__ unsigned long long occ_pack(int kx, int ky, int kz)
{
    return ((unsigned long long)kx << 32) | ((unsigned long long)ky << 16) | (unsigned long long)kz;
}

__device__ __forceinline__ uint32_t occ_hash(unsigned long long k) { return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> 32); }

__device__ __forceinline__ unsigned long long occ_load_key(const unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot of `cell`, claimed when it has none; -1 when every slot holds another key
__device__ int occ_find_or_claim(const OccTable& t, unsigned long long cell, uint32_t seq)
{
    uint32_t s = occ_hash(cell) & t.mask;
    for (uint32_t probes = 0; probes <= t.mask; probes++, s = (s + 1) & t.mask) {
        const unsigned long long k = occ_load_key(&t.key[s]);
        if (k == cell) return (int)s;
        if (k != kOccEmpty) continue;
        const unsigned long long prev = atomicCAS(&t.key[s], kOccEmpty, cell);
        if (prev == kOccEmpty) {   // a new voxel: log-odds 0, white; read only after this launch
            t.val[s] = 0.0f;
            t.rgb[s] = kOccWhite;
            t.born[s] = seq;
            return (int)s;
        }
        if (prev == cell) return (int)s;
    }
    return -1;
}

// the slot of `cell` or -1, nothing claimed (no launch that claims runs beside this one)
__device__ int occ_find(const OccTable& t, unsigned long long cell)
{
    uint32_t s = occ_hash(cell) & t.mask;
    for (uint32_t probes = 0; probes <= t.mask; probes++, s = (s + 1) & t.mask) {
        const unsigned long long k = t.key[s];
        if (k == cell) return (int)s;
        if (k == kOccEmpty) return -1;
    }
    return -1;
}

// computeRayKeys' walk from o to e
struct OccRay {
    int cur[3], end[3], step[3];
    double tmax[3], tdelta[3], length;
};

// false: the ray has no cell (an invalid key, or both ends in one voxel)
__device__ bool occ_ray_begin(const OccCfg& g, const float* o, const float* e, OccRay* r)
{
    const bool vo = occ_key3(g.rf, o, r->cur), ve = occ_key3(g.rf, e, r->end);
    if (!vo || !ve) return false;
    if (r->cur[0] == r->end[0] && r->cur[1] == r->end[1] && r->cur[2] == r->end[2]) return false;
    float d[3] = {e[0] - o[0], e[1] - o[1], e[2] - o[2]};
    const float nsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float length = (float)sqrt((double)nsq);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        d[i] = d[i] / length;
        r->step[i] = (d[i] > 0.0f ? 1 : 0) - (d[i] < 0.0f ? 1 : 0);
        r->tmax[i] = DBL_MAX;
        r->tdelta[i] = DBL_MAX;
        if (r->step[i] != 0) {
            const double border = ((double)(r->cur[i] - kOccTmax) + 0.5) * g.res + (double)(float)(((double)r->step[i] * g.res) * 0.5);
            r->tmax[i] = (border - (double)o[i]) / (double)d[i];
            r->tdelta[i] = g.res / fabs((double)d[i]);
        }
    }
    r->length = (double)length;
    return true;
}

// one step; false: the walk is over, true: r->cur is the next cell of the ray
__device__ bool occ_ray_step(OccRay* r)
{
    int dim;
    if (r->tmax[0] < r->tmax[1]) dim = r->tmax[0] < r->tmax[2] ? 0 : 2;
    else dim = r->tmax[1] < r->tmax[2] ? 1 : 2;
    int c = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)   // no dynamic indexing: the state stays in registers
        if (i == dim) {
            r->cur[i] += r->step[i];
            r->tmax[i] += r->tdelta[i];
            c = r->cur[i];
        }
    if (c < 0 || c >= 2 * kOccTmax) return false;
    if (r->cur[0] == r->end[0] && r->cur[1] == r->end[1] && r->cur[2] == r->end[2]) return false;
    if (fmin(fmin(r->tmax[0], r->tmax[1]), r->tmax[2]) > r->length) return false;
    return true;
}

__global__ __launch_bounds__(kOccMarkThreads) void k_occ_mark(OccTable t, OccCfg g, const rgbd_point* __restrict__ pts, int n,
                                                              const OccPose* __restrict__ pose, double maxrange, uint32_t seq,
                                                              const OccHdr* __restrict__ hdr, OccScan* __restrict__ scan,
                                                              unsigned long long* __restrict__ pkey)
{
    if (hdr->stop) return;
    const int lane = threadIdx.x, i = blockIdx.x * kOccMarkThreads + lane;
    // 0: the ray's first cell, 1: walking, 2: the end cell, 3: done
    int st = 3;
    OccRay ray{};
    bool ray_ok = false, have_end = false, end_occ = false;
    unsigned long long end_key = kOccEmpty;
    if (i < n) {
        const rgbd_point p = pts[i];
        const OccPose P = *pose;
        float w[3];
#pragma unroll
        for (int r = 0; r < 3; r++) w[r] = ((P.T[4 * r] * p.x + P.T[4 * r + 1] * p.y) + P.T[4 * r + 2] * p.z) + P.T[4 * r + 3];
        const bool fin = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]);
        unsigned long long pk = kOccEmpty;   // the voxel the colour phase looks up
        if (fin) {
            int kp[3];
            if (occ_key3(g.rf, w, kp)) pk = occ_pack(kp[0], kp[1], kp[2]);
            const float d[3] = {w[0] - P.o[0], w[1] - P.o[1], w[2] - P.o[2]};
            const float nsq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            const double norm = sqrt((double)nsq);
            if (maxrange < 0.0 || norm <= maxrange) {
                ray_ok = occ_ray_begin(g, P.o, w, &ray);
                have_end = pk != kOccEmpty;
                end_key = pk;
                end_occ = true;
            } else {
                const float fn = (float)norm, fm = (float)maxrange;
                float e[3];
#pragma unroll
                for (int r = 0; r < 3; r++) e[r] = P.o[r] + (d[r] / fn) * fm;
                ray_ok = occ_ray_begin(g, P.o, e, &ray);
                int ke[3];
                have_end = occ_key3(g.rf, e, ke);
                if (have_end) end_key = occ_pack(ke[0], ke[1], ke[2]);
                end_occ = false;
            }
            st = 0;
        }
        pkey[i] = pk;
    }
    for (;;) {
        // every lane that is not done yields one cell per round
        bool emit = false, occ = false;
        unsigned long long cell = kOccEmpty;
        if (st == 0) {
            if (ray_ok) {
                emit = true;
                st = 1;
            } else {
                st = 2;
            }
        } else if (st == 1) {
            emit = occ_ray_step(&ray);
            if (!emit) st = 2;
        }
        if (emit) cell = occ_pack(ray.cur[0], ray.cur[1], ray.cur[2]);
        if (!emit && st == 2) {
            if (have_end) {
                emit = true;
                occ = end_occ;
                cell = end_key;
            }
            st = 3;
        }
        if (!__any(emit)) break;
        int slot = -1;
        bool first = false;
        if (emit) {
            slot = occ_find_or_claim(t, cell, seq);
            if (slot < 0) {   // the table is full: the scan does not fit
                atomicExch(&scan->overflow, 1);
                st = 3;
            } else {
                const uint32_t old = atomicMax(&t.stamp[slot], 2u * seq + (occ ? 1u : 0u));
                first = old < 2u * seq;
            }
        }
        const unsigned long long firsts = __ballot(first);
        if (firsts) {
            const int leader = __ffsll((long long)firsts) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&scan->n_touched, __popcll(firsts));
            base = __shfl(base, leader, 64);
            const uint32_t at = (uint32_t)(base + __popcll(firsts & ((1ull << lane) - 1ull)));
            if (first && at <= t.mask) t.touched[at] = slot;
        }
    }
}

__global__ __launch_bounds__(kOccApplyThreads) void k_occ_apply(OccTable t, OccCfg g, uint32_t seq, OccHdr* __restrict__ hdr,
                                                                const OccScan* __restrict__ scan)
{
    if (hdr->stop) return;
    const int n = min(scan->n_touched, (int)t.mask + 1);   // at most one entry per slot (capacity <= 2^30)
    const bool overflow = scan->overflow != 0;
    int born = 0;
    for (int i = blockIdx.x * kOccApplyThreads + threadIdx.x; i < n; i += gridDim.x * kOccApplyThreads) {
        const int slot = t.touched[i];
        if ((uint32_t)slot > t.mask) continue;
        const bool is_new = t.born[slot] == seq;
        if (overflow) {   // the map as it was: the voxels this scan claimed are free again
            if (is_new) t.key[slot] = kOccEmpty;
            continue;
        }
        float v = t.val[slot] + ((t.stamp[slot] & 1u) ? g.l_hit : g.l_miss);
        if (v < g.l_min) v = g.l_min;
        if (v > g.l_max) v = g.l_max;
        t.val[slot] = v;
        born += is_new ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) born += __shfl_xor(born, o, 64);
    if ((threadIdx.x & 63) == 0 && born) atomicAdd(&hdr->size, born);
}

__global__ __launch_bounds__(kOccColourThreads) void k_occ_colour(OccTable t, const rgbd_point* __restrict__ pts,
                                                                  const unsigned long long* __restrict__ pkey, int n, int sc,
                                                                  OccHdr* __restrict__ hdr, const OccScan* __restrict__ scan)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];   // sc: n rounded up to a power of two
    const int tid = threadIdx.x;
    if (hdr->stop) return;
    if (scan->overflow) {   // the scan did not fit: the colours stay, the rest of the batch is not applied
        if (tid == 0) hdr->stop = 1;
        return;
    }
    for (int i = tid; i < sc; i += kOccColourThreads) {
        unsigned long long k = ~0ull;
        if (i < n && pkey[i] != kOccEmpty) {
            const int slot = occ_find(t, pkey[i]);
            if (slot >= 0) k = ((unsigned long long)slot << 14) | (unsigned long long)i;
        }
        keys[i] = k;
    }
    __syncthreads();
    for (int size = 2; size <= sc; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = tid; x < (sc >> 1); x += kOccColourThreads) {
                const int lo = 2 * x - (x & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == up) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    // one lane per voxel (the first key of a run) folds its points in cloud order
    for (int j = tid; j < n; j += kOccColourThreads) {
        const unsigned long long k = keys[j];
        if (k == ~0ull) continue;
        const unsigned long long slot = k >> 14;
        if (j > 0 && (keys[j - 1] >> 14) == slot) continue;
        uint32_t c = t.rgb[slot];
        for (int e = j; e < n && (keys[e] >> 14) == slot; e++) {
            const rgbd_point p = pts[(int)(keys[e] & 16383ull)];
            const uint32_t pc = (uint32_t)p.r | ((uint32_t)p.g << 8) | ((uint32_t)p.b << 16);
            if (c != kOccWhite) {
                const uint32_t r = ((c & 255u) + p.r) / 2u, gch = (((c >> 8) & 255u) + p.g) / 2u, b = (((c >> 16) & 255u) + p.b) / 2u;
                c = r | (gch << 8) | (b << 16);
            } else {
                c = pc;
            }
        }
        t.rgb[slot] = c;
    }
    if (tid == 0) hdr->applied += 1;
}

hipError_t launch_occ_mark(const OccTable& t, const OccCfg& g, const rgbd_point* pts, int n, const OccPose* pose, double maxrange,
                           uint32_t seq, const OccHdr* hdr, OccScan* scan, unsigned long long* pkey, hipStream_t st)
{
    return dispatch(k_occ_mark, dim3((n + kOccMarkThreads - 1) / kOccMarkThreads), dim3(kOccMarkThreads), 0, st, t, g, pts, n, pose,
                    maxrange, seq, hdr, scan, pkey);
}

hipError_t launch_occ_apply(const OccTable& t, const OccCfg& g, uint32_t seq, OccHdr* hdr, const OccScan* scan, hipStream_t st)
{
    // a grid-stride walk of the touched list, whose length only the device knows
    const uint32_t cap = t.mask + 1u;
    const int blocks = (int)std::min<uint32_t>((cap + kOccApplyThreads - 1) / kOccApplyThreads, 1024u);
    return dispatch(k_occ_apply, dim3(blocks), dim3(kOccApplyThreads), 0, st, t, g, seq, hdr, scan);
}

hipError_t launch_occ_colour(const OccTable& t, const rgbd_point* pts, const unsigned long long* pkey, int n, OccHdr* hdr,
                             const OccScan* scan, hipStream_t st)
{
    int sc = 1;
    while (sc < n) sc <<= 1;
    return dispatch(k_occ_colour, dim3(1), dim3(kOccColourThreads), (size_t)sc * 8, st, t, pts, pkey, n, sc, hdr, scan);
}

}  // namespace rgbd
