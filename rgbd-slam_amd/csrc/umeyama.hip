// umeyama.hip -- the Umeyama RANSAC, Ransac::compute (Solver/Ransac.cpp:46-181), on gfx950.
// Operator: DESIGN.md "Umeyama RANSAC definition" (tests/umeyama_ransac_model.py is the same text as numpy); the
// rules are umeyama_dev.h's, shared with the host.
//
//   k_umeyama         one 256-thread workgroup per problem, the whole call in one launch.  The gated matches'
//                     point pairs are compacted into LDS in match order.  Then rounds of up to 256 hypotheses (64 in the first):
//                     wave 0 advances the glibc generator and writes each hypothesis's positions and the rand()
//                     count after it; every lane fits its own sample in registers and scores it over all the
//                     matches (every lane reads the same match at the same time: an LDS broadcast); thread 0
//                     walks the round's counts in order through the accept rule and the bound table and finds
//                     whether, and where, the loop ends.  The winner's inliers are recomputed by all threads and
//                     compacted in match order, the re-fit's sequential sums run one accumulator per lane, and
//                     the subset test, the identity test and the outputs follow.
//   k_umeyama_gather  the point pairs of rgbd_ransac_umeyama_frames from the last extraction's xyz, and the gated
//                     count per pair (the host sizes the bound tables by it).
//
// Every early exit and every loop bound is read from LDS after a barrier or computed from uniform values, so no
// wave skips a barrier the others wait at.
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "../../include/rgbd_hip.h"
#include "lane_replay_dev.h"
#include "umeyama_dev.h"

namespace rgbd {

namespace {

struct UmCtl {
    int consumed, ended, best_h, bound, best, n_acc;
};

struct UmLds {
    int cum[kUmThreads];                    // rand() calls of the round up to and including hypothesis h
    int cnt[kUmThreads];                    // inliers of hypothesis h, -1 where the model failed
    unsigned short pos[kUmThreads * kUmMaxPairs];
    int32_t rng0[33];                       // the generator at the round's start
    float Rt[12];                           // the best model, then the re-fit
    float mean[6];
    float sigma[9];
    int wsum[4];
    UmCtl ctl;
};

// rank of this thread's flag among the workgroup's flags in thread order, and their total
__device__ __forceinline__ int um_rank(bool f, int* wsum, int* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kUmThreads / 64; w++) {
        const int c = wsum[w];
        before += w < wv ? c : 0;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

struct LdsPts {
    const float* pts;
    const unsigned short* idx;   // null: the rows themselves
    __device__ __forceinline__ void operator()(int i, float* p) const
    {
        const float* r = pts + 6 * (idx ? (int)idx[i] : i);
#pragma unroll
        for (int k = 0; k < 6; k++) p[k] = r[k];
    }
};

}  // namespace

__global__ __launch_bounds__(kUmThreads) void k_umeyama(const float* __restrict__ pts_g, const UmProb* __restrict__ probs,
                                                        UmPrm prm, const int* __restrict__ tables, int32_t* __restrict__ rngs,
                                                        int32_t* __restrict__ inl, UmRes* __restrict__ res, UmDbg dbg, int cap)
{
    extern __shared__ __align__(16) unsigned char um_dyn[];
    __shared__ UmLds L;
    float* pts = reinterpret_cast<float*>(um_dyn);                                  // [cap][6]: F1 point, F2 point
    unsigned short* orig = reinterpret_cast<unsigned short*>(pts + 6 * (size_t)cap);   // gated row -> match row
    unsigned short* blist = orig + cap;                                             // the best model's inliers
    unsigned short* flist = blist + cap;                                            // the final inliers
    const int tid = threadIdx.x, pb = blockIdx.x;
    const UmProb pr = probs[pb];
    if (!pr.run) return;
    const int M0 = pr.count;
    const int np = prm.used_pairs;

    // ---- gather and gate (:72-83), compacted in match order
    int M = 0;
    for (int base = 0; base < M0; base += kUmThreads) {
        const int i = base + tid;
        float p[6];
        bool keep = false;
        if (i < M0) {
            const float* r = pts_g + 6 * ((size_t)pr.off + i);
#pragma unroll
            for (int k = 0; k < 6; k++) p[k] = r[k];
            keep = !um_gated_out(p[2], p[5]);
        }
        int tot;
        const int at = M + um_rank(keep, L.wsum, &tot);
        if (keep) {
#pragma unroll
            for (int k = 0; k < 6; k++) pts[6 * at + k] = p[k];
            orig[at] = (unsigned short)i;
        }
        M += tot;
    }
    __syncthreads();
    UmRes* out = res + pb;
    if (M < prm.min_matches) {   // uniform (:86-89)
        if (tid < 16) out->T[tid] = (tid % 5 == 0) ? 1.0f : 0.0f;
        if (tid == 0) {
            out->n_inliers = 0;
            out->iterations = 0;
            out->ok = 0;
            out->best_count = 0;
            out->n_accepts = 0;
            out->gated = M;
        }
        return;
    }
    const int* tab = tables + pr.tab_off;
    int32_t* rng = rngs + 33 * (size_t)pb;

    // ---- the loop (:95-157) in rounds
    WaveGlibc g;
    if (tid < 64) g.load(rng);
    if (tid == 0) L.ctl = UmCtl{0, 0, -1, kUmIters0, 0, 0};
    __syncthreads();
    int it0 = 0, bound = kUmIters0, best = 0;
    for (;;) {
        const int maxb = bound > prm.max_bound ? bound : prm.max_bound;
        // the first round is one wave's worth: most pairs' first accepted model drops the bound to a handful
        const int nh = min(it0 == 0 ? 64 : kUmThreads, maxb - it0);   // >= 1: the loop has not ended
        if (tid < 64) {
            g.store(L.rng0);
            int calls = 0;
            for (int h = 0; h < nh; h++) {
                int ids[kUmMaxPairs];
                um_sample(g, M, np, ids, calls);
                if (tid == 0) {
#pragma unroll
                    for (int k = 0; k < kUmMaxPairs; k++)
                        if (k < np) L.pos[h * kUmMaxPairs + k] = (unsigned short)ids[k];
                    L.cum[h] = calls;
                }
            }
        }
        __syncthreads();
        float Rt[12];
        if (tid < nh) {
            const LdsPts get{pts, L.pos + tid * kUmMaxPairs};
            bool sneg = false;
            const bool valid = um_fit(get, np, Rt, &sneg);
            int count = -1;
            if (valid) {
                count = 0;
                for (int i = 0; i < M; i++) {
                    float p[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) p[k] = pts[6 * i + k];
                    count += um_inlier(Rt, p, prm.adaptive, prm.thr) ? 1 : 0;
                }
            }
            L.cnt[tid] = count;
            const int gi = it0 + tid;
            if (dbg.count && gi < dbg.cap) {
                dbg.count[gi] = count;
                dbg.sneg[gi] = sneg ? 1 : 0;
                for (int k = 0; k < np; k++) dbg.pos[(size_t)gi * kUmMaxPairs + k] = L.pos[tid * kUmMaxPairs + k];
            }
        }
        __syncthreads();
        if (tid == 0) {
            UmLoop s;
            s.i = it0;
            s.bound = bound;
            s.best = best;
            s.best_i = -1;
            int n_acc = L.ctl.n_acc;
            int h = 0;
            for (; h < nh; h++) {
                const int before = s.best;
                if (!um_step(s, L.cnt[h], tab)) break;
                if (s.best != before) {
                    if (dbg.accepts && n_acc <= kUmMaxM) {
                        dbg.accepts[3 * n_acc] = s.best_i;
                        dbg.accepts[3 * n_acc + 1] = s.best;
                        dbg.accepts[3 * n_acc + 2] = s.bound;
                    }
                    n_acc++;
                }
            }
            L.ctl = UmCtl{h, s.i >= s.bound ? 1 : 0, s.best_i >= 0 ? s.best_i - it0 : -1, s.bound, s.best, n_acc};
        }
        __syncthreads();
        const UmCtl c = L.ctl;
        if (c.best_h == tid)
#pragma unroll
            for (int k = 0; k < 12; k++) L.Rt[k] = Rt[k];
        it0 += c.consumed;
        bound = c.bound;
        best = c.best;
        if (c.ended) {   // uniform
            if (tid < 64) {   // the generator after the last hypothesis the loop drew
                g.load(L.rng0);
                const int calls = L.cum[c.consumed - 1];
                for (int k = 0; k < calls; k++) (void)g.next();
                g.store(rng);
            }
            break;
        }
        __syncthreads();   // ctl, cnt and rng0 are free for the next round
    }
    __syncthreads();

    // ---- the winner's inliers in match order, the re-fit on them (:159-161), the subset test (:162-165)
    int nb = 0;
    if (best > 0) {
        float Rb[12];
#pragma unroll
        for (int k = 0; k < 12; k++) Rb[k] = L.Rt[k];
        for (int base = 0; base < M; base += kUmThreads) {
            const int i = base + tid;
            bool in = false;
            if (i < M) {
                float p[6];
#pragma unroll
                for (int k = 0; k < 6; k++) p[k] = pts[6 * i + k];
                in = um_inlier(Rb, p, prm.adaptive, prm.thr);
            }
            int tot;
            const int at = nb + um_rank(in, L.wsum, &tot);
            if (in) blist[at] = (unsigned short)i;
            nb += tot;
        }
        __syncthreads();
    }
    float Rf[12];
    um_identity(Rf);
    if (nb > 0) {   // uniform
        const float inv_n = 1.0f / (float)nb;
        if (tid < 6) {
            float a = pts[6 * blist[0] + tid];
            for (int i = 1; i < nb; i++) a = a + pts[6 * blist[i] + tid];
            L.mean[tid] = a * inv_n;
        }
        __syncthreads();
        if (tid < 9) {
            const int a = tid / 3, b = tid % 3;
            const float ma = L.mean[a], mb = L.mean[3 + b];
            float s = 0.0f;
            for (int i = 0; i < nb; i++) {
                const float* r = pts + 6 * blist[i];
                const float v = (r[a] - ma) * (r[3 + b] - mb);
                s = i == 0 ? v : s + v;
            }
            L.sigma[tid] = s * inv_n;
        }
        __syncthreads();
        float sg[3][3], mean[6];
#pragma unroll
        for (int k = 0; k < 9; k++) sg[k / 3][k % 3] = L.sigma[k];
#pragma unroll
        for (int k = 0; k < 6; k++) mean[k] = L.mean[k];
        bool sneg;
        if (!um_model(sg, mean, mean + 3, Rf, &sneg)) um_identity(Rf);   // its failure is ignored (:240-243)
    }
    int nf = 0;
    for (int base = 0; base < nb; base += kUmThreads) {
        const int j = base + tid;
        bool in = false;
        int i = 0;
        if (j < nb) {
            i = blist[j];
            float p[6];
#pragma unroll
            for (int k = 0; k < 6; k++) p[k] = pts[6 * i + k];
            in = um_inlier(Rf, p, prm.adaptive, prm.thr);
        }
        int tot;
        const int at = nf + um_rank(in, L.wsum, &tot);
        if (in) flist[at] = (unsigned short)i;
        nf += tot;
    }
    __syncthreads();
    if (um_below_ratio(best, M, prm.min_ratio)) {   // uniform (:168-171)
        um_identity(Rf);
        nf = 0;
    }
    float T[16];
    um_T16(Rf, T);
    for (int j = tid; j < nf; j += kUmThreads) inl[pr.off + j] = orig[flist[j]];
    if (tid < 16) out->T[tid] = T[tid];
    if (tid == 0) {
        out->n_inliers = nf;
        out->iterations = it0;
        out->ok = um_is_identity(T) ? 0 : 1;
        out->best_count = best;
        out->n_accepts = L.ctl.n_acc;
        out->gated = M;
    }
}

// Row p K + i of pts = the point pair of match i of pair p (F1 = frame qf[p], F2 = frame tf[p]); gated[p] = the
// matches that pass the depth gate; an index outside [0, K) raises *err.
__global__ __launch_bounds__(256) void k_umeyama_gather(const rgbd_dmatch* __restrict__ matches, const int* __restrict__ counts,
                                                        const int* __restrict__ qf, const int* __restrict__ tf,
                                                        const float* __restrict__ xyz, int K, float* __restrict__ pts,
                                                        int* __restrict__ gated, int* __restrict__ err)
{
    __shared__ int s_n;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int q = qf[p];
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (q >= 0) {
        const int t = tf[p], n = counts[p];
        int kept = 0;
        for (int i = tid; i < n; i += 256) {
            const size_t o = (size_t)p * K + i;
            const rgbd_dmatch m = matches[o];
            float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if ((unsigned)m.queryIdx >= (unsigned)K || (unsigned)m.trainIdx >= (unsigned)K) {
                *err = 1;
            } else {
                const float* a = xyz + ((size_t)q * K + m.queryIdx) * 3;
                const float* b = xyz + ((size_t)t * K + m.trainIdx) * 3;
                v[0] = a[0]; v[1] = a[1]; v[2] = a[2];
                v[3] = b[0]; v[4] = b[1]; v[5] = b[2];
            }
#pragma unroll
            for (int k = 0; k < 6; k++) pts[6 * o + k] = v[k];
            kept += um_gated_out(v[2], v[5]) ? 0 : 1;
        }
        if (kept) atomicAdd(&s_n, kept);
    }
    __syncthreads();
    if (tid == 0) gated[p] = s_n;
}

size_t um_lds_bytes(int max_m)
{
    const size_t cap = (size_t)((max_m > 0 ? max_m : 1) + 1) & ~(size_t)1;
    return cap * (6 * sizeof(float) + 3 * sizeof(unsigned short));
}

hipError_t launch_umeyama(const float* pts, const UmProb* probs, const UmPrm& prm, const int* tables, int32_t* rngs,
                          int32_t* inl, UmRes* res, const UmDbg& dbg, int max_m, int P, hipStream_t st)
{
    if (max_m < 0 || max_m > kUmMaxM) return hipErrorInvalidValue;
    const int cap = ((max_m > 0 ? max_m : 1) + 1) & ~1;
    return dispatch(k_umeyama, dim3(P), dim3(kUmThreads), um_lds_bytes(max_m), st, pts, probs, prm, tables, rngs, inl, res,
                    dbg, cap);
}

hipError_t launch_umeyama_gather(const void* matches, const int* counts, const int* qf, const int* tf, const float* xyz,
                                 int K, int P, float* pts, int* gated, int* err, hipStream_t st)
{
    return dispatch(k_umeyama_gather, dim3(P), dim3(256), 0, st, static_cast<const rgbd_dmatch*>(matches), counts, qf, tf,
                    xyz, K, pts, gated, err);
}

}  // namespace rgbd
