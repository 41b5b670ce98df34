// bow.hip -- bag-of-words place recognition (DESIGN.md "Bag-of-words and loop detection definition"):
//   k_bow_words   the descent of every descriptor of a batch of frames through the k-ary Hamming tree
//   k_bow_vector  per frame: the TF-IDF / L1 BoW vector and the feature vector
//   k_bow_score   the L1 score of one query vector against every vector of the keyframe database
// Every f64 operation is a plain IEEE +, fabs or /, in the order of the definition.
#include <hip/hip_runtime.h>

#include "bow_dev.h"
#include "dispatch.h"

namespace rgbd {

namespace {

__device__ __forceinline__ int bow_frame_n(const BowFrame& f, const int* cnt, int K)
{
    if (f.cnt_idx < 0) return f.n;
    const int n = cnt[f.cnt_idx];
    return n < 0 ? 0 : (n > K ? K : n);
}

__device__ __forceinline__ int popc128(const uint4& a, const uint4& b)
{
    return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

}  // namespace

// One 32-lane group per descriptor, lane c on child c.  A level is one dependent gather of the children's run
// (n_children x 32 B, two 16-byte loads per lane); the query stays in registers.  The minimum is taken over the key
// (distance << 8 | child), so the lowest child wins a tie, as the strict < in child order does.  The host has
// checked that the root is an inner node and that no node lies below level L, so L steps reach a leaf.
__global__ __launch_bounds__(kBowThreads) void k_bow_words(BowVoc v, const uint8_t* __restrict__ desc,
                                                            const BowFrame* __restrict__ frames, const int* __restrict__ cnt,
                                                            int K, int nid_level, int32_t* __restrict__ word,
                                                            double* __restrict__ weight, int32_t* __restrict__ node,
                                                            uint8_t* __restrict__ path)
{
    const BowFrame fr = frames[blockIdx.y];
    const int n = bow_frame_n(fr, cnt, K);
    const int c = threadIdx.x & (kBowGroup - 1);
    const int i = blockIdx.x * (kBowThreads / kBowGroup) + (threadIdx.x / kBowGroup);
    const bool valid = i < n;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (valid) {
        const uint4* q = reinterpret_cast<const uint4*>(desc + ((size_t)fr.in_row + i) * 32);
        q0 = q[0];
        q1 = q[1];
    }
    const size_t orow = (size_t)fr.out_row + i;
    int cur = 0, nid = 0;
    bool done = !valid;
    for (int lvl = 1; lvl <= v.L; lvl++) {
        int fc = 0, nc = 0;
        if (!done) {
            fc = v.first_child[cur];
            nc = v.n_children[cur];
        }
        unsigned key = 0xFFFFFFFFu;
        if (c < nc) {
            const uint4* d = v.desc + 2 * ((size_t)fc + c);
            const uint4 d0 = d[0], d1 = d[1];
            key = ((unsigned)(popc128(q0, d0) + popc128(q1, d1)) << 8) | (unsigned)c;
        }
#pragma unroll
        for (int m = kBowGroup / 2; m >= 1; m >>= 1) {
            const unsigned o = __shfl_xor(key, m, kBowGroup);
            key = o < key ? o : key;
        }
        if (!done) {
            const int ch = (int)(key & 255u);
            cur = fc + ch;
            if (path && c == 0) path[orow * kBowMaxL + (lvl - 1)] = (uint8_t)ch;
            if (lvl == nid_level) nid = v.node_id[cur];
            if (v.n_children[cur] == 0) done = true;
        }
    }
    if (valid && c == 0) {
        word[orow] = v.word_id[cur];
        weight[orow] = v.weight[cur];
        node[orow] = nid;
    }
}

namespace {

// ascending bitonic sort of keys[0, n2), n2 a power of two; the keys of the live entries are distinct
__device__ void bow_sort(unsigned long long* keys, int n2)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n2; i += kBowThreads) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long a = keys[i], b = keys[o];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[o] = a;
                    }
                }
            }
            __syncthreads();
        }
}

constexpr unsigned long long kBowDead = ~0ull;

}  // namespace

// One workgroup per frame.  The (word, feature index) pairs of the features whose word has a weight above zero are
// sorted (distinct keys: the order is the stable one); the thread that finds the head of a word's run adds the run's
// weights one by one in feature order; one thread takes the L1 norm in ascending word order; every entry is divided
// by it.  The feature vector is the same sort over (node, feature index).
__global__ __launch_bounds__(kBowThreads) void k_bow_vector(const BowFrame* __restrict__ frames, const int* __restrict__ cnt, int K,
                                                             const int32_t* __restrict__ word, const double* __restrict__ weight,
                                                             const int32_t* __restrict__ node, uint32_t* __restrict__ bow_ids,
                                                             double* __restrict__ bow_vals, int32_t* __restrict__ n_words,
                                                             int32_t* __restrict__ fv_node, int32_t* __restrict__ fv_idx,
                                                             int32_t* __restrict__ n_fv, int cap2)
{
    extern __shared__ __align__(16) unsigned char bow_smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(bow_smem);
    double* vals = reinterpret_cast<double*>(keys + cap2);
    double* s_norm = vals + cap2;
    int* scan = reinterpret_cast<int*>(s_norm + 1);   // [2][kBowThreads]
    int* s_nv = scan + 2 * kBowThreads;

    const int p = blockIdx.x, tid = threadIdx.x;
    const BowFrame fr = frames[p];
    const int n = bow_frame_n(fr, cnt, K);
    const size_t row = (size_t)fr.out_row;
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    if (n2 > cap2) n2 = cap2;   // the launcher sized cap2 from the largest frame

    if (tid == 0) *s_nv = 0;
    for (int j = tid; j < n2; j += kBowThreads)
        keys[j] = (j < n && weight[row + j] > 0.0) ? (((unsigned long long)(uint32_t)word[row + j] << 12) | (unsigned)j) : kBowDead;
    __syncthreads();
    bow_sort(keys, n2);
    for (int j = tid; j < n2; j += kBowThreads)
        if (keys[j] != kBowDead && (j + 1 == n2 || keys[j + 1] == kBowDead)) *s_nv = j + 1;
    __syncthreads();
    const int nv = *s_nv;

    // heads of the word runs: a chunk of consecutive positions per thread, ranked by a block scan
    const int per = (n2 + kBowThreads - 1) / kBowThreads;
    const int j0 = tid * per, j1 = min(j0 + per, nv);
    int heads = 0;
    for (int j = j0; j < j1; j++) heads += (j == 0 || (keys[j] >> 12) != (keys[j - 1] >> 12)) ? 1 : 0;
    scan[tid] = heads;
    __syncthreads();
    int src = 0;
    for (int d = 1; d < kBowThreads; d <<= 1) {
        const int a = scan[src * kBowThreads + tid] + (tid >= d ? scan[src * kBowThreads + tid - d] : 0);
        scan[(src ^ 1) * kBowThreads + tid] = a;
        src ^= 1;
        __syncthreads();
    }
    const int nw = scan[src * kBowThreads + kBowThreads - 1];
    int at = scan[src * kBowThreads + tid] - heads;
    for (int j = j0; j < j1; j++) {
        const unsigned long long w = keys[j] >> 12;
        if (j != 0 && w == (keys[j - 1] >> 12)) continue;
        double s = 0.0;
        for (int q = j; q < nv && (keys[q] >> 12) == w; q++) s += weight[row + (int)(keys[q] & 4095u)];
        vals[at] = s;
        bow_ids[row + at] = (uint32_t)w;
        at++;
    }
    __syncthreads();
    if (tid == 0) {   // one lane, word order; 64 entries per LDS read and scalar lane reads measured slower
        double norm = 0.0;
        for (int i = 0; i < nw; i++) norm += fabs(vals[i]);
        *s_norm = norm;
        n_words[p] = nw;
        n_fv[p] = nv;
    }
    __syncthreads();
    const double norm = *s_norm;
    for (int i = tid; i < nw; i += kBowThreads) bow_vals[row + i] = norm > 0.0 ? vals[i] / norm : vals[i];

    // feature vector: (node, feature index) ascending over the same features
    __syncthreads();
    for (int j = tid; j < n2; j += kBowThreads)
        keys[j] = (j < n && weight[row + j] > 0.0) ? (((unsigned long long)(uint32_t)node[row + j] << 12) | (unsigned)j) : kBowDead;
    __syncthreads();
    bow_sort(keys, n2);
    for (int j = tid; j < nv; j += kBowThreads) {
        fv_node[row + j] = (int32_t)(keys[j] >> 12);
        fv_idx[row + j] = (int32_t)(keys[j] & 4095u);
    }
}

// One wave per database entry.  A lane takes one word of the entry and looks it up in the query's ids (LDS, binary
// search); the terms of the wave's common words are then added by every lane in lane order, which is ascending word
// order, one add per common word.  query_first: the query is L1Scoring::score's first argument.
__global__ __launch_bounds__(kBowThreads) void k_bow_score(const uint32_t* __restrict__ q_ids, const double* __restrict__ q_vals, int nq,
                                                            const int64_t* __restrict__ db_off, const uint32_t* __restrict__ db_ids,
                                                            const double* __restrict__ db_vals, int E, int query_first,
                                                            double* __restrict__ score, int32_t* __restrict__ n_shared,
                                                            int32_t* __restrict__ min_shared)
{
    extern __shared__ __align__(16) unsigned char bow_smem[];
    uint32_t* s_ids = reinterpret_cast<uint32_t*>(bow_smem);
    for (int i = threadIdx.x; i < nq; i += kBowThreads) s_ids[i] = q_ids[i];
    __syncthreads();
    const int e = blockIdx.x * (kBowThreads / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= E) return;
    const int64_t b0 = db_off[e], b1 = db_off[e + 1];
    double s = 0.0;
    int shared = 0, first = -1;
    for (int64_t base = b0; base < b1; base += 64) {
        const int64_t j = base + lane;
        bool found = false;
        double term = 0.0;
        uint32_t w = 0;
        if (j < b1) {
            w = db_ids[j];
            int lo = 0, hi = nq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_ids[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && s_ids[lo] == w) {
                found = true;
                const double a = q_vals[lo], b = db_vals[j];
                const double vi = query_first ? a : b, wi = query_first ? b : a;
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
        }
        unsigned long long mask = __ballot(found);
        if (mask && first < 0) first = (int)__shfl(w, __ffsll((long long)mask) - 1);
        shared += __popcll(mask);
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            s += __shfl(term, l);
            mask &= mask - 1;
        }
    }
    if (lane == 0) {
        score[e] = -s / 2.0;
        n_shared[e] = shared;
        min_shared[e] = first;
    }
}

hipError_t launch_bow_words(const BowVoc& v, const uint8_t* desc, const BowFrame* frames, const int* cnt, int K, int nid_level,
                            int32_t* word, double* weight, int32_t* node, uint8_t* path, int max_n, int P, hipStream_t st)
{
    if (max_n < 0 || max_n > kBowMaxDesc || v.L < 1 || v.L > kBowMaxL) return hipErrorInvalidValue;
    const int per = kBowThreads / kBowGroup;
    return dispatch(k_bow_words, dim3((max_n + per - 1) / per, P), dim3(kBowThreads), 0, st, v, desc, frames, cnt, K, nid_level, word,
                    weight, node, path);
}

hipError_t launch_bow_vector(const BowFrame* frames, const int* cnt, int K, const int32_t* word, const double* weight,
                             const int32_t* node, uint32_t* bow_ids, double* bow_vals, int32_t* n_words, int32_t* fv_node,
                             int32_t* fv_idx, int32_t* n_fv, int max_n, int P, hipStream_t st)
{
    if (max_n < 0 || max_n > kBowMaxDesc) return hipErrorInvalidValue;
    int cap2 = 2;
    while (cap2 < max_n) cap2 <<= 1;
    const size_t lds = (size_t)cap2 * 16 + 8 + (2 * kBowThreads + 2) * sizeof(int);
    return dispatch(k_bow_vector, dim3(P), dim3(kBowThreads), lds, st, frames, cnt, K, word, weight, node, bow_ids, bow_vals, n_words,
                    fv_node, fv_idx, n_fv, cap2);
}

hipError_t launch_bow_score(const uint32_t* q_ids, const double* q_vals, int nq, const int64_t* db_off, const uint32_t* db_ids,
                            const double* db_vals, int E, int query_first, double* score, int32_t* n_shared,
                            int32_t* min_shared, hipStream_t st)
{
    if (nq < 0 || nq > kBowMaxDesc || E < 0) return hipErrorInvalidValue;
    const int per = kBowThreads / 64;
    return dispatch(k_bow_score, dim3((E + per - 1) / per), dim3(kBowThreads), (size_t)(nq > 0 ? nq : 1) * 4, st, q_ids, q_vals, nq,
                    db_off, db_ids, db_vals, E, query_first, score, n_shared, min_shared);
}

}  // namespace rgbd
