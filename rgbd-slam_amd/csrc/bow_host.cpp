// bow_host.cpp -- C ABI of the bag-of-words place recognition (bow.hip): the vocabulary upload, the transform of one
// frame, a batch of frames and the frames of the last extraction, the L1 score, and the keyframe database.  The hard
// limits are checked before any copy or launch (DESIGN.md "Bag-of-words and loop detection definition").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bow_dev.h"
#include "context.h"

using namespace rgbd;

namespace rgbd {

struct BowWS {
    // the vocabulary, immutable after rgbd_voc_set
    bool has_voc = false;
    int k = 0, L = 0;
    DevBuf<uint4> v_desc;
    DevBuf<int32_t> v_first, v_word, v_node;
    DevBuf<uint8_t> v_nch;
    DevBuf<double> v_weight;
    // a transform
    DevBuf<uint8_t> d_desc, d_path;
    DevBuf<BowFrame> d_frames;
    DevBuf<int32_t> d_word, d_node, d_nw, d_fvn, d_fvi, d_nfv;
    DevBuf<double> d_weight, d_vals;
    DevBuf<uint32_t> d_ids;
    // the keyframe database: CSR, mirrored on the host so that it can grow
    std::vector<int64_t> off{0};
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    DevBuf<int64_t> db_off;
    DevBuf<uint32_t> db_ids;
    DevBuf<double> db_vals;
    size_t up_entries = 0;   // entries already on the device
    // a query
    DevBuf<uint32_t> q_ids;
    DevBuf<double> q_vals, d_score;
    DevBuf<int32_t> d_shared, d_minw;
    // rgbd_bow_score's one-entry database
    DevBuf<int64_t> p_off;
    DevBuf<uint32_t> p_ids;
    DevBuf<double> p_vals;

    BowVoc view() const { return BowVoc{v_desc, v_first, v_nch, v_weight, v_word, v_node, L}; }
};

void bow_free(rgbd_ctx* c)
{
    delete c->bow;
    c->bow = nullptr;
}

}  // namespace rgbd

namespace {

BowWS* ws_get(rgbd_ctx* c)
{
    if (!c->bow) c->bow = new BowWS();
    return c->bow;
}

struct BowOut {
    uint32_t* bow_ids;
    double* bow_vals;
    int32_t* n_words;
    int32_t* fv_node;
    int32_t* fv_idx;
    int32_t* n_fv;
    bool ok() const { return bow_ids && bow_vals && n_words && fv_node && fv_idx && n_fv; }
};
struct BowDebug {
    int32_t* word;
    double* weight;
    int32_t* node;
    uint8_t* path;
};

// The two launches over frames already described: d_desc rows (or the extraction's), rows output slots.
rgbd_status transform_dev(rgbd_ctx* c, BowWS* w, const std::vector<BowFrame>& frames, const uint8_t* d_desc, const int* d_cnt, int K,
                          int levelsup, int max_n, size_t rows, const BowOut* out, const BowDebug* dbg)
{
    const size_t P = frames.size(), R = std::max<size_t>(rows, 1);
    rgbd_status s = check_hip(c, w->d_frames.reserve(P), "bow frames");
    if (!s) s = check_hip(c, w->d_word.reserve(R), "bow words");
    if (!s) s = check_hip(c, w->d_weight.reserve(R), "bow weights");
    if (!s) s = check_hip(c, w->d_node.reserve(R), "bow nodes");
    if (!s && dbg) s = check_hip(c, w->d_path.reserve(R * kBowMaxL), "bow paths");
    if (!s && out) {
        s = check_hip(c, w->d_ids.reserve(R), "bow vector ids");
        if (!s) s = check_hip(c, w->d_vals.reserve(R), "bow vector values");
        if (!s) s = check_hip(c, w->d_fvn.reserve(R), "bow feature nodes");
        if (!s) s = check_hip(c, w->d_fvi.reserve(R), "bow feature indices");
        if (!s) s = check_hip(c, w->d_nw.reserve(P), "bow vector sizes");
        if (!s) s = check_hip(c, w->d_nfv.reserve(P), "bow feature sizes");
    }
    if (s) return s;
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(w->d_frames, frames.data(), P * sizeof(BowFrame), hipMemcpyHostToDevice, st), "bow frames up");
    if (!s && dbg) s = check_hip(c, hipMemsetAsync(w->d_path, kBowNoChild, R * kBowMaxL, st), "bow paths clear");
    if (s) return s;
    const int nid_level = w->L - levelsup;
    int tk = timer_begin(c, "k_bow_words");
    RGBD_TRY(c, launch_bow_words(w->view(), d_desc, w->d_frames, d_cnt, K, nid_level, w->d_word, w->d_weight, w->d_node,
                                 dbg ? w->d_path.get() : nullptr, max_n, (int)P, st), "bow_words");
    timer_end(c, tk);
    if (out) {
        tk = timer_begin(c, "k_bow_vector");
        RGBD_TRY(c, launch_bow_vector(w->d_frames, d_cnt, K, w->d_word, w->d_weight, w->d_node, w->d_ids, w->d_vals, w->d_nw, w->d_fvn,
                                      w->d_fvi, w->d_nfv, max_n, (int)P, st), "bow_vector");
        timer_end(c, tk);
        if (rows) {
            s = check_hip(c, hipMemcpyAsync(out->bow_ids, w->d_ids, rows * 4, hipMemcpyDeviceToHost, st), "bow vector ids");
            if (!s) s = check_hip(c, hipMemcpyAsync(out->bow_vals, w->d_vals, rows * 8, hipMemcpyDeviceToHost, st), "bow vector values");
            if (!s) s = check_hip(c, hipMemcpyAsync(out->fv_node, w->d_fvn, rows * 4, hipMemcpyDeviceToHost, st), "bow feature nodes");
            if (!s) s = check_hip(c, hipMemcpyAsync(out->fv_idx, w->d_fvi, rows * 4, hipMemcpyDeviceToHost, st), "bow feature indices");
        }
        if (!s) s = check_hip(c, hipMemcpyAsync(out->n_words, w->d_nw, P * 4, hipMemcpyDeviceToHost, st), "bow vector sizes");
        if (!s) s = check_hip(c, hipMemcpyAsync(out->n_fv, w->d_nfv, P * 4, hipMemcpyDeviceToHost, st), "bow feature sizes");
    }
    if (!s && dbg && rows) {
        s = check_hip(c, hipMemcpyAsync(dbg->word, w->d_word, rows * 4, hipMemcpyDeviceToHost, st), "bow words");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->weight, w->d_weight, rows * 8, hipMemcpyDeviceToHost, st), "bow weights");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->node, w->d_node, rows * 4, hipMemcpyDeviceToHost, st), "bow nodes");
        if (!s) s = check_hip(c, hipMemcpyAsync(dbg->path, w->d_path, rows * kBowMaxL, hipMemcpyDeviceToHost, st), "bow paths");
    }
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    return s;
}

// the checks every transform shares; nullptr when they pass
const char* transform_limits(rgbd_ctx* c, int levelsup, rgbd_status* code)
{
    *code = RGBD_ERR_ARG;
    if (!c->bow || !c->bow->has_voc) return "bow: no vocabulary (rgbd_voc_set)";
    if (levelsup < 0) return "bow: negative levelsup";
    return nullptr;
}

// host descriptors: counts[p] rows each, concatenated; outputs at the same offsets
rgbd_status transform_host(rgbd_ctx* c, int P, const uint8_t* desc, const int32_t* counts, int levelsup, const BowOut* out,
                           const BowDebug* dbg)
{
    if (!c || P < 0) return RGBD_ERR_ARG;
    rgbd_status code;
    if (const char* why = transform_limits(c, levelsup, &code)) return fail(c, code, why);
    if (P > 0 && !counts) return fail(c, RGBD_ERR_ARG, "bow: null counts");
    if (out && P > 0 && !(out->n_words && out->n_fv)) return fail(c, RGBD_ERR_ARG, "bow: null output");
    size_t rows = 0;
    int max_n = 0;
    std::vector<BowFrame> frames(P);
    for (int p = 0; p < P; p++) {
        if (counts[p] < 0) return fail(c, RGBD_ERR_ARG, "bow: negative descriptor count");
        if (counts[p] > kBowMaxDesc) return fail(c, RGBD_ERR_UNSUPPORTED, "bow: more than 4096 descriptors per frame");
        if (rows + (size_t)counts[p] > 0x7FFFFFFFu) return fail(c, RGBD_ERR_UNSUPPORTED, "bow: batch of more than 2^31 descriptors");
        frames[p] = BowFrame{(int32_t)rows, counts[p], -1, (int32_t)rows};
        rows += (size_t)counts[p];
        max_n = std::max(max_n, counts[p]);
    }
    if (rows > 0 && (!desc || (out && !out->ok()) || (dbg && !(dbg->word && dbg->weight && dbg->node && dbg->path))))
        return fail(c, RGBD_ERR_ARG, "bow: null argument");
    if (P == 0) return RGBD_OK;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    BowWS* w = c->bow;
    if ((s = check_hip(c, w->d_desc.reserve(std::max<size_t>(rows, 1) * 32), "bow descriptors"))) return s;
    if (rows && (s = check_hip(c, hipMemcpyAsync(w->d_desc, desc, rows * 32, hipMemcpyHostToDevice, c->stream), "bow descriptors up")))
        return s;
    return transform_dev(c, w, frames, w->d_desc, nullptr, 0, levelsup, max_n, rows, out, dbg);
}

// one score launch of a query already on the device against a CSR database
rgbd_status score_dev(rgbd_ctx* c, BowWS* w, int nq, const int64_t* d_off, const uint32_t* d_ids, const double* d_vals, int E,
                      int query_first, double* score, int32_t* n_shared, int32_t* min_shared)
{
    rgbd_status s = check_hip(c, w->d_score.reserve((size_t)E), "bow scores");
    if (!s) s = check_hip(c, w->d_shared.reserve((size_t)E), "bow shared counts");
    if (!s) s = check_hip(c, w->d_minw.reserve((size_t)E), "bow shared words");
    if (s) return s;
    const hipStream_t st = c->stream;
    const int tk = timer_begin(c, "k_bow_score");
    RGBD_TRY(c, launch_bow_score(w->q_ids, w->q_vals, nq, d_off, d_ids, d_vals, E, query_first, w->d_score, w->d_shared, w->d_minw, st),
             "bow_score");
    timer_end(c, tk);
    s = check_hip(c, hipMemcpyAsync(score, w->d_score, (size_t)E * 8, hipMemcpyDeviceToHost, st), "bow scores");
    if (!s && n_shared) s = check_hip(c, hipMemcpyAsync(n_shared, w->d_shared, (size_t)E * 4, hipMemcpyDeviceToHost, st), "bow shared counts");
    if (!s && min_shared) s = check_hip(c, hipMemcpyAsync(min_shared, w->d_minw, (size_t)E * 4, hipMemcpyDeviceToHost, st), "bow shared words");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    return s;
}

// a BoW vector as an argument: ids strictly ascending, at most 4096 of them
const char* vector_check(const uint32_t* ids, const double* vals, int n, rgbd_status* code)
{
    *code = RGBD_ERR_ARG;
    if (n < 0) return "bow: negative vector size";
    *code = RGBD_ERR_UNSUPPORTED;
    if (n > kBowMaxDesc) return "bow: a vector of more than 4096 words";
    *code = RGBD_ERR_ARG;
    if (n > 0 && (!ids || !vals)) return "bow: null vector";
    for (int i = 1; i < n; i++)
        if (ids[i] <= ids[i - 1]) return "bow: word ids not strictly ascending";
    return nullptr;
}

rgbd_status query_up(rgbd_ctx* c, BowWS* w, const uint32_t* ids, const double* vals, int n)
{
    rgbd_status s = check_hip(c, w->q_ids.reserve((size_t)std::max(n, 1)), "bow query ids");
    if (!s) s = check_hip(c, w->q_vals.reserve((size_t)std::max(n, 1)), "bow query values");
    if (!s && n) s = check_hip(c, hipMemcpyAsync(w->q_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream), "bow query ids up");
    if (!s && n) s = check_hip(c, hipMemcpyAsync(w->q_vals, vals, (size_t)n * 8, hipMemcpyHostToDevice, c->stream), "bow query values up");
    return s;
}

}  // namespace

extern "C" {

rgbd_status rgbd_voc_set(rgbd_ctx* c, int32_t k, int32_t L, int32_t weighting, int32_t scoring, int32_t desc_bytes, int64_t n_nodes,
                         const int32_t* parent, const uint8_t* descriptor, const double* weight, const uint8_t* is_leaf,
                         const int32_t* word_id)
{
    if (!c) return RGBD_ERR_ARG;
    if (weighting != RGBD_VOC_TF_IDF || scoring != RGBD_VOC_L1_NORM)
        return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: only TF_IDF weighting with L1_NORM scoring");
    if (desc_bytes != 32) return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: 32-byte descriptors only");
    if (k < 2 || k > kBowMaxK) return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: k outside [2, 32]");
    if (L < 1 || L > kBowMaxL) return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: L outside [1, 10]");
    if (n_nodes >= ((int64_t)1 << 31)) return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: 2^31 nodes or more");
    if (n_nodes < 2 || !parent || !descriptor || !weight || !is_leaf || !word_id) return fail(c, RGBD_ERR_ARG, "vocabulary: null or empty tree");
    const int32_t N = (int32_t)n_nodes;
    // children in node-id order
    std::vector<int32_t> nch(N, 0), first(N + 1, 0);
    for (int32_t i = 1; i < N; i++) {
        if (parent[i] < 0 || parent[i] >= N || parent[i] == i) return fail(c, RGBD_ERR_ARG, "vocabulary: a parent outside the tree");
        nch[parent[i]]++;
    }
    int32_t n_leaves = 0;
    for (int32_t i = 0; i < N; i++) {
        if (!std::isfinite(weight[i]) || weight[i] < 0.0) return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: a weight that is not finite and >= 0");
        if (is_leaf[i]) {
            if (nch[i]) return fail(c, RGBD_ERR_ARG, "vocabulary: a leaf with children");
            n_leaves++;
        } else if (nch[i] < 1 || nch[i] > k) {
            return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: an inner node without children or with more than k");
        }
    }
    std::vector<uint8_t> seen(n_leaves, 0);
    for (int32_t i = 0; i < N; i++) {
        if (!is_leaf[i]) continue;
        if (word_id[i] < 0 || word_id[i] >= n_leaves || seen[word_id[i]]) return fail(c, RGBD_ERR_ARG, "vocabulary: word ids are not 0 .. words - 1, once each");
        seen[word_id[i]] = 1;
    }
    for (int32_t i = 0; i < N; i++) first[i + 1] = first[i] + nch[i];
    std::vector<int32_t> kids(N > 1 ? N - 1 : 1), fill(first.begin(), first.end() - 1);
    for (int32_t i = 1; i < N; i++) kids[fill[parent[i]]++] = i;
    // breadth-first renumbering: the children of a node become one run
    std::vector<int32_t> order, level(N, -1), n_first(N, 0);
    order.reserve(N);
    order.push_back(0);
    level[0] = 0;
    for (size_t h = 0; h < order.size(); h++) {
        const int32_t u = order[h];
        n_first[h] = (int32_t)order.size();
        for (int32_t q = first[u]; q < first[u + 1]; q++) {
            const int32_t v = kids[q];
            if (level[v] >= 0) return fail(c, RGBD_ERR_ARG, "vocabulary: a node reached twice");
            level[v] = level[u] + 1;
            if (level[v] > L) return fail(c, RGBD_ERR_UNSUPPORTED, "vocabulary: a node below level L");
            order.push_back(v);
        }
    }
    if ((int32_t)order.size() != N) return fail(c, RGBD_ERR_ARG, "vocabulary: nodes not reachable from node 0");
    std::vector<uint8_t> h_desc((size_t)N * 32), h_nch(N);
    std::vector<double> h_w(N);
    std::vector<int32_t> h_word(N);
    for (int32_t j = 0; j < N; j++) {
        const int32_t u = order[j];
        std::memcpy(&h_desc[(size_t)j * 32], descriptor + (size_t)u * 32, 32);
        h_nch[j] = (uint8_t)nch[u];
        h_w[j] = weight[u];
        h_word[j] = is_leaf[u] ? word_id[u] : -1;
    }
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    BowWS* w = ws_get(c);
    w->has_voc = false;
    s = check_hip(c, w->v_desc.reserve((size_t)N * 2), "vocabulary descriptors");
    if (!s) s = check_hip(c, w->v_first.reserve(N), "vocabulary children");
    if (!s) s = check_hip(c, w->v_nch.reserve(N), "vocabulary children");
    if (!s) s = check_hip(c, w->v_weight.reserve(N), "vocabulary weights");
    if (!s) s = check_hip(c, w->v_word.reserve(N), "vocabulary words");
    if (!s) s = check_hip(c, w->v_node.reserve(N), "vocabulary node ids");
    const hipStream_t st = c->stream;
    if (!s) s = check_hip(c, hipMemcpyAsync(w->v_desc, h_desc.data(), (size_t)N * 32, hipMemcpyHostToDevice, st), "vocabulary up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->v_first, n_first.data(), (size_t)N * 4, hipMemcpyHostToDevice, st), "vocabulary up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->v_nch, h_nch.data(), (size_t)N, hipMemcpyHostToDevice, st), "vocabulary up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->v_weight, h_w.data(), (size_t)N * 8, hipMemcpyHostToDevice, st), "vocabulary up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->v_word, h_word.data(), (size_t)N * 4, hipMemcpyHostToDevice, st), "vocabulary up");
    if (!s) s = check_hip(c, hipMemcpyAsync(w->v_node, order.data(), (size_t)N * 4, hipMemcpyHostToDevice, st), "vocabulary up");
    if (!s) s = check_hip(c, hipStreamSynchronize(st), "sync");
    if (s) return s;
    w->k = k;
    w->L = L;
    w->has_voc = true;
    return RGBD_OK;
}

rgbd_status rgbd_voc_clear(rgbd_ctx* c)
{
    if (!c) return RGBD_ERR_ARG;
    if (c->bow) c->bow->has_voc = false;
    return RGBD_OK;
}

rgbd_status rgbd_bow_transform(rgbd_ctx* c, const uint8_t* desc, int32_t n, int32_t levelsup, uint32_t* bow_ids, double* bow_vals,
                               int32_t* n_words, int32_t* fv_node, int32_t* fv_idx, int32_t* n_fv)
{
    const BowOut out{bow_ids, bow_vals, n_words, fv_node, fv_idx, n_fv};
    return transform_host(c, 1, desc, &n, levelsup, &out, nullptr);
}

rgbd_status rgbd_bow_transform_batch(rgbd_ctx* c, int32_t P, const uint8_t* desc, const int32_t* counts, int32_t levelsup,
                                     uint32_t* bow_ids, double* bow_vals, int32_t* n_words, int32_t* fv_node, int32_t* fv_idx,
                                     int32_t* n_fv)
{
    const BowOut out{bow_ids, bow_vals, n_words, fv_node, fv_idx, n_fv};
    return transform_host(c, P, desc, counts, levelsup, &out, nullptr);
}

rgbd_status rgbd_debug_bow_words(rgbd_ctx* c, const uint8_t* desc, int32_t n, int32_t levelsup, int32_t* word, double* weight,
                                 int32_t* node, uint8_t* path)
{
    const BowDebug dbg{word, weight, node, path};
    return transform_host(c, 1, desc, &n, levelsup, nullptr, &dbg);
}

rgbd_status rgbd_bow_transform_frames(rgbd_ctx* c, int32_t P, const int32_t* frame, int32_t levelsup, uint32_t* bow_ids,
                                      double* bow_vals, int32_t* n_words, int32_t* fv_node, int32_t* fv_idx, int32_t* n_fv)
{
    if (!c || P < 0) return RGBD_ERR_ARG;
    rgbd_status code;
    if (const char* why = transform_limits(c, levelsup, &code)) return fail(c, code, why);
    const BowOut out{bow_ids, bow_vals, n_words, fv_node, fv_idx, n_fv};
    if (P > 0 && (!frame || !out.ok())) return fail(c, RGBD_ERR_ARG, "bow frames: null argument");
    const int B = c->last_B, K = c->cfg.kp_cap;
    if (P > 0 && B < 1) return fail(c, RGBD_ERR_ARG, "bow frames: no extracted batch");
    if (K > kBowMaxDesc) return fail(c, RGBD_ERR_UNSUPPORTED, "bow: more than 4096 descriptors per frame");
    if ((size_t)P * (size_t)K > 0x7FFFFFFFu) return fail(c, RGBD_ERR_UNSUPPORTED, "bow: batch of more than 2^31 descriptors");
    std::vector<BowFrame> frames(P);
    for (int p = 0; p < P; p++) {
        if (frame[p] < 0 || frame[p] >= B) return fail(c, RGBD_ERR_ARG, "bow frames: frame index outside the last batch");
        frames[p] = BowFrame{frame[p] * K, 0, frame[p], p * K};
    }
    if (P == 0) return RGBD_OK;
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    if ((s = order_after_extraction(c))) return s;
    return transform_dev(c, c->bow, frames, c->out.desc, c->out.count, K, levelsup, K, (size_t)P * K, &out, nullptr);
}

rgbd_status rgbd_bow_score(rgbd_ctx* c, const uint32_t* ids_a, const double* val_a, int32_t na, const uint32_t* ids_b,
                           const double* val_b, int32_t nb, double* score)
{
    if (!c || !score) return RGBD_ERR_ARG;
    rgbd_status code;
    if (const char* why = vector_check(ids_a, val_a, na, &code)) return fail(c, code, why);
    if (const char* why = vector_check(ids_b, val_b, nb, &code)) return fail(c, code, why);
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    BowWS* w = ws_get(c);
    if ((s = query_up(c, w, ids_a, val_a, na))) return s;
    s = check_hip(c, w->p_off.reserve(2), "bow pair");
    if (!s) s = check_hip(c, w->p_ids.reserve((size_t)std::max(nb, 1)), "bow pair");
    if (!s) s = check_hip(c, w->p_vals.reserve((size_t)std::max(nb, 1)), "bow pair");
    if (s) return s;
    const int64_t off[2] = {0, nb};
    const hipStream_t st = c->stream;
    s = check_hip(c, hipMemcpyAsync(w->p_off, off, 16, hipMemcpyHostToDevice, st), "bow pair up");
    if (!s && nb) s = check_hip(c, hipMemcpyAsync(w->p_ids, ids_b, (size_t)nb * 4, hipMemcpyHostToDevice, st), "bow pair up");
    if (!s && nb) s = check_hip(c, hipMemcpyAsync(w->p_vals, val_b, (size_t)nb * 8, hipMemcpyHostToDevice, st), "bow pair up");
    if (s) return s;
    return score_dev(c, w, na, w->p_off, w->p_ids, w->p_vals, 1, 1, score, nullptr, nullptr);
}

rgbd_status rgbd_loopdb_add(rgbd_ctx* c, const uint32_t* ids, const double* vals, int32_t n, int32_t* entry)
{
    if (!c) return RGBD_ERR_ARG;
    rgbd_status code;
    if (const char* why = vector_check(ids, vals, n, &code)) return fail(c, code, why);
    BowWS* w = ws_get(c);
    if (w->off.size() - 1 >= 0x7FFFFFFFu) return fail(c, RGBD_ERR_CAPACITY, "loop database: too many entries");
    if (entry) *entry = (int32_t)(w->off.size() - 1);
    w->ids.insert(w->ids.end(), ids, ids + n);
    w->vals.insert(w->vals.end(), vals, vals + n);
    w->off.push_back((int64_t)w->ids.size());
    return RGBD_OK;   // uploaded by the next query
}

rgbd_status rgbd_loopdb_clear(rgbd_ctx* c)
{
    if (!c) return RGBD_ERR_ARG;
    if (BowWS* w = c->bow) {
        w->off.assign(1, 0);
        w->ids.clear();
        w->vals.clear();
        w->up_entries = 0;
    }
    return RGBD_OK;
}

int32_t rgbd_loopdb_size(const rgbd_ctx* c)
{
    return c && c->bow ? (int32_t)(c->bow->off.size() - 1) : 0;
}

rgbd_status rgbd_loopdb_query(rgbd_ctx* c, const uint32_t* ids, const double* vals, int32_t n, int32_t query_first, int32_t cap,
                              double* score, int32_t* n_shared, int32_t* min_shared, int32_t* n_entries)
{
    if (!c || !n_entries || cap < 0) return RGBD_ERR_ARG;
    rgbd_status code;
    if (const char* why = vector_check(ids, vals, n, &code)) return fail(c, code, why);
    BowWS* w = ws_get(c);
    const size_t E = w->off.size() - 1;
    *n_entries = (int32_t)E;
    if (E == 0) return RGBD_OK;
    if ((size_t)cap < E) return fail(c, RGBD_ERR_CAPACITY, "loop database: output capacity below the entry count");
    if (!score || !n_shared || !min_shared) return fail(c, RGBD_ERR_ARG, "loop database: null output");
    rgbd_status s = check_hip(c, hipSetDevice(c->device), "hipSetDevice");
    if (s) return s;
    const hipStream_t st = c->stream;
    // the entries added since the last query; a buffer that has to grow is filled again from the host mirror
    const size_t nnz = w->ids.size();
    size_t from = w->up_entries;
    if (w->db_off.capacity() < E + 1 || w->db_ids.capacity() < nnz || w->db_vals.capacity() < nnz) from = 0;
    s = check_hip(c, w->db_off.reserve(E + 1), "loop database");
    if (!s) s = check_hip(c, w->db_ids.reserve(std::max<size_t>(nnz, 1)), "loop database");
    if (!s) s = check_hip(c, w->db_vals.reserve(std::max<size_t>(nnz, 1)), "loop database");
    if (s) return s;
    w->up_entries = 0;
    const size_t z0 = (size_t)w->off[from];
    s = check_hip(c, hipMemcpyAsync(w->db_off + from, &w->off[from], (E + 1 - from) * 8, hipMemcpyHostToDevice, st), "loop database up");
    if (!s && nnz > z0) s = check_hip(c, hipMemcpyAsync(w->db_ids + z0, &w->ids[z0], (nnz - z0) * 4, hipMemcpyHostToDevice, st), "loop database up");
    if (!s && nnz > z0) s = check_hip(c, hipMemcpyAsync(w->db_vals + z0, &w->vals[z0], (nnz - z0) * 8, hipMemcpyHostToDevice, st), "loop database up");
    if (!s) s = query_up(c, w, ids, vals, n);
    if (s) return s;
    if ((s = score_dev(c, w, n, w->db_off, w->db_ids, w->db_vals, (int)E, query_first ? 1 : 0, score, n_shared, min_shared))) return s;
    w->up_entries = E;
    return RGBD_OK;
}

// LoopDetector::obtainCandidates' rules over the per-entry arrays of a query (host only)
rgbd_status rgbd_loop_candidates(int32_t n, const double* score, const int32_t* n_shared, const int32_t* min_shared,
                                 const int32_t* frame_id, const uint8_t* skip, int32_t query_id, double min_score,
                                 int32_t interval, int32_t* out, int32_t* n_out)
{
    if (n < 0 || !n_out || (n > 0 && (!score || !n_shared || !min_shared || !frame_id || !skip || !out))) return RGBD_ERR_ARG;
    // discovery order: by the smallest shared word, then by insertion
    std::vector<int32_t> disc;
    for (int32_t e = 0; e < n; e++)
        if (n_shared[e] > 0 && !skip[e]) disc.push_back(e);
    std::stable_sort(disc.begin(), disc.end(), [&](int32_t a, int32_t b) { return min_shared[a] < min_shared[b]; });
    std::vector<int32_t> kept;
    for (int32_t e : disc)
        if (score[e] > min_score && std::abs(frame_id[e] - query_id) > interval) kept.push_back(e);
    if (kept.size() > 5) {
        std::sort(kept.begin(), kept.end(), [&](int32_t a, int32_t b) { return score[a] > score[b]; });   // Frame::CompareBoWscore
        kept.resize(5);
    }
    for (size_t i = 0; i < kept.size(); i++) out[i] = kept[i];
    *n_out = (int32_t)kept.size();
    return RGBD_OK;
}

}  // extern "C"
