// bow_dev.h -- what bow.hip and bow_host.cpp share: the device view of the vocabulary tree, the per-frame
// descriptor of a transform, and the launchers (DESIGN.md "Bag-of-words and loop detection definition").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbd {

constexpr int kBowMaxK = 32;        // branching: one lane of a 32-lane group per child
constexpr int kBowMaxL = 10;        // depth: the path of a descriptor is at most 10 children
constexpr int kBowMaxDesc = 4096;   // descriptors per frame: the 12-bit feature index of the sort keys
constexpr int kBowGroup = 32;       // lanes per descriptor in k_bow_words
constexpr int kBowThreads = 256;
constexpr int kBowNoChild = 255;    // path entries below the leaf

// The tree laid out breadth first so that the children of a node are one run: node j's children are
// first_child[j] .. first_child[j] + n_children[j] - 1, in the order of the caller's node ids.
struct BowVoc {
    const uint4* desc;            // [n_nodes][2]: the 32-byte descriptor
    const int32_t* first_child;   // [n_nodes]
    const uint8_t* n_children;    // [n_nodes]; 0 = leaf
    const double* weight;         // [n_nodes]
    const int32_t* word_id;       // [n_nodes]; -1 on inner nodes
    const int32_t* node_id;       // [n_nodes]: the caller's node id
    int32_t L;
};

// One frame of a transform: its descriptors are rows in_row .. in_row + n - 1 of the descriptor array, its outputs
// the slots out_row .. of the output arrays.  cnt_idx >= 0: n = min(cnt[cnt_idx], K) is read on the device.
struct BowFrame {
    int32_t in_row, n, cnt_idx, out_row;
};

hipError_t launch_bow_words(const BowVoc& v, const uint8_t* desc, const BowFrame* frames, const int* cnt, int K, int nid_level,
                            int32_t* word, double* weight, int32_t* node, uint8_t* path, int max_n, int P, hipStream_t st);
hipError_t launch_bow_vector(const BowFrame* frames, const int* cnt, int K, const int32_t* word, const double* weight,
                             const int32_t* node, uint32_t* bow_ids, double* bow_vals, int32_t* n_words, int32_t* fv_node,
                             int32_t* fv_idx, int32_t* n_fv, int max_n, int P, hipStream_t st);
hipError_t launch_bow_score(const uint32_t* q_ids, const double* q_vals, int nq, const int64_t* db_off, const uint32_t* db_ids,
                            const double* db_vals, int E, int query_first, double* score, int32_t* n_shared,
                            int32_t* min_shared, hipStream_t st);

}  // namespace rgbd
