// umeyama_loop_check.cpp -- the Umeyama RANSAC rules the host and the kernel share (csrc/umeyama_dev.h: the sampler,
// the f32 Jacobi SVD and Umeyama, the scoring predicate, the accept rule, the bound table, the fuzzy identity test),
// run as plain host code and printed, for tests/test_umeyama_ransac_model.py to compare with the numpy model bit for
// bit.  Own main, no device, no library: hipcc -ffp-contract=off -fno-fast-math, the product's arithmetic flags.
//   iters R...      um_iters of each argument
//   svd PATH        per line 9 hex f32 words (a 3 x 3 matrix, row-major): prints U (9 words) and V (9 words)
//   solve PATH      one problem: "prm error_version used_pairs min_matches thr min_ratio" (the doubles as hex u64),
//                   "rng" + 33 words, "pts M" + M lines of 6 hex f32 words (the F1 point, the F2 point).  Prints the
//                   whole call's result as the kernel computes it, the loop run one hypothesis at a time.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "umeyama_dev.h"

using namespace rgbd;

static float f_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static double d_of(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }

struct Rows {
    const float* pts;
    const int* idx;
    void operator()(int i, float* p) const { std::memcpy(p, pts + 6 * (idx ? idx[i] : i), 24); }
};

static int solve(const char* path)
{
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    UmPrm prm{};
    int ev = 0, M0 = 0;
    uint64_t thr = 0, mr = 0;
    int32_t rng[33];
    if (std::fscanf(f, " prm %d %d %d %" SCNx64 " %" SCNx64, &ev, &prm.used_pairs, &prm.min_matches, &thr, &mr) != 5) return 2;
    prm.adaptive = ev == 4;
    prm.thr = d_of(thr);
    prm.min_ratio = d_of(mr);
    prm.max_bound = um_iters(prm.min_ratio);
    if (std::fscanf(f, " rng") != 0) return 2;
    for (int i = 0; i < 33; i++)
        if (std::fscanf(f, "%d", &rng[i]) != 1) return 2;
    if (std::fscanf(f, " pts %d", &M0) != 1) return 2;
    std::vector<float> all((size_t)M0 * 6 + 6);
    for (int i = 0; i < M0 * 6; i++) {
        uint32_t u;
        if (std::fscanf(f, "%x", &u) != 1) return 2;
        all[i] = f_of(u);
    }
    std::fclose(f);
    // gate, compacted in match order
    std::vector<float> pts;
    std::vector<int> orig;
    for (int i = 0; i < M0; i++)
        if (!um_gated_out(all[6 * i + 2], all[6 * i + 5])) {
            pts.insert(pts.end(), all.begin() + 6 * i, all.begin() + 6 * i + 6);
            orig.push_back(i);
        }
    const int M = (int)orig.size();
    float Rf[12];
    um_identity(Rf);
    std::vector<int> fin;
    UmLoop s;
    int n_acc = 0;
    if (M >= prm.min_matches) {
        std::vector<int> tab((size_t)M + 1);
        um_bound_table(M, prm.min_ratio, tab.data());
        UmHostGen g{rng};
        float Rb[12];
        for (;;) {
            if (s.i >= s.bound) break;
            int ids[kUmMaxPairs], calls = 0;
            um_sample(g, M, prm.used_pairs, ids, calls);
            float Rt[12];
            bool sneg = false;
            const bool valid = um_fit(Rows{pts.data(), ids}, prm.used_pairs, Rt, &sneg);
            int count = -1;
            if (valid) {
                count = 0;
                for (int i = 0; i < M; i++) count += um_inlier(Rt, &pts[6 * i], prm.adaptive, prm.thr) ? 1 : 0;
            }
            std::printf("hyp %d %d %d", s.i, count, sneg ? 1 : 0);
            for (int k = 0; k < prm.used_pairs; k++) std::printf(" %d", ids[k]);
            std::printf("\n");
            const int before = s.best;
            um_step(s, count, tab.data());
            if (s.best != before) {
                std::memcpy(Rb, Rt, sizeof Rb);
                std::printf("accept %d %d %d\n", s.best_i, s.best, s.bound);
                n_acc++;
            }
        }
        std::vector<int> bl;
        if (s.best > 0)
            for (int i = 0; i < M; i++)
                if (um_inlier(Rb, &pts[6 * i], prm.adaptive, prm.thr)) bl.push_back(i);
        if (!bl.empty()) {
            bool sneg;
            if (!um_fit(Rows{pts.data(), bl.data()}, (int)bl.size(), Rf, &sneg)) um_identity(Rf);
        }
        for (int i : bl)
            if (um_inlier(Rf, &pts[6 * i], prm.adaptive, prm.thr)) fin.push_back(i);
        if (um_below_ratio(s.best, M, prm.min_ratio)) {
            um_identity(Rf);
            fin.clear();
        }
    }
    float T[16];
    um_T16(Rf, T);
    std::printf("T");
    for (int i = 0; i < 16; i++) std::printf(" %08x", u_of(T[i]));
    std::printf("\nresult %d %d %d %d %d\n", um_is_identity(T) ? 0 : 1, s.i, s.best, M, n_acc);
    std::printf("inliers");
    for (int i : fin) std::printf(" %d", orig[i]);
    std::printf("\nrng");
    for (int i = 0; i < 33; i++) std::printf(" %d", rng[i]);
    std::printf("\n");
    return 0;
}

static int svd(const char* path)
{
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    for (;;) {
        float A[3][3], U[3][3], V[3][3];
        uint32_t u;
        int got = 0;
        for (int i = 0; i < 9; i++)
            if (std::fscanf(f, "%x", &u) == 1) {
                A[i / 3][i % 3] = f_of(u);
                got++;
            }
        if (got != 9) break;
        um_svd3(A, U, V);
        for (int i = 0; i < 9; i++) std::printf("%08x ", u_of(U[i / 3][i % 3]));
        for (int i = 0; i < 9; i++) std::printf("%08x ", u_of(V[i / 3][i % 3]));
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "iters")) {
        for (int i = 2; i < argc; i++) std::printf("%d\n", um_iters(std::atof(argv[i])));
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "svd")) return svd(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "solve")) return solve(argv[2]);
    std::fprintf(stderr, "usage: umeyama_loop_check iters R... | svd PATH | solve PATH\n");
    return 1;
}
