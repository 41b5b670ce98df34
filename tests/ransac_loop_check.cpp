// ransac_loop_check.cpp -- the RANSAC loop rules the host and the kernels share (csrc/pnp_dev.h, csrc/ransac_dev.h),
// run as plain host code and printed, for tests/test_ransac_loop.py to compare with the oracle.  Own main, no
// device, no library: hipcc -ffp-contract=off -fno-fast-math, the product's arithmetic flags.
//   uni             update_num_iters(0.85, (count - g) / count, 5, maxIters): one checksum per count, then clamps
//   unidump COUNT   the same values for one count, one per line (to name a first mismatch)
//   rng             20000 uniform(0, count) values of CvRng(~0) per count
//   subset          2000 get_subset results per count
//   file PATH       cases written by the test: "good" (PnP replay), "rand" + "sample" (sampleMatches), "se3"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pnp_dev.h"
#include "ransac_dev.h"

using namespace rgbd;

static const int kMaxIters[5] = {1, 2, 24, 500, 3000};
static const int kCounts[5] = {5, 6, 61, 400, 4096};

static void uni_values(int count, std::vector<int>& v)
{
    v.clear();
    for (int g = 5; g <= count; g++)
        for (int mi : kMaxIters) v.push_back(update_num_iters(0.85, (double)(count - g) / count, kPnpModel, mi));
}

// sum of (k + 1) * value_k mod 2^64: order-sensitive, the same in numpy uint64
static unsigned long long checksum(const std::vector<int>& v)
{
    unsigned long long s = 0;
    for (size_t k = 0; k < v.size(); k++) s += (unsigned long long)(k + 1) * (unsigned long long)(long long)v[k];
    return s;
}

// the PnP loop over good[0..n) with the hypotheses arriving in spans: span0, 2 span0, 4 span0, ... (0: one span)
static void replay_case(const std::vector<int>& good, int count, int iterations, double conf, int span0)
{
    PnpLoop s{-1, 0, 0, iterations};
    const int n = (int)good.size();
    int evaluated = 0, span = span0 > 0 ? span0 : n;
    while (s.iter < s.niters && evaluated < n) {
        evaluated += span < n - evaluated ? span : n - evaluated;
        span *= 2;
        pnp_replay(s, evaluated, count, conf, [&](int i) { return good[i]; }, [&](int i) { s.best = i; });
    }
    printf("replay span %d: %d %d %d %d\n", span0, s.iter, s.niters, s.maxGood, s.best);
}

struct RawGen {   // Random::randomInt on recorded rand() outputs
    const std::vector<int>* raw;
    size_t pos;
    int random_int(int M) { return pos < raw->size() ? glibc_random_int((*raw)[pos++], M) : (pos++, 0); }
};

static std::vector<int> ints(char* p)
{
    std::vector<int> v;
    for (char* e = p;; p = e) {
        const long x = strtol(p, &e, 10);
        if (e == p) break;
        v.push_back((int)x);
    }
    return v;
}

static int run_file(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) return 2;
    std::vector<char> line(1 << 22);
    std::vector<int> raw;
    while (fgets(line.data(), (int)line.size(), f)) {
        char* p = line.data();
        if (!strncmp(p, "good ", 5)) {   // good COUNT ITERATIONS g0 g1 ...
            std::vector<int> v = ints(p + 5);
            const int count = v[0], iterations = v[1];
            v.erase(v.begin(), v.begin() + 2);
            printf("case good\n");
            for (int span0 : {0, 8}) replay_case(v, count, iterations, 0.85, span0);
        } else if (!strncmp(p, "rand ", 5)) {
            raw = ints(p + 5);
        } else if (!strncmp(p, "sample ", 7)) {   // sample M SS NH
            const std::vector<int> v = ints(p + 7);
            RawGen g{&raw, 0};
            int calls = 0;
            printf("case sample %d %d\n", v[0], v[1]);
            for (int h = 0; h < v[2]; h++) {
                int ids[8];
                const int n = sample_matches(g, v[0], v[1], ids, calls);
                printf("%d %d:", n, calls);
                for (int k = 0; k < n; k++) printf(" %d", ids[k]);
                printf("\n");
            }
            if (g.pos != (size_t)calls || g.pos > raw.size()) return 3;   // two draws per attempt, none past the record
        } else if (!strncmp(p, "se3 ", 4)) {   // se3 M MINTH ITERS H, then H lines "n err"
            const std::vector<int> v = ints(p + 4);
            const int M = v[0], iters = v[2], H = v[3];
            Se3Loop s;
            std::vector<HypOut> ho(H);
            for (int h = 0; h < H; h++) {
                if (!fgets(line.data(), (int)line.size(), f)) return 4;
                char* e = nullptr;
                ho[h].n = (int)strtol(line.data(), &e, 10);
                ho[h].err = strtod(e, nullptr);
            }
            int h = 0;
            for (int n = 0; n < iters; n++) {
                if (h >= H) return 5;
                h++;
                if (!se3_accept(s, h - 1, ho[h - 1], M, (uint32_t)v[1], n)) break;
            }
            printf("case se3\n%d %d %d %zu %a\n", h, s.bestH, s.validIters, s.bestN, (double)s.rmse);
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    std::vector<int> v;
    if (mode == "uni") {
        for (int count = 5; count <= 600; count++) {
            uni_values(count, v);
            printf("uni %d %llu\n", count, checksum(v));
        }
        // the clamps: p <= 0, p >= 1, ep = 0, ep = 1 (and beyond)
        const double ps[] = {-1.0, 0.0, 0.85, 1.0, 2.0}, eps[] = {-0.5, 0.0, 0.3, 1.0, 1.5};
        for (double p : ps)
            for (double ep : eps)
                for (int mi : kMaxIters) printf("clamp %g %g %d %d\n", p, ep, mi, update_num_iters(p, ep, kPnpModel, mi));
    } else if (mode == "unidump" && argc > 2) {
        uni_values(atoi(argv[2]), v);
        for (int x : v) printf("%d\n", x);
    } else if (mode == "rng") {
        for (int count : kCounts) {
            CvRng rng(~0ull);
            printf("rng %d:", count);
            for (int k = 0; k < 20000; k++) printf(" %d", rng.uniform(0, count));
            printf("\n");
        }
    } else if (mode == "subset") {
        for (int count : kCounts) {
            CvRng rng(~0ull);
            printf("subset %d:", count);
            for (int k = 0; k < 2000; k++) {
                int idx[kPnpModel];
                get_subset([&]() { return rng.uniform(0, count); }, idx);
                for (int j = 0; j < kPnpModel; j++) printf(" %d", idx[j]);
            }
            printf("\n");
        }
    } else if (mode == "file" && argc > 2) {
        const int e = run_file(argv[2]);
        if (e) {
            printf("ransac_loop_check: input error %d\n", e);
            return e;
        }
    } else {
        fprintf(stderr, "usage: ransac_loop_check uni | unidump COUNT | rng | subset | file PATH\n");
        return 1;
    }
    return 0;
}
