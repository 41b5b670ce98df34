// loop_example.cpp -- place recognition as the reference's PoseGraph thread drives it: every keyframe runs
// Frame::computeBoW and LoopDetector::add, and the last one asks LoopDetector::obtainCandidates, written against the
// drop-in surfaces of include/rgbd/frontend.hpp.
// Input: a raw file of F frames (BGR8 640x480 then u16 depth, each), a DBoW3 text vocabulary, and the number of
// keyframes K.  Keyframe i holds frame i % F, is connected to keyframe i - 1 and has frame id 12 i.
// Output (stdout): per keyframe "bow <id> <words> <features>", then for the last keyframe one line "<word id> <f64
// bit pattern, hex>" per word, "candidates <n>" and one line "<frame id> <score bit pattern, hex>" per candidate.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rgbd/frontend.hpp"

int main(int argc, char** argv)
{
    if (argc < 15) {
        std::fprintf(stderr, "usage: %s frames.raw fx fy cx cy k1 k2 p1 p2 k3 factor vocabulary.yml F K\n", argv[0]);
        return 2;
    }
    rgbd_camera cam{(float)std::atof(argv[2]), (float)std::atof(argv[3]), (float)std::atof(argv[4]),
                    (float)std::atof(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]),
                    (float)std::atof(argv[8]), (float)std::atof(argv[9]), (float)std::atof(argv[10]),
                    1.0f / (float)std::atof(argv[11])};
    const int F = std::atoi(argv[13]), K = std::atoi(argv[14]);
    const int W = 640, H = 480;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || F < 1 || K < 1) return 3;
    std::vector<std::vector<uint8_t>> bgr(F, std::vector<uint8_t>((size_t)W * H * 3));
    std::vector<std::vector<uint16_t>> depth(F, std::vector<uint16_t>((size_t)W * H));
    for (int i = 0; i < F; i++) {
        if (std::fread(bgr[i].data(), 1, bgr[i].size(), f) != bgr[i].size()) return 4;
        if (std::fread(depth[i].data(), 2, depth[i].size(), f) != depth[i].size()) return 4;
    }
    std::fclose(f);
    try {
        rgbd::Extractor extractor(rgbd::Extractor::ORB2, rgbd::Extractor::ORB2, rgbd::Extractor::NORMAL, W, H, cam);
        auto voc = rgbd::Vocabulary::load(extractor.ctx(), argv[12]);
        rgbd::LoopDetector looper(voc);
        std::vector<rgbd::Frame::Ptr> kfs;
        for (int i = 0; i < K; i++) {
            rgbd::Frame::nextId() = 12 * i;   // eleven tracked frames between two keyframes
            auto kf = std::make_shared<rgbd::Frame>(bgr[i % F].data(), depth[i % F].data(), i / 30.0, extractor);
            kf->computeBoW(*voc);
            looper.add(kf);
            if (i) {
                kf->addConnection(kfs.back().get());
                kfs.back()->addConnection(kf.get());
            }
            size_t feats = 0;
            for (const auto& kv : kf->mFeatVec) feats += kv.second.size();
            std::printf("bow %d %zu %zu\n", kf->id(), kf->mBowVec.size(), feats);
            kfs.push_back(kf);
        }
        for (const auto& kv : kfs.back()->mBowVec) {
            uint64_t b;
            std::memcpy(&b, &kv.second, 8);
            std::printf("%u %016" PRIx64 "\n", kv.first, b);
        }
        const std::vector<rgbd::Frame::Ptr> cand = looper.obtainCandidates(kfs.back());
        std::printf("candidates %zu\n", cand.size());
        for (const auto& c : cand) {
            uint64_t b;
            std::memcpy(&b, &c->mScore, 8);
            std::printf("%d %016" PRIx64 "\n", c->id(), b);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
