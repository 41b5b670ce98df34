// ransac_example.cpp -- the plain 3D-3D solver: one pair through the extractor, Matcher::match and Ransac
// (Solver/Ransac.cpp:12-59, Umeyama fits under an adaptive iteration count), written against the drop-in surfaces
// of include/rgbd/frontend.hpp.
// Input: a raw file of two frames (BGR8 640x480 then u16 depth, each), as track_example reads.
// Output (stdout): "matches <n>" and one line "queryIdx trainIdx imgIdx distance" per match, "ransac <ok> <inliers>
// <iterations>", "T <16 f32 bit patterns, hex>" (x1 = T x2), "pose <16 hex>" (the second frame's Tcw), one line per
// inlier, then "outliers <matched train indices left flagged>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rgbd/frontend.hpp"

static void print_pose(const char* tag, const rgbd::Pose& P)
{
    std::printf("%s", tag);
    for (int i = 0; i < 16; i++) {
        uint32_t b;
        std::memcpy(&b, &P[i], 4);
        std::printf(" %08x", b);
    }
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc < 12) {
        std::fprintf(stderr, "usage: %s pair.raw fx fy cx cy k1 k2 p1 p2 k3 factor [seed [error_version [threshold]]]\n", argv[0]);
        return 2;
    }
    rgbd_camera cam{(float)std::atof(argv[2]), (float)std::atof(argv[3]), (float)std::atof(argv[4]),
                    (float)std::atof(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]),
                    (float)std::atof(argv[8]), (float)std::atof(argv[9]), (float)std::atof(argv[10]),
                    1.0f / (float)std::atof(argv[11])};
    const uint32_t seed = argc > 12 ? (uint32_t)std::atoi(argv[12]) : 2024u;
    const int version = argc > 13 ? std::atoi(argv[13]) : (int)rgbd::Ransac::EUCLIDEAN_ERROR;
    const double thr = argc > 14 ? std::atof(argv[14]) : 0.03;
    const int W = 640, H = 480;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<uint8_t> bgr((size_t)W * H * 3);
    std::vector<uint16_t> depth((size_t)W * H);
    try {
        rgbd::Extractor extractor(rgbd::Extractor::ORB2, rgbd::Extractor::ORB2, rgbd::Extractor::NORMAL, W, H, cam);
        rgbd::Session session(seed);
        rgbd::Matcher matcher(extractor.ctx(), 0.9f);
        rgbd::Frame::Ptr F[2];
        for (int i = 0; i < 2; i++) {
            if (std::fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) return 4;
            if (std::fread(depth.data(), 2, depth.size(), f) != depth.size()) return 4;
            F[i] = std::make_shared<rgbd::Frame>(bgr.data(), depth.data(), i / 30.0, extractor);
        }
        F[0]->setPose(rgbd::identity());
        std::vector<rgbd_dmatch> m;
        matcher.match(*F[0], *F[1], m);
        std::printf("matches %d\n", (int)m.size());
        for (const rgbd_dmatch& d : m) std::printf("%d %d %d %.9g\n", d.queryIdx, d.trainIdx, d.imgIdx, d.distance);
        rgbd::Ransac::parameters prm{};
        prm.errorVersion = version;
        prm.inlierThresholdEuclidean = thr;
        prm.minimalInlierRatioThreshold = 0.1;
        prm.minimalNumberOfMatches = 10;
        prm.usedPairs = 3;
        rgbd::Ransac sac(extractor.ctx(), session, *F[0], *F[1], m, prm);
        std::vector<rgbd_dmatch> inl;
        const bool ok = sac.compute(inl);
        std::printf("ransac %d %d %d\n", ok ? 1 : 0, (int)inl.size(), sac.iterations);
        print_pose("T", sac.mT12);
        print_pose("pose", F[1]->getPose());
        for (const rgbd_dmatch& d : inl) std::printf("%d %d %d %.9g\n", d.queryIdx, d.trainIdx, d.imgIdx, d.distance);
        int flagged = 0;
        for (const rgbd_dmatch& d : m) flagged += F[1]->isOutlier((size_t)d.trainIdx) ? 1 : 0;
        std::printf("outliers %d\n", flagged);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    std::fclose(f);
    return 0;
}
