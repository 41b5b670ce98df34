// pnp_solver_example.cpp -- pose refinement from a guess: one pair tracked with Matcher::match + RansacSE3
// (System/Tracking.cpp:126-131), re-matched with Matcher::projectionMatch under the estimated pose
// (Features/Matcher.cpp:35-104), then refined by PnPSolver (Solver/PnPSolver.cpp:31-150), written against the
// drop-in surfaces of include/rgbd/frontend.hpp.
// Input: a raw file of two frames (BGR8 640x480 then u16 depth, each), as track_example reads.
// Output (stdout): "ok n_knn_matches n_inliers" of RansacSE3, "guess <16 f32 bit patterns, hex>" (the second
// frame's Tcw before the refinement), "matches <n>" and one line "queryIdx trainIdx imgIdx distance" per
// projection match, "solver <ok>", "pose <16 hex>" (the refined Tcw), "inliers <n>" and one line per inlier in
// the order PnPSolver returns them (ascending trainIdx), then "outliers <matched train indices left flagged>".
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
        std::fprintf(stderr, "usage: %s pair.raw fx fy cx cy k1 k2 p1 p2 k3 factor [th [as_written]]\n", argv[0]);
        return 2;
    }
    rgbd_camera cam{(float)std::atof(argv[2]), (float)std::atof(argv[3]), (float)std::atof(argv[4]),
                    (float)std::atof(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]),
                    (float)std::atof(argv[8]), (float)std::atof(argv[9]), (float)std::atof(argv[10]),
                    1.0f / (float)std::atof(argv[11])};
    const float th = argc > 12 ? (float)std::atof(argv[12]) : 5.0f;
    const bool as_written = argc > 13 && std::atoi(argv[13]) != 0;
    const int W = 640, H = 480;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<uint8_t> bgr((size_t)W * H * 3);
    std::vector<uint16_t> depth((size_t)W * H);
    try {
        rgbd::Extractor extractor(rgbd::Extractor::ORB2, rgbd::Extractor::ORB2, rgbd::Extractor::NORMAL, W, H, cam);
        rgbd::Session session(2024);
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
        rgbd::RansacSE3 sac(extractor.ctx(), session, 200, 10, 3.0f, 4);
        const bool ok = sac.compute(*F[0], *F[1], m);   // sets F[1]'s pose = mT21 * pose(F[0])
        std::printf("%d %d %d\n", ok ? 1 : 0, (int)m.size(), (int)sac.mvInliers.size());
        print_pose("guess", F[1]->getPose());
        std::vector<rgbd_dmatch> pm;
        const int n = matcher.projectionMatch(*F[0], *F[1], pm, th);
        std::printf("matches %d\n", n);
        for (const rgbd_dmatch& d : pm) std::printf("%d %d %d %.9g\n", d.queryIdx, d.trainIdx, d.imgIdx, d.distance);
        rgbd::PnPSolver solver(extractor.ctx(), *F[0], *F[1], pm, as_written);
        std::vector<rgbd_dmatch> inl;
        const bool sok = solver.compute(inl);
        std::printf("solver %d\n", sok ? 1 : 0);
        print_pose("pose", F[1]->getPose());
        std::printf("inliers %d\n", (int)inl.size());
        for (const rgbd_dmatch& d : inl) std::printf("%d %d %d %.9g\n", d.queryIdx, d.trainIdx, d.imgIdx, d.distance);
        int flagged = 0;
        for (const rgbd_dmatch& d : pm) flagged += F[1]->isOutlier((size_t)d.trainIdx) ? 1 : 0;
        std::printf("outliers %d\n", flagged);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    std::fclose(f);
    return 0;
}
