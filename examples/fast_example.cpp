// fast_example.cpp -- the reference's stock FAST front end as a caller configures it: Extractor(FAST, BRIEF, NORMAL)
// and Extractor(FAST, ORB, NORMAL), each shared by every Frame of a sequence (cv::FastFeatureDetector::create(),
// retainBest(nfeatures), then BriefDescriptorExtractor or cv::ORB::create()->compute()).  Written against the drop-in surfaces of include/rgbd/frontend.hpp.
// Input: a raw file of F frames (BGR8 640x480 then u16 depth, each).
// Output (stdout): per frame "<index> <BRIEF keypoints> <FNV-1a 64 of their and their descriptors' bytes, hex>
// <ORB keypoints> <their hash> <corners cv::FAST found>", then "FAST FREAK: throws" (a descriptor that is not built).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rgbd/frontend.hpp"

static uint64_t fnv1a(uint64_t h, const void* p, size_t n)
{
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

int main(int argc, char** argv)
{
    if (argc < 13) {
        std::fprintf(stderr, "usage: %s frames.raw F fx fy cx cy k1 k2 p1 p2 k3 factor\n", argv[0]);
        return 2;
    }
    const int F = std::atoi(argv[2]);
    rgbd_camera cam{(float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]),
                    (float)std::atof(argv[6]), (float)std::atof(argv[7]), (float)std::atof(argv[8]),
                    (float)std::atof(argv[9]), (float)std::atof(argv[10]), (float)std::atof(argv[11]),
                    1.0f / (float)std::atof(argv[12])};
    const int W = 640, H = 480;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || F < 1) return 3;
    std::vector<uint8_t> bgr((size_t)W * H * 3);
    std::vector<uint16_t> depth((size_t)W * H);
    try {
        rgbd::Extractor brief(rgbd::Extractor::FAST, rgbd::Extractor::BRIEF, rgbd::Extractor::NORMAL, W, H, cam);
        rgbd::Extractor orb(rgbd::Extractor::FAST, rgbd::Extractor::ORB, rgbd::Extractor::NORMAL, W, H, cam);
        for (int i = 0; i < F; i++) {
            if (std::fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) return 4;
            if (std::fread(depth.data(), 2, depth.size(), f) != depth.size()) return 4;
            std::printf("%d", i);
            for (rgbd::Extractor* ex : {&brief, &orb}) {
                rgbd::Frame frame(bgr.data(), depth.data(), i / 30.0, *ex);
                uint64_t h = 0xcbf29ce484222325ull;
                h = fnv1a(h, frame.mvKeys.data(), frame.mvKeys.size() * sizeof(rgbd_keypoint));
                h = fnv1a(h, frame.mDescriptors.data(), frame.mDescriptors.size());
                std::printf(" %d %016llx", frame.N, (unsigned long long)h);
            }
            int32_t ncand = 0;
            if (rgbd_fast_debug_corners(orb.ctx(), 0, &ncand, nullptr, 0, nullptr) != RGBD_OK) return 5;
            std::printf(" %d\n", ncand);
        }
        std::fclose(f);
        try {
            rgbd::Extractor other(rgbd::Extractor::FAST, rgbd::Extractor::FREAK, rgbd::Extractor::NORMAL, W, H, cam);
            std::printf("FAST FREAK: constructed\n");
        } catch (const rgbd::Error&) {
            std::printf("FAST FREAK: throws\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
