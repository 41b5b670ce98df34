// cvorb_example.cpp -- OpenCV's stock ORB front end as a caller configures it: Extractor(ORB, ORB, NORMAL) shared by
// every Frame of a sequence (cv::ORB::create(nfeatures, scaleFactor, nlevels) as detector, cv::ORB::create() as
// descriptor).  Written against the drop-in surfaces of include/rgbd/frontend.hpp.
// Input: a raw file of F frames (BGR8 640x480 then u16 depth, each).
// Output (stdout): per frame "<index> <keypoints> <FNV-1a 64 of the keypoints' and descriptors' bytes, hex>
// <level 0's FAST corners after the border filter>", then "ORB BRIEF: throws" (mixed pairs are not built) and
// "ORB ADAPTIVE: throws" (neither is the ORB adjuster).
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
        rgbd::Extractor extractor(rgbd::Extractor::ORB, rgbd::Extractor::ORB, rgbd::Extractor::NORMAL, W, H, cam);
        for (int i = 0; i < F; i++) {
            if (std::fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) return 4;
            if (std::fread(depth.data(), 2, depth.size(), f) != depth.size()) return 4;
            rgbd::Frame frame(bgr.data(), depth.data(), i / 30.0, extractor);
            uint64_t h = 0xcbf29ce484222325ull;
            h = fnv1a(h, frame.mvKeys.data(), frame.mvKeys.size() * sizeof(rgbd_keypoint));
            h = fnv1a(h, frame.mDescriptors.data(), frame.mDescriptors.size());
            int32_t nfast = 0;
            if (rgbd_cvorb_debug_level(extractor.ctx(), 0, 0, 0, nullptr, nullptr, 0, &nfast) != RGBD_OK) return 5;
            std::printf("%d %d %016llx %d\n", i, frame.N, (unsigned long long)h, nfast);
        }
        std::fclose(f);
        try {
            rgbd::Extractor other(rgbd::Extractor::ORB, rgbd::Extractor::BRIEF, rgbd::Extractor::NORMAL, W, H, cam);
            std::printf("ORB BRIEF: constructed\n");
        } catch (const rgbd::Error&) {
            std::printf("ORB BRIEF: throws\n");
        }
        try {
            rgbd::Extractor other(rgbd::Extractor::ORB, rgbd::Extractor::ORB, rgbd::Extractor::ADAPTIVE, W, H, cam);
            std::printf("ORB ADAPTIVE: constructed\n");
        } catch (const rgbd::Error&) {
            std::printf("ORB ADAPTIVE: throws\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
