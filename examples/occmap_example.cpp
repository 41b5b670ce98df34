// occmap_example.cpp -- the coloured occupancy map as the reference's map drawer drives it: every keyframe builds its
// filtered cloud (Tracking::createKeyFrame) and MapDrawer::drawOctomap inserts it once; a loop closure ("big change")
// resets the map and inserts every keyframe again.  Written against the drop-in surfaces of include/rgbd/frontend.hpp.
// Input: a raw file of F frames (BGR8 640x480 then u16 depth, each) and a raw file of F poses (Tcw, 16 f32 each).
// Output (stdout): "size <n>" after each keyframe, "rebuilt <n>" after the reset and re-insertion, then one line
// "<kx> <ky> <kz> <log-odds bit pattern, hex> <r> <g> <b>" per leaf in key order, and "render <n>" = the leaves with
// occupancy >= 0.9.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rgbd/frontend.hpp"

int main(int argc, char** argv)
{
    if (argc < 14) {
        std::fprintf(stderr, "usage: %s frames.raw fx fy cx cy k1 k2 p1 p2 k3 factor poses.raw F\n", argv[0]);
        return 2;
    }
    rgbd_camera cam{(float)std::atof(argv[2]), (float)std::atof(argv[3]), (float)std::atof(argv[4]),
                    (float)std::atof(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7]),
                    (float)std::atof(argv[8]), (float)std::atof(argv[9]), (float)std::atof(argv[10]),
                    1.0f / (float)std::atof(argv[11])};
    const int F = std::atoi(argv[13]);
    const int W = 640, H = 480;
    FILE* f = std::fopen(argv[1], "rb");
    FILE* fp = std::fopen(argv[12], "rb");
    if (!f || !fp || F < 1) return 3;
    std::vector<std::vector<uint8_t>> bgr(F, std::vector<uint8_t>((size_t)W * H * 3));
    std::vector<std::vector<uint16_t>> depth(F, std::vector<uint16_t>((size_t)W * H));
    std::vector<rgbd::Pose> poses(F);
    for (int i = 0; i < F; i++) {
        if (std::fread(bgr[i].data(), 1, bgr[i].size(), f) != bgr[i].size()) return 4;
        if (std::fread(depth[i].data(), 2, depth[i].size(), f) != depth[i].size()) return 4;
        if (std::fread(poses[i].data(), 4, 16, fp) != 16) return 4;
    }
    std::fclose(f);
    std::fclose(fp);
    try {
        rgbd::Extractor extractor(rgbd::Extractor::ORB2, rgbd::Extractor::ORB2, rgbd::Extractor::NORMAL, W, H, cam);
        rgbd::OctomapDrawer drawer(extractor.ctx(), 1 << 16);
        std::vector<rgbd::Frame::Ptr> kfs;
        for (int i = 0; i < F; i++) {
            auto kf = std::make_shared<rgbd::Frame>(bgr[i].data(), depth[i].data(), i / 30.0, extractor);
            kf->setPose(poses[i]);
            kf->createFilteredCloud(extractor, bgr[i].data(), depth[i].data());
            kfs.push_back(kf);
            for (auto& k : kfs)   // drawOctomap without a big change: the ids already in the map are passed over
                if (k->isValidCloud()) drawer.insertCloud(*k);
            std::printf("size %zu\n", drawer.size());
        }
        drawer.reset();           // a big change
        for (auto& k : kfs)
            if (k->isValidCloud()) drawer.insertCloud(*k);
        std::printf("rebuilt %zu\n", drawer.size());
        std::vector<uint16_t> keys;
        std::vector<float> lo;
        std::vector<uint8_t> rgb;
        const size_t n = drawer.leaves(keys, lo, rgb);
        for (size_t i = 0; i < n; i++) {
            uint32_t b;
            std::memcpy(&b, &lo[i], 4);
            std::printf("%u %u %u %08x %u %u %u\n", keys[3 * i], keys[3 * i + 1], keys[3 * i + 2], b, rgb[3 * i], rgb[3 * i + 1],
                        rgb[3 * i + 2]);
        }
        std::printf("render %zu\n", drawer.leaves(keys, lo, rgb, 0.9));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
