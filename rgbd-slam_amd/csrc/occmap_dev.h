// occmap_dev.h -- what occmap.hip and occmap_host.cpp share: the device view of the voxel table, the per-scan control
// words and the launchers (DESIGN.md "Occupancy map definition").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rgbd_hip.h"

namespace rgbd {

constexpr int kOccMaxPoints = 16384;              // points per scan: the 14-bit point index of the colour sort keys
constexpr int kOccTmax = 32768;                   // tree depth 16
constexpr unsigned long long kOccEmpty = ~0ull;   // a free slot; a voxel key is (kx << 32) | (ky << 16) | kz
constexpr uint32_t kOccWhite = 0x00FFFFFFu;       // colour word: r | g << 8 | b << 16
constexpr int kOccMarkThreads = 64;               // one ray per lane, one wave per workgroup
constexpr int kOccApplyThreads = 256;
constexpr int kOccColourThreads = 1024;

// Open addressing with linear probing over cap = mask + 1 slots.  stamp: 2 * scan_seq + occupied of the last scan
// that touched the slot; born: the scan_seq that claimed it (a scan that does not fit frees what it claimed).
struct OccTable {
    unsigned long long* key;
    float* val;
    uint32_t* rgb;
    uint32_t* stamp;
    uint32_t* born;
    int32_t* touched;   // [cap]: the slots of this scan, each once
    uint32_t mask;
};

struct OccCfg {
    double res, rf;
    float l_hit, l_miss, l_min, l_max;
};

struct OccHdr {    // one per map
    int32_t stop;      // a scan of this batch did not fit: every later kernel of the batch returns
    int32_t applied;   // scans applied by this batch
    int32_t size;      // voxels in the map
    int32_t pad;
};
struct OccScan {   // one per scan of a batch, zeroed before the batch
    int32_t n_touched, overflow;
};
struct OccPose {
    float T[12];   // [R' | Ow], row-major 3x4
    float o[3];    // the scan's origin
    float pad;
};

hipError_t launch_occ_mark(const OccTable& t, const OccCfg& g, const rgbd_point* pts, int n, const OccPose* pose, double maxrange,
                           uint32_t seq, const OccHdr* hdr, OccScan* scan, unsigned long long* pkey, hipStream_t st);
hipError_t launch_occ_apply(const OccTable& t, const OccCfg& g, uint32_t seq, OccHdr* hdr, const OccScan* scan, hipStream_t st);
hipError_t launch_occ_colour(const OccTable& t, const rgbd_point* pts, const unsigned long long* pkey, int n, OccHdr* hdr,
                             const OccScan* scan, hipStream_t st);

}  // namespace rgbd
