// geometry.h -- the extraction geometry of one context: everything the extraction kernels take on trust, derived
// once on the host (geometry.cpp).  Host only, no HIP dependency: tests/geometry_check.cpp links geometry.cpp alone.
#pragma once
#include <string>
#include <vector>

#include "../../include/rgbd_hip.h"
#include "blur_tab.h"
#include "rgbd_internal.h"

namespace rgbd {

struct Geometry {
    ExtractCfg cfg;
    std::vector<Cell> cells;
    std::vector<FastSeg> segs;            // k_fast segments (per level: gathered leftovers, then full cell-row runs)
    std::vector<ResizeX> rsx;
    std::vector<ResizeY> rsy;
    std::vector<QuadX> qx;
    std::vector<BlurLevelTab> blur_tab;   // the matrix-core blur's operand tables, one set per level it takes
};

// RGBD_OK, or RGBD_ERR_UNSUPPORTED with the reason in err (g is then partly filled)
rgbd_status build_geometry(int W, int H, const rgbd_orb_params& o, const rgbd_camera& k, Geometry& g, std::string& err);

}  // namespace rgbd
