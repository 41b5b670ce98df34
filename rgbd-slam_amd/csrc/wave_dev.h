// wave_dev.h -- wave64 helpers shared by the kernels: the LDS ordering fence among the lanes of one wave and the
// inclusive integer scan on DPP.  (extract.hip keeps a second scan form of its own, tied to fast_rank16; see there.)
#pragma once
#include <hip/hip_runtime.h>

namespace rgbd {

// ordering of LDS traffic among the lanes of one wave: writes before it are visible to the reads after it
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// inclusive wave64 scan on DPP: row_shr 1/2/4/8 inside 16-lane rows, then row_bcast:15 / row_bcast:31
// carry the row totals (out-of-row sources and masked rows contribute 0)
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

}  // namespace rgbd
