// dist_layout.h -- the LDS layout of k_distribute (extract.hip), one definition for the kernel, its launcher and
// the host geometry (geometry.cpp).  Host only unless compiled by hipcc: no HIP header is needed.
#pragma once
#include <stddef.h>

#include "rgbd_internal.h"

// quadtree round state in LDS: per candidate its u32 key + its state, node index and quadrant in that node
// (a u8 + 2 bits while node_cap <= 256, else a u16), within RGBD_DIST_LDS_KB per workgroup (four 512-thread
// workgroups per CU).  At node_cap 256 (1000 features, 640 x 480: 280 level-0 cells) the node arrays take
// 24,272 B and leave 2,768 keys with their state (14,532 B); a level with more candidates keeps its keys in
// HBM and its state alone in that region (1.25 B each: up to 11.6k candidates), and past that both in HBM.  Round 4
// (level-major dispatch): 32 / 38 / 44 / 52 / 80 KB measured 0.54 / 0.53 / 0.62 / 0.61 / 0.74 ms per 1024
// frames -- occupancy beats residency for this latency-bound kernel
#define RGBD_DIST_LDS_KB 38   // LDS per quadtree workgroup (four 512-thread workgroups per CU)

namespace rgbd {

// LDS of k_distribute's node arrays, before the key region (16-byte aligned for the keys' 128-bit reads):
// sortkey 8NC + childcnt x2 32NC + tmp/tmp2 8SC + size/cid A,B 16NC + best 4NC + dest 8NC + ord 2NC + bbox A,B 16NC
RGBD_HD constexpr size_t dist_node_bytes(int NC, int SC)
{
    return (((size_t)NC * 86 + (size_t)SC * 8) + 15) & ~(size_t)15;
}
// ... and of the key region for kc keys (kc a multiple of 16): the u32 keys + their state
RGBD_HD constexpr size_t dist_key_bytes(int kc, bool u8) { return (size_t)kc * 4 + (size_t)(kc >> 2) * (u8 ? 5 : 8); }

inline size_t distribute_lds_bytes(int NC, int SC)
{
    return dist_node_bytes(NC, SC) + 64;   // the node arrays + the kernel's static LDS
}

// keys per level (a multiple of 16) whose round state fits in room bytes of LDS beside the node arrays
inline int distribute_key_capacity(long room, int NC)
{
    // per group of four keys: 16 bytes of keys + their state (u8 node ids + 2-bit quadrants: 5 bytes; u16: 8);
    // a multiple of 16 keys keeps the quadrant plane whole dwords
    const int per4 = (int)dist_key_bytes(4, NC <= 256);
    return room > 0 ? (int)(room / per4 * 4 / 16 * 16) : 0;
}

}  // namespace rgbd
