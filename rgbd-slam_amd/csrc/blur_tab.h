// blur_tab.h -- operand tables of the level blur on the matrix cores (k_fast's blur_tile_walk, extract.hip).
// Host only, no HIP dependency: geometry.cpp builds the tables, tests/blur_tab_check.cpp emulates the products.
//
// The 7x7 level blur (kernel {18,34,49,54,49,34,18}/256 both ways, BORDER_REFLECT_101, ufixedpoint16) of a
// 32 x 32 output tile is two products of v_mfma_i32_32x32x32_i8, each K = 64 (two MFMAs):
//
//   horizontal  D[r][n] = sum_k (p[r][c0 + k] - 128) * Th[k][n]        k = 0..63: the tile column's byte window
//       p - 128 is the pixel byte XOR 0x80 read as i8.  Th's columns sum to 256 (or are all zero: x >= w), so
//       D = H - 32768 with H the horizontal ufixedpoint16 sum, D in [-32768, 32512].
//   split       D = 256 hi + lo + 128,  hi = D >> 8 in [-128, 127],  lo = ((D & 255) XOR 0x80) as i8
//   vertical    S_hi[n][m] = sum_s hi[s][n] * Tv[s][m],  S_lo likewise   s = 0..63: the row block's row window
//       Tv's columns sum to 256 too, so sum_s H[s][n] Tv[s][m] = 256 S_hi + S_lo + 256 (128 + 32768) and
//       out = (sum + 32768) >> 16 = (256 S_hi + S_lo + kBlurC) >> 16 with kBlurC = 0x810000.
//   bounds      |S_hi|, |S_lo| <= 128 * 256 = 32768; 256 S_hi + S_lo + kBlurC in [32768, 16809728]; the exact
//       value sum + 32768 lies in [32768, 65280 * 256 + 32768] < 2^24, so the output is byte 2 of an i32.
//
// Windows.  Tile column t reads the 64 bytes from c0 = clamp(32 t - 4, 0, stride - 64) of each row (row strides
// are multiples of 64 and >= w; bytes at or past w get zero weight).  Row block j sums over the rows
// clamp(32 j - 4 + s, 0, h - 1), s = 0..63 (a duplicated row gets its weight once, in its first slot); its
// output rows past h - 1 are row h - 1 again.
// REFLECT_101 is part of the tables: an edge tile is another constant matrix.
//
// Slots.  An MFMA operand is 16 bytes per lane; byte e of lane half hh = lane / 32 is "slot (hh, e)" and both
// operands of a product give a slot the same k, so the MFMA's own k order never matters.
//   horizontal, MFMA mm: slot (hh, e) = window byte 32 mm + 16 hh + e (a lane's 16 consecutive row bytes)
//   vertical,   MFMA mm: slot (hh, e) = window row  32 mm + 8 (e / 4) + 4 hh + e % 4: accumulator register e of
//       the horizontal product (the 32x32 C/D layout), so its bytes are the vertical A operand as they stand.
// A table is [mm][lane][e]: lane = output column n (Th) or output row m (Tv) of the tile + 32 hh.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define RGBD_BLUR_TAB_HD __host__ __device__
#else
#define RGBD_BLUR_TAB_HD
#endif

namespace rgbd {

constexpr int kBlurTapW[7] = {18, 34, 49, 54, 49, 34, 18};
constexpr int32_t kBlurC = 0x810000;
constexpr int kBlurTabBytes = 2 * 64 * 16;   // one operand table
// per level and direction: table 0 = first tile, 1 = interior, 2 / 3 = the last two tiles
struct BlurLevelTab {
    int8_t th[4][2][64][16];
    int8_t tv[4][2][64][16];
};

inline int blur_tab_tiles(int n) { return (n + 31) / 32; }
RGBD_BLUR_TAB_HD inline int blur_tab_index(int i, int ntiles) { return i == 0 ? 0 : i + 2 >= ntiles ? 2 + (i - (ntiles - 2)) : 1; }
inline int blur_tab_reflect101(int p, int n)
{
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}
inline int blur_tab_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
inline int blur_tab_col0(int t, int stride) { return blur_tab_clamp(32 * t - 4, 0, stride - 64); }
inline int blur_tab_row(int j, int s, int h) { return blur_tab_clamp(32 * j - 4 + s, 0, h - 1); }
// window slot k = 0..63 -> (MFMA, lane half, byte)
inline void blur_tab_hslot(int k, int& mm, int& hh, int& e) { mm = k >> 5; hh = (k >> 4) & 1; e = k & 15; }
inline void blur_tab_vslot(int s, int& mm, int& hh, int& e) { mm = s >> 5; hh = (s >> 2) & 1; e = 4 * ((s & 31) >> 3) + (s & 3); }

// weights of the 32 outputs from o0 on over the 64 window slots whose source index is src[slot] (-1: none).
// Outputs past the level: zero (columns: they land in the row padding) or, repeat_last, the last output's
// weights again (rows: the kernel stores such a row at the last row's address, the same bytes twice, so its
// stores need no condition)
inline bool blur_tab_weights(int o0, int n, const int src[64], int wt[64][32], bool repeat_last)
{
    memset(wt, 0, sizeof(int) * 64 * 32);
    for (int o = 0; o < 32; o++) {
        if (o0 + o >= n && !repeat_last) continue;
        const int x = o0 + o < n ? o0 + o : n - 1;
        for (int j = 0; j < 7; j++) {
            const int q = blur_tab_reflect101(x + j - 3, n);
            int k = 0;
            while (k < 64 && src[k] != q) k++;
            if (k == 64) return false;   // the window misses a tap
            wt[k][o] += kBlurTapW[j];
        }
    }
    for (int k = 0; k < 64; k++)
        for (int o = 0; o < 32; o++)
            if (wt[k][o] > 127) return false;   // (at most 18 + 34 + 49 = 101)
    return true;
}

// one table, or (filled: this index was built before) the check that it is the same one
inline bool blur_tab_put(int8_t tab[2][64][16], bool& filled, const int wt[64][32], bool vertical)
{
    int8_t t[2][64][16];
    for (int k = 0; k < 64; k++) {
        int mm, hh, e;
        if (vertical) blur_tab_vslot(k, mm, hh, e);
        else blur_tab_hslot(k, mm, hh, e);
        for (int o = 0; o < 32; o++) t[mm][32 * hh + o][e] = (int8_t)wt[k][o];
    }
    if (filled) return memcmp(tab, t, sizeof(t)) == 0;
    memcpy(tab, t, sizeof(t));
    filled = true;
    return true;
}

// The tables of a w x h level with the given row stride.  false: the level is not one for the tile path (too
// small, a window that misses a tap, a weight past i8, or tiles sharing a table index that differ).
inline bool blur_tab_build(int w, int h, int stride, BlurLevelTab& T)
{
    memset(&T, 0, sizeof(T));
    if (w < 64 || h < 32 || stride < w || stride % 64 != 0) return false;
    int wt[64][32];
    int src[64];
    bool fh[4] = {false, false, false, false}, fv[4] = {false, false, false, false};
    const int nt = blur_tab_tiles(w), nb = blur_tab_tiles(h);
    for (int t = 0; t < nt; t++) {
        const int c0 = blur_tab_col0(t, stride);
        for (int k = 0; k < 64; k++) src[k] = c0 + k < w ? c0 + k : -1;
        const int ix = blur_tab_index(t, nt);
        if (!blur_tab_weights(32 * t, w, src, wt, false) || !blur_tab_put(T.th[ix], fh[ix], wt, false)) return false;
    }
    for (int j = 0; j < nb; j++) {
        for (int s = 0; s < 64; s++) src[s] = blur_tab_row(j, s, h);   // (clamped duplicates: the first slot is found)
        const int ix = blur_tab_index(j, nb);
        if (!blur_tab_weights(32 * j, h, src, wt, true) || !blur_tab_put(T.tv[ix], fv[ix], wt, true)) return false;
    }
    return true;
}

}  // namespace rgbd
