// blur_tab_check.cpp -- the level blur's matrix-core operand tables (csrc/blur_tab.h) and the arithmetic of the
// two products, emulated as plain int8 x int8 -> int32 sums over the same slot maps the kernel uses
// (blur_tile_walk, csrc/extract.hip), against a direct integer 7x7 REFLECT_101 blur, (sum + 32768) >> 16.
// Own main, no device, no library.  Sizes: the 640 x 480 pyramid's eight levels, synthetic sizes that sweep
// w mod 32 and h mod 32 over 0..31, and any "W H" pairs given as arguments.  Images per size: random, all 0,
// all 255, a 0/255 checkerboard (the extremes reach the ends of the signed split).  The row padding holds
// random bytes (zero weight) and the emulation reads it as the kernel does.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blur_tab.h"

using namespace rgbd;

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static void direct_blur(const std::vector<uint8_t>& img, int w, int h, int stride, std::vector<uint8_t>& out)
{
    std::vector<int> hs((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int s = 0;
            for (int j = 0; j < 7; j++) s += kBlurTapW[j] * img[(size_t)y * stride + blur_tab_reflect101(x + j - 3, w)];
            hs[(size_t)y * w + x] = s;
        }
    out.assign((size_t)w * h, 0);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int s = 0;
            for (int j = 0; j < 7; j++) s += kBlurTapW[j] * hs[(size_t)blur_tab_reflect101(y + j - 3, h) * w + x];
            out[(size_t)y * w + x] = (uint8_t)((s + 32768) >> 16);
        }
}

// lane fragments of one horizontal block: hi / lo bytes [lane][e], lane = column n + 32 hh, e = accumulator register
struct HBlock { int8_t hi[64][16], lo[64][16]; };

static bool h_block(const std::vector<uint8_t>& img, int h, int stride, int c0, int i, const int8_t th[2][64][16], HBlock& B)
{
    for (int lane = 0; lane < 64; lane++) {
        const int n = lane & 31, hh = lane >> 5;
        for (int e = 0; e < 16; e++) {
            const int r = 8 * (e >> 2) + 4 * hh + (e & 3);   // C/D layout: the block row of register e
            const int row = blur_tab_row(i, r, h);
            int32_t d = 0;
            for (int mm = 0; mm < 2; mm++)        // A lane (row r, half ah), byte ae <-> B lane (column n, half ah), byte ae
                for (int ah = 0; ah < 2; ah++)
                    for (int ae = 0; ae < 16; ae++) {
                        const int8_t a = (int8_t)(img[(size_t)row * stride + c0 + 32 * mm + 16 * ah + ae] ^ 0x80);
                        d += (int32_t)a * (int32_t)th[mm][32 * ah + n][ae];
                    }
            if (d < -32768 || d > 32512) return false;
            B.hi[lane][e] = (int8_t)(d >> 8);
            B.lo[lane][e] = (int8_t)((d & 255) ^ 0x80);
            if (256 * (int32_t)B.hi[lane][e] + (int32_t)B.lo[lane][e] + 128 != d) return false;
        }
    }
    return true;
}

static long emulate(const std::vector<uint8_t>& img, int w, int h, int stride, const BlurLevelTab& T,
                    const std::vector<uint8_t>& ref)
{
    const int nt = blur_tab_tiles(w), nb = blur_tab_tiles(h);
    long bad = 0;
    std::vector<HBlock> H(nb + 1);
    for (int t = 0; t < nt; t++) {
        const int c0 = blur_tab_col0(t, stride);
        if (c0 % 4 != 0 || c0 < 0 || c0 + 64 > stride) return -1;
        for (int i = 0; i <= nb; i++)
            if (!h_block(img, h, stride, c0, i, T.th[blur_tab_index(t, nt)], H[i])) return -2;
        for (int j = 0; j < nb; j++) {
            const int8_t (*tv)[64][16] = T.tv[blur_tab_index(j, nb)];
            for (int lane = 0; lane < 64; lane++) {   // result lane: output row m, registers = columns
                const int m = lane & 31, hh = lane >> 5;
                for (int reg = 0; reg < 16; reg++) {
                    const int n = 8 * (reg >> 2) + 4 * hh + (reg & 3);
                    int32_t shi = 0, slo = 0;
                    for (int mm = 0; mm < 2; mm++)    // A lane (column n, half ah), byte ae <-> B lane (row m, half ah), byte ae
                        for (int ah = 0; ah < 2; ah++)
                            for (int ae = 0; ae < 16; ae++) {
                                const int8_t b = tv[mm][32 * ah + m][ae];
                                shi += (int32_t)H[j + mm].hi[32 * ah + n][ae] * b;
                                slo += (int32_t)H[j + mm].lo[32 * ah + n][ae] * b;
                            }
                    const int64_t x = (int64_t)shi * 256 + slo + kBlurC;
                    // (a row past the level is stored at the last row's address: it must hold that row's bytes)
                    const int y = 32 * j + m < h ? 32 * j + m : h - 1, xx = 32 * t + n;
                    if (xx >= w) continue;
                    if (x < 0 || x >= (1 << 24)) { bad++; continue; }
                    if ((uint8_t)(x >> 16) != ref[(size_t)y * w + xx]) bad++;
                }
            }
        }
    }
    return bad;
}

static int check_size(int w, int h)
{
    const int stride = (w + 63) / 64 * 64;
    BlurLevelTab* T = new BlurLevelTab;
    if (!blur_tab_build(w, h, stride, *T)) {
        printf("FAIL %d x %d: tables not built\n", w, h);
        delete T;
        return 1;
    }
    int fails = 0;
    static const char* names[4] = {"random", "zeros", "ones", "checker"};
    for (int kind = 0; kind < 4; kind++) {
        std::vector<uint8_t> img((size_t)stride * h), ref;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < stride; x++)
                img[(size_t)y * stride + x] = x >= w || kind == 0 ? (uint8_t)rnd()
                                              : kind == 1 ? 0 : kind == 2 ? 255 : ((x + y) & 1 ? 255 : 0);
        direct_blur(img, w, h, stride, ref);
        const long bad = emulate(img, w, h, stride, *T, ref);
        if (bad != 0) {
            printf("FAIL %d x %d %s: %ld\n", w, h, names[kind], bad);
            fails++;
        }
    }
    delete T;
    return fails;
}

int main(int argc, char** argv)
{
    static const int pyr[8][2] = {{640, 480}, {533, 400}, {444, 333}, {370, 278}, {309, 231}, {257, 193}, {214, 161}, {179, 134}};
    int fails = 0, sizes = 0;
    for (auto& s : pyr) { fails += check_size(s[0], s[1]); sizes++; }
    for (int k = 0; k < 32; k++) {   // every residue of w and h mod 32, at one, two, three and more tiles
        fails += check_size(64 + k, 32 + (k * 7 + 3) % 32 + 32 * (k % 3));
        fails += check_size(96 + (k * 5 + 1) % 32 + 32 * (k % 2), 32 + k);
        sizes += 2;
    }
    for (int a = 1; a + 1 < argc; a += 2) { fails += check_size(atoi(argv[a]), atoi(argv[a + 1])); sizes++; }
    // a level below the tile path's floor must be refused
    BlurLevelTab* T = new BlurLevelTab;
    if (blur_tab_build(63, 100, 64, *T) || blur_tab_build(100, 31, 128, *T)) { printf("FAIL small level accepted\n"); fails++; }
    delete T;
    printf("%s sizes %d fails %d\n", fails ? "FAILED" : "OK", sizes, fails);
    return fails ? 1 : 0;
}
