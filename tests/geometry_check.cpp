// geometry_check.cpp -- the extraction geometry (csrc/geometry.cpp) on the host.  Own main, no device, no library:
// it links geometry.cpp alone.
//
//   geometry_check case W H nfeatures nlevels scale [W H ...]
//       per case: status, table sizes and an FNV-1a digest over the bytes of cfg, cells, segs, rsx, rsy, qx and
//       blur_tab in that order, the refusal's message, then every level's w, h, N and scale bits and umax
//   geometry_check sweep nfeatures strict
//       W in 64..1280 step 16, H in {80, 240, 480, 720}, nlevels in {1, 4, 8, 12}, scale 1.2: every accepted
//       configuration must satisfy what the kernels take on trust (check() below).  strict = 1: the quadtree's
//       LDS rule holds as it stands; 0: a configuration whose node arrays alone pass the budget must have
//       dist_kc == 0 instead (its keys stay in HBM)
//
// The camera is fx = fy = 525, cx = W / 2, cy = H / 2, depth_map_factor = 5000; ORB thresholds 20 / 7.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dist_layout.h"
#include "geometry.h"

using namespace rgbd;

static uint64_t g_hash;
static void fnv(const void* p, size_t n)
{
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; i++) g_hash = (g_hash ^ b[i]) * 1099511628211ull;
}
template <typename T> static void fnv_vec(const std::vector<T>& v) { if (!v.empty()) fnv(v.data(), v.size() * sizeof(T)); }

static rgbd_status build(int W, int H, int nf, int nl, float scale, Geometry& g, std::string& err)
{
    rgbd_camera cam{};
    cam.fx = cam.fy = 525.f;
    cam.cx = (float)(W / 2);
    cam.cy = (float)(H / 2);
    cam.depth_map_factor = 5000.f;
    const rgbd_orb_params orb{nf, scale, nl, 20, 7};
    return build_geometry(W, H, orb, cam, g, err);
}

static int g_fails;
static char g_where[96];
#define EXPECT(cond, ...)                                      \
    do {                                                       \
        if (!(cond)) {                                         \
            if (g_fails++ < 40) {                              \
                printf("FAIL %s: %s: ", g_where, #cond);       \
                printf(__VA_ARGS__);                           \
                printf("\n");                                  \
            }                                                  \
            return;                                            \
        }                                                      \
    } while (0)

static int align_up(int v, int a) { return (v + a - 1) / a * a; }

static void check(const Geometry& g, bool strict)
{
    const ExtractCfg& C = g.cfg;
    const int nl = C.nlevels, ncells = (int)g.cells.size();
    // k_fast segments
    std::vector<int> used(ncells, 0);
    std::vector<int> seen_plain(nl, 0);
    for (size_t si = 0; si < g.segs.size(); si++) {
        const FastSeg& s = g.segs[si];
        EXPECT(s.lpc == 16 || (s.lpc >= 17 && s.lpc <= 32), "seg %zu lpc %d", si, s.lpc);
        const int cpw = 64 / s.lpc;
        EXPECT(s.ncell >= 1 && s.ncell <= cpw, "seg %zu ncell %d lpc %d", si, s.ncell, s.lpc);
        for (int k = 0; k < s.ncell; k++) EXPECT(s.cell[k] >= 0 && s.cell[k] < ncells, "seg %zu cell %d", si, s.cell[k]);
        const Cell& c0 = g.cells[s.cell[0]];
        EXPECT(c0.level >= 0 && c0.level < nl, "seg %zu level %d", si, c0.level);
        const LevelCfg& L = C.lv[c0.level];
        for (int k = 0; k < s.ncell; k++) {
            const Cell& c = g.cells[s.cell[k]];
            EXPECT(s.cell[k] >= L.cell_begin && s.cell[k] < L.cell_begin + L.cell_count && c.level == c0.level,
                   "seg %zu slot %d: cell %d not of level %d", si, k, s.cell[k], c0.level);
            EXPECT(c.y1 - c.y0 == c0.y1 - c0.y0, "seg %zu slot %d ROI height", si, k);
            used[s.cell[k]]++;
        }
        if (s.gathered) {
            EXPECT(!seen_plain[c0.level], "seg %zu: gathered after a plain segment of level %d", si, c0.level);
            for (int k = 0; k < s.ncell; k++) {
                const Cell& c = g.cells[s.cell[k]];
                EXPECT(align_up(c.x1 + 6 - (c.x0 & ~3), 4) <= kFastRowBytes / cpw / 4 * 4, "seg %zu slot %d width", si, k);
            }
        } else {
            seen_plain[c0.level] = 1;
            for (int k = 1; k < s.ncell; k++)
                EXPECT(s.cell[k] == s.cell[0] + k && g.cells[s.cell[k]].y0 == c0.y0, "seg %zu slot %d not a run", si, k);
            const int bytes = g.cells[s.cell[s.ncell - 1]].x1 + 6 - (c0.x0 & ~15);
            EXPECT(bytes <= kFastPlainRowBytes, "seg %zu row bytes %d", si, bytes);
        }
    }
    for (int q = 0; q < ncells; q++) EXPECT(used[q] == 1, "cell %d in %d segments", q, used[q]);
    // k_pyramid strips
    EXPECT(C.pyr_top >= 1 && C.pyr_top <= nl && C.pyr_top <= kPyrStripLevels, "pyr_top %d", C.pyr_top);
    for (int l = 0; l < C.pyr_top; l++) {
        const int h = C.lv[l].h;
        std::vector<int> cov(h, 0);
        for (int s = 0; s < kPyrStrips; s++) {
            const int r0 = C.strip_r0[s][l], r1 = C.strip_r1[s][l];
            EXPECT(0 <= r0 && r0 <= r1 && r1 <= h, "level %d strip %d rows [%d, %d) of %d", l, s, r0, r1, h);
            for (int y = r0; y < r1; y++) cov[y] = 1;
            if (l + 1 < C.pyr_top)
                for (int y = C.strip_r0[s][l + 1]; y < C.strip_r1[s][l + 1]; y++) {
                    const ResizeY& e = g.rsy[C.lv[l + 1].rsy_off + y];
                    EXPECT(e.sy0 >= r0 && e.sy1 < r1 && e.sy0 <= e.sy1,
                           "level %d strip %d: row %d of the next level reads %d..%d outside [%d, %d)", l, s, y, e.sy0, e.sy1, r0, r1);
                }
        }
        for (int y = 0; y < h; y++) EXPECT(cov[y], "level %d row %d in no strip", l, y);
    }
    EXPECT(C.pyr_lds + C.pyr_rsy_lds <= kPyrLdsLimit, "pyramid LDS %d + %d", C.pyr_lds, C.pyr_rsy_lds);
    // QuadX: both taps of every pixel within the 8 bytes from sx0, the shifted window within its 12 bytes
    for (size_t i = 0; i < g.qx.size(); i++) {
        const QuadX& q = g.qx[i];
        for (int k = 0; k < 4; k++) {
            const int o0 = q.sel[k] & 0xff, o1 = (q.sel[k] >> 16) & 0xff;
            EXPECT(o0 <= 7 && o1 <= 7, "quad %zu pixel %d taps at %d, %d", i, k, o0, o1);
        }
        EXPECT((q.wbpi >> 16) <= 3 && (q.wbpi & 3) == 0, "quad %zu window %08x", i, q.wbpi);
    }
    // key and selection regions
    int key = 0, sel = 0, node = 8;
    for (int l = 0; l < nl; l++) {
        const LevelCfg& L = C.lv[l];
        EXPECT(L.key_off == key && L.key_cap % 4 == 0 && L.key_cap >= L.cell_count * C.cell_cap,
               "level %d keys at %d (+%d), expected at %d", l, L.key_off, L.key_cap, key);
        key += L.key_cap;
        EXPECT(L.sel_off == sel && C.sel_off_tab[l] == sel, "level %d selection at %d, expected at %d", l, L.sel_off, sel);
        sel += align_up(L.N + 3 > 4 * L.nIni ? L.N + 3 : 4 * L.nIni, 4);
        const int need = L.N + 8 > 4 * L.nIni + 8 ? L.N + 8 : 4 * L.nIni + 8;
        if (need > node) node = need;
    }
    EXPECT(key == C.keys_per_frame && sel == C.sel_per_frame, "totals %d / %d keys, %d / %d selected", key, C.keys_per_frame, sel,
           C.sel_per_frame);
    for (int l = nl; l < kMaxLevels; l++) EXPECT(C.sel_off_tab[l] == INT32_MAX, "sel_off_tab[%d]", l);
    // quadtree capacities
    EXPECT(C.node_cap > 0 && (C.node_cap & (C.node_cap - 1)) == 0 && C.node_cap >= node, "node_cap %d for %d", C.node_cap, node);
    EXPECT(C.dist_kc >= 0 && C.dist_kc % 16 == 0, "dist_kc %d", C.dist_kc);
    const size_t budget = (size_t)RGBD_DIST_LDS_KB * 1024, nodes = dist_node_bytes(C.node_cap, C.scan_cap) + 64;
    if (strict || nodes <= budget)
        EXPECT(nodes + dist_key_bytes(C.dist_kc, C.node_cap <= 256) <= budget, "quadtree LDS %zu + %zu (node_cap %d, dist_kc %d)",
               nodes, dist_key_bytes(C.dist_kc, C.node_cap <= 256), C.node_cap, C.dist_kc);
    else
        EXPECT(C.dist_kc == 0, "dist_kc %d with node arrays of %zu B", C.dist_kc, nodes);
    // blur partition
    for (int l = 0; l < kMaxLevels; l++) {
        const int t = C.blur_t0[l + 1] - C.blur_t0[l], e = C.blur_e0[l + 1] - C.blur_e0[l], m = C.blur_m0[l + 1] - C.blur_m0[l];
        EXPECT(t >= 0 && e >= 0 && m >= 0, "level %d blur partition decreases", l);
        EXPECT(m == 0 || t + e == 0, "level %d has %d tile waves and %d threads", l, m, t + e);
        EXPECT(l < nl || t + e + m == 0, "level %d past nlevels has blur work", l);
    }
}

static int run_cases(int argc, char** argv)
{
    if ((argc - 2) % 5 != 0) return 2;
    for (int a = 2; a + 4 < argc; a += 5) {
        const int W = atoi(argv[a]), H = atoi(argv[a + 1]), nf = atoi(argv[a + 2]), nl = atoi(argv[a + 3]);
        const float scale = strtof(argv[a + 4], nullptr);
        Geometry g;
        std::string err;
        const rgbd_status s = build(W, H, nf, nl, scale, g, err);
        g_hash = 1469598103934665603ull;
        fnv(&g.cfg, sizeof(g.cfg));
        fnv_vec(g.cells);
        fnv_vec(g.segs);
        fnv_vec(g.rsx);
        fnv_vec(g.rsy);
        fnv_vec(g.qx);
        fnv_vec(g.blur_tab);
        printf("CASE %d %d %d %d %s status %d cells %zu segs %zu digest %016" PRIx64 " msg %s\n", W, H, nf, nl, argv[a + 4], (int)s,
               g.cells.size(), g.segs.size(), g_hash, err.c_str());
        if (s) continue;
        for (int l = 0; l < nl; l++) {
            uint32_t bits;
            memcpy(&bits, &g.cfg.lv[l].scale, 4);
            printf("LV %d %d %d %d %08x\n", l, g.cfg.lv[l].w, g.cfg.lv[l].h, g.cfg.lv[l].N, bits);
        }
        printf("UMAX");
        for (int i = 0; i < 16; i++) printf(" %d", g.cfg.umax[i]);
        printf("\n");
    }
    return 0;
}

static int run_sweep(int nf, bool strict)
{
    const int Hs[4] = {80, 240, 480, 720}, NLs[4] = {1, 4, 8, 12};
    int configs = 0, accepted = 0;
    for (int W = 64; W <= 1280; W += 16)
        for (int H : Hs)
            for (int nl : NLs) {
                Geometry g;
                std::string err;
                configs++;
                if (build(W, H, nf, nl, 1.2f, g, err)) continue;
                accepted++;
                snprintf(g_where, sizeof(g_where), "%dx%d nfeatures %d nlevels %d", W, H, nf, nl);
                check(g, strict);
            }
    printf("SWEEP nfeatures %d configs %d accepted %d fails %d\n", nf, configs, accepted, g_fails);
    return g_fails ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "case")) return run_cases(argc, argv);
    if (argc == 4 && !strcmp(argv[1], "sweep")) return run_sweep(atoi(argv[2]), atoi(argv[3]) != 0);
    fprintf(stderr, "usage: geometry_check case W H nfeatures nlevels scale ... | sweep nfeatures strict\n");
    return 2;
}
