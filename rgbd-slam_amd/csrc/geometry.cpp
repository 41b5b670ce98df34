// geometry.cpp -- the extraction geometry (geometry.h), host only.
//
// Geometry is derived here once per context with the reference's own float/double rules:
//   ORBextractor ctor (Features/ORBextractor.cpp:348-406): scale factors, per-level budgets, umax
//   ComputePyramid (:773-797): level sizes; OpenCV resize tables (xofs/ialpha/yofs/ibeta)
//   ComputeKeyPointsOctTree (:613-672): borders, 30-px cell grid, ROI ranges
//   DistributeOctTree (:420-422): nIni, hX
#include "geometry.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "dist_layout.h"

namespace rgbd {
namespace {

inline int round_half_even_f(float v) { return (int)std::nearbyintf(v); }
inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

rgbd_status unsupported(std::string& err, const char* msg)
{
    err = msg;
    return RGBD_ERR_UNSUPPORTED;
}

struct OrbBudgets {
    std::vector<float> sf, inv;   // mvScaleFactor, mvInvScaleFactor
    std::vector<int> N;           // mnFeaturesPerLevel
};

// ORBextractor ctor
OrbBudgets orb_budgets(const rgbd_orb_params& o, ExtractCfg& C)
{
    const int nl = o.nlevels;
    const double scaleFactor = (double)o.scale_factor;
    std::vector<float> sf(nl), inv(nl);
    sf[0] = 1.0f;
    for (int i = 1; i < nl; i++) sf[i] = (float)((double)sf[i - 1] * scaleFactor);
    for (int i = 0; i < nl; i++) inv[i] = 1.0f / sf[i];
    const float factor = (float)(1.0f / scaleFactor);
    float nDesired = o.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
    std::vector<int> N(nl);
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) {
        N[l] = round_half_even_f(nDesired);
        sum += N[l];
        nDesired *= factor;
    }
    N[nl - 1] = std::max(o.nfeatures - sum, 0);
    {
        int umax[16];
        const int HP = 15;
        const int vmax = (int)std::floor(HP * std::sqrt(2.f) / 2 + 1);
        const int vmin = (int)std::ceil(HP * std::sqrt(2.f) / 2);
        const double hp2 = HP * HP;
        int v, v0;
        for (v = 0; v <= vmax; ++v) umax[v] = (int)std::nearbyint(std::sqrt(hp2 - v * v));
        for (v = HP, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
        for (int i = 0; i < 16; i++) C.umax[i] = umax[i];
        for (int r = 0; r < 31; r++) {
            const int um = umax[r < 15 ? 15 - r : r - 15];
            for (int k = 0; k < 8; k++) {
                uint32_t wu = 0, w1 = 0;
                for (int i = 0; i < 4; i++) {
                    const int u = 4 * k + i - 15;
                    if (u >= -um && u <= um) {
                        wu |= (uint32_t)(u + 16) << (8 * i);
                        w1 |= 1u << (8 * i);
                    }
                }
                C.ic_wu[r][k] = wu;
                C.ic_w1[r][k] = w1;
            }
        }
    }
    return OrbBudgets{std::move(sf), std::move(inv), std::move(N)};
}

// level l: size, stride, borders and its cells; off / cell_cap: the running pyramid bytes and slot capacity
rgbd_status level_cells(int l, const OrbBudgets& B, Geometry& g, int& off, int& cell_cap, std::string& err)
{
    const ExtractCfg& C = g.cfg;
    const std::vector<float>& sf = B.sf;
    const std::vector<float>& inv = B.inv;
    LevelCfg& L = g.cfg.lv[l];
    L.w = round_half_even_f((float)C.W * inv[l]);
    L.h = round_half_even_f((float)C.H * inv[l]);
    if (L.w < 48 || L.h < 48) return unsupported(err, "pyramid level smaller than 48 px");
    L.stride = align_up(L.w, 64);
    L.off = off;
    off += align_up(L.stride * L.h, 256);
    L.scale = sf[l];
    L.size = (float)(int)(31 * sf[l]);
    L.N = B.N[l];
    const int EDGE = 19;
    L.minBX = EDGE - 3;
    L.minBY = EDGE - 3;
    L.maxBX = L.w - EDGE + 3;
    L.maxBY = L.h - EDGE + 3;
    // cells (:627-667)
    const float Wc = 30;
    const float width = (float)(L.maxBX - L.minBX), height = (float)(L.maxBY - L.minBY);
    const int nCols = (int)(width / Wc), nRows = (int)(height / Wc);
    if (nCols <= 0 || nRows <= 0) return unsupported(err, "level too small for the 30-px cell grid");
    const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
    L.cell_begin = (int)g.cells.size();
    for (int i = 0; i < nRows; i++) {
        const float iniY = (float)(L.minBY + i * hCell);
        float maxY = iniY + hCell + 6;
        if (iniY >= L.maxBY - 3) continue;
        if (maxY > L.maxBY) maxY = (float)L.maxBY;
        for (int j = 0; j < nCols; j++) {
            const float iniX = (float)(L.minBX + j * wCell);
            float maxX = iniX + wCell + 6;
            if (iniX >= L.maxBX - 6) continue;
            if (maxX > L.maxBX) maxX = (float)L.maxBX;
            Cell cc;
            cc.level = (int16_t)l;
            cc.x0 = (int16_t)(int)iniX;
            cc.y0 = (int16_t)(int)iniY;
            cc.x1 = (int16_t)(int)maxX;
            cc.y1 = (int16_t)(int)maxY;
            cc.pad = 0;
            const int cw = cc.x1 - cc.x0, ch = cc.y1 - cc.y0;
            if (cw > kCellStride || ch > kCellStride)
                return unsupported(err, "FAST cell ROI larger than 48 px");
            const int a = std::max(cw - 6, 0), b = std::max(ch - 6, 0);
            cell_cap = std::max(cell_cap, ((a + 1) / 2) * ((b + 1) / 2));
            g.cells.push_back(cc);
        }
    }
    L.cell_count = (int)g.cells.size() - L.cell_begin;
    return RGBD_OK;
}

// k_fast segments of level L (its cells are the last of the table): consecutive cells of one cell row,
// 64 / lanes-per-cell of them per wave
rgbd_status fast_segments(const LevelCfg& L, const std::vector<Cell>& cells, std::vector<FastSeg>& segs, std::string& err)
{
    int np_max = 1;
    for (int q = L.cell_begin; q < (int)cells.size(); q++)
        np_max = std::max(np_max, (cells[q].x1 - cells[q].x0 - 6 + 1) / 2);
    // 16 lanes (a DPP row) per cell when the pairs fit, else exactly the widest cell's pairs: a level
    // whose cells hold 17-19 pairs (640 x 480: levels 5 and 7) packs 3 cells per wave, not 2 of 32 lanes
    const int lpc = np_max <= 16 ? 16 : np_max;
    if (lpc > 32) return unsupported(err, "FAST cell interior wider than 64 px");
    const int cpw = 64 / lpc;
    // a plain segment's staged row (16-B aligned start .. x1 + 6) must fit kFastPlainRowBytes = 160
    auto row_bytes = [&](int q0, int e0) { return cells[e0 - 1].x1 + 6 - (cells[q0].x0 & ~15); };
    auto plain_seg = [&](int q0, int e0) {
        FastSeg s{{q0, q0, q0, q0}, (int16_t)(e0 - q0), (int16_t)lpc, 0, 0};
        for (int k = 0; k < e0 - q0; k++) s.cell[k] = q0 + k;
        return s;
    };
    // full waves stay plain segments; with RGBD_FAST_GATHER the short segments' cells (the n % cpw last
    // cells of each cell row) are pooled by ROI height (the last cell row of a level may be shorter, and
    // the walk's row bounds are wave-uniform) and packed cpw per wave into gathered segments
    std::vector<FastSeg> full;
    std::vector<std::pair<int, std::vector<int>>> pool;   // (ROI height, cells) in order of appearance
    for (int q = L.cell_begin; q < (int)cells.size();) {
        int e = q + 1;
        while (e < (int)cells.size() && e - q < cpw && cells[e].y0 == cells[q].y0 &&
               row_bytes(q, e + 1) <= kFastPlainRowBytes)
            e++;
        if (row_bytes(q, e) > kFastPlainRowBytes)
            return unsupported(err, "FAST segment row wider than 160 B");
        if (RGBD_FAST_GATHER && e - q < cpw) {
            const int ch = cells[q].y1 - cells[q].y0;
            auto it = pool.begin();
            while (it != pool.end() && it->first != ch) ++it;
            if (it == pool.end()) it = pool.insert(it, {ch, {}});
            for (int k = q; k < e; k++) it->second.push_back(k);
        } else {
            full.push_back(plain_seg(q, e));
        }
        q = e;
    }
    // the level's gathered segments lead its full ones, so they are never the last blocks of a frame
    const int slot_bytes = kFastRowBytes / cpw / 4 * 4;
    for (const auto& grp : pool) {
        const std::vector<int>& v = grp.second;
        for (size_t i = 0; i < v.size(); i += cpw) {
            const int n = (int)std::min(v.size() - i, (size_t)cpw);
            bool run = true;   // one run of a cell row: a plain segment after all
            for (int k = 1; k < n; k++)
                run = run && v[i + k] == v[i] + k && cells[v[i + k]].y0 == cells[v[i]].y0;
            if (run && row_bytes(v[i], v[i] + n) <= kFastPlainRowBytes) {
                segs.push_back(plain_seg(v[i], v[i] + n));
                continue;
            }
            FastSeg s{{v[i], v[i], v[i], v[i]}, (int16_t)n, (int16_t)lpc, 1, 0};
            for (int k = 0; k < n; k++) {
                const Cell& cc = cells[v[i + k]];
                // the slot holds the ROI row from its 4-B aligned start to the last lane's read (x1 + 6)
                if (align_up(cc.x1 + 6 - (cc.x0 & ~3), 4) > slot_bytes)
                    return unsupported(err, "FAST gathered segment slot wider than its share of 192 B");
                s.cell[k] = v[i + k];
            }
            segs.push_back(s);
        }
    }
    segs.insert(segs.end(), full.begin(), full.end());
    return RGBD_OK;
}

// DistributeOctTree roots (:420-422) of level L and its selection slots; maxNode: the running node demand
rgbd_status quadtree_roots(LevelCfg& L, int& sel_off, int& maxNode, std::string& err)
{
    const int dX = L.maxBX - L.minBX, dY = L.maxBY - L.minBY;
    L.nIni = (int)std::round(static_cast<float>(dX) / dY);
    if (L.nIni < 1) return unsupported(err, "image taller than 2x its width (nIni == 0)");
    L.hX = static_cast<float>(dX) / L.nIni;
    const int selCap = std::max(L.N + 3, 4 * L.nIni);
    L.sel_off = sel_off;
    sel_off += align_up(selCap, 4);
    maxNode = std::max(maxNode, std::max(L.N + 8, 4 * L.nIni + 8));
    return RGBD_OK;
}

// the key and selection regions of a frame and the quadtree's capacities, once every level has its cells
rgbd_status quadtree_capacities(ExtractCfg& C, int cell_cap, int sel_off, int maxNode, std::string& err)
{
    const int nl = C.nlevels;
    int key_off = 0;
    C.cell_cap = cell_cap;
    for (int l = 0; l < nl; l++) {
        LevelCfg& L = C.lv[l];
        L.key_off = key_off;
        L.key_cap = align_up(L.cell_count * cell_cap, 4);   // k_distribute reads keys and state four at a time
        key_off += L.key_cap;
        if (L.key_cap >= (1 << 24)) return unsupported(err, "too many FAST candidates per level");
    }
    C.keys_per_frame = key_off;
    C.sel_per_frame = sel_off;
    for (int l = 0; l < kMaxLevels; l++) C.sel_off_tab[l] = l < nl ? C.lv[l].sel_off : INT32_MAX;
    int NC = 64;
    while (NC < maxNode) NC <<= 1;
    if (NC > 4096) return unsupported(err, "nfeatures too large for the quadtree node capacity");
    C.node_cap = NC;
    {
        int mc = 0;
        for (int l = 0; l < nl; l++) mc = std::max(mc, C.lv[l].cell_count);
        C.scan_cap = std::max(NC, mc) + 1;
    }
    // the keys whose round state fits in LDS beside the node arrays (dist_layout.h: the layout and the budget)
    C.dist_kc = distribute_key_capacity((long)RGBD_DIST_LDS_KB * 1024 - (long)distribute_lds_bytes(NC, C.scan_cap), NC);
    C.kp_cap = align_up(sel_off, 4);
    return RGBD_OK;
}

// resize(INTER_LINEAR) tables of OpenCV 3.4 resize() for src (sw,sh) -> dst (dw,dh)
void resize_tables(int sw, int sh, int dw, int dh, Geometry& g, LevelCfg& D)
{
    const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    D.rs_scale_x = scale_x;
    D.rs_scale_y = scale_y;
    D.qx_off = 0;
    D.rsx_off = (int)g.rsx.size();
    D.rsy_off = (int)g.rsy.size();
    int xmax = dw;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)std::floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= sw) {
            xmax = std::min(xmax, dx);
            if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        }
        const float c0 = 1.f - fx, c1 = fx;
        ResizeX e;
        e.sx = (int16_t)sx;
        e.a0 = (int16_t)std::min(std::max(round_half_even_f(c0 * 2048), -32768), 32767);
        e.a1 = (int16_t)std::min(std::max(round_half_even_f(c1 * 2048), -32768), 32767);
        e.pad = 0;
        g.rsx.push_back(e);
    }
    auto clip = [](int x, int a, int b) { return x >= a ? (x < b ? x : b - 1) : a; };
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)std::floor(fy);
        fy -= sy;
        const float c0 = 1.f - fy, c1 = fy;
        ResizeY e;
        e.sy0 = (int16_t)clip(sy, 0, sh);
        e.sy1 = (int16_t)clip(sy + 1, 0, sh);
        e.b0 = (int16_t)std::min(std::max(round_half_even_f(c0 * 2048), -32768), 32767);
        e.b1 = (int16_t)std::min(std::max(round_half_even_f(c1 * 2048), -32768), 32767);
        g.rsy.push_back(e);
    }
    D.rs_xmax = xmax;
    int x = 0;
    for (; x <= dw - 16; x += 16) {}
    for (; x < dw - 4; x += 4) {}
    D.rs_simd = x;
}

// k_pyramid strips (levels < pyr_top): each strip owns an equal share of every level's rows (written to HBM); walking
// down from the top level, level l-1 must also hold the source rows (sy0, sy1) of the rows level l
// computes.  The strips blur nothing (the level blur of every level runs inside the k_fast grid), so a
// strip's rows come from the resize alone.
rgbd_status pyramid_strips(Geometry& g, std::string& err)
{
    ExtractCfg& C = g.cfg;
    const int nl = C.nlevels;
    {
        size_t lds_a = 0, lds_b = 0;   // even / odd level strip buffers
        const int top = std::min(nl, kPyrStripLevels);   // levels top .. nl-1: k_pyr_tail, no strip rows
        C.pyr_top = top;
        int r0[kPyrStrips][kMaxLevels], r1[kPyrStrips][kMaxLevels];
        for (int s_ = 0; s_ < kPyrStrips; s_++)
            for (int l = 0; l < kMaxLevels; l++) C.strip_r0[s_][l] = C.strip_r1[s_][l] = 0;
        for (int l = top - 1; l >= 0; l--) {
            const int h = C.lv[l].h;
            for (int s_ = 0; s_ < kPyrStrips; s_++) {
                r0[s_][l] = (int)((long)h * s_ / kPyrStrips);
                r1[s_][l] = (int)((long)h * (s_ + 1) / kPyrStrips);
                if (l + 1 < top && r1[s_][l + 1] > r0[s_][l + 1]) {
                    const ResizeY& a = g.rsy[C.lv[l + 1].rsy_off + r0[s_][l + 1]];
                    const ResizeY& z = g.rsy[C.lv[l + 1].rsy_off + r1[s_][l + 1] - 1];
                    r0[s_][l] = std::min(r0[s_][l], (int)a.sy0);
                    r1[s_][l] = std::max(r1[s_][l], (int)z.sy1 + 1);
                }
            }
        }
        for (int s_ = 0; s_ < kPyrStrips; s_++) {
            for (int l = 0; l < top; l++) {
                const size_t bytes = (size_t)(r1[s_][l] - r0[s_][l]) * C.lv[l].stride;
                if (l % 2 == 0) lds_a = std::max(lds_a, bytes);
                else lds_b = std::max(lds_b, bytes);
                C.strip_r0[s_][l] = (int16_t)r0[s_][l];
                C.strip_r1[s_][l] = (int16_t)r1[s_][l];
            }
        }
        lds_a = (lds_a + 15) / 16 * 16;

        C.pyr_lds_b = (int)lds_a;
        C.pyr_lds = (int)((lds_a + lds_b + 16 + 15) / 16 * 16);   // + 16: a quad's 12-byte tap window may run past the last row
        // + the strip's resize row entries of levels 1..L-1 (k_pyramid stages them after the level buffers)
        int rows = 0;
        for (int s_ = 0; s_ < kPyrStrips; s_++) {
            int n = 0;
            for (int l = 1; l < top; l++) n += r1[s_][l] - r0[s_][l];
            rows = std::max(rows, n);
        }
        C.pyr_rsy_lds = (int)(rows * sizeof(ResizeY));
    }
    if (C.pyr_lds + C.pyr_rsy_lds > kPyrLdsLimit) return unsupported(err, "pyramid strip does not fit in LDS");
    return RGBD_OK;
}

// k_pyramid reads a quad's horizontal taps from the 12-byte window (sx of its first pixel) & ~3 ..
// + 11 of each source row, aligned to the 8 bytes from that pixel's left tap (two v_alignbyte per
// row): the right tap of its last pixel must lie within them (scale <= ~2)
rgbd_status quad_taps(Geometry& g, std::string& err)
{
    ExtractCfg& C = g.cfg;
    g.qx.clear();
    for (int l = 1; l < C.nlevels; l++) {
        LevelCfg& D = C.lv[l];
        const int sw = C.lv[l - 1].w;
        D.qx_off = (int)g.qx.size();
        for (int dx = 0; dx < D.w; dx += 4) {
            const int sx0 = g.rsx[D.rsx_off + dx].sx, wb = sx0 & ~3;
            const int sx3 = g.rsx[D.rsx_off + std::min(dx + 3, D.w - 1)].sx;
            if (std::min(sx3 + 1, sw - 1) - sx0 > 7)
                return unsupported(err, "pyramid scale factor too large for the resize tap window");
            QuadX q{};
            for (int i = 0; i < 4; i++) {
                const ResizeX& rx = g.rsx[D.rsx_off + std::min(dx + i, D.w - 1)];
                const int pad = rx.sx + 1 < sw ? rx.sx + 1 : rx.sx;
                const int o0 = rx.sx - sx0, o1 = pad - sx0;   // bytes of the 8-byte window from sx0
                q.sel[i] = (uint32_t)o0 | 0x0c00u | ((uint32_t)o1 << 16) | 0x0c000000u;
                const int a0 = dx + i < D.rs_xmax ? rx.a0 : 2048, a1 = dx + i < D.rs_xmax ? rx.a1 : 0;
                q.wt[i] = (uint32_t)(16 * a0) | ((uint32_t)(16 * a1) << 16);
                q.simd |= (dx + i < D.rs_simd ? 1u : 0u) << i;
            }
            q.wbpi = (uint32_t)wb | ((uint32_t)(sx0 - wb) << 16);   // window base | its byte shift
            g.qx.push_back(q);
        }
    }
    return RGBD_OK;
}

// level blur threads: one per column quad of each 32-row strip of each level; inner quads (bytes
// x - 4 .. x + 11 inside the row) first, edge quads after them
rgbd_status blur_partition(Geometry& g, std::string& err)
{
    ExtractCfg& C = g.cfg;
    const int nl = C.nlevels;
    g.blur_tab.clear();
    {
        int t = 0, e = 0, m = 0;
        for (int l = 0; l < kMaxLevels; l++) {
            C.blur_t0[l] = t;
            C.blur_e0[l] = e;
            C.blur_m0[l] = m;
            C.blur_tx[l] = C.blur_ex[l] = C.blur_mt[l] = C.blur_ms[l] = C.blur_tab_off[l] = 0;
            if (l >= nl) continue;
            const int w = C.lv[l].w, Q = (w + 3) / 4, ty = (C.lv[l].h + kBlurTH - 1) / kBlurTH;
            if (w < 16 || C.lv[l].h < 8) return unsupported(err, "pyramid level smaller than 16x8");
            const int qe = (w - 8) / 4 + 1;   // first quad with 4q + 8 > w
            C.blur_tx[l] = qe - 1;            // inner quads 1 .. qe - 1
            C.blur_ex[l] = 1 + (Q - qe);      // quad 0 and quads qe .. Q - 1
            // levels of a multi-level pyramid (level 0 included) that hold a 64-byte window and a 32-row block:
            // 32 x 32 tiles on the matrix cores, one wave per 32-column strip of up to kBlurMS row blocks; a taller
            // level's nb blocks go to ceil(nb / kBlurMS) strips of near-equal length (15 at 480 rows: 8 + 7)
            BlurLevelTab bt;
            if (RGBD_BLUR_MFMA && nl > 1 && blur_tab_build(w, C.lv[l].h, C.lv[l].stride, bt)) {
                const int nb = blur_tab_tiles(C.lv[l].h), strips = (nb + kBlurMS - 1) / kBlurMS;
                C.blur_mt[l] = blur_tab_tiles(w);
                C.blur_ms[l] = (nb + strips - 1) / strips;
                C.blur_tab_off[l] = (int)(g.blur_tab.size() * sizeof(BlurLevelTab));
                g.blur_tab.push_back(bt);
                m += C.blur_mt[l] * ((nb + C.blur_ms[l] - 1) / C.blur_ms[l]);
                continue;
            }
            t += C.blur_tx[l] * ty;
            e += C.blur_ex[l] * ty;
        }
        C.blur_t0[kMaxLevels] = t;
        C.blur_e0[kMaxLevels] = e;
        C.blur_m0[kMaxLevels] = m;
    }
    return RGBD_OK;
}

void camera_block(const rgbd_camera& k, ExtractCfg& C)
{
    C.fx = k.fx; C.fy = k.fy; C.cx = k.cx; C.cy = k.cy;
    C.invfx = 1.0f / k.fx;
    C.invfy = 1.0f / k.fy;
    C.k1 = k.k1; C.k2 = k.k2; C.p1 = k.p1; C.p2 = k.p2; C.k3 = k.k3;
    C.depth_factor = k.depth_map_factor;
    C.undistort = (k.k1 != 0.0f) ? 1 : 0;
}

}  // namespace

rgbd_status build_geometry(int W, int H, const rgbd_orb_params& o, const rgbd_camera& k, Geometry& g, std::string& err)
{
    ExtractCfg& C = g.cfg;
    std::memset(&C, 0, sizeof(C));
    const int nl = o.nlevels;
    if (nl < 1 || nl > kMaxLevels) return unsupported(err, "nlevels must be in [1, 12]");
    if (W % 16 != 0 || W < 64 || H <= 64) return unsupported(err, "width must be a multiple of 16 and >= 64");
    if (W > 16 * kPyrThreads) return unsupported(err, "width above 16 x the pyramid's threads per strip");
    C.W = W;
    C.H = H;
    C.nlevels = nl;
    C.ini_th = std::min(std::max(o.ini_th_fast, 0), 255);
    C.min_th = std::min(std::max(o.min_th_fast, 0), 255);
    const OrbBudgets B = orb_budgets(o, C);
    rgbd_status s;
    int off = 0, cell_cap = 1, sel_off = 0, maxNode = 8;
    g.cells.clear();
    g.segs.clear();
    g.rsx.clear();
    g.rsy.clear();
    for (int l = 0; l < nl; l++) {
        if ((s = level_cells(l, B, g, off, cell_cap, err))) return s;
        if ((s = fast_segments(C.lv[l], g.cells, g.segs, err))) return s;
        if ((s = quadtree_roots(C.lv[l], sel_off, maxNode, err))) return s;
    }
    C.frame_pyr_bytes = off;
    C.n_cells = (int)g.cells.size();
    if ((s = quadtree_capacities(C, cell_cap, sel_off, maxNode, err))) return s;
    // resize tables (level l from level l-1)
    for (int l = 1; l < nl; l++)
        resize_tables(C.lv[l - 1].w, C.lv[l - 1].h, C.lv[l].w, C.lv[l].h, g, C.lv[l]);
    if ((s = pyramid_strips(g, err))) return s;
    if ((s = quad_taps(g, err))) return s;
    if ((s = blur_partition(g, err))) return s;
    camera_block(k, C);
    return RGBD_OK;
}

}  // namespace rgbd
