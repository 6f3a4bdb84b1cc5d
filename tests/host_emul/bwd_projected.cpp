// bwd_projected.cpp -- TEST INFRASTRUCTURE.  The blend backward's per-pixel walk (as host_emul.cpp's emul_render_bwd) run
// twice over the same pairs: once with the product's bwd_pair_core (one running value u = sum over the planes of upstream
// gradient x what lies behind), once with the eight per-plane running values it replaced (accum_rec[3], accum_depth_rec,
// accum_alpha_rec, accum_normal_rec[3], backward.cu:337-380).  Both feed bwd_pair_geometry; the accumulators must agree up
// to fp32 re-association.  Never loaded by the product package.
#include <stdint.h>
#include <string.h>

#include "../../vidu4d_amd/csrc/surfel_math.h"

using namespace surfel;

namespace {

struct Behind8 {
    float rgb[3] = {0, 0, 0}, depth = 0, alpha = 0, normal[3] = {0, 0, 0};
};

// dL/dalpha and the recurrences of one pair with the eight running values (the formulation before the projection)
template <int MODE>
PairGrad pair_core_eight(BwdPixel& s, Behind8& b, const PairEval& e, const float normal[3], const float rgb[3], bool is_median)
{
    const float alpha = e.alpha, c_d = e.depth;
    const float one_m_alpha = 1.f - alpha;
    const float inv_1ma = fast_rcp(one_m_alpha);
    s.T = s.T * inv_1ma;
    const float w = alpha * s.T;
    float dL_dalpha = 0.0f;
    for (int ch = 0; ch < 3; ch++) dL_dalpha += (rgb[ch] - b.rgb[ch]) * s.dL_dpixel[ch];
    float dL_dz = 0.0f;
    if (MODE == BLEND_FULL) {
        float dL_dweight = 0.0f;
        const float inv_d = fast_rcp((FAR_PLANE - NEAR_PLANE) * c_d);
        const float m_d = (FAR_PLANE * c_d - FAR_PLANE * NEAR_PLANE) * inv_d - s.m0;
        const float dmd_dd = (FAR_PLANE * NEAR_PLANE * (FAR_PLANE - NEAR_PLANE)) * inv_d * inv_d;
        if (is_median) {
            dL_dz += s.dL_dmedian_depth;
            dL_dweight += s.dL_dmax_dweight;
        }
        dL_dweight += (s.final_D2 + m_d * m_d * s.final_A - 2.0f * m_d * s.final_D) * s.dL_dreg;
        dL_dalpha += dL_dweight - s.last_dL_dT;
        s.last_dL_dT = dL_dweight * alpha + one_m_alpha * s.last_dL_dT;
        const float dL_dmd = 2.0f * w * (m_d * s.final_A - s.final_D) * s.dL_dreg;
        dL_dz += dL_dmd * dmd_dd;
    }
    if (MODE != BLEND_LITE) dL_dalpha += (c_d - b.depth) * s.dL_ddepth;
    dL_dalpha += (1.0f - b.alpha) * s.dL_daccum;
    if (MODE != BLEND_LITE)
        for (int ch = 0; ch < 3; ch++) dL_dalpha += (normal[ch] - b.normal[ch]) * s.dL_dnormal2D[ch];
    dL_dalpha *= s.T;
    dL_dalpha += (-s.T_final * inv_1ma) * s.bg_dot_dpixel;
    for (int ch = 0; ch < 3; ch++) {
        b.rgb[ch] = fmaf(alpha, rgb[ch] - b.rgb[ch], b.rgb[ch]);
        b.normal[ch] = fmaf(alpha, normal[ch] - b.normal[ch], b.normal[ch]);
    }
    b.depth = fmaf(alpha, c_d - b.depth, b.depth);
    b.alpha = fmaf(alpha, 1.0f - b.alpha, b.alpha);
    if (MODE != BLEND_LITE) dL_dz += w * s.dL_ddepth;
    PairGrad r;
    r.w = w;
    r.dL_dalpha = dL_dalpha;
    r.dL_dz = dL_dz;
    return r;
}

template <int MODE>
void walk(int W, int H, const uint32_t* ranges, const uint32_t* point_list, const float* rec, const float* bg,
          const float* final_T, const uint32_t* n_contrib, const float* dL_dcolor, const float* dL_dothers, double* acc_new,
          double* acc_eight)
{
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    const size_t HW = (size_t)W * H;
    for (int tile = 0; tile < gx * gy; tile++)
        for (int l = 0; l < TILE * TILE; l++) {
            const int px = (tile % gx) * TILE + l % TILE, py = (tile / gx) * TILE + l / TILE;
            if (px >= W || py >= H) continue;
            const float pixx = px + 0.5f, pixy = py + 0.5f;
            const size_t pid = (size_t)py * W + px;
            BwdPixel s;
            s.T_final = final_T[pid];
            s.final_D = s.final_D2 = 0.f;
            s.last_contributor = n_contrib[pid];
            s.median_contributor = 0;
            for (int c = 0; c < 3; c++) s.dL_dpixel[c] = dL_dcolor[c * HW + pid];
            s.dL_daccum = dL_dothers[pid + HW];
            s.dL_ddepth = s.dL_dmedian_depth = s.dL_dreg = s.dL_dmax_dweight = 0.f;
            for (int c = 0; c < 3; c++) s.dL_dnormal2D[c] = 0.f;
            if (MODE != BLEND_LITE) {
                s.dL_ddepth = dL_dothers[pid];
                for (int c = 0; c < 3; c++) s.dL_dnormal2D[c] = dL_dothers[pid + (2 + c) * HW];
            }
            if (MODE == BLEND_FULL) {
                s.final_D = final_T[pid + HW];
                s.final_D2 = final_T[pid + 2 * HW];
                s.median_contributor = n_contrib[pid + HW];
                s.dL_dmedian_depth = dL_dothers[pid + 5 * HW];
                s.dL_dreg = dL_dothers[pid + 6 * HW];
                s.dL_dmax_dweight = dL_dothers[pid + 7 * HW];
            }
            s.T = s.T_final;
            s.final_A = 1.0f - s.T_final;
            s.bg_dot_dpixel = bg[0] * s.dL_dpixel[0] + bg[1] * s.dL_dpixel[1] + bg[2] * s.dL_dpixel[2];
            BwdPixel s8 = s;
            Behind8 b;
            const uint32_t r0 = ranges[2 * tile];
            for (int ci = (int)s.last_contributor - 1; ci >= 0; ci--) {
                const uint32_t id = point_list[r0 + ci];
                const float* r = rec + (size_t)id * REC_FLOATS;
                PairEval e;
                if (!eval_pair_flat(r, r + 3, r + 6, r[R_CX], r[R_CY], r[R_OPAC], pixx, pixy, e)) continue;
                const bool is_median = (uint32_t)ci + 1 == s.median_contributor;
                float g[ACC_FLOATS];
                const PairGrad pg = bwd_pair_core<MODE>(s, e, r + R_NX, r + R_RGB, is_median);
                bwd_pair_geometry<MODE>(s, e, pg, r + 6, r[R_OPAC], pixx, pixy, g);
                for (int k = 0; k < ACC_FLOATS; k++) acc_new[(size_t)id * ACC_FLOATS + k] += (double)g[k];
                const PairGrad p8 = pair_core_eight<MODE>(s8, b, e, r + R_NX, r + R_RGB, is_median);
                bwd_pair_geometry<MODE>(s8, e, p8, r + 6, r[R_OPAC], pixx, pixy, g);
                for (int k = 0; k < ACC_FLOATS; k++) acc_eight[(size_t)id * ACC_FLOATS + k] += (double)g[k];
            }
        }
}

}  // namespace

// mode: 0 BLEND_FULL, 1 BLEND_LITE, 2 BLEND_GEOM (acc_* [P][20], zeroed by the caller)
extern "C" void bwd_projected_walk(int mode, int W, int H, const uint32_t* ranges, const uint32_t* point_list,
                                   const float* rec, const float* bg, const float* final_T, const uint32_t* n_contrib,
                                   const float* dL_dcolor, const float* dL_dothers, double* acc_new, double* acc_eight)
{
    if (mode == BLEND_LITE)
        walk<BLEND_LITE>(W, H, ranges, point_list, rec, bg, final_T, n_contrib, dL_dcolor, dL_dothers, acc_new, acc_eight);
    else if (mode == BLEND_GEOM)
        walk<BLEND_GEOM>(W, H, ranges, point_list, rec, bg, final_T, n_contrib, dL_dcolor, dL_dothers, acc_new, acc_eight);
    else
        walk<BLEND_FULL>(W, H, ranges, point_list, rec, bg, final_T, n_contrib, dL_dcolor, dL_dothers, acc_new, acc_eight);
}
