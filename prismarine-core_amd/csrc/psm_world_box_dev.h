// psm_world_box_dev.h -- the device pieces the box and the triangle queries of a world share (world_box.hip, world_tri.hip;
// DESIGN.md 4.16, 4.20): the forward pose of a point and of a vector, the margin constants of the prune inside an instance, and
// WorldBoxPrune: the top-level test and the in-instance prune of a world-space box [lo, hi] that is never moved. Moved here from
// world_box.hip's anonymous namespace as they were; a body derives from WorldBoxPrune and sets lo, hi and qmax in begin().
// fwd_vec and fwd_point also compile for the host: a stand-alone program defines PSM_WORLD_BOX_FN as a host function's decoration
// before it includes this file (tests/cpp/world_tri_pose_host.cpp).
#pragma once
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"   // WorldArgs, load_row, WORLD_QSLACK
#include "psm_box_dev.h"     // box_row

#ifndef PSM_WORLD_BOX_FN
#define PSM_WORLD_BOX_FN PSM_D
#endif

namespace psm {

namespace {

// The margin of the prune inside an instance, beside box_row's own h (DESIGN.md 4.16 has the chain). With N = M3 R^T (float32),
// W_k = |N_k0| + |N_k1| + |N_k2|, D the largest |coordinate| of the box shifted by -T and Q the largest |coordinate| of the box,
//   g_k = WORLD_BOX_PAD (2 + (W_k (D + WORLD_BOX_QREL Q) + |M_k3|))
// covers: R^T R = 1 + E, |E_ij| <= 1e-5 (the forward image of an object point and the box's way back differ by 5.2e-5 W_k D:
// 0.107 of the grant); the rounding of N (5.4e-7 W_k D); the rounding of the forward posing, eps (16 D + Q) W_k (1 / 32 of the
// grant of Q); and box_tri's 16 eps |e'| under a row of condition number <= 16 (4.6e-5 against the constant 2 WORLD_BOX_PAD).
// The triangle queries run the same chain on the query's bounding box.
constexpr float WORLD_BOX_PAD = 0x1p-11f;
constexpr float WORLD_BOX_QREL = 0x1p-8f;

// the forward pose of a point and of a vector: float32, one rounding per operation, world_inst_boxes' order for cw
PSM_WORLD_BOX_FN v3 fwd_vec(const float* m, v3 d) {
    return mk3((m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[4] * d.x + m[5] * d.y) + m[6] * d.z, (m[8] * d.x + m[9] * d.y) + m[10] * d.z);
}
PSM_WORLD_BOX_FN v3 fwd_point(const float* m, v3 x) {
    return mk3(((m[0] * x.x + m[1] * x.y) + m[2] * x.z) + m[3], ((m[4] * x.x + m[5] * x.y) + m[6] * x.z) + m[7],
               ((m[8] * x.x + m[9] * x.y) + m[10] * x.z) + m[11]);
}

PSM_D float absmax3(v3 a) { return smaxf(smaxf(pabs(a.x), pabs(a.y)), pabs(a.z)); }

// The two tests of a world box [lo, hi] (closed, never moved) that a body of world_walk takes over: against a top-level node's
// child boxes, and against the child boxes of the hierarchy of the instance the lane is in.
struct WorldBoxPrune {
    const uint4* node32;   // (load_row sets these three)
    const float4* tri48;
    int inst;
    v3 lo, hi;             // the world box
    float qmax;            // its largest |coordinate|
    float glx, gly, glz, ghx, ghy, ghz;   // the grown image interval per normalised axis of the instance the lane is in

    // a top-level child box [c, C] grown by the query's slack against the closed world box (negations: a NaN keeps the box; an
    // instance without triangles has c = +inf, C = -inf and is dropped). A leaf's box that passes, passes in every ancestor:
    // an inner box is the exact min / max union of leaf boxes and the two roundings are monotone.
    PSM_D bool keep_top(float cx, float cy, float cz, float Cx, float Cy, float Cz) const {
        const float pad = WORLD_QSLACK * qmax;
        bool out = (Cx + pad) < lo.x;
        out |= (cx - pad) > hi.x;
        out |= (Cy + pad) < lo.y;
        out |= (cy - pad) > hi.y;
        out |= (Cz + pad) < lo.z;
        out |= (cz - pad) > hi.z;
        return !out;
    }
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& kL, float& kR) const {
        okL = keep_top(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y);
        okR = keep_top(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w);
        kL = 0.f;
        kR = 0.f;
    }
    // one normalised axis of the instance: row k of N = M3 R^T with M's own m_k3, over the box shifted by -T
    PSM_D static void axis(const float* M, const float* m, int k, v3 sl, v3 sh, float reach, float& glo, float& ghi) {
        float N[4];
#pragma unroll
        for (int j = 0; j < 3; j++) N[j] = (M[4 * k] * m[4 * j] + M[4 * k + 1] * m[4 * j + 1]) + M[4 * k + 2] * m[4 * j + 2];
        N[3] = M[4 * k + 3];
        box_row(N, 0, sl, sh, glo, ghi);
        const float W = (pabs(N[0]) + pabs(N[1])) + pabs(N[2]);
        const float g = (2.0f + (W * reach + pabs(N[3]))) * WORLD_BOX_PAD;
        glo = glo - g;
        ghi = ghi + g;
    }
    // the row of instance `in` and the grown intervals of the box in that instance's normalised space
    PSM_D RowLoad enter_row(const WorldArgs& w, int in) {
        const RowLoad r = load_row(w, in, *this);
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(r.sm[SM_M + k]);
        intervals(M, r.m);
        return r;
    }
    // ... from the hierarchy's fit transform M and the instance's pose m (world_grid.hip comes here with a row its wave loaded)
    PSM_D void intervals(const float* M, const float* m) {
        const v3 T = mk3(m[3], m[7], m[11]);
        const v3 sl = lo - T, sh = hi - T;
        const float reach = smaxf(absmax3(sl), absmax3(sh)) + WORLD_BOX_QREL * qmax;
        axis(M, m, 0, sl, sh, reach, glx, ghx);
        axis(M, m, 1, sl, sh, reach, gly, ghy);
        axis(M, m, 2, sl, sh, reach, glz, ghz);
    }
    // a child box [mn, mx] is kept iff it meets the grown interval on all three axes (negations: a NaN keeps the box)
    PSM_D bool keep(float mnx, float mny, float mnz, float mxx, float mxy, float mxz) const {
        bool out = mxx < glx;
        out |= mnx > ghx;
        out |= mxy < gly;
        out |= mny > ghy;
        out |= mxz < glz;
        out |= mnz > ghz;
        return !out;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        okL = keep(half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        okR = keep(half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        kL = 0.f;
        kR = 0.f;
    }
};

}  // namespace

}  // namespace psm
