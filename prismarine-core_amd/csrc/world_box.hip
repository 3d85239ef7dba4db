// world_box.hip -- box queries over an instance world (new; no reference counterpart; include/psm_hip.h "box queries over a
// world"): whether, how many and which (instance, triangle) pairs of a world overlap an axis-aligned WORLD box.
//
// The box stays where it is and is never moved: the candidate triangle is posed forward, v0' = fwd_point(m, v0), e1' =
// fwd_vec(m, e1), e2' = fwd_vec(m, e2) (the edges are R e1 and R e2, not differences of posed vertices), and box.hip's box_tri
// (psm_box_dev.h, unchanged) decides on (v0', e1', e2', lo, hi). The walk is world.hip's (world_walk, psm_world_dev.h); a body adds
//   * the top-level test: the world box against a node's child box grown by WORLD_QSLACK |q|_inf, closed, NaN keeps;
//   * the prune inside an instance: the box's image in the hierarchy's normalised space as an interval per axis under
//     N = M_build [R^T | -R^T T], evaluated on the box shifted by -T and grown by the margin of WorldBoxBody::enter;
//   * for the triangles query the list of the k lowest (instance, triangle) that count (psm_world_box_list.h).
// No result depends on the order of the walk: a flag, a sum, the k lowest pairs. The order keys are 0.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"   // world_walk, WorldArgs, load_row / load_pose, WORLD_QSLACK
#include "psm_box_dev.h"     // box_tri, box_row

#define PSM_WORLD_BOX_LIST_FN PSM_D
#include "psm_world_box_list.h"

namespace psm {

namespace {

// The margin of the prune inside an instance, beside box_row's own h (DESIGN.md 4.16 has the chain). With N = M3 R^T (float32),
// W_k = |N_k0| + |N_k1| + |N_k2|, D the largest |coordinate| of the box shifted by -T and Q the largest |coordinate| of the box,
//   g_k = WORLD_BOX_PAD (2 + (W_k (D + WORLD_BOX_QREL Q) + |M_k3|))
// covers: R^T R = 1 + E, |E_ij| <= 1e-5 (the forward image of an object point and the box's way back differ by 5.2e-5 W_k D:
// 0.107 of the grant); the rounding of N (5.4e-7 W_k D); the rounding of the forward posing, eps (16 D + Q) W_k (1 / 32 of the
// grant of Q); and box_tri's 16 eps |e'| under a row of condition number <= 16 (4.6e-5 against the constant 2 WORLD_BOX_PAD).
constexpr float WORLD_BOX_PAD = 0x1p-11f;
constexpr float WORLD_BOX_QREL = 0x1p-8f;

// a lane's column of the wave's key list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint64_t* key_column() {
    extern __shared__ uint64_t world_box_keys[];
    return world_box_keys + threadIdx.x;
}

// the forward pose of a point and of a vector: float32, one rounding per operation, world_inst_boxes' order for cw
PSM_D v3 fwd_vec(const float* m, v3 d) {
    return mk3((m[0] * d.x + m[1] * d.y) + m[2] * d.z, (m[4] * d.x + m[5] * d.y) + m[6] * d.z, (m[8] * d.x + m[9] * d.y) + m[10] * d.z);
}
PSM_D v3 fwd_point(const float* m, v3 x) {
    return mk3(((m[0] * x.x + m[1] * x.y) + m[2] * x.z) + m[3], ((m[4] * x.x + m[5] * x.y) + m[6] * x.z) + m[7],
               ((m[8] * x.x + m[9] * x.y) + m[10] * x.z) + m[11]);
}

PSM_D float absmax3(v3 a) { return smaxf(smaxf(pabs(a.x), pabs(a.y)), pabs(a.z)); }

enum { WBOX_ANY = 0, WBOX_COUNT = 1, WBOX_TRIS = 2 };

// MODE: what is kept of the candidates that count -- a flag (the walk ends at the first), their number, the k lowest pairs
template <int MODE>
struct WorldBoxBody {
    const WorldArgs& w;
    WorldBoxList<QUERY_BLOCK> L;
    const uint4* node32;   // (load_row sets these three)
    const float4* tri48;
    int inst;
    v3 lo, hi;             // the world box
    float qmax;            // its largest |coordinate|
    float glx, gly, glz, ghx, ghy, ghz;   // the grown image interval per normalised axis of the instance the lane is in
    uint32_t cnt;

    PSM_D WorldBoxBody(const WorldArgs& a, uint64_t* keys, uint32_t slots) : w(a), L(keys, slots) {}

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(-1.f, -1.f, -1.f, 0.f);   // a dead lane: lo > hi
        if (alive) { r0 = w.rays[2 * i]; r1 = w.rays[2 * i + 1]; }
        lo = mk3(r0.x, r0.y, r0.z);
        hi = mk3(r1.x, r1.y, r1.z);
        qmax = smaxf(absmax3(lo), absmax3(hi));
        cnt = 0u;
        L.clear();   // per query: the grid-stride loop comes here again
        return alive && finite3(lo) && finite3(hi) && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
    }
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
    PSM_D int enter(int in) {
        const RowLoad r = load_row(w, in, *this);
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(r.sm[SM_M + k]);
        const v3 T = mk3(r.m[3], r.m[7], r.m[11]);
        const v3 sl = lo - T, sh = hi - T;
        const float reach = smaxf(absmax3(sl), absmax3(sh)) + WORLD_BOX_QREL * qmax;
        axis(M, r.m, 0, sl, sh, reach, glx, ghx);
        axis(M, r.m, 1, sl, sh, reach, gly, ghy);
        axis(M, r.m, 2, sl, sh, reach, glz, ghz);
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;   // -2: no tree (0 or 1 leaves)
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
    // the triangle posed forward (the pose re-read: 12 floats are not kept live over the walk), then 4.15's test, unchanged
    PSM_D void leaf(int tri) {
        float m[12];
        (void)load_pose(w, (uint32_t)inst, m);
        const float4 A = tri48[(size_t)3 * tri + 0], B = tri48[(size_t)3 * tri + 1], C = tri48[(size_t)3 * tri + 2];
        const v3 v0 = fwd_point(m, mk3(A.x, A.y, A.z)), e1 = fwd_vec(m, mk3(B.x, B.y, B.z)), e2 = fwd_vec(m, mk3(C.x, C.y, C.z));
        if (!box_tri(v0, e1, e2, lo, hi)) return;
        if (MODE == WBOX_TRIS) L.offer((uint32_t)inst, (uint32_t)tri);
        else cnt++;
    }
    PSM_D bool done() const { return MODE == WBOX_ANY && cnt != 0u; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (MODE == WBOX_ANY) w.occluded[i] = cnt != 0u ? 1 : 0;
        if (MODE == WBOX_COUNT) w.count[i] = cnt;
        if (MODE == WBOX_TRIS) {
            int32_t* __restrict__ row = (int32_t*)w.hits + i * L.k;
            int32_t* __restrict__ irow = w.geom + i * L.k;
            for (uint32_t s = 0; s < L.k; s++) {
                const uint64_t e = s < L.cnt ? L.key[(size_t)s * QUERY_BLOCK] : ~(uint64_t)0;   // (past count: -1 and -1)
                row[s] = (int32_t)(uint32_t)e;
                irow[s] = (int32_t)(uint32_t)(e >> 32);
            }
            w.count[i] = L.cnt;
        }
    }
};

}  // namespace

// WorldArgs: rays = the boxes (psm_box_query: lo.xyz pad | hi.xyz pad, where a ray's two float4 are); occluded / count = the
// output of the kind; the triangles query: hits = its int32 [n][k] triangle rows, geom its [n][k] instance rows, count its
// counts, samples = k (the launch gives k x 64 x 8 B of dynamic LDS beside the stack). 128 VGPRs, as world.hip's kernels.
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_box_any(WorldArgs w) {
    WorldBoxBody<WBOX_ANY> q(w, nullptr, 0u);
    world_walk(w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_box_count(WorldArgs w) {
    WorldBoxBody<WBOX_COUNT> q(w, nullptr, 0u);
    world_walk(w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_box_tris(WorldArgs w) {
    WorldBoxBody<WBOX_TRIS> q(w, key_column(), w.samples);
    world_walk(w, q);
}

// world.hip's host path (world_query(): the checks, the stale refusal, the stack area, the grid) launches through this. mode:
// 0 overlaps, 1 count, 2 triangles (a.samples = k, 1 .. PSM_QUERY_K_MAX: the list's LDS is the launch's)
int world_box_launch(psm_ctx* c, int mode, uint32_t grid, const WorldArgs& a) {
    if (mode == WBOX_ANY) world_query_box_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (mode == WBOX_COUNT) world_query_box_count<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else world_query_box_tris<<<grid, QUERY_BLOCK, (size_t)a.samples * QUERY_BLOCK * sizeof(uint64_t), c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
