// box.hip -- box queries against a built hierarchy (new; no reference counterpart; include/psm_hip.h "box queries", DESIGN.md
// 4.15): whether, how many and which of the hierarchy's triangles overlap an axis-aligned box.
//
// The walk is query.hip's (query_walk, psm_query_dev.h): one query per lane, one wave64 per workgroup, grid-stride, the stack
// [depth][lane] in LDS with its tail in the context's spill area. A body adds the candidate test (box_tri: the 13 axes of a
// triangle and a box, multiplications, additions and compares only), the prune (the box's image in the build's normalised space
// as an interval per axis, grown by h) and, for the triangles query, the list of the k lowest ids that count (psm_box_list.h).
// No result depends on the order of the walk: a flag, a sum, the k lowest ids. The order keys are 0: the left child first.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"

#define PSM_BOX_LIST_FN PSM_D
#include "psm_box_list.h"

namespace psm {

namespace {

// a lane's column of the wave's id list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint32_t* id_column() {
    extern __shared__ uint32_t box_ids[];
    return box_ids + threadIdx.x;
}

// one term of bmin(a): a >= 0 ? a L : a H (bmax: the same with L and H swapped)
PSM_D float bterm(float a, float l, float h) { return a >= 0.f ? a * l : a * h; }

// does the axis with the triangle's projections {0, p} (relative to v0) and the box's [bmin, bmax] separate them
PSM_D bool separates(float p, float bmin, float bmax) {
    const float pmx = p > 0.f ? p : 0.f, pmn = p < 0.f ? p : 0.f;
    return !(pmx >= bmin && pmn <= bmax);
}

// an edge axis unit_k x f: its two components that are not zero by construction, a1 on the axis of (l1, h1) and a2 on the axis
// of (l2, h2) in component order, and the matching components g1, g2 of the edge whose projection is the triangle's other value
PSM_D bool edge_separates(float a1, float a2, float l1, float h1, float l2, float h2, float g1, float g2) {
    const float bmin = bterm(a1, l1, h1) + bterm(a2, l2, h2);
    const float bmax = bterm(a1, h1, l1) + bterm(a2, h2, l2);
    return separates(a1 * g1 + a2 * g2, bmin, bmax);
}

// the three edge axes of f (unit_x x f, unit_y x f, unit_z x f) with g the edge that gives the projection
PSM_D bool edge_axes_separate(v3 f, v3 g, v3 L, v3 H) {
    bool sep = edge_separates(-f.z, f.y, L.y, H.y, L.z, H.z, g.y, g.z);   // (0, -fz, fy)
    sep |= edge_separates(f.z, -f.x, L.x, H.x, L.z, H.z, g.x, g.z);       // (fz, 0, -fx)
    sep |= edge_separates(-f.y, f.x, L.x, H.x, L.y, H.y, g.x, g.y);       // (-fy, fx, 0)
    return sep;
}

// a unit axis: the triangle's {0, a, b} against [l, h] directly
PSM_D bool unit_separates(float a, float b, float l, float h) {
    float pmx = a > 0.f ? a : 0.f, pmn = a < 0.f ? a : 0.f;
    pmx = b > pmx ? b : pmx;
    pmn = b < pmn ? b : pmn;
    return !(pmx >= l && pmn <= h);
}

// The candidate test (include/psm_hip.h "box queries" states it; tests/box_query_model.py restates it in numpy): triangle
// (v0, e1, e2) against the closed box [lo, hi], one float32 operation order, no division, no square root.
PSM_D bool box_tri(v3 v0, v3 e1, v3 e2, v3 lo, v3 hi) {
    const v3 L = lo - v0, H = hi - v0;
    const v3 f3 = e2 - e1;
    bool sep = unit_separates(e1.x, e2.x, L.x, H.x);
    sep |= unit_separates(e1.y, e2.y, L.y, H.y);
    sep |= unit_separates(e1.z, e2.z, L.z, H.z);
    sep |= edge_axes_separate(e1, e2, L, H);
    sep |= edge_axes_separate(e2, e1, L, H);
    sep |= edge_axes_separate(f3, e1, L, H);
    const v3 n = cross3(e1, e2);
    const float bmin = (bterm(n.x, L.x, H.x) + bterm(n.y, L.y, H.y)) + bterm(n.z, L.z, H.z);
    const float bmax = (bterm(n.x, H.x, L.x) + bterm(n.y, H.y, L.y)) + bterm(n.z, H.z, L.z);
    sep |= separates(0.f, bmin, bmax);
    return !sep;
}

// Row k of the build's affine map applied to the box [lo, hi]: the interval of the image on normalised axis k, the sums in
// affine_row's order, grown by affine_row's margin h = 2^-16 (2 + S) with S the sum of the larger magnitudes and |m3|. For a
// diagonal 3 x 3 part (the plain fit) the interval is the image; for a full one (an optimisation matrix) it is the image's
// bounding interval, which the row sums make right. DESIGN.md 4.15 has why no triangle that counts is cut.
PSM_D void box_row(const float* M, int k, v3 lo, v3 hi, float& glo, float& ghi) {
    const float m0 = M[4 * k + 0], m1 = M[4 * k + 1], m2 = M[4 * k + 2], m3 = M[4 * k + 3];
    const float ax = m0 * lo.x, bx = m0 * hi.x, ay = m1 * lo.y, by = m1 * hi.y, az = m2 * lo.z, bz = m2 * hi.z;
    const float ilo = ((sminf(ax, bx) + sminf(ay, by)) + sminf(az, bz)) + m3;
    const float ihi = ((smaxf(ax, bx) + smaxf(ay, by)) + smaxf(az, bz)) + m3;
    const float S = ((smaxf(pabs(ax), pabs(bx)) + smaxf(pabs(ay), pabs(by))) + smaxf(pabs(az), pabs(bz))) + pabs(m3);
    const float h = (2.0f + S) * 0x1p-16f;
    glo = ilo - h;
    ghi = ihi + h;
}

enum { BOX_ANY = 0, BOX_COUNT = 1, BOX_TRIS = 2 };

// MODE: what is kept of the candidates that count -- a flag (the walk ends at the first), their number, the k lowest ids
template <int MODE>
struct BoxBody {
    const QueryArgs& a;
    BoxIdList<QUERY_BLOCK> L;
    v3 lo, hi;
    float glx, gly, glz, ghx, ghy, ghz;   // the grown image interval per normalised axis
    uint32_t cnt;

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(-1.f, -1.f, -1.f, 0.f);   // a dead lane: lo > hi
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        lo = mk3(r0.x, r0.y, r0.z);
        hi = mk3(r1.x, r1.y, r1.z);
        const bool valid = alive && finite3(lo) && finite3(hi) && lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z;
        cnt = 0u;
        L.clear();   // per query: the grid-stride loop comes here again
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        box_row(M, 0, lo, hi, glx, ghx);
        box_row(M, 1, lo, hi, gly, ghy);
        box_row(M, 2, lo, hi, glz, ghz);
        return valid;
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
    // (the record's fp16 corners in the order the slab and the point tests read them: mn.xyz, mx.xyz)
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        okL = keep(half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        okR = keep(half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        kL = 0.f;
        kR = 0.f;
    }
    PSM_D void leaf(int tri) {
        const float4 A = a.tri48[(size_t)3 * tri + 0], B = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        if (!box_tri(mk3(A.x, A.y, A.z), mk3(B.x, B.y, B.z), mk3(C.x, C.y, C.z), lo, hi)) return;
        if (MODE == BOX_TRIS) L.offer((uint32_t)tri);
        else cnt++;
    }
    PSM_D bool done() const { return MODE == BOX_ANY && cnt != 0u; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (MODE == BOX_ANY) a.occluded[i] = cnt != 0u ? 1 : 0;
        if (MODE == BOX_COUNT) a.count[i] = cnt;
        if (MODE == BOX_TRIS) {
            int32_t* __restrict__ row = (int32_t*)a.hits + i * L.k;
            for (uint32_t s = 0; s < L.k; s++) row[s] = s < L.cnt ? (int32_t)L.id[(size_t)s * QUERY_BLOCK] : -1;
            a.count[i] = L.cnt;
        }
    }
};

}  // namespace

// QueryArgs: rays = the boxes (psm_box_query: lo.xyz pad | hi.xyz pad, where a ray's two float4 are); occluded / count / hits =
// the output of the kind (hits: the int32 [n][k] rows of the triangles query, count its counts); samples = k.
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_box_any(QueryArgs a) {
    BoxBody<BOX_ANY> q{a, BoxIdList<QUERY_BLOCK>(nullptr, 0u)};
    query_walk(a, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_box_count(QueryArgs a) {
    BoxBody<BOX_COUNT> q{a, BoxIdList<QUERY_BLOCK>(nullptr, 0u)};
    query_walk(a, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_box_tris(QueryArgs a) {
    BoxBody<BOX_TRIS> q{a, BoxIdList<QUERY_BLOCK>(id_column(), a.samples)};
    query_walk(a, q);
}

// query.hip's host path (query(): the checks, the stack area, the grid) launches through this. mode: 0 overlaps, 1 count,
// 2 triangles (a.samples = k, 1 .. PSM_QUERY_K_MAX: the list's LDS is the launch's)
int box_launch(psm_ctx* c, int mode, uint32_t grid, const QueryArgs& a) {
    if (mode == BOX_ANY) bvh_query_box_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (mode == BOX_COUNT) bvh_query_box_count<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else bvh_query_box_tris<<<grid, QUERY_BLOCK, (size_t)a.samples * QUERY_BLOCK * sizeof(uint32_t), c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
