// tri_dist.hip -- clearance queries against a built hierarchy (new; no reference counterpart; include/psm_hip.h "clearance
// queries"): which of the hierarchy's triangles is nearest to a given triangle, how far and at which two points
// (bvh_query_tri_closest), and whether any is within a radius (bvh_query_tri_within).
//
// The walk is query.hip's (query_walk, psm_query_dev.h): one query per lane, one wave64 per workgroup, grid-stride, the stack
// [depth][lane] in LDS with its tail in the context's spill area. The body is the point queries' with another candidate test
// and the query's bounding box in place of the point: tri_dist (psm_tri_dist_dev.h: fifteen features and tri_tri), the prune
// by point_bound on the gaps between a child box and the box's image interval per normalised axis (box_row, as tri.hip's
// begin() takes it), the children ordered by LB^2. The result does not depend on the order of the walk: the smallest d2, on a
// bit-equal d2 the lowest id; a flag.
// The lane carries the nine coordinates, the six interval bounds, the best d2 and the winner's four weights and id; the
// query's edges are formed per leaf, relative to the candidate's v0, as in tri.hip.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_tri_dist_dev.h"   // tri_dist; tri_min3 / tri_max3 and box_row through psm_tri_dev.h

namespace psm {

namespace {

// Waves per SIMD the kernels are bounded for (DESIGN.md 4.23 has the table): what the bodies take unforced -- the closest kernel
// 113 registers (4 waves), the within kernel, whose fifteen features carry no weights and are scheduled side by side, 143
// (3 waves; held to 4 waves it spills 21 registers to scratch). The bounds ask for exactly that and force nothing.
constexpr int TRI_DIST_WAVES = 4, TRI_DIST_WITHIN_WAVES = 3;

template <bool WITHIN>
struct TriDistBody {
    const QueryArgs& a;
    const PointBound B;
    v3 qa, qb, qc;
    float glx, gly, glz, ghx, ghy, ghz;   // the grown image interval of the query's bounding box per normalised axis
    float rmax, best, bu, bv, bs, bt;     // best: the pruning bound -- the best d2 so far, the rmax bound until one is found
    int btri;
    bool found;

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, -1.f), r1 = make_float4(0.f, 0.f, 0.f, 0.f), r2 = r1;   // a dead lane: rmax < 0
        if (alive) { r0 = a.rays[3 * i]; r1 = a.rays[3 * i + 1]; r2 = a.rays[3 * i + 2]; }
        qa = mk3(r0.x, r0.y, r0.z);
        qb = mk3(r1.x, r1.y, r1.z);
        qc = mk3(r2.x, r2.y, r2.z);
        rmax = r0.w;
        const bool valid = alive && finite3(qa) && finite3(qb) && finite3(qc) && rmax >= 0.f;   // NaN or negative rmax: a miss
        best = (rmax * rmax) * 1.00000095367431640625f + 0x1p-126f;   // fl(rmax^2) (1 + 2^-20) + 2^-126
        bu = 0.f; bv = 0.f; bs = 0.f; bt = 0.f;   // per query: the grid-stride loop comes here again
        btri = -1;
        found = false;
        // the bounding box, exact: selections of the coordinates
        const v3 lo = mk3(tri_min3(qa.x, qb.x, qc.x), tri_min3(qa.y, qb.y, qc.y), tri_min3(qa.z, qb.z, qc.z));
        const v3 hi = mk3(tri_max3(qa.x, qb.x, qc.x), tri_max3(qa.y, qb.y, qc.y), tri_max3(qa.z, qb.z, qc.z));
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        box_row(M, 0, lo, hi, glx, ghx);
        box_row(M, 1, lo, hi, gly, ghy);
        box_row(M, 2, lo, hi, glz, ghz);
        return valid;
    }
    // LB^2 of one child box (mn / mx: its fp16 corners): tri_dist_lb2 (psm_tri_dist_dev.h) on this query's intervals
    PSM_D float lb2(float mnx, float mny, float mnz, float mxx, float mxy, float mxz) const {
        return tri_dist_lb2(B, glx, gly, glz, ghx, ghy, ghz, mnx, mny, mnz, mxx, mxy, mxz);
    }
    // kept iff LB^2 <= best (<=: a triangle as near as the best and of a lower id still counts); the order key is LB^2
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = lb2(half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        kR = lb2(half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        okL = kL <= best;
        okR = kR <= best;
    }
    // a candidate: within rmax, and (closest) nearer than the best so far or as near and of a lower id
    // ((uint32_t) btri: -1 is the largest; before the first, best is the rmax bound, >= every d2 that counts)
    // Once a triangle at d2 == 0 is held, only one at d2 == 0 AND of a lower id can replace it: a higher id is not tested at all
    // (the same record, bit for bit; a query that cuts through the mesh meets every leaf under its box, and would run the
    // fifteen features on each).
    PSM_D void leaf(int tri) {
        if (!WITHIN && found && best == 0.f && (uint32_t)tri > (uint32_t)btri) return;
        const float4 A = a.tri48[(size_t)3 * tri + 0], Bv = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        const TriDist w = tri_dist(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(C.x, C.y, C.z), qa, qb, qc);
        if (sqrtf(w.d2) <= rmax && (w.d2 < best || (w.d2 == best && (uint32_t)tri < (uint32_t)btri))) {
            found = true;
            if (!WITHIN) { best = w.d2; bu = w.u; bv = w.v; bs = w.s; bt = w.t; btri = tri; }
        }
    }
    PSM_D bool done() const { return WITHIN && found; }   // within: the lane retires at its first counting candidate
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (WITHIN) {
            a.occluded[i] = found ? 1 : 0;
        } else {   // psm_tri_hit: two float4 stores
            a.hits[2 * i] = found ? make_float4(bu, bv, sqrtf(best), __int_as_float(btri)) : miss_hit();
            a.hits[2 * i + 1] = make_float4(bs, bt, 0.f, 0.f);
        }
    }
};

template <bool WITHIN>
PSM_D void tri_dist_body(const QueryArgs& a) {
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
    TriDistBody<WITHIN> q{a, point_bound(M)};
    query_walk(a, q);
}

}  // namespace

// QueryArgs: rays = the query triangles (psm_tri_dist_query: a.xyz rmax | b.xyz pad | c.xyz pad, three float4 per query);
// hits = psm_tri_hit per query (hits[2 i], hits[2 i + 1]) / occluded = the flag
__global__ __launch_bounds__(QUERY_BLOCK, TRI_DIST_WAVES) void bvh_query_tri_closest(QueryArgs a) { tri_dist_body<false>(a); }

__global__ __launch_bounds__(QUERY_BLOCK, TRI_DIST_WITHIN_WAVES) void bvh_query_tri_within(QueryArgs a) { tri_dist_body<true>(a); }

// query.hip's host path (query(): the checks, the stack area, the grid) launches through this
int tri_dist_launch(psm_ctx* c, bool within, uint32_t grid, const QueryArgs& a) {
    if (within) bvh_query_tri_within<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else bvh_query_tri_closest<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
