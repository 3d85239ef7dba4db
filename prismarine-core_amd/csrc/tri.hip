// tri.hip -- triangle queries against a built hierarchy (new; no reference counterpart; include/psm_hip.h "triangle queries",
// DESIGN.md 4.19): whether, how many and which of the hierarchy's triangles meet a given triangle.
//
// The walk is query.hip's (query_walk, psm_query_dev.h): one query per lane, one wave64 per workgroup, grid-stride, the stack
// [depth][lane] in LDS with its tail in the context's spill area. The body is box.hip's with another candidate test: tri_tri
// (psm_tri_dev.h: 20 separating axes, multiplications, additions, subtractions and compares only), the box family's prune on
// the query triangle's bounding box (box_row: its image in the build's normalised space as an interval per axis, grown by h)
// and, for the triangles query, the list of the k lowest ids that count (psm_box_list.h). No result depends on the order of the
// walk: a flag, a sum, the k lowest ids. The order keys are 0: the left child first.
// What belongs to the query alone in real numbers (its edges and normal) is defined relative to each candidate's v0
// (g1 = B - A with A = a - v0, ...) and is computed per leaf: the lane carries the nine coordinates and the six prune bounds.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_tri_dev.h"   // tri_tri; box_row through psm_box_dev.h

#define PSM_BOX_LIST_FN PSM_D
#include "psm_box_list.h"

namespace psm {

namespace {

// a lane's column of the wave's id list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint32_t* tri_id_column() {
    extern __shared__ uint32_t tri_ids[];
    return tri_ids + threadIdx.x;
}

enum { TRI_ANY = 0, TRI_COUNT = 1, TRI_TRIS = 2 };

// Waves per SIMD the kernels are bounded for: the body carries nine query coordinates more than the box body
// and a 20-axis test, and does not fit the box kernels' 64 registers without scratch. The flag and the count kernel take 70 (72
// allocated: 7 waves), the list kernel 80 (6 waves); the bounds ask for exactly that and force nothing.
constexpr int TRI_WAVES = 7, TRI_LIST_WAVES = 6;

// MODE: what is kept of the candidates that count -- a flag (the walk ends at the first), their number, the k lowest ids
template <int MODE>
struct TriBody {
    const QueryArgs& a;
    BoxIdList<QUERY_BLOCK> L;
    v3 qa, qb, qc;
    float glx, gly, glz, ghx, ghy, ghz;   // the grown image interval of the query's bounding box per normalised axis
    uint32_t cnt;

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
        if (alive) { r0 = a.rays[3 * i]; r1 = a.rays[3 * i + 1]; r2 = a.rays[3 * i + 2]; }
        qa = mk3(r0.x, r0.y, r0.z);
        qb = mk3(r1.x, r1.y, r1.z);
        qc = mk3(r2.x, r2.y, r2.z);
        const bool valid = alive && finite3(qa) && finite3(qb) && finite3(qc);
        cnt = 0u;
        L.clear();   // per query: the grid-stride loop comes here again
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
        if (!tri_tri(mk3(A.x, A.y, A.z), mk3(B.x, B.y, B.z), mk3(C.x, C.y, C.z), qa, qb, qc)) return;
        if (MODE == TRI_TRIS) L.offer((uint32_t)tri);
        else cnt++;
    }
    PSM_D bool done() const { return MODE == TRI_ANY && cnt != 0u; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (MODE == TRI_ANY) a.occluded[i] = cnt != 0u ? 1 : 0;
        if (MODE == TRI_COUNT) a.count[i] = cnt;
        if (MODE == TRI_TRIS) {
            int32_t* __restrict__ row = (int32_t*)a.hits + i * L.k;
            for (uint32_t s = 0; s < L.k; s++) row[s] = s < L.cnt ? (int32_t)L.id[(size_t)s * QUERY_BLOCK] : -1;
            a.count[i] = L.cnt;
        }
    }
};

}  // namespace

// QueryArgs: rays = the query triangles (psm_tri_query: a.xyz pad | b.xyz pad | c.xyz pad, three float4 per query); occluded /
// count / hits = the output of the kind (hits: the int32 [n][k] rows of the triangles query, count its counts); samples = k.
__global__ __launch_bounds__(QUERY_BLOCK, TRI_WAVES) void bvh_query_tri_any(QueryArgs a) {
    TriBody<TRI_ANY> q{a, BoxIdList<QUERY_BLOCK>(nullptr, 0u)};
    query_walk(a, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, TRI_WAVES) void bvh_query_tri_count(QueryArgs a) {
    TriBody<TRI_COUNT> q{a, BoxIdList<QUERY_BLOCK>(nullptr, 0u)};
    query_walk(a, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, TRI_LIST_WAVES) void bvh_query_tri_tris(QueryArgs a) {
    TriBody<TRI_TRIS> q{a, BoxIdList<QUERY_BLOCK>(tri_id_column(), a.samples)};
    query_walk(a, q);
}

// query.hip's host path (query(): the checks, the stack area, the grid) launches through this. mode: 0 overlaps, 1 count,
// 2 triangles (a.samples = k, 1 .. PSM_QUERY_K_MAX: the list's LDS is the launch's)
int tri_launch(psm_ctx* c, int mode, uint32_t grid, const QueryArgs& a) {
    if (mode == TRI_ANY) bvh_query_tri_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (mode == TRI_COUNT) bvh_query_tri_count<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else bvh_query_tri_tris<<<grid, QUERY_BLOCK, (size_t)a.samples * QUERY_BLOCK * sizeof(uint32_t), c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
