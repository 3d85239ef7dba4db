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
#include "psm_box_dev.h"   // box_tri, box_row

#define PSM_BOX_LIST_FN PSM_D
#include "psm_box_list.h"

namespace psm {

namespace {

// a lane's column of the wave's id list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint32_t* id_column() {
    extern __shared__ uint32_t box_ids[];
    return box_ids + threadIdx.x;
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
