// sweep.hip -- sphere sweeps against a built hierarchy (new; no reference counterpart; include/psm_hip.h "sweep queries",
// DESIGN.md 4.17): where a sphere that moves along a line first touches the hierarchy's triangles, and on which.
//
// The walk is query.hip's (query_walk, psm_query_dev.h): one query per lane, one wave64 per workgroup, grid-stride, the stack
// [depth][lane] in LDS with its tail in the context's spill area. A body adds the candidate test (sweep_tri, psm_sweep_dev.h:
// closest_on_tri for the start, then the face, the three vertices and the three edges by closest approach) and the prune: the
// ray queries' slab test in the build's normalised space with every box grown by the image of the sphere (sweep_axis). The
// result is the smallest t, on a bit-equal t the lowest triangle id: nothing depends on the order of the walk.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_sweep_dev.h"   // sweep_tri, sweep_axis

namespace psm {

namespace {

// the first contact (ANY = false) and whether there is one (ANY = true); psm_sweep_query
template <bool ANY>
struct SweepBody {
    const QueryArgs& a;
    v3 o, d;
    float r, tmax, best, bu, bv;
    int btri;
    bool found;
    Axis X, Y, Z;

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, -1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);   // a dead lane: a negative radius
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        o = mk3(r0.x, r0.y, r0.z);
        d = normalize3(mk3(r1.x, r1.y, r1.z));   // t is the distance along the unit direction, as a query ray's
        r = r0.w;
        tmax = r1.w;
        // NaN anywhere, a zero direction (normalize3 gives NaN), a negative or infinite radius, a negative tmax: a miss
        const bool valid = alive && finite3(o) && finite3(d) && r >= 0.f && r < __builtin_inff() && tmax >= 0.f;
        best = tmax;
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        found = false;
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        X = sweep_axis(M, 0, o, d, r);
        Y = sweep_axis(M, 1, o, d, r);
        Z = sweep_axis(M, 2, o, d, r);
        return valid;
    }
    // a child box, grown, is kept iff the centre's line is inside it somewhere in [0, limit]: limit is tmax, lowered to the
    // best t so far (<=: an equal contact of a lower id still counts). Negations: a NaN keeps the box. The order key is tNear.
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        const float lim = ANY ? tmax : best;
        okL = !(nL > fL) & !(nL > lim) & !(fL < 0.f);
        okR = !(nR > fR) & !(nR > lim) & !(fR < 0.f);
    }
    // a candidate: a contact within tmax, and (first contact) before the best so far or as early and of a lower id
    // ((uint32_t) btri: -1 is the largest, so the first contact within tmax always counts; t = +inf is no contact)
    PSM_D void leaf(int tri) {
        const float4 A = a.tri48[(size_t)3 * tri + 0], B = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        const SweepHit h = sweep_tri(mk3(A.x, A.y, A.z), mk3(B.x, B.y, B.z), mk3(C.x, C.y, C.z), o, d, r);
        if (h.t < __builtin_inff() && (h.t < best || (h.t == best && (uint32_t)tri < (uint32_t)btri))) {
            found = true;
            if (!ANY) { best = h.t; bu = h.u; bv = h.v; btri = tri; }
        }
    }
    PSM_D bool done() const { return ANY && found; }   // occluded: the lane retires at its first contact
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (ANY) a.occluded[i] = found ? 1 : 0;
        else a.hits[i] = found ? make_float4(bu, bv, best, __int_as_float(btri)) : miss_hit();
    }
};

}  // namespace

// QueryArgs: rays = the sweeps (psm_sweep_query: origin.xyz radius | direct.xyz tmax, where a ray's two float4 are); hits /
// occluded = the output of the kind.
__global__ __launch_bounds__(QUERY_BLOCK, 6) void bvh_query_sweep(QueryArgs a) {
    SweepBody<false> q{a};
    query_walk(a, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, 6) void bvh_query_sweep_any(QueryArgs a) {
    SweepBody<true> q{a};
    query_walk(a, q);
}

// query.hip's host path (query(): the checks, the stack area, the grid) launches through this
int sweep_launch(psm_ctx* c, bool any, uint32_t grid, const QueryArgs& a) {
    if (any) bvh_query_sweep_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else bvh_query_sweep<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
