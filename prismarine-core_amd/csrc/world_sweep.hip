// world_sweep.hip -- sphere sweeps over an instance world (new; no reference counterpart; include/psm_hip.h "sweep queries over a
// world"): where a sphere that moves along a WORLD line first touches a triangle of a posed instance, and on
// which instance and triangle.
//
// The sweep is moved into each instance it enters as a world ray is (WorldRay::enter_ray: o' = inst_point(m, origin), d' =
// normalize3(inst_rotate(m, direct)), the origin and direction as given, re-read from memory); radius and tmax are unchanged,
// poses are rigid. The candidate test is sweep.hip's sweep_tri (psm_sweep_dev.h) on (o', d', radius), unchanged. The walk is
// world.hip's (world_walk, psm_world_dev.h); a body adds
//   * the top-level test: the world ray's slab test (WorldRay::top_boxes) with every instance box grown by
//     G = WORLD_QSLACK |origin|_inf + radius (1 + 2^-11) in the place of the query's pad alone, against [0, limit];
//   * the prune inside an instance: sweep.hip's, the slab test in the build's normalised space with every box grown by the image
//     of the sphere (sweep_axis on the moved sweep);
//   * the best record of a world (WorldBest): the smallest t, on a bit-equal t the lowest (instance, triangle).
// Nothing depends on the order of the walk.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"   // world_walk, WorldArgs, load_row, WorldBest, WorldRay, the WORLD_* slacks
#include "psm_sweep_dev.h"   // sweep_tri, sweep_axis

namespace psm {

namespace {

// the first contact (ANY = false) and whether there is one (ANY = true); psm_sweep_query in world space. WorldRay's o, d are the
// moved sweep of the instance the lane is in, X, Y, Z its sweep_axis axes; its wo, wiv are the world line, its qpad is G.
template <bool ANY>
struct WorldSweepBody : WorldRay {
    const WorldArgs& w;
    WorldBest b;
    float r;
    bool found, alive;
    size_t idx;

    PSM_D WorldSweepBody(const WorldArgs& a) : w(a) {}
    PSM_D void sweep(float4& r0, float4& r1) const {
        r0 = make_float4(0.f, 0.f, 0.f, -1.f);   // a dead lane: a negative radius
        r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = w.rays[2 * idx]; r1 = w.rays[2 * idx + 1]; }
    }
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        float4 r0, r1;
        sweep(r0, r1);
        const v3 orig = mk3(r0.x, r0.y, r0.z);
        r = r0.w;
        tmin = 0.f;
        tmax = r1.w;
        const v3 dir = mk3(r1.x, r1.y, r1.z);
        world_ray(orig, dir);
        // the growth of the top-level test: the query's pad and the sphere (DESIGN.md 4.18 has the chain)
        qpad = qpad + r * 1.00048828125f;
        b.clear(tmax);
        found = false;
        // SweepBody::begin's rule on the world sweep: NaN anywhere, a zero direction (normalize3 gives NaN), a negative or
        // infinite radius, a negative tmax: a miss. (A direction whose length overflows normalises to 0: valid, a sphere that
        // does not move, and world_ray's nocull keeps every box for it.)
        return al && finite3(orig) && finite3(normalize3(dir)) && r >= 0.f && r < __builtin_inff() && tmax >= 0.f;
    }
    // an instance box, grown by G, is kept iff the centre's world line is inside it somewhere in [0, limit], slackened: limit
    // is tmax, lowered to the best t so far (an object-space value: equal to the world one to 1.5e-5)
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& nL, float& nR) const {
        top_boxes(w0, w1, w2, ANY ? tmax : b.best, okL, okR, nL, nR);
    }
    // the sweep (re-read: origin and direction as given, not the normalised world direction) moved as enter_ray moves a ray,
    // then sweep.hip's axes; the lone leaf of a one-leaf hierarchy is tested here
    PSM_D int enter(int in) {
        float4 r0, r1;
        sweep(r0, r1);
        const RowLoad row = load_row(w, in, *this);
        o = inst_point(row.m, mk3(r0.x, r0.y, r0.z));
        d = normalize3(inst_rotate(row.m, mk3(r1.x, r1.y, r1.z)));
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(row.sm[SM_M + k]);
        X = sweep_axis(M, 0, o, d, r);
        Y = sweep_axis(M, 1, o, d, r);
        Z = sweep_axis(M, 2, o, d, r);
        if (!(finite3(o) && finite3(d))) return -1;   // the moved sweep is invalid in this instance: skipped
        if (row.sm[SM_COUNT] == 1u) leaf(row.sorted_tri[0]);
        const int root = (int)row.sm[SM_ROOT];
        return root >= 0 ? root : -2;   // -2: valid here, no tree (0 or 1 leaves)
    }
    // SweepBody::children: a child box, grown, is kept iff the centre's line is inside it somewhere in [0, limit] (<=: an equal
    // contact of a lower (instance, triangle) still counts). Negations: a NaN keeps the box. The order key is tNear.
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        psm::slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        psm::slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        const float lim = ANY ? tmax : b.best;
        okL = !(nL > fL) & !(nL > lim) & !(fL < 0.f);
        okR = !(nR > fR) & !(nR > lim) & !(fR < 0.f);
    }
    // a candidate: a contact within tmax, and (first contact) before the best so far or as early and of a lower (instance,
    // triangle) (no record: binst = btri = -1, the largest as unsigned, so a first contact at tmax counts; t = +inf is none)
    PSM_D void leaf(int tri) {
        const float4 A = tri48[(size_t)3 * tri + 0], B = tri48[(size_t)3 * tri + 1], C = tri48[(size_t)3 * tri + 2];
        const SweepHit h = sweep_tri(mk3(A.x, A.y, A.z), mk3(B.x, B.y, B.z), mk3(C.x, C.y, C.z), o, d, r);
        if (h.t < __builtin_inff() && b.wins(h.t, inst, tri)) {
            found = true;
            if (!ANY) b.take(h.t, h.u, h.v, inst, tri);
        }
    }
    PSM_D bool done() const { return ANY && found; }   // occluded: the lane retires at its first contact
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (ANY) {
            w.occluded[i] = found ? 1 : 0;
        } else {
            w.hits[i] = found ? make_float4(b.bu, b.bv, b.best, __int_as_float(b.btri)) : miss_hit();
            w.geom[i] = b.binst;
        }
    }
};

}  // namespace

// WorldArgs: rays = the sweeps (psm_sweep_query: origin.xyz radius | direct.xyz tmax, where a ray's two float4 are); hits and
// geom / occluded = the output of the kind. 128 VGPRs, as world.hip's kernels (DESIGN.md 4.18 has the counts).
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_sweep(WorldArgs w) {
    WorldSweepBody<false> q(w);
    world_walk(w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_sweep_any(WorldArgs w) {
    WorldSweepBody<true> q(w);
    world_walk(w, q);
}

// world.hip's host path (world_query(): the checks, the empty world, the stale refusal, the stack area, the grid) launches
// through this
int world_sweep_launch(psm_ctx* c, bool any, uint32_t grid, const WorldArgs& a) {
    if (any) world_query_sweep_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else world_query_sweep<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
