// world_tri_dist.hip -- clearance queries over an instance world (new; no reference counterpart; include/psm_hip.h "clearance
// queries over a world"): which (instance, triangle) pair of a world is nearest to a WORLD triangle, how far and
// at which two points (world_query_tri_closest), and whether any is within a radius (world_query_tri_within).
//
// The query triangle stays where it is and is never moved, as in world_tri.hip: the candidate is posed forward, v0' =
// fwd_point(m, v0), e1' = fwd_vec(m, e1), e2' = fwd_vec(m, e2), and tri_dist (psm_tri_dist_dev.h, unchanged) judges (v0', e1',
// e2', a, b, c) -- so dist == 0 exactly where world_tri.hip's tri_tri counts the pair. The walk is world.hip's (world_walk); the
// body joins WorldBoxPrune's intervals of the query's bounding box (psm_world_box_dev.h: enter_row, the same constants) with
// tri_dist.hip's bound (tri_dist_lb2 on point_bound of the instance's fit matrix) and world.hip's point queries' top-level test
// with the bounding box where the point was. Both levels compare a lower bound with best (1 + WORLD_PSLACK); DESIGN.md 4.25
// has the chain that no pair that counts is cut. The result does not depend on the order of the walk: the smallest float32 d2,
// on a bit-equal d2 the lexicographically lowest (instance, triangle) (WorldBest::wins); a flag.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"       // world_walk, WorldArgs, load_pose, WorldBest
#include "psm_world_box_dev.h"   // fwd_point, fwd_vec, absmax3, WorldBoxPrune
#include "psm_tri_dist_dev.h"    // tri_dist, tri_dist_lb2; tri_min3 / tri_max3 through psm_tri_dev.h

namespace psm {

namespace {

// Waves per SIMD the kernels are bounded for (DESIGN.md 4.25 has the table as compiled): what the bodies take unforced -- the
// closest kernel 142 registers (3 waves; held to 4 it spills 16 to scratch), the within kernel 171 (2 waves; held to 3, 168
// registers, it spills 4). The bodies carry the row pointers, the instance, the world box and a per-lane PointBound beside
// what tri_dist.hip's carry. The bounds ask for exactly that and force nothing.
constexpr int WORLD_TRI_DIST_WAVES = 3, WORLD_TRI_DIST_WITHIN_WAVES = 2;

template <bool WITHIN>
struct WorldTriDistBody : WorldBoxPrune {
    const WorldArgs& w;
    PointBound B;          // of the fit matrix of the instance the lane is in
    v3 qa, qb, qc;         // the world triangle; WorldBoxPrune's lo, hi are its bounding box
    float rmax, bs, bt;
    WorldBest b;           // best: the pruning bound -- the best d2 so far, the rmax bound until one is found
    bool found;

    PSM_D WorldTriDistBody(const WorldArgs& a) : w(a) {}

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, -1.f), r1 = make_float4(0.f, 0.f, 0.f, 0.f), r2 = r1;   // a dead lane: rmax < 0
        if (alive) { r0 = w.rays[3 * i]; r1 = w.rays[3 * i + 1]; r2 = w.rays[3 * i + 2]; }
        qa = mk3(r0.x, r0.y, r0.z);
        qb = mk3(r1.x, r1.y, r1.z);
        qc = mk3(r2.x, r2.y, r2.z);
        rmax = r0.w;
        // the bounding box, exact: selections of the coordinates
        lo = mk3(tri_min3(qa.x, qb.x, qc.x), tri_min3(qa.y, qb.y, qc.y), tri_min3(qa.z, qb.z, qc.z));
        hi = mk3(tri_max3(qa.x, qb.x, qc.x), tri_max3(qa.y, qb.y, qc.y), tri_max3(qa.z, qb.z, qc.z));
        qmax = smaxf(absmax3(lo), absmax3(hi));   // the largest |coordinate| of the nine
        b.clear((rmax * rmax) * 1.00000095367431640625f + 0x1p-126f);   // fl(rmax^2) (1 + 2^-20) + 2^-126 (tri_dist.hip)
        bs = 0.f; bt = 0.f;   // per query: the grid-stride loop comes here again
        found = false;
        return alive && finite3(qa) && finite3(qb) && finite3(qc) && rmax >= 0.f;   // NaN or negative rmax: a miss
    }
    // a record at d2 == 0 is held: only a lexicographically lower pair, also at 0, can replace it
    PSM_D bool settled() const { return !WITHIN && found && b.best == 0.f; }
    // the squared gap between the bounding box and a top-level child box grown by the query's slack: WorldPointBody::gap2 with
    // [lo, hi] where the point was (a NaN term is taken as 0 by smaxf; an instance without triangles has an infinite gap)
    PSM_D float gap2(float lx, float ly, float lz, float hx, float hy, float hz) const {
        const float pad = WORLD_QSLACK * qmax;
        const float tx = smaxf(smaxf((lx - pad) - hi.x, lo.x - (hx + pad)), 0.f);
        const float ty = smaxf(smaxf((ly - pad) - hi.y, lo.y - (hy + pad)), 0.f);
        const float tz = smaxf(smaxf((lz - pad) - hi.z, lo.z - (hz + pad)), 0.f);
        return (tx * tx + ty * ty) + tz * tz;
    }
    // kept iff the gap is not above best (1 + WORLD_PSLACK) (negations: a NaN keeps the box); the order key is the gap
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = gap2(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y);
        kR = gap2(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w);
        const float lim = b.best + WORLD_PSLACK * b.best;
        okL = !(kL > lim);
        okR = !(kR > lim);
    }
    // the row and the grown image intervals (WorldBoxPrune), the bound of that instance's fit matrix, the lone leaf
    PSM_D int enter(int in) {
        if (settled() && (uint32_t)in > (uint32_t)b.binst) return -1;   // (no pair of it can replace the record)
        const RowLoad r = enter_row(w, in);
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(r.sm[SM_M + k]);
        B = point_bound(M);
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;   // -2: no tree (0 or 1 leaves)
    }
    // tri_dist.hip's LB^2 on the gaps between a child's fp16 box and the grown intervals; kept iff LB^2 <= best (1 +
    // WORLD_PSLACK) (<=: a pair as near as the best and lexicographically lower still counts); the order key is LB^2
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = tri_dist_lb2(B, glx, gly, glz, ghx, ghy, ghz, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        kR = tri_dist_lb2(B, glx, gly, glz, ghx, ghy, ghz, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        const float lim = b.best + WORLD_PSLACK * b.best;
        okL = kL <= lim;
        okR = kR <= lim;
    }
    // the triangle posed forward (the pose re-read: 12 floats are not kept live over the walk), then tri_dist, unchanged. Once a
    // pair at d2 == 0 is held a higher pair is not tested at all (tri_dist.hip's shortcut with (instance, triangle) for the id)
    PSM_D void leaf(int tri) {
        if (settled() && !((uint32_t)inst < (uint32_t)b.binst || (inst == b.binst && (uint32_t)tri < (uint32_t)b.btri))) return;
        float m[12];
        (void)load_pose(w, (uint32_t)inst, m);
        const float4 A = tri48[(size_t)3 * tri + 0], Bv = tri48[(size_t)3 * tri + 1], C = tri48[(size_t)3 * tri + 2];
        const v3 v0 = fwd_point(m, mk3(A.x, A.y, A.z)), e1 = fwd_vec(m, mk3(Bv.x, Bv.y, Bv.z)), e2 = fwd_vec(m, mk3(C.x, C.y, C.z));
        const TriDist d = tri_dist(v0, e1, e2, qa, qb, qc);
        if (sqrtf(d.d2) <= rmax && b.wins(d.d2, inst, tri)) {
            found = true;
            if (!WITHIN) { b.take(d.d2, d.u, d.v, inst, tri); bs = d.s; bt = d.t; }
        }
    }
    PSM_D bool done() const { return WITHIN && found; }   // within: the lane retires at its first counting candidate
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (WITHIN) {
            w.occluded[i] = found ? 1 : 0;
        } else {   // psm_tri_hit: two float4 stores, and the instance
            w.hits[2 * i] = found ? make_float4(b.bu, b.bv, sqrtf(b.best), __int_as_float(b.btri)) : miss_hit();
            w.hits[2 * i + 1] = make_float4(bs, bt, 0.f, 0.f);
            w.geom[i] = b.binst;
        }
    }
};

}  // namespace

// WorldArgs: rays = the query triangles (psm_tri_dist_query: a.xyz rmax | b.xyz pad | c.xyz pad, three float4 per query);
// hits = psm_tri_hit per query (hits[2 i], hits[2 i + 1]) and geom = the instance / occluded = the flag
__global__ __launch_bounds__(QUERY_BLOCK, WORLD_TRI_DIST_WAVES) void world_query_tri_closest(WorldArgs w) {
    WorldTriDistBody<false> q(w);
    world_walk(w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, WORLD_TRI_DIST_WITHIN_WAVES) void world_query_tri_within(WorldArgs w) {
    WorldTriDistBody<true> q(w);
    world_walk(w, q);
}

// an empty world's answer to the closest query: every record a miss, every instance -1
__global__ __launch_bounds__(256) void world_tri_dist_fill_miss(float4* hits, int32_t* geom, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    hits[2 * i] = make_float4(0.f, 0.f, __builtin_inff(), __int_as_float(-1));
    hits[2 * i + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
    geom[i] = -1;
}

// world.hip's host path (world_query(): the checks, the stale refusal, the stack area, the grid) launches through this. A world
// without instances (a.rows == NULL; the closest query alone comes here with one): the miss records, no walk
int world_tri_dist_launch(psm_ctx* c, bool within, uint32_t grid, const WorldArgs& a) {
    if (!a.rows) world_tri_dist_fill_miss<<<(unsigned)((a.n + 255) / 256), 256, 0, c->stream>>>(a.hits, a.geom, a.n);
    else if (within) world_query_tri_within<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else world_query_tri_closest<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
