// world_tri.hip -- triangle queries over an instance world (new; no reference counterpart; include/psm_hip.h "triangle queries
// over a world"): whether, how many and which (instance, triangle) pairs of a world meet a WORLD triangle.
//
// The query triangle stays where it is and is never moved: the candidate triangle is posed forward, v0' = fwd_point(m, v0), e1' =
// fwd_vec(m, e1), e2' = fwd_vec(m, e2) (the edges are R e1 and R e2, not differences of posed vertices), and tri.hip's tri_tri
// (psm_tri_dev.h, unchanged) decides on (v0', e1', e2', a, b, c). The walk is world.hip's (world_walk, psm_world_dev.h); the body
// is world_box.hip's with another candidate test: both of WorldBoxPrune's tests (psm_world_box_dev.h: the top-level test and the
// prune inside an instance, with the same constants) run on the query's bounding box [min(a, b, c), max(a, b, c)], taken by
// selections and therefore exact -- tri_tri's three unit axes are box_tri's unit axes for that box, so the chain
// of 4.16 that no candidate that counts is cut carries over (4.20 states it) -- and the triangles query keeps the k lowest
// (instance, triangle) in world_box.hip's key list (psm_world_box_list.h). No result depends on the order of the walk: a flag, a
// sum, the k lowest pairs. The order keys are 0.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"       // world_walk, WorldArgs, load_pose
#include "psm_world_box_dev.h"   // fwd_point, fwd_vec, absmax3, WorldBoxPrune
#include "psm_tri_dev.h"         // tri_tri, tri_min3 / tri_max3

#define PSM_WORLD_BOX_LIST_FN PSM_D
#include "psm_world_box_list.h"

namespace psm {

namespace {

// a lane's column of the wave's key list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint64_t* tri_key_column() {
    extern __shared__ uint64_t world_tri_keys[];
    return world_tri_keys + threadIdx.x;
}

enum { WTRI_ANY = 0, WTRI_COUNT = 1, WTRI_TRIS = 2 };

// Waves per SIMD the kernels are bounded for: 128 VGPRs, as world_box.hip's and world.hip's kernels (DESIGN.md 4.20 has the
// counts as compiled; nothing spills)
constexpr int WORLD_TRI_WAVES = 4;

// MODE: what is kept of the candidates that count -- a flag (the walk ends at the first), their number, the k lowest pairs
template <int MODE>
struct WorldTriBody : WorldBoxPrune {
    const WorldArgs& w;
    WorldBoxList<QUERY_BLOCK> L;
    v3 qa, qb, qc;         // the world triangle; WorldBoxPrune's lo, hi are its bounding box
    uint32_t cnt;

    PSM_D WorldTriBody(const WorldArgs& a, uint64_t* keys, uint32_t slots) : w(a), L(keys, slots) {}

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
        if (alive) { r0 = w.rays[3 * i]; r1 = w.rays[3 * i + 1]; r2 = w.rays[3 * i + 2]; }
        qa = mk3(r0.x, r0.y, r0.z);
        qb = mk3(r1.x, r1.y, r1.z);
        qc = mk3(r2.x, r2.y, r2.z);
        // the bounding box, exact: selections of the coordinates
        lo = mk3(tri_min3(qa.x, qb.x, qc.x), tri_min3(qa.y, qb.y, qc.y), tri_min3(qa.z, qb.z, qc.z));
        hi = mk3(tri_max3(qa.x, qb.x, qc.x), tri_max3(qa.y, qb.y, qc.y), tri_max3(qa.z, qb.z, qc.z));
        qmax = smaxf(absmax3(lo), absmax3(hi));   // the largest |coordinate| of the nine
        cnt = 0u;
        L.clear();   // per query: the grid-stride loop comes here again
        return alive && finite3(qa) && finite3(qb) && finite3(qc);
    }
    // the top-level test, the intervals of the prune and the prune itself: WorldBoxPrune's on the bounding box
    PSM_D int enter(int in) {
        const RowLoad r = enter_row(w, in);
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;   // -2: no tree (0 or 1 leaves)
    }
    // the triangle posed forward (the pose re-read: 12 floats are not kept live over the walk), then 4.19's test, unchanged
    PSM_D void leaf(int tri) {
        float m[12];
        (void)load_pose(w, (uint32_t)inst, m);
        const float4 A = tri48[(size_t)3 * tri + 0], B = tri48[(size_t)3 * tri + 1], C = tri48[(size_t)3 * tri + 2];
        const v3 v0 = fwd_point(m, mk3(A.x, A.y, A.z)), e1 = fwd_vec(m, mk3(B.x, B.y, B.z)), e2 = fwd_vec(m, mk3(C.x, C.y, C.z));
        if (!tri_tri(v0, e1, e2, qa, qb, qc)) return;
        if (MODE == WTRI_TRIS) L.offer((uint32_t)inst, (uint32_t)tri);
        else cnt++;
    }
    PSM_D bool done() const { return MODE == WTRI_ANY && cnt != 0u; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (MODE == WTRI_ANY) w.occluded[i] = cnt != 0u ? 1 : 0;
        if (MODE == WTRI_COUNT) w.count[i] = cnt;
        if (MODE == WTRI_TRIS) {
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

// WorldArgs: rays = the query triangles (psm_tri_query: a.xyz pad | b.xyz pad | c.xyz pad, three float4 per query); occluded /
// count = the output of the kind; the triangles query: hits = its int32 [n][k] triangle rows, geom its [n][k] instance rows,
// count its counts, samples = k (the launch gives k x 64 x 8 B of dynamic LDS beside the stack).
__global__ __launch_bounds__(QUERY_BLOCK, WORLD_TRI_WAVES) void world_query_tri_any(WorldArgs w) {
    WorldTriBody<WTRI_ANY> q(w, nullptr, 0u);
    world_walk(w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, WORLD_TRI_WAVES) void world_query_tri_count(WorldArgs w) {
    WorldTriBody<WTRI_COUNT> q(w, nullptr, 0u);
    world_walk(w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, WORLD_TRI_WAVES) void world_query_tri_tris(WorldArgs w) {
    WorldTriBody<WTRI_TRIS> q(w, tri_key_column(), w.samples);
    world_walk(w, q);
}

// world.hip's host path (world_query(): the checks, the stale refusal, the stack area, the grid) launches through this. mode:
// 0 overlaps, 1 count, 2 triangles (a.samples = k, 1 .. PSM_QUERY_K_MAX: the list's LDS is the launch's)
int world_tri_launch(psm_ctx* c, int mode, uint32_t grid, const WorldArgs& a) {
    if (mode == WTRI_ANY) world_query_tri_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (mode == WTRI_COUNT) world_query_tri_count<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else world_query_tri_tris<<<grid, QUERY_BLOCK, (size_t)a.samples * QUERY_BLOCK * sizeof(uint64_t), c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
