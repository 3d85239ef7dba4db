// world_box.hip -- box queries over an instance world (new; no reference counterpart; include/psm_hip.h "box queries over a
// world"): whether, how many and which (instance, triangle) pairs of a world overlap an axis-aligned WORLD box.
//
// The box stays where it is and is never moved: the candidate triangle is posed forward, v0' = fwd_point(m, v0), e1' =
// fwd_vec(m, e1), e2' = fwd_vec(m, e2) (the edges are R e1 and R e2, not differences of posed vertices), and box.hip's box_tri
// (psm_box_dev.h, unchanged) decides on (v0', e1', e2', lo, hi). The walk is world.hip's (world_walk, psm_world_dev.h); a body adds
//   * the top-level test: the world box against a node's child box grown by WORLD_QSLACK |q|_inf, closed, NaN keeps;
//   * the prune inside an instance: the box's image in the hierarchy's normalised space as an interval per axis under
//     N = M_build [R^T | -R^T T], evaluated on the box shifted by -T and grown by the margin of WorldBoxPrune::enter_row;
//   * for the triangles query the list of the k lowest (instance, triangle) that count (psm_world_box_list.h).
// No result depends on the order of the walk: a flag, a sum, the k lowest pairs. The order keys are 0.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"   // world_walk, WorldArgs, load_row / load_pose, WORLD_QSLACK
#include "psm_box_dev.h"     // box_tri, box_row
#include "psm_world_box_dev.h"   // fwd_point, fwd_vec, WorldBoxPrune: the top-level test and the prune inside an instance

#define PSM_WORLD_BOX_LIST_FN PSM_D
#include "psm_world_box_list.h"

namespace psm {

namespace {

// a lane's column of the wave's key list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint64_t* key_column() {
    extern __shared__ uint64_t world_box_keys[];
    return world_box_keys + threadIdx.x;
}

enum { WBOX_ANY = 0, WBOX_COUNT = 1, WBOX_TRIS = 2 };

// MODE: what is kept of the candidates that count -- a flag (the walk ends at the first), their number, the k lowest pairs
template <int MODE>
struct WorldBoxBody : WorldBoxPrune {
    const WorldArgs& w;
    WorldBoxList<QUERY_BLOCK> L;
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
    // the top-level test, the intervals of the prune and the prune itself: WorldBoxPrune's (psm_world_box_dev.h)
    PSM_D int enter(int in) {
        const RowLoad r = enter_row(w, in);
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;   // -2: no tree (0 or 1 leaves)
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
