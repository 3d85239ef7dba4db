// world_mesh.hip -- mesh queries over an instance world (new; no reference counterpart; include/psm_hip.h "mesh queries over a
// world"): whether, how many and which (instance, triangle) pairs of a world meet each stored triangle of ANOTHER
// built hierarchy at each of p rigid poses that take its object space into WORLD space -- the triangle queries over a world
// (world_tri.hip) with the query triangles made on the device as the mesh queries (mesh.hip) make them.
//
// Two proven halves joined, nothing restated: begin() is mesh.hip's -- query i is pose q = i / L and the other's leaf j = i % L in
// SLOT order (mesh_split: no division), the query triangle is mesh_query_tri of the stored record and the pose -- and from there
// the body is world_tri.hip's: WorldBoxPrune's two tests on the query's bounding box (selections: exact), the candidate posed
// forward and judged by tri_tri, the k lowest (instance, triangle) in WorldBoxList. The query's nine numbers are all either test
// ever sees, so 4.20's chain holds for them however they came about. Results go to [q][t], t the leaf's load-order id; the host
// path (world.hip, world_mesh_query()) clears the outputs first, so a triangle the other's build dropped reads 0 / -1.
//
// skip: the instance left out (-1: none). It is decided in enter(), where an instance is entered -- the single-leaf shortcut and
// a world of one come through there too -- and never by a filter after the test: a skipped instance costs one comparison.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"       // world_walk, WorldArgs, WorldMeshArgs, load_pose
#include "psm_world_box_dev.h"   // fwd_point, fwd_vec, absmax3, WorldBoxPrune (enter_row)
#include "psm_tri_dev.h"         // tri_tri, tri_min3 / tri_max3
#include "psm_mesh_dev.h"        // mesh_split, mesh_query_tri

#define PSM_WORLD_BOX_LIST_FN PSM_D
#include "psm_world_box_list.h"

namespace psm {

namespace {

// a lane's column of the wave's key list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint64_t* mesh_key_column() {
    extern __shared__ uint64_t world_mesh_keys[];
    return world_mesh_keys + threadIdx.x;
}

enum { WMESH_ANY = 0, WMESH_COUNT = 1, WMESH_TRIS = 2 };

// Waves per SIMD the kernels are bounded for: 128 VGPRs, as world_tri.hip's (DESIGN.md 4.22 has the counts as compiled; nothing
// spills). The output index is 32 bits wide (the host refuses p x T >= 2^32).
constexpr int WORLD_MESH_WAVES = 4;

// MODE: what is kept of the candidates that count -- a flag per pose (the walk ends at the first), their number, the k lowest pairs
template <int MODE>
struct WorldMeshBody : WorldBoxPrune {
    const WorldMeshArgs& m;
    const WorldArgs& w;
    WorldBoxList<QUERY_BLOCK> L;
    v3 qa, qb, qc;         // the query triangle in world space; WorldBoxPrune's lo, hi are its bounding box
    uint32_t cnt;
    uint32_t out;          // where the answer goes: the pose (flag), else q * T + t (below 2^32: the host checks)

    PSM_D WorldMeshBody(const WorldMeshArgs& a, uint64_t* keys, uint32_t slots) : m(a), w(a.w), L(keys, slots) {}

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, p0 = r0, p1 = r0, p2 = r0;
        uint64_t q = 0;
        uint32_t t = 0u;
        if (alive) {
            uint32_t j;
            mesh_split(i, m.L, m.magic, q, j);
            t = (uint32_t)m.leaf_tri[j];
            r0 = m.tri48[(size_t)3 * t]; r1 = m.tri48[(size_t)3 * t + 1]; r2 = m.tri48[(size_t)3 * t + 2];
            p0 = m.poses[3 * q]; p1 = m.poses[3 * q + 1]; p2 = m.poses[3 * q + 2];
        }
        out = MODE == WMESH_ANY ? (uint32_t)q : (uint32_t)q * m.T + t;
        const float pose[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
        mesh_query_tri(pose, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), mk3(r2.x, r2.y, r2.z), qa, qb, qc);
        bool valid = alive && finite3(qa) && finite3(qb) && finite3(qc);
        // the bounding box, exact: selections of the coordinates
        lo = mk3(tri_min3(qa.x, qb.x, qc.x), tri_min3(qa.y, qb.y, qc.y), tri_min3(qa.z, qb.z, qc.z));
        hi = mk3(tri_max3(qa.x, qb.x, qc.x), tri_max3(qa.y, qb.y, qc.y), tri_max3(qa.z, qb.z, qc.z));
        qmax = smaxf(absmax3(lo), absmax3(hi));   // the largest |coordinate| of the nine
        cnt = 0u;
        L.clear();   // per query: the grid-stride loop comes here again
        // The flag of a pose is the OR over its leaves and a 1 is final: a lane that reads one has nothing to add. The load is
        // atomic (relaxed): made here, at every query, never hoisted; whether it sees another wave's store changes the work only.
        if (MODE == WMESH_ANY && (m.flags & WORLD_MESH_FLAG_SKIP) && valid) valid = __atomic_load_n(w.occluded + out, __ATOMIC_RELAXED) == 0;
        return valid;
    }
    // The instance left out is never entered: neither its row nor its lone leaf is read. Otherwise world_tri.hip's enter(): the
    // top-level test, the intervals of the prune and the prune itself are WorldBoxPrune's on the bounding box
    PSM_D int enter(int in) {
        if (in == m.skip) return -1;
        const RowLoad r = enter_row(w, in);
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;   // -2: no tree (0 or 1 leaves)
    }
    // the triangle posed forward (the pose re-read: 12 floats are not kept live over the walk), then 4.19's test, unchanged
    PSM_D void leaf(int tri) {
        float p[12];
        (void)load_pose(w, (uint32_t)inst, p);
        const float4 A = tri48[(size_t)3 * tri + 0], B = tri48[(size_t)3 * tri + 1], C = tri48[(size_t)3 * tri + 2];
        const v3 v0 = fwd_point(p, mk3(A.x, A.y, A.z)), e1 = fwd_vec(p, mk3(B.x, B.y, B.z)), e2 = fwd_vec(p, mk3(C.x, C.y, C.z));
        if (!tri_tri(v0, e1, e2, qa, qb, qc)) return;
        if (MODE == WMESH_TRIS) L.offer((uint32_t)inst, (uint32_t)tri);
        else cnt++;
    }
    PSM_D bool done() const { return MODE == WMESH_ANY && cnt != 0u; }
    PSM_D bool again() const { return false; }
    // (the flag: the host path cleared it, and only a 1 is ever stored -- by as many lanes as find one, the same byte value)
    PSM_D void finish(size_t) const {
        if (MODE == WMESH_ANY) {
            if (cnt != 0u) w.occluded[out] = 1;
        }
        if (MODE == WMESH_COUNT) w.count[out] = cnt;
        if (MODE == WMESH_TRIS) {
            int32_t* __restrict__ row = (int32_t*)w.hits + (size_t)out * L.k;
            int32_t* __restrict__ irow = w.geom + (size_t)out * L.k;
            for (uint32_t s = 0; s < L.k; s++) {
                const uint64_t e = s < L.cnt ? L.key[(size_t)s * QUERY_BLOCK] : ~(uint64_t)0;   // (past count: -1 and -1)
                row[s] = (int32_t)(uint32_t)e;
                irow[s] = (int32_t)(uint32_t)(e >> 32);
            }
            w.count[out] = L.cnt;
        }
    }
};

}  // namespace

// WorldMeshArgs (psm_world_dev.h): w.n = p x L; w.occluded = the flag per pose / w.count = the counts [p][T]; the triangles
// query: w.hits = its int32 [p][T][k] triangle rows, w.geom its instance rows, w.count its counts, w.samples = k (the launch
// gives k x 64 x 8 B of dynamic LDS beside the stack). w.rays is not read.
__global__ __launch_bounds__(QUERY_BLOCK, WORLD_MESH_WAVES) void world_query_mesh_any(WorldMeshArgs m) {
    WorldMeshBody<WMESH_ANY> q(m, nullptr, 0u);
    world_walk(m.w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, WORLD_MESH_WAVES) void world_query_mesh_count(WorldMeshArgs m) {
    WorldMeshBody<WMESH_COUNT> q(m, nullptr, 0u);
    world_walk(m.w, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, WORLD_MESH_WAVES) void world_query_mesh_tris(WorldMeshArgs m) {
    WorldMeshBody<WMESH_TRIS> q(m, mesh_key_column(), m.w.samples);
    world_walk(m.w, q);
}

// world.hip's host path (world_mesh_query(): the stale refusal, the clears, the grid and, shared with the other posed-mesh
// entry points through mesh.hip, the checks and the upload) launches through this. mode: 0 overlaps, 1 count, 2 triangles
// (a.w.samples = k, 1 .. PSM_QUERY_K_MAX: the list's LDS is the launch's)
int world_mesh_launch(psm_ctx* c, int mode, uint32_t grid, WorldMeshArgs a) {
    a.magic = mesh_magic(a.L);
    if (mode == WMESH_ANY) world_query_mesh_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (mode == WMESH_COUNT) world_query_mesh_count<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else world_query_mesh_tris<<<grid, QUERY_BLOCK, (size_t)a.w.samples * QUERY_BLOCK * sizeof(uint64_t), c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
