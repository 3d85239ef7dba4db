// psm_query_host.h -- the host path every query entry point shares (query.hip, world.hip): the kinds, what
// their messages call things, the data and list checks, the context's stack area, the launch. The functions are defined once,
// in query.hip; the pieces the posed-mesh calls share in mesh.hip (4.28), those of the grid calls in grid.hip (4.32), which also
// refuse through mesh_refuse / mesh_pointers / mesh_aligned. api.hip takes the declarations alone (PSM_QUERY_HOST_DECLARATIONS_ONLY): it holds no kernels, and the
// templates below need the walk's constants of psm_query_dev.h.
#pragma once
#include "psm_internal.h"

namespace psm {

void query_release(psm_ctx* c);               // query.hip, for psm_ctx_destroy: the context's stack area goes with it
void mesh_release(psm_ctx* c);                // mesh.hip, for psm_ctx_destroy: the device copy of the mesh queries' poses goes with it
void grid_release(psm_ctx* c);                // grid.hip, for psm_ctx_destroy: the solid grids' scratch goes with it
void sparse_release(psm_ctx* c);              // grid_sparse.hip, for grid_release: the sparse grids' scratch goes with it
// mesh.hip: the host pieces the twelve posed-mesh entry points share (mesh.hip, mesh_dist.hip and world.hip's two host functions;
// DESIGN.md 4.28). A check answers PSM_OK, or refuses under the entry point's name with the context's error set.
int mesh_refuse(psm_ctx* c, int code, const char* format, ...) __attribute__((format(printf, 3, 4)));   // the formatted text as the error
int mesh_pointers(psm_ctx* c, const char* name, bool all);                                               // "<name>: NULL pointer" unless all
int mesh_aligned(psm_ctx* c, const char* name, const char* what, const void* ptr, unsigned align);      // "<name>: <what> not <align>-byte aligned"
int mesh_poses_rigid(psm_ctx* c, const char* name, const float* poses, size_t p);                        // the first pose pose_fault() refuses, by index
int mesh_answers_fit(psm_ctx* c, const char* name, size_t p, uint32_t T);                                // p x T below 2^32, else PSM_ERR_CAPACITY
// The upload of a call, on the context's stream: the poses into the context's pose area (grown on demand, released by
// mesh_release), the area of one 64-bit word per pose a clearance call's lanes share (d_keys NULL: none), other's leaf count L
// back, one synchronisation for all of it; L above other's triangle count is refused
int mesh_upload(psm_ctx* c, const psm_bvh* o, const float* poses, size_t p, void** d_poses, void** d_keys, uint32_t* L);
// Whether a flag kernel's lanes skip a pose already flagged: PSM_MESH_SKIP, else whether a launch of `queries` lanes strides
bool mesh_skip(size_t queries);
// PSM_MESH_BOUND's letter for the clearance kernels' shared bound, '1' when unset
char mesh_bound();
uint64_t bvh_generation(const psm_bvh* b);    // api.hip: bumped by every build of the hierarchy

// grid.hip: the host pieces the eleven grid entry points share (grid.hip's grid_query(), grid_dist.hip's dist_query(), world.hip's
// world_grid_query() and world_grid_dist_query()). A grid as the host reads it: the bricks per axis and in all
struct GridShape {
    uint32_t nb[3];
    uint64_t bricks;
};
// Why a grid is refused, or NULL with s filled in (psm_hip.h "voxel grids": the rules in their order)
const char* grid_fault(const psm_grid* g, GridShape& s);
// The front of every grid call, PSM_OK or the refusal under the entry point's name with the context's error set: "<name>: NULL
// pointer" for a NULL grid or out, "<name>: invalid grid: <grid_fault()>" (else s is filled in), "<name>: <what> not <align>-byte
// aligned" by the bits of `aligned` (the outputs' addresses ORed), then rmax ("must be >= 0") and samples ("must be 1, 3 or 5"),
// each NULL where the call has none
int grid_front(psm_ctx* c, const char* name, const psm_grid* grid, const void* out, GridShape& s, const char* what, const void* aligned,
               unsigned align, const float* rmax, const uint32_t* samples);
// A hierarchy's state for a grid call: PSM_ERR_STATE before its first build, PSM_ERR_CAPACITY when deeper than the wave's stack
int grid_built(const psm_bvh* b);
// The slabs solid and signed work in, and the context's scratch for one slab (grown on demand, released by grid_release): the
// slab's 64 centres a brick in lane order (psm_point_query records), then solid's flags or, at the same place, signed's hits.
// Solid's slab is at most GRID_SLAB_BRICKS bricks, signed's half of that with twice the bytes a brick
constexpr uint32_t GRID_SLAB_BRICKS = 1u << 16;
struct GridSlabs {
    uint32_t slab = 0;
    float4* points = nullptr;
    float4* hits = nullptr;
    uint8_t* flags = nullptr;
};
int slabs_for(psm_ctx* c, uint64_t bricks, bool sign, GridSlabs& a);
// body(first, bricks) for each slab of at most `slab` bricks in order, until one does not answer PSM_OK
template <class Body>
int grid_slabs(uint64_t bricks, uint32_t slab, Body body) {
    for (uint64_t first = 0; first < bricks; first += slab) {
        const uint64_t left = bricks - first;
        const int rc = body((uint32_t)first, left < slab ? (uint32_t)left : slab);
        if (rc != PSM_OK) return rc;
    }
    return PSM_OK;
}
// the launches around the inside query or the sign kernel of a slab, the bricks [first, first + bricks) of the grid, on the
// context's stream: the centres into points; the ballots of flags ORed into words (a word per brick of the whole grid)
int grid_centres_launch(psm_ctx* c, const psm_grid* g, const GridShape& s, uint32_t first, uint32_t bricks, void* points);
int grid_fill_launch(psm_ctx* c, const psm_grid* g, const GridShape& s, uint32_t first, uint32_t bricks, const uint8_t* flags, uint64_t* words);
// query.hip, for the signed distance grids (grid_dist.hip): the sign kernel of psm_bvh_signed_distance_dev alone over n points
// and their closest-point records, on the context's stream; the caller has checked the hierarchy and samples
int sign_launch(psm_bvh* b, const void* d_points, size_t n, uint32_t samples, void* d_hits);
// grid_dist.hip, for the signed distance grids over a world (world.hip's world_grid_dist_query()): a slab's records (lane order,
// after the sign kernel) into the dense dist / tri of the whole grid, on the context's stream; d_tri may be NULL
int grid_dist_scatter_launch(psm_ctx* c, const psm_grid* g, const GridShape& s, uint32_t first, uint32_t bricks, const void* hits,
                             float* d_dist, int32_t* d_tri);

// (Q_FIRST_HITS, Q_NEAREST: the k-best queries of kbest.hip and of world.hip's worlds: no entry in the kernel tables; Q_BOX_ANY,
// Q_BOX_COUNT, Q_BOX_TRIS: the box queries of box.hip and world_box.hip: no entry there either; Q_SWEEP, Q_SWEEP_ANY: the sphere
// sweeps of sweep.hip and world_sweep.hip: no entry there either; Q_TRI_ANY, Q_TRI_COUNT, Q_TRI_TRIS: the triangle queries of tri.hip and world_tri.hip: no entry
// there either; Q_TRI_CLOSEST, Q_TRI_WITHIN: the clearance queries of tri_dist.hip: no entry there either)
enum QueryKind { Q_CLOSEST, Q_ANY, Q_POINT, Q_WITHIN, Q_COUNT, Q_INSIDE, Q_SIGNED, Q_FIRST_HITS, Q_NEAREST, Q_BOX_ANY, Q_BOX_COUNT, Q_BOX_TRIS, Q_SWEEP, Q_SWEEP_ANY, Q_TRI_ANY, Q_TRI_COUNT, Q_TRI_TRIS, Q_TRI_CLOSEST, Q_TRI_WITHIN };
// per kind: the single-hierarchy entry point, what the input and the output are called in its messages (out: NULL when its
// alignment is not checked: a byte per query), the output's alignment, the family in the state / capacity texts
struct QueryDesc {
    const char* name;
    const char* in;
    const char* out;
    unsigned out_align;
    bool points;
};
extern const QueryDesc QUERY_DESC[];

// the context's stack entries beyond the LDS part (allocated on the context's first query)
int spill_for(psm_ctx* c, void** out);
// ceil(log2(n)) for n >= 1
int ceil_log2(size_t n);
// the builder's height bound of a hierarchy (QSTACK_MAX in psm_query_dev.h): 63 + ceil(log2(capacity))
int depth_bound(const psm_bvh* b);
// Why a pose is refused, or NULL (psm_hip.h)
const char* pose_fault(const float* m);
// The data checks every query shares, under the entry point's name (query.hip has the rules)
int check_data(psm_ctx* c, const char* name, const char* index, QueryKind kind, const void* d_in, const void* d_out, const int32_t* d_geom,
               uint32_t samples);
// The per-entry checks of a list of instances against the context c, the message naming the first failing index: every handle
// (NULL, another context), every pose, every hierarchy's state (not built, too deep for the stack); all on the host
int check_instances(psm_ctx* c, const psm_instance* list, uint32_t count, const char* name);

}  // namespace psm

#ifndef PSM_QUERY_HOST_DECLARATIONS_ONLY
#include "psm_query_dev.h"

namespace psm {

// a family's seven kernels by QueryKind (Q_SIGNED: the sign kernel)
template <class Args>
struct Kernels {
    void (*k[7])(Args);
};

// The launch of every query. Q_SIGNED is two launches: the family's unchanged closest-point kernel, then the sign of what it
// found (the same stream: in order)
template <class Args>
int launch(psm_ctx* c, const Kernels<Args>& kernels, QueryKind kind, uint32_t grid, const Args& a) {
    if (kind == Q_SIGNED) {
        kernels.k[Q_POINT]<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
        PSM_HIP(c, hipGetLastError());
    }
    kernels.k[kind]<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

// The context's stack area (a context's first query allocates: a later one can be captured into a graph), the grid, and the
// scalars QueryArgs, SceneArgs, InstArgs and WorldArgs share
template <class Args>
int batch_args(psm_ctx* c, const void* d_in, size_t n, void* d_out, uint32_t samples, Args& a, uint32_t& grid) {
    void* spill = nullptr;
    const int rc = spill_for(c, &spill);
    if (rc != PSM_OK) return rc;
    const size_t waves = (n + QUERY_BLOCK - 1) / QUERY_BLOCK;
    grid = (uint32_t)(waves < QUERY_GRID_CAP ? waves : QUERY_GRID_CAP);
    a.rays = (const float4*)d_in; a.n = n;
    a.spill = (int*)spill;
    a.hits = (float4*)d_out; a.occluded = (uint8_t*)d_out; a.count = (uint32_t*)d_out;   // (a kernel reads its own)
    a.samples = samples;
    return PSM_OK;
}

}  // namespace psm
#endif
