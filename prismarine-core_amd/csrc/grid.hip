// grid.hip -- voxel grids over a built hierarchy (new; no reference counterpart; include/psm_hip.h "voxel grids", DESIGN.md
// 4.27): which voxels of a regular grid a triangle overlaps (surface), how many triangles each voxel holds (counts), and the
// surface with the inside filled (solid). Every voxel is answered bit for bit as box.hip answers the voxel's box.
//
// The walk is not query_walk's one query per lane: a 4 x 4 x 4 brick of voxels is one wave64, lane j = (z & 3) * 16 + (y & 3) * 4
// + (x & 3), and the wave walks the tree ONCE for its 64 voxels. The node link is wave-uniform (readfirstlane: the record's two
// 16-byte loads and a leaf's triangle are fetched once per wave, as scalars), each lane judges the two child boxes with its own
// voxel's grown interval (BoxBody::keep's compares), and a child is entered iff some lane that still wants an answer keeps it
// (__ballot). The wave has one stack of QSTACK_MAX links in LDS: no spill area. The boxes are never stored: a lane makes its
// voxel's box from the grid's nine numbers, which travel as kernel arguments. A brick's surface answer leaves as one 64-bit
// ballot word, written by one lane with an ordinary store.
//
// The file also defines the host pieces all eleven grid entry points share (psm_query_host.h): how a grid is read
// (grid_fault), the front of a call (grid_front), a hierarchy's state (grid_built), the context's scratch and the slabs of solid
// and signed (slabs_for, walked by grid_slabs), and the launches around a slab's inside query or sign kernel.
#include <cmath>
#include <mutex>
#include <unordered_map>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_host.h"
#include "psm_query_dev.h"
#include "psm_box_dev.h"   // box_tri, box_row
#include "psm_grid_dev.h"
#include "psm_grid_walk.h"   // grid_walk: shared with the list-driven kernels of grid_sparse.hip

namespace psm {

// (GridArgs, voxel_of, grid_for, grid_args: psm_grid_dev.h; Interval, keep and the walk itself: psm_grid_walk.h)

__global__ __launch_bounds__(QUERY_BLOCK, 8) void grid_surface(GridArgs g, const uint4* __restrict__ node32, const float4* __restrict__ tri48,
                                                               uint64_t* __restrict__ words) {
    grid_walk<GRID_SURFACE>(g, DenseBricks(), node32, tri48, words);
}
__global__ __launch_bounds__(QUERY_BLOCK, 8) void grid_counts(GridArgs g, const uint4* __restrict__ node32, const float4* __restrict__ tri48,
                                                              uint32_t* __restrict__ counts) {
    grid_walk<GRID_COUNTS>(g, DenseBricks(), node32, tri48, counts);
}

// solid, before the inside launch: the centres of the slab's voxels as psm_point_query records in lane order (rmax is not read).
// A voxel outside dims gets a centre too (its flag is dropped by grid_fill)
__global__ __launch_bounds__(QUERY_BLOCK, 8) void grid_centres(GridArgs g) {
    const int lane = (int)threadIdx.x;
    for (uint32_t b = blockIdx.x; b < g.bricks; b += gridDim.x) {
        const Voxel v = voxel_of(g, g.first + b, lane);
        g.points[(size_t)b * QUERY_BLOCK + lane] =
            make_float4(g.ox + ((float)v.ix + 0.5f) * g.cx, g.oy + ((float)v.iy + 0.5f) * g.cy, g.oz + ((float)v.iz + 0.5f) * g.cz, 0.f);
    }
}

// solid, after it: the ballot of the slab's flags ORed into the words the surface launch wrote
__global__ __launch_bounds__(QUERY_BLOCK, 8) void grid_fill(GridArgs g) {
    const int lane = (int)threadIdx.x;
    for (uint32_t b = blockIdx.x; b < g.bricks; b += gridDim.x) {
        const Voxel v = voxel_of(g, g.first + b, lane);
        const unsigned long long word = __ballot(v.inside && g.flags[(size_t)b * QUERY_BLOCK + lane] != 0);
        if (lane == 0) g.words[g.first + b] |= word;
    }
}

// A grid as the host reads it: the brick counts, or why it is refused (psm_hip.h "voxel grids": the rules in their order;
// GridShape: psm_query_host.h -- the grids over a world, world.hip, read a grid by the same rules)
const char* grid_fault(const psm_grid* g, GridShape& s) {
    s = GridShape();
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(g->origin[k])) return "origin is not finite";
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(g->cell[k]) || !(g->cell[k] > 0.f)) return "cell must be finite and > 0";
    for (int k = 0; k < 3; k++)
        if (g->dims[k] < 1u || g->dims[k] > PSM_GRID_DIM_MAX) return "dims must be 1 .. 2^20";
    for (int k = 0; k < 3; k++) {
        const float top = (float)g->dims[k] * g->cell[k];   // (the last voxel's hi: one multiplication, one addition)
        const float hi = g->origin[k] + top;
        if (!std::isfinite(hi)) return "the last voxel's hi is not finite";
    }
    for (int k = 0; k < 3; k++) s.nb[k] = (g->dims[k] + 3u) / 4u;
    s.bricks = (uint64_t)s.nb[0] * s.nb[1] * s.nb[2];   // (each <= 2^18: no overflow)
    if (s.bricks >= ((uint64_t)1 << 31)) return "2^31 bricks or more";
    return nullptr;
}

// ---- The host pieces the eleven grid entry points share (psm_query_host.h): grid_query() below, grid_dist.hip's
// dist_query(), world.hip's world_grid_query() and world_grid_dist_query() are sequences of these and of what is their own.

// The front of every grid call, under the entry point's name, on the host, nothing launched and no output byte changed: NULL grid
// or output, the grid's rules (s filled in), the outputs' alignment, rmax and samples where the call has them (else NULL)
int grid_front(psm_ctx* c, const char* name, const psm_grid* grid, const void* out, GridShape& s, const char* what, const void* aligned,
               unsigned align, const float* rmax, const uint32_t* samples) {
    int rc = mesh_pointers(c, name, grid && out);
    if (rc != PSM_OK) return rc;
    if (const char* why = grid_fault(grid, s)) return mesh_refuse(c, PSM_ERR_INVALID, "%s: invalid grid: %s", name, why);
    rc = mesh_aligned(c, name, what, aligned, align);
    if (rc != PSM_OK) return rc;
    if (rmax && !(*rmax >= 0.f)) return mesh_refuse(c, PSM_ERR_INVALID, "%s: rmax must be >= 0", name);   // (NaN too; -0 is 0, +inf is no limit)
    if (samples && *samples != 1 && *samples != 3 && *samples != 5) return mesh_refuse(c, PSM_ERR_INVALID, "%s: samples must be 1, 3 or 5", name);
    return PSM_OK;
}

// A hierarchy's state as a grid call needs it: built, and no deeper than the wave's one stack
int grid_built(const psm_bvh* b) {
    if (!b->built) return set_err(b->ctx, PSM_ERR_STATE, "grid query before build");
    if (depth_bound(b) > QSTACK_MAX) return set_err(b->ctx, PSM_ERR_CAPACITY, "grid query: hierarchy deeper than the query stack");
    return PSM_OK;
}

namespace {

// the scratch of solid and signed, per context (grown on demand, at most GRID_SLAB_BRICKS bricks of points and flags: 68 MiB; every
// call runs on the context's stream, never two at once)
constexpr size_t SLAB_BRICK_BYTES = (size_t)QUERY_BLOCK * (sizeof(float4) + sizeof(uint8_t));
struct Scratch {
    void* ptr = nullptr;
    uint32_t bricks = 0;
};
std::mutex scratch_mu;
std::unordered_map<const psm_ctx*, Scratch> scratch_area;

int scratch_for(psm_ctx* c, uint32_t bricks, void** out) {
    std::lock_guard<std::mutex> lk(scratch_mu);
    Scratch& a = scratch_area[c];
    if (a.bricks < bricks) {
        // (a kernel that reads the old area is in stream order before the free)
        if (a.ptr) PSM_HIP(c, hipStreamSynchronize(c->stream));
        if (a.ptr) PSM_HIP(c, hipFree(a.ptr));
        a = Scratch();
        uint32_t want = 64;
        while (want < bricks) want *= 2;
        PSM_HIP(c, hipMalloc(&a.ptr, (size_t)want * SLAB_BRICK_BYTES));
        a.bricks = want;
    }
    *out = a.ptr;
    return PSM_OK;
}

}  // namespace

// The slabs of a solid or a signed call over `bricks` bricks and the context's scratch for one of them: the slab's centres first,
// then solid's flags or signed's hits. A voxel of signed takes 32 bytes where solid's takes 17: a slab of n bricks asks for the
// area of 2 n of solid's, and a slab is half of solid's at most
int slabs_for(psm_ctx* c, uint64_t bricks, bool sign, GridSlabs& a) {
    const uint32_t cap = sign ? GRID_SLAB_BRICKS / 2u : GRID_SLAB_BRICKS;
    a.slab = bricks < cap ? (uint32_t)bricks : cap;
    void* area = nullptr;
    const int rc = scratch_for(c, sign ? 2u * a.slab : a.slab, &area);
    a.points = (float4*)area;
    a.hits = a.points + (size_t)a.slab * QUERY_BLOCK;
    a.flags = (uint8_t*)a.hits;
    return rc;
}

int grid_centres_launch(psm_ctx* c, const psm_grid* grid, const GridShape& s, uint32_t first, uint32_t bricks, void* points) {
    GridArgs g = grid_args(grid, s);
    g.first = first; g.bricks = bricks;
    g.points = (float4*)points;
    grid_centres<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

int grid_fill_launch(psm_ctx* c, const psm_grid* grid, const GridShape& s, uint32_t first, uint32_t bricks, const uint8_t* flags, uint64_t* words) {
    GridArgs g = grid_args(grid, s);
    g.first = first; g.bricks = bricks;
    g.flags = flags; g.words = words;
    grid_fill<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

namespace {

const char* const GRID_NAME[] = {"psm_grid_surface_dev", "psm_grid_counts_dev", "psm_grid_solid_dev"};
enum { CALL_SURFACE = 0, CALL_COUNTS = 1, CALL_SOLID = 2 };

// A grid call: a NULL hierarchy is answered before anything else; then the front every grid call shares (grid_front), the state
// and the depth (grid_built) -- all on the host, before any launch, the output untouched --, the walk over the whole grid, and for
// solid the inside of the surface slab by slab
int grid_query(psm_bvh* b, const psm_grid* grid, int call, uint32_t samples, void* d_out) {
    if (!b) return PSM_ERR_INVALID;
    psm_ctx* c = b->ctx;
    GridShape s;
    int rc = grid_front(c, GRID_NAME[call], grid, d_out, s, call == CALL_COUNTS ? "counts" : "bricks", d_out, call == CALL_COUNTS ? 4u : 8u,
                        nullptr, call == CALL_SOLID ? &samples : nullptr);
    if (rc == PSM_OK) rc = grid_built(b);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    GridArgs g = grid_args(grid, s);
    g.sm = b->d_small; g.sorted_tri = b->d_sorted_tri;
    GridSlabs a;
    if (call == CALL_SOLID) {   // (the last thing that can fail before the output changes)
        rc = slabs_for(c, s.bricks, false, a);
        if (rc != PSM_OK) return rc;
    }
    if (call == CALL_COUNTS) grid_counts<<<grid_for(s.bricks), QUERY_BLOCK, 0, c->stream>>>(g, b->d_node32, b->d_tri48, (uint32_t*)d_out);
    else grid_surface<<<grid_for(s.bricks), QUERY_BLOCK, 0, c->stream>>>(g, b->d_node32, b->d_tri48, (uint64_t*)d_out);
    PSM_HIP(c, hipGetLastError());
    if (call != CALL_SOLID) return PSM_OK;
    // the inside of the surface, a slab of bricks at a time, all in stream order: the centres, query.hip's inside path over
    // them, the flags' ballots ORed into the words
    return grid_slabs(s.bricks, a.slab, [&](uint32_t first, uint32_t bricks) {
        int rc = grid_centres_launch(c, grid, s, first, bricks, a.points);
        if (rc == PSM_OK) rc = psm_bvh_inside_dev(b, (const psm_point_query*)a.points, (size_t)bricks * QUERY_BLOCK, samples, a.flags);
        if (rc == PSM_OK) rc = grid_fill_launch(c, grid, s, first, bricks, a.flags, (uint64_t*)d_out);
        return rc;
    });
}

}  // namespace

// for psm_ctx_destroy: solid's scratch goes with the context
void grid_release(psm_ctx* c) {
    sparse_release(c);   // (grid_sparse.hip: the sparse grids' flags and candidate ids)
    std::lock_guard<std::mutex> lk(scratch_mu);
    auto it = scratch_area.find(c);
    if (it == scratch_area.end()) return;
    if (it->second.ptr) (void)hipFree(it->second.ptr);
    scratch_area.erase(it);
}

}  // namespace psm

int psm_grid_surface_dev(psm_bvh* bvh, const psm_grid* grid, uint64_t* d_bricks) {
    return psm::grid_query(bvh, grid, psm::CALL_SURFACE, 0, d_bricks);
}

int psm_grid_counts_dev(psm_bvh* bvh, const psm_grid* grid, uint32_t* d_counts) {
    return psm::grid_query(bvh, grid, psm::CALL_COUNTS, 0, d_counts);
}

int psm_grid_solid_dev(psm_bvh* bvh, const psm_grid* grid, uint32_t samples, uint64_t* d_bricks) {
    return psm::grid_query(bvh, grid, psm::CALL_SOLID, samples, d_bricks);
}

uint64_t psm_grid_brick_count(const psm_grid* grid) {
    psm::GridShape s;
    if (!grid || psm::grid_fault(grid, s)) return 0;
    return s.bricks;
}
