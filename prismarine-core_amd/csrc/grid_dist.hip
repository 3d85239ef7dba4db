// grid_dist.hip -- distance-field grids over a built hierarchy (new; no reference counterpart; include/psm_hip.h "voxel grids",
// DESIGN.md 4.30): the distance from every voxel centre of a regular grid to the nearest triangle within rmax, and that
// triangle's id; signed, the distance with the sign of the inside test. Every voxel is answered bit for bit as
// psm_bvh_closest_point_dev / psm_bvh_signed_distance_dev answer the voxel's centre.
//
// The walk is grid.hip's: a 4 x 4 x 4 brick of voxels is one wave64 (voxel_of's lane order), and the wave walks the tree ONCE
// for its 64 centres. The node link is wave-uniform (readfirstlane: the record's two 16-byte loads and a leaf's 48-byte triangle
// are fetched once per wave, as scalars). Each lane keeps what PointBody<false> (query.hip) keeps for one point -- its
// PointImage, best, btri, found -- and judges the two child boxes with PointImage::children against its own best; a child is
// entered iff some live lane keeps it (__ballot). A leaf is tested by every live lane with PointBody::leaf's comparison. The
// answer does not depend on which boxes the wave enters beyond a lane's own, nor on the order: a box a lane would have dropped
// holds no triangle that passes that lane's comparison (LB^2 > best: psm_query_dev.h), and the comparison takes the smaller d2
// and on a bit-equal d2 the lower id, whatever came first. The wave has one stack of QSTACK_MAX links in LDS: no spill area.
// The host function is a sequence of the pieces every grid call shares (grid.hip, psm_query_host.h).
#include <cmath>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_host.h"
#include "psm_query_dev.h"
#include "psm_grid_dev.h"
#include "psm_grid_walk.h"   // dist_walk: shared with the list-driven kernels of grid_sparse.hip

namespace psm {

__global__ __launch_bounds__(QUERY_BLOCK, 4) void grid_dist_dense(GridArgs g, float rmax, const uint4* __restrict__ node32,
                                                                  const float4* __restrict__ tri48, float* __restrict__ dist,
                                                                  int32_t* __restrict__ tri) {
    dist_walk<DIST_DENSE>(g, DenseBricks(), rmax, node32, tri48, dist, tri, nullptr, nullptr);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void grid_dist_records(GridArgs g, float rmax, const uint4* __restrict__ node32,
                                                                    const float4* __restrict__ tri48, float4* __restrict__ hits) {
    dist_walk<DIST_RECORDS>(g, DenseBricks(), rmax, node32, tri48, nullptr, nullptr, hits, nullptr);
}

// signed, after the sign kernel: the slab's records (lane order) into the dense dist / tri of the whole grid
__global__ __launch_bounds__(QUERY_BLOCK, 8) void grid_dist_scatter(GridArgs g, const float4* __restrict__ hits, float* __restrict__ dist,
                                                                    int32_t* __restrict__ tri) {
    const int lane = (int)threadIdx.x;
    for (uint32_t b = blockIdx.x; b < g.bricks; b += gridDim.x) {
        const Voxel v = voxel_of(g, g.first + b, lane);
        if (!v.inside) continue;
        const float4 h = hits[(size_t)b * QUERY_BLOCK + lane];
        const size_t i = ((size_t)v.iz * g.ny + v.iy) * g.nx + v.ix;
        dist[i] = h.z;
        if (tri) tri[i] = __float_as_int(h.w);
    }
}

// world.hip's signed distance grids over a world (world_grid_dist_query()) scatter their slabs through this: the
// one copy of the kernel. The bricks [first, first + bricks) of the grid, the records in lane order, tri may be NULL
int grid_dist_scatter_launch(psm_ctx* c, const psm_grid* grid, const GridShape& s, uint32_t first, uint32_t bricks, const void* hits,
                             float* d_dist, int32_t* d_tri) {
    GridArgs g = grid_args(grid, s);
    g.first = first; g.bricks = bricks;
    grid_dist_scatter<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g, (const float4*)hits, d_dist, d_tri);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

namespace {

// A distance grid call: grid_query's sequence (grid.hip) with rmax between the alignment and samples -- the shared front and the
// hierarchy's state, all on the host, before any launch, the outputs untouched.
int dist_query(psm_bvh* b, const psm_grid* grid, float rmax, bool sign, uint32_t samples, float* d_dist, int32_t* d_tri) {
    if (!b) return PSM_ERR_INVALID;
    psm_ctx* c = b->ctx;
    GridShape s;
    int rc = grid_front(c, sign ? "psm_grid_signed_distance_dev" : "psm_grid_distance_dev", grid, d_dist, s, "dist or tri",
                        (const void*)((uintptr_t)d_dist | (uintptr_t)d_tri), 4, &rmax, sign ? &samples : nullptr);
    if (rc == PSM_OK) rc = grid_built(b);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    GridArgs g = grid_args(grid, s);
    g.sm = b->d_small; g.sorted_tri = b->d_sorted_tri;
    if (!sign) {
        grid_dist_dense<<<grid_for(s.bricks), QUERY_BLOCK, 0, c->stream>>>(g, rmax, b->d_node32, b->d_tri48, d_dist, d_tri);
        PSM_HIP(c, hipGetLastError());
        return PSM_OK;
    }
    // signed, a slab of bricks at a time, all in stream order: the centres, the walk's records beside them, query.hip's sign
    // kernel over both, the records into the dense arrays
    GridSlabs a;
    rc = slabs_for(c, s.bricks, true, a);   // (the last thing that can fail before the outputs change)
    if (rc != PSM_OK) return rc;
    return grid_slabs(s.bricks, a.slab, [&](uint32_t first, uint32_t bricks) {
        int rc = grid_centres_launch(c, grid, s, first, bricks, a.points);
        if (rc != PSM_OK) return rc;
        g.first = first; g.bricks = bricks;
        grid_dist_records<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g, rmax, b->d_node32, b->d_tri48, a.hits);
        PSM_HIP(c, hipGetLastError());
        rc = sign_launch(b, a.points, (size_t)bricks * QUERY_BLOCK, samples, a.hits);
        if (rc != PSM_OK) return rc;
        return grid_dist_scatter_launch(c, grid, s, first, bricks, a.hits, d_dist, d_tri);
    });
}

}  // namespace

}  // namespace psm

int psm_grid_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, float* d_dist, int32_t* d_tri) {
    return psm::dist_query(bvh, grid, rmax, false, 0, d_dist, d_tri);
}

int psm_grid_signed_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, uint32_t samples, float* d_dist, int32_t* d_tri) {
    return psm::dist_query(bvh, grid, rmax, true, samples, d_dist, d_tri);
}
