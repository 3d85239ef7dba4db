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

namespace psm {

namespace {

// One wave per brick, grid-stride over the bricks. RECORDS = false: the dense dist / tri [nz][ny][nx] of the whole grid (tri
// may be NULL); RECORDS = true: a psm_hit per lane of the launch's bricks in lane order (u = v = 0), a miss for a lane outside
// dims, for the sign kernel of query.hip.
// Visiting order: where both children are internal and kept, the wave goes first to the one that most of the lanes that keep a
// child find nearer (their own kL <= kR): one ballot and two scalar bit counts per node on top of the two ballots that decide
// the entry, where the minimum key over the lanes would take a cross-lane reduction per child. The 64 centres lie within one brick, so the vote is rarely close.
template <bool RECORDS>
PSM_D void dist_walk(const GridArgs& g, float rmax, const uint4* __restrict__ node32, const float4* __restrict__ tri48,
                     float* __restrict__ dist, int32_t* __restrict__ tri, float4* __restrict__ hits) {
    __shared__ int stack[QSTACK_MAX];   // the wave's: every lane writes and reads the same entry
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const int root = (int)g.sm[SM_ROOT];
    const uint32_t count = g.sm[SM_COUNT];
    const int lone = (count == 1u) ? g.sorted_tri[0] : -1;   // one leaf: no tree, the leaf's triangle is the only candidate
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
    const PointBound B = point_bound(M);
    for (uint32_t b = blockIdx.x; b < g.bricks; b += gridDim.x) {
        const Voxel v = voxel_of(g, g.first + b, lane);
        // the centre as grid_centres writes it (grid.hip): one operation per rounding
        const v3 p = mk3(g.ox + ((float)v.ix + 0.5f) * g.cx, g.oy + ((float)v.iy + 0.5f) * g.cy, g.oz + ((float)v.iz + 0.5f) * g.cz);
        const bool live = v.inside && finite3(p);   // (PointBody::begin's valid; rmax was checked on the host)
        PointImage P;
        P.set(M, p);
        // per brick: the grid-stride loop comes here again
        float best = (rmax * rmax) * 1.00000095367431640625f + 0x1p-126f;   // fl(rmax^2) (1 + 2^-20) + 2^-126 (PointBody::begin)
        int btri = -1;
        bool found = false;
        int t0 = lone, t1 = -1;   // the leaves to test, wave-uniform
        int cur = root, sp = 0;
        bool walking = root >= 0;
        for (;;) {
            // the accepted leaves, one test after the other: the triangle is loaded once for the wave
            while (t0 >= 0) {
                const int id = __builtin_amdgcn_readfirstlane(t0);
                const float4* tp = tri48 + (size_t)3 * (size_t)id;
                const float4 A = tp[0], Bv = tp[1], C = tp[2];
                float u, w;
                const float d2 = closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(C.x, C.y, C.z), p, u, w);
                // (PointBody::leaf, compare for compare)
                if (live && sqrtf(d2) <= rmax && (d2 < best || (d2 == best && (uint32_t)id < (uint32_t)btri))) {
                    found = true;
                    best = d2;
                    btri = id;
                }
                t0 = t1;
                t1 = -1;
            }
            if (!walking) break;
            cur = __builtin_amdgcn_readfirstlane(cur);
            const uint4* np = (const uint4*)((const char*)node32 + ((size_t)(uint32_t)cur << 5));
            const uint4 n0 = np[0], n1 = np[1];
            const int lkx = (int)n1.z, lky = (int)n1.w;
            bool keepL, keepR;
            float kL, kR;
            P.children(B, n0, n1, best, keepL, keepR, kL, kR);
            const unsigned long long mL = __ballot(keepL && live), mR = __ballot(keepR && live);
            const bool okL = mL != 0ull, okR = mR != 0ull;
            const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
            t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
            t1 = (leafL && leafR) ? ~lky : -1;
            const bool intL = okL && !leafL, intR = okR && !leafR;
            // nearer child first, by the majority of the lanes that keep one
            const unsigned long long nearL = __ballot(live && (keepL || keepR) && kL <= kR);
            const bool leftFirst = intL && (!intR || 2 * __popcll(nearL) >= __popcll(mL | mR));
            const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
            if (intL && intR) {
                // (sp < QSTACK_MAX always: one entry per internal ancestor of the current node, as a lane's own stack; the host
                // refuses hierarchies whose bound exceeds it. The test keeps every store and every pop inside the array)
                if (sp < QSTACK_MAX) {
                    stack[sp] = second;
                    sp++;
                }
            }
            cur = first;
            if (!(intL || intR)) {
                if (sp == 0) walking = false;   // (the node's leaves are still tested)
                else {
                    sp--;
                    cur = stack[sp];
                }
            }
        }
        const float t = found ? sqrtf(best) : __builtin_inff();
        if (RECORDS) hits[(size_t)b * QUERY_BLOCK + lane] = make_float4(0.f, 0.f, t, __int_as_float(btri));
        else if (v.inside) {
            const size_t i = ((size_t)v.iz * g.ny + v.iy) * g.nx + v.ix;
            dist[i] = t;
            if (tri) tri[i] = btri;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, 4) void grid_dist_dense(GridArgs g, float rmax, const uint4* __restrict__ node32,
                                                                  const float4* __restrict__ tri48, float* __restrict__ dist,
                                                                  int32_t* __restrict__ tri) {
    dist_walk<false>(g, rmax, node32, tri48, dist, tri, nullptr);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void grid_dist_records(GridArgs g, float rmax, const uint4* __restrict__ node32,
                                                                    const float4* __restrict__ tri48, float4* __restrict__ hits) {
    dist_walk<true>(g, rmax, node32, tri48, nullptr, nullptr, hits);
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
