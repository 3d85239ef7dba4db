// world_grid.hip -- voxel grids over an instance world (new; no reference counterpart; include/psm_hip.h "voxel grids over a
// world"): which voxels of a regular WORLD grid a posed triangle of some instance overlaps (surface), how many
// (instance, triangle) pairs each voxel holds (counts), and the lowest instance that has a triangle in each voxel (instances).
// Every voxel is answered bit for bit as world_box.hip answers the voxel's box.
//
// The walk is grid.hip's, over two levels: a 4 x 4 x 4 brick of voxels is one wave64, lane j = (z & 3) * 16 + (y & 3) * 4 +
// (x & 3), and the wave walks the tree over the instances and the hierarchies of the instances it enters ONCE for its 64
// voxels. The link is wave-uniform (readfirstlane): a top-level node, a table row, a hierarchy's record and a leaf's triangle
// are fetched once per wave. Each lane judges with its own voxel's box -- WorldBoxPrune's top-level test, its intervals in the
// instance entered, its compares (psm_world_box_dev.h, unchanged) --, and a child is entered iff some lane that still wants an
// answer keeps it (__ballot). A kept leaf's triangle is posed forward once per wave, as WorldBoxBody::leaf poses it, and the
// lanes that want an answer judge it with box_tri. The wave has ONE stack of QSTACK_MAX links in LDS for both levels (top-level
// links carry WORLD_TOP): psm_world_set_instances guarantees depth + deepest + 1 <= QSTACK_MAX, and every push and pop is
// guarded. The boxes are never stored: a lane makes its voxel's box from the grid's nine numbers.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"       // WorldRow, WorldNode, WorldGridArgs, WORLD_TOP, WORLD_QSLACK
#include "psm_box_dev.h"         // box_tri
#include "psm_world_box_dev.h"   // fwd_point, fwd_vec, WorldBoxPrune
#include "psm_world_uni_dev.h"   // uni, uni_ptr, PSM_CONST, words4, floats3

namespace psm {

namespace {

// One wave per brick, grid-stride over the bricks. MODE: WGRID_SURFACE -- a lane that has its bit stops voting, and the walk
// ends when no lane wants anything --, WGRID_COUNTS -- every live lane wants every pair its tests keep --, WGRID_INSTANCES -- a
// lane wants the instances below the one it holds.
// rows: the world's table; nodes: the tree over the instances; out: a uint64_t word per brick (surface) or the dense
// [nz][ny][nx] uint32_t counts / int32_t labels
template <int MODE, class Out>
PSM_D void world_grid_walk(const WorldGridArgs& g, const WorldRow* __restrict__ rows, const WorldNode* __restrict__ nodes, Out* __restrict__ out) {
    __shared__ int stack[QSTACK_MAX];   // the wave's: every lane writes and reads the same entry
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    for (uint32_t b = blockIdx.x; b < g.bricks; b += gridDim.x) {
        const uint32_t bx = b % g.nbx, bt = b / g.nbx, by = bt % g.nby, bz = bt / g.nby;
        const uint32_t ix = 4u * bx + ((uint32_t)lane & 3u), iy = 4u * by + (((uint32_t)lane >> 2) & 3u), iz = 4u * bz + ((uint32_t)lane >> 4);
        const bool inside = ix < g.nx && iy < g.ny && iz < g.nz;
        WorldBoxPrune P;   // (node32, tri48 and inst are the wave's, below: P's are not read)
        P.lo = mk3(0.f, 0.f, 0.f);
        P.hi = mk3(-1.f, -1.f, -1.f);   // a dead lane: lo > hi (WorldBoxBody::begin)
        if (inside) {
            // one multiplication, then one addition (the build contracts nothing): neighbours share their face plane bit for bit
            P.lo = mk3(g.ox + (float)ix * g.cx, g.oy + (float)iy * g.cy, g.oz + (float)iz * g.cz);
            P.hi = mk3(g.ox + (float)(ix + 1u) * g.cx, g.oy + (float)(iy + 1u) * g.cy, g.oz + (float)(iz + 1u) * g.cz);
        }
        P.qmax = smaxf(absmax3(P.lo), absmax3(P.hi));
        const bool valid = inside && finite3(P.lo) && finite3(P.hi) && P.lo.x <= P.hi.x && P.lo.y <= P.hi.y && P.lo.z <= P.hi.z;
        // per brick: the grid-stride loop comes here again
        uint32_t cnt = 0u;
        int label = -1;
        // the instance the wave is in: its records, its triangles, its pose
        const PSM_CONST uint32_t* node32 = nullptr;
        const PSM_CONST uint32_t* tri48 = nullptr;
        float m[12] = {};
        int inst = -1;
        int cur = g.root < 0 ? g.root : (g.root | WORLD_TOP), sp = 0;
        for (;;) {
            // what a lane still wants of the whole world, and of the instance the wave is in
            const bool live = MODE == WGRID_SURFACE ? (valid && cnt == 0u) : valid;
            if (__ballot(live) == 0ull) break;
            cur = __builtin_amdgcn_readfirstlane(cur);
            int t0 = -1, t1 = -1;   // the leaves to test, wave-uniform
            bool pop = false;
            if (cur < 0) {
                // an instance is entered: its row once for the wave, every lane's intervals in its normalised space
                inst = ~cur;
                const bool wants = MODE == WGRID_INSTANCES ? (valid && (uint32_t)inst < (uint32_t)label) : live;
                pop = true;
                if (__ballot(wants) != 0ull) {
                    const uint4* rp = (const uint4*)(rows + inst);
                    const uint4 ra = rp[0], rb = rp[1], rc = rp[2], rd = rp[3], re = rp[4];
                    node32 = uni_ptr(ra.x, ra.y);
                    tri48 = uni_ptr(ra.z, ra.w);
                    const PSM_CONST uint32_t* sm = uni_ptr(rb.x, rb.y);
                    const PSM_CONST uint32_t* sorted_tri = uni_ptr(rb.z, rb.w);
                    m[0] = u2f(uni(rc.x)); m[1] = u2f(uni(rc.y)); m[2] = u2f(uni(rc.z)); m[3] = u2f(uni(rc.w));
                    m[4] = u2f(uni(rd.x)); m[5] = u2f(uni(rd.y)); m[6] = u2f(uni(rd.z)); m[7] = u2f(uni(rd.w));
                    m[8] = u2f(uni(re.x)); m[9] = u2f(uni(re.y)); m[10] = u2f(uni(re.z)); m[11] = u2f(uni(re.w));
                    float M[16];
#pragma unroll
                    for (int k = 0; k < 16; k++) M[k] = u2f(sm[SM_M + k]);
                    P.intervals(M, m);   // (WorldBoxPrune::enter_row's arithmetic, on the lane's own box)
                    const int root = (int)uni(sm[SM_ROOT]);
                    if (uni(sm[SM_COUNT]) == 1u) t0 = (int)uni(sorted_tri[0]);   // one leaf: no tree
                    if (root >= 0) {
                        cur = root;
                        pop = false;
                    }
                }
            } else if (cur & WORLD_TOP) {
                const WorldNode* np = (const WorldNode*)((const char*)nodes + ((size_t)(uint32_t)(cur & ~WORLD_TOP) << 6));
                const float4 w0 = np->w0, w1 = np->w1, w2 = np->w2;
                const int4 w3 = np->w3;
                const bool keepL = P.keep_top(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y);
                const bool keepR = P.keep_top(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w);
                const bool okL = __ballot(keepL && live) != 0ull, okR = __ballot(keepR && live) != 0ull;
                const int lx = (int)uni((uint32_t)w3.x), ly = (int)uni((uint32_t)w3.y);
                const int lkL = lx < 0 ? lx : (lx | WORLD_TOP), lkR = ly < 0 ? ly : (ly | WORLD_TOP);
                if (okL && okR) {
                    // (sp < QSTACK_MAX always: psm_world_set_instances refuses a world whose two depths exceed it. The test keeps
                    // every store and every pop inside the array)
                    if (sp < QSTACK_MAX) {
                        stack[sp] = lkR;
                        sp++;
                    }
                }
                cur = okL ? lkL : lkR;
                pop = !(okL || okR);
            } else {
                const bool wants = MODE == WGRID_INSTANCES ? (valid && (uint32_t)inst < (uint32_t)label) : live;
                const PSM_CONST uint32_t* np = node32 + ((size_t)(uint32_t)cur << 3);   // (a record is 32 bytes)
                const uint4 n0 = words4(np), n1 = words4(np + 4);
                const int lkx = (int)uni(n1.z), lky = (int)uni(n1.w);
                // each lane judges both children against its own intervals (WorldBoxPrune::children's reading of the record)
                const bool keepL = P.keep(half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
                const bool keepR = P.keep(half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
                const bool okL = __ballot(keepL && wants) != 0ull, okR = __ballot(keepR && wants) != 0ull;
                const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
                t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
                t1 = (leafL && leafR) ? ~lky : -1;
                const bool intL = okL && !leafL, intR = okR && !leafR;
                if (intL && intR) {
                    if (sp < QSTACK_MAX) {
                        stack[sp] = lky;
                        sp++;
                    }
                }
                cur = intL ? lkx : lky;
                pop = !(intL || intR);
            }
            // the accepted leaves, one test after the other: the triangle is loaded and posed forward once for the wave
            // (WorldBoxBody::leaf: v0' = R v0 + T, e1' = R e1, e2' = R e2), and each lane that still wants it judges it
            while (t0 >= 0) {
                const PSM_CONST uint32_t* tp = tri48 + (size_t)12 * (size_t)t0;   // (v0, e1, e2: a float4 each)
                const v3 v0 = fwd_point(m, floats3(tp)), e1 = fwd_vec(m, floats3(tp + 4)), e2 = fwd_vec(m, floats3(tp + 8));
                const bool wants = MODE == WGRID_SURFACE    ? (valid && cnt == 0u)
                                   : MODE == WGRID_COUNTS   ? valid
                                                            : (valid && (uint32_t)inst < (uint32_t)label);
                if (wants && box_tri(v0, e1, e2, P.lo, P.hi)) {
                    cnt++;
                    label = inst;
                }
                t0 = t1;
                t1 = -1;
            }
            if (pop) {
                if (sp == 0) break;
                sp--;
                cur = stack[sp];
            }
        }
        if (MODE == WGRID_SURFACE) {
            const unsigned long long word = __ballot(cnt != 0u);
            if (lane == 0) out[b] = (Out)word;
        } else if (inside) {
            out[((size_t)iz * g.ny + iy) * g.nx + ix] = MODE == WGRID_COUNTS ? (Out)cnt : (Out)label;
        }
    }
}

}  // namespace

// the bound of the other kernels of a world (128 VGPRs; hipcc takes 46 to 51, so eight waves fit a SIMD as with grid.hip; under
// grid.hip's bound of 8 it spills five to seven SGPRs into VGPR lanes: DESIGN.md 4.29)
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_grid_surface(WorldGridArgs g, const WorldRow* __restrict__ rows, const WorldNode* __restrict__ nodes,
                                                                     uint64_t* __restrict__ words) {
    world_grid_walk<WGRID_SURFACE>(g, rows, nodes, words);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_grid_counts(WorldGridArgs g, const WorldRow* __restrict__ rows, const WorldNode* __restrict__ nodes,
                                                                    uint32_t* __restrict__ counts) {
    world_grid_walk<WGRID_COUNTS>(g, rows, nodes, counts);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_grid_instances(WorldGridArgs g, const WorldRow* __restrict__ rows, const WorldNode* __restrict__ nodes,
                                                                       int32_t* __restrict__ labels) {
    world_grid_walk<WGRID_INSTANCES>(g, rows, nodes, labels);
}

// world.hip's host path (world_grid_query(): the checks, the empty world, the stale refusal) launches through this
int world_grid_launch(psm_ctx* c, int mode, uint32_t grid, const WorldGridArgs& g, const WorldRow* rows, const WorldNode* nodes, void* out) {
    if (mode == WGRID_SURFACE) world_grid_surface<<<grid, QUERY_BLOCK, 0, c->stream>>>(g, rows, nodes, (uint64_t*)out);
    else if (mode == WGRID_COUNTS) world_grid_counts<<<grid, QUERY_BLOCK, 0, c->stream>>>(g, rows, nodes, (uint32_t*)out);
    else world_grid_instances<<<grid, QUERY_BLOCK, 0, c->stream>>>(g, rows, nodes, (int32_t*)out);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
