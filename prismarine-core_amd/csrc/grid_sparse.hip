// grid_sparse.hip -- sparse grids over a built hierarchy (new; no reference counterpart; include/psm_hip.h "voxel grids: sparse",
// DESIGN.md 4.33): which 4 x 4 x 4 bricks of a regular grid hold anything at all -- a surface bit, or a voxel centre with a
// triangle within rmax --, as an ascending list, and the surface words or the (signed) distances of the bricks of a list. Every
// answer is the dense call's (grid.hip, grid_dist.hip), bit for bit.
//
// Listing is four steps, all in stream order with no host synchronisation:
//   1. coarse candidates: a wave takes a 4 x 4 x 4 block of BRICKS, one brick per lane, and walks the tree once for them with
//      the walk of grid.hip -- a wave-uniform node link, the record as scalars, one stack of QSTACK_MAX links in LDS. A lane
//      judges a child box with its brick's whole box (surface: box_row's grown interval, keep) or with its brick's centre and
//      the radius rmax + the farthest voxel centre's offset + slack (distance: PointImage::lb2). A lane that keeps a leaf's box
//      is a candidate and stops voting. No triangle is read. DESIGN.md 4.33 has why no brick the exact walk lists is missed.
//   2. an ordered compaction of the candidates' flags into an ascending list whose count stays on the device;
//   3. brick-any: one wave per candidate walks as the dense kernel does (psm_grid_walk.h: the same text) and leaves as soon as
//      one lane has a hit; a byte per candidate;
//   4. the same compaction of those bytes into the caller's list and count.
// With the coarse pass off (rmax = +inf, or PSM_SPARSE_COARSE=0) every brick is a candidate and steps 1 and 2 are not run.
// The fills are the dense walks over ListBricks: brick ids[b] instead of brick g.first + b, the answer at slot b.
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_host.h"
#include "psm_query_dev.h"
#include "psm_box_dev.h"
#include "psm_grid_dev.h"
#include "psm_grid_walk.h"

namespace psm {

namespace {

constexpr uint32_t SCAN_BLOCK = 1024;   // flags per workgroup of the compaction (256 threads, four rounds)

// the coarse pass: the grid, the bricks per axis, the blocks of 4 x 4 x 4 bricks per axis and in all, the distance pass's bound
struct CoarseArgs {
    GridArgs g;
    uint32_t nbz;
    uint32_t sbx, sby, supers;
    float best;   // distance: fl(R^2) (1 + 2^-20) + 2^-126 with R the coarse radius (coarse_radius)
};

// One wave per block of 64 bricks, grid-stride over the blocks; lane j is brick (4 sx + (j & 3), 4 sy + ((j >> 2) & 3), 4 sz +
// (j >> 4)). cand: a byte per brick of the grid, written for every brick.
template <bool DIST>
PSM_D void coarse_walk(const CoarseArgs& a, const uint4* __restrict__ node32, uint8_t* __restrict__ cand) {
    __shared__ int stack[QSTACK_MAX];   // the wave's: every lane writes and reads the same entry
    const GridArgs& g = a.g;
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const int root = (int)g.sm[SM_ROOT];
    const uint32_t count = g.sm[SM_COUNT];
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
    const PointBound B = point_bound(M);
    for (uint32_t s = blockIdx.x; s < a.supers; s += gridDim.x) {
        const uint32_t sx = s % a.sbx, t = s / a.sbx, sy = t % a.sby, sz = t / a.sby;
        const uint32_t bx = 4u * sx + ((uint32_t)lane & 3u), by = 4u * sy + (((uint32_t)lane >> 2) & 3u), bz = 4u * sz + ((uint32_t)lane >> 4);
        const bool inside = bx < g.nbx && by < g.nby && bz < a.nbz;
        Interval I = {};
        PointImage P = {};
        bool hit = false;
        if (DIST) {
            // the brick's centre: the corner of voxel 4 b + 2, one operation per rounding as a voxel's centre
            const v3 q = mk3(g.ox + ((float)(4u * bx) + 2.0f) * g.cx, g.oy + ((float)(4u * by) + 2.0f) * g.cy, g.oz + ((float)(4u * bz) + 2.0f) * g.cz);
            P.set(M, q);
            hit = inside && !finite3(q);   // (nothing is proved about such a centre: a candidate)
        } else {
            // the brick's box: lo of voxel 4 b, hi of the brick's last voxel inside dims, as the voxels' own planes
            const uint32_t ex = 4u * bx + 4u < g.nx ? 4u * bx + 4u : g.nx, ey = 4u * by + 4u < g.ny ? 4u * by + 4u : g.ny;
            const uint32_t ez = 4u * bz + 4u < g.nz ? 4u * bz + 4u : g.nz;
            const v3 lo = mk3(g.ox + (float)(4u * bx) * g.cx, g.oy + (float)(4u * by) * g.cy, g.oz + (float)(4u * bz) * g.cz);
            const v3 hi = mk3(g.ox + (float)ex * g.cx, g.oy + (float)ey * g.cy, g.oz + (float)ez * g.cz);
            box_row(M, 0, lo, hi, I.glx, I.ghx);
            box_row(M, 1, lo, hi, I.gly, I.ghy);
            box_row(M, 2, lo, hi, I.glz, I.ghz);
        }
        if (count == 1u) hit = inside;   // one leaf: no tree to prove a brick empty with
        bool wants = inside && !hit;
        int cur = root, sp = 0;
        bool walking = root >= 0;
        while (walking && __ballot(wants) != 0ull) {
            cur = __builtin_amdgcn_readfirstlane(cur);
            const uint4* np = (const uint4*)((const char*)node32 + ((size_t)(uint32_t)cur << 5));
            const uint4 n0 = np[0], n1 = np[1];
            const int lkx = (int)n1.z, lky = (int)n1.w;
            bool keepL, keepR;
            if (DIST) {
                float kL, kR;
                P.children(B, n0, n1, a.best, keepL, keepR, kL, kR);
            } else {
                keepL = keep(I, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
                keepR = keep(I, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
            }
            // a lane that keeps a leaf's box is a candidate, and wants nothing more
            hit = hit || (wants && ((keepL && lkx < 0) || (keepR && lky < 0)));
            wants = inside && !hit;
            const bool intL = lkx >= 0 && __ballot(keepL && wants) != 0ull, intR = lky >= 0 && __ballot(keepR && wants) != 0ull;
            if (intL && intR) {
                // (sp < QSTACK_MAX always, as in grid_walk: the test keeps every store and every pop inside the array)
                if (sp < QSTACK_MAX) {
                    stack[sp] = lky;
                    sp++;
                }
            }
            cur = intL ? lkx : lky;
            if (!(intL || intR)) {
                if (sp == 0) walking = false;
                else {
                    sp--;
                    cur = stack[sp];
                }
            }
        }
        if (inside) cand[((size_t)bz * g.nby + by) * g.nbx + bx] = (uint8_t)hit;
    }
}

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, 8) void sparse_coarse_surface(CoarseArgs a, const uint4* __restrict__ node32, uint8_t* __restrict__ cand) {
    coarse_walk<false>(a, node32, cand);
}
__global__ __launch_bounds__(QUERY_BLOCK, 8) void sparse_coarse_distance(CoarseArgs a, const uint4* __restrict__ node32, uint8_t* __restrict__ cand) {
    coarse_walk<true>(a, node32, cand);
}

// brick-any: a byte per slot of the list, whether the brick holds anything
__global__ __launch_bounds__(QUERY_BLOCK, 4) void sparse_any_surface(GridArgs g, ListBricks l, const uint4* __restrict__ node32,
                                                                     const float4* __restrict__ tri48, uint8_t* __restrict__ any) {
    grid_walk<GRID_ANY>(g, l, node32, tri48, any);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void sparse_any_distance(GridArgs g, ListBricks l, float rmax, const uint4* __restrict__ node32,
                                                                      const float4* __restrict__ tri48, uint8_t* __restrict__ any) {
    dist_walk<DIST_ANY>(g, l, rmax, node32, tri48, nullptr, nullptr, nullptr, any);
}

// the fills: the dense answers of the list's bricks, slot by slot
__global__ __launch_bounds__(QUERY_BLOCK, 4) void sparse_fill_surface(GridArgs g, ListBricks l, const uint4* __restrict__ node32,
                                                                      const float4* __restrict__ tri48, uint64_t* __restrict__ words) {
    grid_walk<GRID_SURFACE>(g, l, node32, tri48, words);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void sparse_fill_distance(GridArgs g, ListBricks l, float rmax, const uint4* __restrict__ node32,
                                                                       const float4* __restrict__ tri48, float* __restrict__ dist,
                                                                       int32_t* __restrict__ tri) {
    dist_walk<DIST_SLOTS>(g, l, rmax, node32, tri48, dist, tri, nullptr, nullptr);
}
__global__ __launch_bounds__(QUERY_BLOCK, 4) void sparse_fill_records(GridArgs g, ListBricks l, float rmax, const uint4* __restrict__ node32,
                                                                      const float4* __restrict__ tri48, float4* __restrict__ hits) {
    dist_walk<DIST_RECORDS>(g, l, rmax, node32, tri48, nullptr, nullptr, hits, nullptr);
}

// signed, before the sign kernel: the centres of a slab of the list as psm_point_query records in lane order (grid_centres'
// arithmetic; a voxel outside dims gets a centre too: its record is a miss and casts no ray)
__global__ __launch_bounds__(QUERY_BLOCK, 8) void sparse_centres(GridArgs g, ListBricks l, float4* __restrict__ points) {
    const int lane = (int)threadIdx.x;
    for (uint32_t b = blockIdx.x; b < l.count(g); b += gridDim.x) {
        const Voxel v = voxel_of(g, l.brick(g, b), lane);
        points[(size_t)b * QUERY_BLOCK + lane] =
            make_float4(g.ox + ((float)v.ix + 0.5f) * g.cx, g.oy + ((float)v.iy + 0.5f) * g.cy, g.oz + ((float)v.iz + 0.5f) * g.cz, 0.f);
    }
}

// signed, after it: the slab's records into dist / tri [slot][64]
__global__ __launch_bounds__(QUERY_BLOCK, 8) void sparse_unpack(uint32_t bricks, const float4* __restrict__ hits, float* __restrict__ dist,
                                                                int32_t* __restrict__ tri) {
    const int lane = (int)threadIdx.x;
    for (uint32_t b = blockIdx.x; b < bricks; b += gridDim.x) {
        const size_t i = (size_t)b * QUERY_BLOCK + lane;
        const float4 h = hits[i];
        dist[i] = h.z;
        if (tri) tri[i] = __float_as_int(h.w);
    }
}

// ---- the ordered compaction: a byte per entry -> the ascending indices of the non-zero ones (or src's values at them) and their
// number. Three launches, the house pattern of the build's leaf compaction (bvh.hip): a count per workgroup, one workgroup's
// exclusive scan of the counts, a scatter by rank. n entries, or with d_n the number on the device (at most n). No atomics: the
// list is the same under every schedule.

__global__ __launch_bounds__(256) void sparse_count(const uint8_t* __restrict__ flags, uint32_t n, const uint32_t* __restrict__ d_n,
                                                    uint32_t* __restrict__ blockCounts) {
    __shared__ uint32_t wsum[4];
    if (d_n) n = *d_n < n ? *d_n : n;
    uint32_t mine = 0;
    for (uint32_t r = 0; r < 4u; r++) {
        const uint32_t i = blockIdx.x * SCAN_BLOCK + r * 256u + threadIdx.x;
        mine += (uint32_t)__popcll(__ballot(i < n && flags[i] != 0));
    }
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) blockCounts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of nb counts in place; the total -> *total_out (bvh.hip's scan_blocks)
__global__ __launch_bounds__(1024) void sparse_scan(uint32_t* __restrict__ g, uint32_t nb, uint32_t* __restrict__ total_out) {
    __shared__ uint32_t tmp[33];
    const uint32_t total = block_scan_array_1024(g, g, nb, tmp);
    if (threadIdx.x == 0) *total_out = total;
}

// entry i goes to rank = the non-zero entries before it, if that is below capacity: out[rank] = src ? src[i] : i
__global__ __launch_bounds__(256) void sparse_scatter(const uint8_t* __restrict__ flags, uint32_t n, const uint32_t* __restrict__ d_n,
                                                      const uint32_t* __restrict__ blockBase, const uint32_t* __restrict__ src,
                                                      uint32_t* __restrict__ out, uint32_t capacity) {
    __shared__ uint32_t wsum[4][4];
    if (d_n) n = *d_n < n ? *d_n : n;
    const int w = threadIdx.x >> 6;
    bool f[4];
    uint64_t bal[4];
    for (uint32_t r = 0; r < 4u; r++) {
        const uint32_t i = blockIdx.x * SCAN_BLOCK + r * 256u + threadIdx.x;
        f[r] = i < n && flags[i] != 0;
        bal[r] = __ballot(f[r]);
        if (lane_id() == 0) wsum[r][w] = (uint32_t)__popcll(bal[r]);
    }
    __syncthreads();
    uint32_t base = blockBase[blockIdx.x];
    for (uint32_t r = 0; r < 4u; r++) {
        uint32_t before = 0;
        for (int q = 0; q < w; q++) before += wsum[r][q];
        if (f[r]) {
            const uint32_t i = blockIdx.x * SCAN_BLOCK + r * 256u + threadIdx.x;
            const uint32_t to = base + before + (uint32_t)__popcll(bal[r] & lanemask_lt());
            if (to < capacity) out[to] = src ? src[i] : i;
        }
        base += wsum[r][0] + wsum[r][1] + wsum[r][2] + wsum[r][3];
    }
}

namespace {

// the listing calls' scratch, per context (grown on demand; every call runs on the context's stream, never two at once): a byte
// per brick (the candidates' flags, then the bytes of brick-any), a count per SCAN_BLOCK entries, the candidates' number, and
// with the coarse pass the candidates' ids. At most 5 bytes a brick + 4 a SCAN_BLOCK + 256
struct SparseScratch {
    void* ptr = nullptr;
    size_t bytes = 0;
};
std::mutex sparse_mu;
std::unordered_map<const psm_ctx*, SparseScratch> sparse_area;

struct SparseAreas {
    uint8_t* flags;
    uint32_t* blocks;
    uint32_t* ncand;
    uint32_t* cand;
};

size_t round256(size_t v) { return (v + 255u) & ~(size_t)255u; }

int sparse_scratch(psm_ctx* c, uint64_t bricks, bool coarse, SparseAreas& a) {
    const size_t nblk = (size_t)((bricks + SCAN_BLOCK - 1) / SCAN_BLOCK);
    const size_t off_blocks = round256((size_t)bricks), off_n = off_blocks + round256(nblk * 4u), off_cand = off_n + 256u;
    const size_t need = off_cand + (coarse ? (size_t)bricks * 4u : 0u);
    std::lock_guard<std::mutex> lk(sparse_mu);
    SparseScratch& s = sparse_area[c];
    if (s.bytes < need) {
        // (a kernel that reads the old area is in stream order before the free)
        if (s.ptr) PSM_HIP(c, hipStreamSynchronize(c->stream));
        if (s.ptr) PSM_HIP(c, hipFree(s.ptr));
        s = SparseScratch();
        PSM_HIP(c, hipMalloc(&s.ptr, need));
        s.bytes = need;
    }
    char* p = (char*)s.ptr;
    a.flags = (uint8_t*)p;
    a.blocks = (uint32_t*)(p + off_blocks);
    a.ncand = (uint32_t*)(p + off_n);
    a.cand = coarse ? (uint32_t*)(p + off_cand) : nullptr;
    return PSM_OK;
}

// PSM_SPARSE_COARSE = 0 turns the coarse pass off (a study knob: psm_hip.h); the lists are the same either way
bool coarse_on() {
    const char* knob = getenv("PSM_SPARSE_COARSE");
    return knob ? knob[0] != '0' : true;
}

// The coarse radius of a distance listing as its bound: R = ((rmax + 1.5 |cell|) + 2^-18 E) (1 + 2^-10), E the largest
// coordinate magnitude of the grid, and fl(R^2) (1 + 2^-20) + 2^-126 as PointBody::begin makes a bound of a radius (DESIGN.md
// 4.33 derives the two slacks). Overflow gives +inf: every box is kept
float coarse_bound(const psm_grid* grid, float rmax) {
    const float cx = grid->cell[0], cy = grid->cell[1], cz = grid->cell[2];
    const float off = 1.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
    float E = 0.f;
    for (int k = 0; k < 3; k++) {
        const float e = fabsf(grid->origin[k]) + ((float)grid->dims[k] + 4.0f) * grid->cell[k];
        E = e > E ? e : E;
    }
    const float R = ((rmax + off) + E * 0x1p-18f) * (1.0f + 0x1p-10f);
    const float best = (R * R) * 1.00000095367431640625f + 0x1p-126f;
    return best == best ? best : __builtin_inff();
}

// flags[0 .. n) (n on the host, and with d_n on the device) -> out, *d_total
int compact(psm_ctx* c, const SparseAreas& a, uint32_t n, const uint32_t* d_n, const uint32_t* src, uint32_t* out, uint32_t capacity,
            uint32_t* d_total) {
    const uint32_t nblk = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    sparse_count<<<nblk, 256, 0, c->stream>>>(a.flags, n, d_n, a.blocks);
    PSM_HIP(c, hipGetLastError());
    sparse_scan<<<1, 1024, 0, c->stream>>>(a.blocks, nblk, d_total);
    PSM_HIP(c, hipGetLastError());
    if (capacity == 0u) return PSM_OK;
    sparse_scatter<<<nblk, 256, 0, c->stream>>>(a.flags, n, d_n, a.blocks, src, out, capacity);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

// what the five calls refuse after the dense calls' front and state: a NULL list where one is read or written, a grid of more
// bricks than the listing's scratch is laid out for
int sparse_back(psm_ctx* c, const char* name, const GridShape& s, bool ids_ok) {
    const int rc = mesh_pointers(c, name, ids_ok);
    if (rc != PSM_OK) return rc;
    if (s.bricks > PSM_GRID_SPARSE_BRICKS_MAX) return mesh_refuse(c, PSM_ERR_CAPACITY, "%s: more than 2^27 bricks", name);
    return PSM_OK;
}

// A listing call: the dense calls' front (the count is the output it names) and state, the list pointer and the brick cap --
// all on the host, before any launch, the outputs untouched --, then the four steps above
int sparse_list(psm_bvh* b, const psm_grid* grid, bool dist, float rmax, uint32_t capacity, uint32_t* d_ids, uint32_t* d_count) {
    if (!b) return PSM_ERR_INVALID;
    psm_ctx* c = b->ctx;
    const char* name = dist ? "psm_grid_sparse_distance_bricks_dev" : "psm_grid_sparse_surface_bricks_dev";
    GridShape s;
    int rc = grid_front(c, name, grid, d_count, s, "ids or count", (const void*)((uintptr_t)d_ids | (uintptr_t)d_count), 4, dist ? &rmax : nullptr,
                        nullptr);
    if (rc == PSM_OK) rc = grid_built(b);
    if (rc == PSM_OK) rc = sparse_back(c, name, s, d_ids || capacity == 0u);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    const bool coarse = coarse_on() && !(dist && std::isinf(rmax));
    SparseAreas a;
    rc = sparse_scratch(c, s.bricks, coarse, a);   // (the last thing that can fail before the outputs change)
    if (rc != PSM_OK) return rc;
    const uint32_t bricks = (uint32_t)s.bricks;
    GridArgs g = grid_args(grid, s);
    g.sm = b->d_small; g.sorted_tri = b->d_sorted_tri;
    ListBricks l = {nullptr, nullptr, bricks, bricks};
    if (coarse) {
        CoarseArgs ca = {};
        ca.g = g;
        ca.nbz = s.nb[2];
        ca.sbx = (s.nb[0] + 3u) / 4u; ca.sby = (s.nb[1] + 3u) / 4u;
        ca.supers = ca.sbx * ca.sby * ((s.nb[2] + 3u) / 4u);
        ca.best = dist ? coarse_bound(grid, rmax) : 0.f;
        if (dist) sparse_coarse_distance<<<grid_for(ca.supers), QUERY_BLOCK, 0, c->stream>>>(ca, b->d_node32, a.flags);
        else sparse_coarse_surface<<<grid_for(ca.supers), QUERY_BLOCK, 0, c->stream>>>(ca, b->d_node32, a.flags);
        PSM_HIP(c, hipGetLastError());
        rc = compact(c, a, bricks, nullptr, nullptr, a.cand, bricks, a.ncand);
        if (rc != PSM_OK) return rc;
        l.ids = a.cand; l.d_n = a.ncand;
    }
    // (brick-any writes slot i's byte where candidate flag i was: the compaction above has read the flags, in stream order)
    if (dist) sparse_any_distance<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g, l, rmax, b->d_node32, b->d_tri48, a.flags);
    else sparse_any_surface<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g, l, b->d_node32, b->d_tri48, a.flags);
    PSM_HIP(c, hipGetLastError());
    return compact(c, a, bricks, l.d_n, l.ids, d_ids, capacity, d_count);
}

enum { FILL_SURFACE = 0, FILL_DISTANCE = 1, FILL_SIGNED = 2 };
const char* const FILL_NAME[] = {"psm_grid_sparse_surface_dev", "psm_grid_sparse_distance_dev", "psm_grid_sparse_signed_distance_dev"};

// A filling call: the same front, state and back, then the dense walk over the list; signed in slabs of the list, as dist_query
// (grid_dist.hip) works in slabs of the grid: the centres, the walk's records beside them, query.hip's sign kernel, the unpack
int sparse_fill(psm_bvh* b, const psm_grid* grid, int call, float rmax, uint32_t samples, const uint32_t* d_ids, uint32_t n, void* d_out,
                int32_t* d_tri) {
    if (!b) return PSM_ERR_INVALID;
    psm_ctx* c = b->ctx;
    const char* name = FILL_NAME[call];
    GridShape s;
    int rc = call == FILL_SURFACE
                 ? grid_front(c, name, grid, d_out, s, "words or ids", (const void*)(((uintptr_t)d_out & 7u) | ((uintptr_t)d_ids & 3u)), 8, nullptr, nullptr)
                 : grid_front(c, name, grid, d_out, s, "dist, tri or ids", (const void*)((uintptr_t)d_out | (uintptr_t)d_tri | (uintptr_t)d_ids), 4, &rmax,
                              call == FILL_SIGNED ? &samples : nullptr);
    if (rc == PSM_OK) rc = grid_built(b);
    if (rc == PSM_OK) rc = sparse_back(c, name, s, d_ids || n == 0u);
    if (rc != PSM_OK || n == 0u) return rc;
    (void)hipSetDevice(c->device);
    GridArgs g = grid_args(grid, s);
    g.sm = b->d_small; g.sorted_tri = b->d_sorted_tri;
    ListBricks l = {d_ids, nullptr, n, (uint32_t)s.bricks};
    if (call == FILL_SURFACE) {
        sparse_fill_surface<<<grid_for(n), QUERY_BLOCK, 0, c->stream>>>(g, l, b->d_node32, b->d_tri48, (uint64_t*)d_out);
        PSM_HIP(c, hipGetLastError());
        return PSM_OK;
    }
    if (call == FILL_DISTANCE) {
        sparse_fill_distance<<<grid_for(n), QUERY_BLOCK, 0, c->stream>>>(g, l, rmax, b->d_node32, b->d_tri48, (float*)d_out, d_tri);
        PSM_HIP(c, hipGetLastError());
        return PSM_OK;
    }
    GridSlabs a;
    rc = slabs_for(c, n, true, a);   // (the last thing that can fail before the outputs change)
    if (rc != PSM_OK) return rc;
    return grid_slabs(n, a.slab, [&](uint32_t first, uint32_t bricks) -> int {
        const ListBricks part = {d_ids + first, nullptr, bricks, (uint32_t)s.bricks};
        sparse_centres<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g, part, a.points);
        PSM_HIP(c, hipGetLastError());
        sparse_fill_records<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(g, part, rmax, b->d_node32, b->d_tri48, a.hits);
        PSM_HIP(c, hipGetLastError());
        const int rc = sign_launch(b, a.points, (size_t)bricks * QUERY_BLOCK, samples, a.hits);
        if (rc != PSM_OK) return rc;
        const size_t at = (size_t)first * QUERY_BLOCK;
        sparse_unpack<<<grid_for(bricks), QUERY_BLOCK, 0, c->stream>>>(bricks, a.hits, (float*)d_out + at, d_tri ? d_tri + at : nullptr);
        PSM_HIP(c, hipGetLastError());
        return PSM_OK;
    });
}

}  // namespace

// for grid_release (grid.hip): the listing calls' scratch goes with the context
void sparse_release(psm_ctx* c) {
    std::lock_guard<std::mutex> lk(sparse_mu);
    auto it = sparse_area.find(c);
    if (it == sparse_area.end()) return;
    if (it->second.ptr) (void)hipFree(it->second.ptr);
    sparse_area.erase(it);
}

}  // namespace psm

int psm_grid_sparse_surface_bricks_dev(psm_bvh* bvh, const psm_grid* grid, uint32_t capacity, uint32_t* d_ids, uint32_t* d_count) {
    return psm::sparse_list(bvh, grid, false, 0.f, capacity, d_ids, d_count);
}

int psm_grid_sparse_distance_bricks_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, uint32_t capacity, uint32_t* d_ids, uint32_t* d_count) {
    return psm::sparse_list(bvh, grid, true, rmax, capacity, d_ids, d_count);
}

int psm_grid_sparse_surface_dev(psm_bvh* bvh, const psm_grid* grid, const uint32_t* d_ids, uint32_t n, uint64_t* d_words) {
    return psm::sparse_fill(bvh, grid, psm::FILL_SURFACE, 0.f, 0, d_ids, n, d_words, nullptr);
}

int psm_grid_sparse_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, const uint32_t* d_ids, uint32_t n, float* d_dist,
                                 int32_t* d_tri) {
    return psm::sparse_fill(bvh, grid, psm::FILL_DISTANCE, rmax, 0, d_ids, n, d_dist, d_tri);
}

int psm_grid_sparse_signed_distance_dev(psm_bvh* bvh, const psm_grid* grid, float rmax, uint32_t samples, const uint32_t* d_ids, uint32_t n,
                                        float* d_dist, int32_t* d_tri) {
    return psm::sparse_fill(bvh, grid, psm::FILL_SIGNED, rmax, samples, d_ids, n, d_dist, d_tri);
}
