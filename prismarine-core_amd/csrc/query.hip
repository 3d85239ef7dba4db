// query.hip -- batched ray queries against a built hierarchy: closest hit and any hit (new; no reference counterpart).
//
// psm_rt_traverse follows directTraverse.comp bit for bit: a 16-entry stack that drops subtrees (STACK_CAP), a PZERO-tolerant
// "closest", intersectTriangle's clamp of |det| at 1e-6. These kernels answer "what does this ray hit?" exactly instead
// (include/psm_hip.h, psm_query_ray):
//   * the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI), tested by tri_test's arithmetic without the clamp;
//   * a hit counts iff tmin <= t <= tmax; closest = the smallest t, on bit-equal t the lowest triangle id -- a result that does
//     not depend on the traversal order;
//   * the stack never drops an entry: 16 levels in LDS, the rest in a per-lane global area sized to the builder's height bound.
// Structure as rt_traverse (trace.hip): one ray per lane, one wave64 per workgroup, the stack in LDS laid out [depth][lane],
// child boxes by fmaf on the fp16 record coordinates (v_fma_mix_f32), nearer child first. The kernels are grid-stride.
#include <mutex>
#include <unordered_map>

#include "psm_common.h"
#include "psm_internal.h"

namespace psm {

constexpr int SM_M = 0;        // bvh.hip: the fit transform (16 floats, row-major)
constexpr int SM_COUNT = 24;   // bvh.hip: leaf count
constexpr int SM_ROOT = 25;    // bvh.hip: root link (-1: fewer than two leaves)

constexpr int QUERY_BLOCK = 64;          // one wave per workgroup (rt_traverse: TRAV_BLOCK)
constexpr int QSTACK_LDS = 16;           // stack entries per lane in LDS: 4 KB per wave, as rt_traverse's
// The builder's height bound (bvh_emit): above a run of equal Morton codes every internal node's range shares a strictly longer
// key prefix than its parent's (the split is the highest differing bit), and a 63-bit code has prefixes of 1..63 bits: at most
// 63 such levels. A run of equal codes is split at the median (findSplit), ceil(log2 N) more levels for N <= 2^27 leaves. A ray's
// stack holds at most one entry per internal ancestor of its current node: 63 + 27 = 90 entries.
constexpr int QSTACK_MAX = 96;
#ifndef PSM_QUERY_GRID_CAP
#define PSM_QUERY_GRID_CAP 8192
#endif
// workgroups of a launch at most: 32 waves per CU, all the chip holds at 8 waves per SIMD (4096: 0.54 / 1.41 ms against 0.49 / 0.99 ms for
// 2 M primary / bounce rays, profiles/query_r06.txt); the spill area has a lane for each (80 x 8192 x 64 x 4 B = 168 MB per context)
constexpr uint32_t QUERY_GRID_CAP = PSM_QUERY_GRID_CAP;

struct QueryArgs {
    const float4* rays;      // psm_query_ray: origin.xyz tmin | direct.xyz tmax
    size_t n;
    const uint4* node32;     // the build's traversal records (bvh_emit)
    const float4* tri48;     // v0, e1, e2 per triangle (bvh_prepare_tris / bvh_load_mesh)
    const uint32_t* sm;      // transform, leaf count, root
    const int32_t* sorted_tri;  // [0]: the lone leaf's triangle when the leaf count is 1 (bvh_segtree<true> writes it)
    int* spill;              // [QSTACK_MAX - QSTACK_LDS][gridDim.x * 64]
    float4* hits;            // closest: psm_hit per ray
    uint8_t* occluded;       // any: 0 / 1 per ray
};

// tri_test (trace.hip) operation for operation, with invDev = 1 / det instead of 1 / (max(|det|, 1e-6) * sign(det)) and without
// its `t >= -PZERO` rule (the caller's window decides). det == 0 is a miss; u, v, u + v keep the 1e-5 tolerances. Where
// |det| >= 1e-6 the values are tri_test's bit for bit. Returns false on a miss; t may be NaN (no window holds it).
PSM_D bool tri_query(const float4* __restrict__ tri48, int tri, v3 orig, v3 dir, float& T, float& U, float& V) {
    const float4 a = tri48[(size_t)3 * tri + 0], b = tri48[(size_t)3 * tri + 1], c = tri48[(size_t)3 * tri + 2];
    const v3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(b.x, b.y, b.z), e2 = mk3(c.x, c.y, c.z);
    const v3 pvec = cross3(dir, e2);
    const float det = dot3(e1, pvec);
    if (pabs(det) <= 0.0f) return false;
    const float invDev = 1.f / det;
    const v3 tvec = orig - v0;
    const float u = dot3(tvec, pvec) * invDev;
    if (u < -0.00001f || u > 1.00001f) return false;
    const v3 qvec = cross3(tvec, e1);
    const float v = dot3(dir, qvec) * invDev;
    if (v < -0.00001f || (u + v) > 1.00001f) return false;
    T = dot3(e2, qvec) * invDev;
    U = u;
    V = v;
    return true;
}

namespace {

PSM_D bool finite3(v3 a) { return __builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z); }

// One axis of the ray in the build's normalised space, set up so that a box plane b gives its (inflated) distance in ONE fmaf:
//   P = (M (o, 1)).k, D = (M (d, 0)).k      -- the affine map aabbmaker applied to the vertices (mat_vec with w = 1; the w row is
//                                             never read), applied to the line o + t d: the slab distances are WORLD t
//   lo plane: fmaf(b, inv, nlo) = (b - (P + h)) / D,  hi plane: fmaf(b, inv, nhi) = (b - (P - h)) / D
// i.e. the box grown by h on both sides (for either sign of D). h covers the rounding of P, D and the slab arithmetic: each is a
// few ulps of |b| + S (S = |m0 ox| + |m1 oy| + |m2 oz| + |m3| bounds |P| and the rounding of its sum), and the error of D moves the
// plane distance by t |dD| <= 3 eps t sum_j |M_kj d_j|, which for the fit transform (M's 3 x 3 part is diagonal unless the build's
// optimisation matrix rotates) is 3 eps |b - P| <= 3 eps (1 + S). All of it is < 8 eps (2 + S); h = 2^-16 (2 + S) ~ 128 eps (2 + S)
// -- with a 16x margin left for an optimisation matrix whose 3 x 3 part has a condition number up to ~16. A box is then dropped
// only when its exact slab interval misses [tmin, limit]. The hit itself lies in its leaf's exact box: an accepted hit point is
// within ~1e-5 edge lengths of its triangle (the u, v tolerances), and the leaf box is the triangle's padded by PZERO = 5e-4
// before the fp16 rounding (<= 2.44e-4 in [0, 1]), >= 2.5e-4 normalised units of headroom.
// A direction component under 1e-20 in magnitude is taken as +-1e-20 (no infinite reciprocal): the line moves by t * 1e-20,
// below h for every t < 1e15.
struct Axis {
    float inv, nlo, nhi;
};
PSM_D Axis ray_axis(const float* M, int k, v3 o, v3 d) {
    const float m0 = M[4 * k + 0], m1 = M[4 * k + 1], m2 = M[4 * k + 2], m3 = M[4 * k + 3];
    const float P = ((m0 * o.x + m1 * o.y) + m2 * o.z) + m3;
    float D = (m0 * d.x + m1 * d.y) + m2 * d.z;
    const float S = ((pabs(m0 * o.x) + pabs(m1 * o.y)) + pabs(m2 * o.z)) + pabs(m3);
    const float h = (2.0f + S) * 0x1p-16f;
    if (!(pabs(D) >= 1e-20f)) D = __builtin_copysignf(1e-20f, D);
    Axis a;
    a.inv = 1.0f / D;
    a.nlo = -(P + h) * a.inv;
    a.nhi = (h - P) * a.inv;
    return a;
}

// slab test of one child box (slab_child, trace.hip, without the reference's PZERO rules): near / far of the inflated box
PSM_D void slab(const Axis& X, const Axis& Y, const Axis& Z, float mnx, float mny, float mnz, float mxx, float mxy, float mxz,
                float& tNear, float& tFar) {
    const float ax = fmaf(mnx, X.inv, X.nlo), bx = fmaf(mxx, X.inv, X.nhi);
    const float ay = fmaf(mny, Y.inv, Y.nlo), by = fmaf(mxy, Y.inv, Y.nhi);
    const float az = fmaf(mnz, Z.inv, Z.nlo), bz = fmaf(mxz, Z.inv, Z.nhi);
    tNear = smaxf(smaxf(sminf(ax, bx), sminf(ay, by)), sminf(az, bz));
    tFar = sminf(sminf(smaxf(ax, bx), smaxf(ay, by)), smaxf(az, bz));
}

template <bool ANY>
PSM_D void query_body(const QueryArgs& a) {
    __shared__ int stack[QSTACK_LDS][QUERY_BLOCK];
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const size_t spill_stride = (size_t)gridDim.x * QUERY_BLOCK;
    int* __restrict__ spill = a.spill + (size_t)blockIdx.x * QUERY_BLOCK + lane;
    const uint4* __restrict__ node32 = a.node32;
    const float4* __restrict__ tri48 = a.tri48;
    const int root = (int)a.sm[SM_ROOT];
    const uint32_t count = a.sm[SM_COUNT];
    const int lone = (count == 1u) ? a.sorted_tri[0] : -1;   // one leaf: no tree, the leaf's triangle is the only candidate
    for (size_t i = (size_t)blockIdx.x * QUERY_BLOCK + (size_t)lane; i - (size_t)lane < a.n; i += spill_stride) {
        const bool alive = i < a.n;
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        const v3 o = mk3(r0.x, r0.y, r0.z);
        const v3 d = normalize3(mk3(r1.x, r1.y, r1.z));   // t is the distance along the unit direction (as the oracle's brute force)
        const float tmin = r0.w, tmax = r1.w;
        // NaN anywhere, a zero direction (normalize3 gives NaN) or an empty window: a miss
        const bool valid = alive && finite3(o) && finite3(d) && tmin <= tmax;
        float best = tmax, bu = 0.f, bv = 0.f;
        int btri = -1;
        bool found = false;
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        const Axis X = ray_axis(M, 0, o, d), Y = ray_axis(M, 1, o, d), Z = ray_axis(M, 2, o, d);
        // a candidate triangle: inside the window, and (closest) before the best so far or as far and of a lower id
        // ((uint32_t) btri: -1 is the largest, so the first hit inside the window always counts)
        auto test = [&](int tri) {
            float t, u, v;
            if (tri_query(tri48, tri, o, d, t, u, v) && t >= tmin && (t < best || (t == best && (uint32_t)tri < (uint32_t)btri))) {
                found = true;
                if (!ANY) { best = t; bu = u; bv = v; btri = tri; }
            }
        };
        if (valid && lone >= 0) test(lone);
        int cur = root, sp = 0;
        bool walking = valid && root >= 0;
        while (walking) {
            const uint4* np = (const uint4*)((const char*)node32 + ((uint32_t)cur << 5));
            const uint4 n0 = np[0], n1 = np[1];
            const int lkx = (int)n1.z, lky = (int)n1.w;
            float nL, fL, nR, fR;
            slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
            slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
            // closest: pruned against the best hit so far (a hit at exactly `best` with a lower id still counts: <=)
            const float lim = ANY ? tmax : best;
            const bool okL = (nL <= fL) & (nL <= lim) & (fL >= tmin);
            const bool okR = (nR <= fR) & (nR <= lim) & (fR >= tmin);
            const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
            // the accepted leaves, one test after the other (one copy of the triangle code in the loop)
            int t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
            int t1 = (leafL && leafR) ? ~lky : -1;
            while (t0 >= 0) {
                test(t0);
                t0 = t1;
                t1 = -1;
            }
            if (ANY && found) break;   // any hit: the lane retires at its first hit
            const bool intL = okL && !leafL, intR = okR && !leafR;
            const bool leftFirst = intL && (!intR || nL <= nR);   // nearer child first
            const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
            if (intL && intR) {
                // (sp < QSTACK_MAX always: see QSTACK_MAX; the host refuses hierarchies whose bound exceeds it)
                if (sp < QSTACK_LDS) stack[sp][lane] = second;
                else if (sp < QSTACK_MAX) spill[(size_t)(sp - QSTACK_LDS) * spill_stride] = second;
                sp++;
            }
            cur = first;
            if (!(intL || intR)) {
                if (sp == 0) break;
                sp--;
                cur = sp < QSTACK_LDS ? stack[sp][lane] : spill[(size_t)(sp - QSTACK_LDS) * spill_stride];
            }
        }
        if (alive) {
            if (ANY) a.occluded[i] = found ? 1 : 0;
            else a.hits[i] = found ? make_float4(bu, bv, best, __int_as_float(btri)) : make_float4(0.f, 0.f, __builtin_inff(), __int_as_float(-1));
        }
    }
}

}  // namespace

// the two kernels, under names of their own (profiles and the codegen test find them by these)
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_closest(QueryArgs a) { query_body<false>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_any(QueryArgs a) { query_body<true>(a); }

namespace {

// the stack entries beyond the LDS part, per context: one column per lane of a launch (allocated on the context's first query)
std::mutex spill_mu;
std::unordered_map<const psm_ctx*, void*> spill_area;

int spill_for(psm_ctx* c, void** out) {
    std::lock_guard<std::mutex> lk(spill_mu);
    void*& p = spill_area[c];
    if (!p) {
        const size_t bytes = (size_t)(QSTACK_MAX - QSTACK_LDS) * QUERY_GRID_CAP * QUERY_BLOCK * sizeof(int);
        PSM_HIP(c, hipMalloc(&p, bytes));
    }
    *out = p;
    return PSM_OK;
}

// ceil(log2(n)) for n >= 1
int ceil_log2(size_t n) {
    int k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

template <bool ANY>
int query(psm_bvh* b, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits, uint8_t* d_hit) {
    if (!b) return PSM_ERR_INVALID;
    if (n == 0) return PSM_OK;
    psm_ctx* c = b->ctx;
    if (!d_rays || (ANY ? (const void*)d_hit : (const void*)d_hits) == nullptr)
        return set_err(c, PSM_ERR_INVALID, ANY ? "psm_bvh_occluded_dev: NULL pointer" : "psm_bvh_intersect_dev: NULL pointer");
    if (((uintptr_t)d_rays & 15u) != 0 || (!ANY && ((uintptr_t)d_hits & 15u) != 0))
        return set_err(c, PSM_ERR_INVALID, ANY ? "psm_bvh_occluded_dev: rays not 16-byte aligned"
                                               : "psm_bvh_intersect_dev: rays or hits not 16-byte aligned");
    (void)hipSetDevice(c->device);
    if (!b->built) return set_err(c, PSM_ERR_STATE, "ray query before build");
    if (63 + ceil_log2(b->cap) > QSTACK_MAX) return set_err(c, PSM_ERR_CAPACITY, "ray query: hierarchy deeper than the query stack");
    void* spill = nullptr;
    const int rc = spill_for(c, &spill);   // (a context's first query allocates: a later one can be captured into a graph)
    if (rc != PSM_OK) return rc;
    const size_t waves = (n + QUERY_BLOCK - 1) / QUERY_BLOCK;
    const uint32_t grid = (uint32_t)(waves < QUERY_GRID_CAP ? waves : QUERY_GRID_CAP);
    QueryArgs qa = {};
    qa.rays = (const float4*)d_rays; qa.n = n;
    qa.node32 = b->d_node32; qa.tri48 = b->d_tri48; qa.sm = b->d_small; qa.sorted_tri = b->d_sorted_tri;
    qa.spill = (int*)spill;
    qa.hits = (float4*)d_hits; qa.occluded = d_hit;
    if (ANY) bvh_query_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(qa);
    else bvh_query_closest<<<grid, QUERY_BLOCK, 0, c->stream>>>(qa);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace

// psm_ctx_destroy (api.hip): the context's spill area goes with it (the stream has been synchronised)
void query_release(psm_ctx* c) {
    std::lock_guard<std::mutex> lk(spill_mu);
    auto it = spill_area.find(c);
    if (it == spill_area.end()) return;
    if (it->second) (void)hipFree(it->second);
    spill_area.erase(it);
}

}  // namespace psm

int psm_bvh_intersect_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits) {
    return psm::query<false>(bvh, d_rays, n, d_hits, nullptr);
}

int psm_bvh_occluded_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::query<true>(bvh, d_rays, n, nullptr, d_hit);
}
