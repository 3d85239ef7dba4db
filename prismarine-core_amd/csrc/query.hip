// query.hip -- batched queries against a built hierarchy (new; no reference counterpart): closest hit and any hit of rays,
// closest point and within-radius of points (the point queries are described at point_body below), and the hit
// count of rays with the inside / outside and signed-distance queries of points built on it (CountRay below).
//
// psm_rt_traverse follows directTraverse.comp bit for bit: a 16-entry stack that drops subtrees (STACK_CAP), a PZERO-tolerant
// "closest", intersectTriangle's clamp of |det| at 1e-6. These kernels answer "what does this ray hit?" exactly instead
// (include/psm_hip.h, psm_query_ray):
//   * the candidates are the hierarchy's leaves (PSM_BVH_LEAF_TRI), tested by tri_test's arithmetic without the clamp;
//   * a hit counts iff tmin <= t <= tmax; closest = the smallest t, on bit-equal t the lowest triangle id -- a result that does
//     not depend on the traversal order;
//   * the stack never drops an entry: 16 levels in LDS, the rest in a per-lane global area sized to the builder's height bound.
// Structure as rt_traverse (trace.hip): one ray per lane, one wave64 per workgroup, the stack in LDS laid out [depth][lane],
// child boxes by fmaf on the fp16 record coordinates (v_fma_mix_f32), nearer child first. The kernels are grid-stride. The walk
// (query_walk: grid-stride loop, stack, leaf scheduling) is shared by the ray and the point kernels; a body says what a query is.
// The same seven queries over a list of hierarchies (scene_walk) and over posed instances (4.9) follow. The host
// side is one path for all 21 entry points: check_list / check_data / batch_args / launch over a per-family kernel table (4.10);
// psm_query_host.h declares the parts of it that world.hip's seven entry points go through as well (4.13).
#include <cmath>
#include <cstdio>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"    // the constants, QueryArgs, the triangle / box / point tests and query_walk (shared with kbest.hip, world.hip)
#include "psm_query_host.h"   // QueryKind, QueryDesc, Kernels, launch, batch_args; the checks defined below (shared with world.hip)

namespace psm {

namespace {

// the ray queries: closest hit (ANY = false) and any hit (ANY = true); psm_query_ray, DESIGN.md 4.5
template <bool ANY>
struct RayBody {
    const QueryArgs& a;
    v3 o, d;
    float tmin, tmax, best, bu, bv;
    int btri;
    bool found;
    Axis X, Y, Z;

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        o = mk3(r0.x, r0.y, r0.z);
        d = normalize3(mk3(r1.x, r1.y, r1.z));   // t is the distance along the unit direction (as the oracle's brute force)
        tmin = r0.w;
        tmax = r1.w;
        // NaN anywhere, a zero direction (normalize3 gives NaN) or an empty window: a miss
        const bool valid = alive && finite3(o) && finite3(d) && tmin <= tmax;
        best = tmax;
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        found = false;
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        X = ray_axis(M, 0, o, d);
        Y = ray_axis(M, 1, o, d);
        Z = ray_axis(M, 2, o, d);
        return valid;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        // closest: pruned against the best hit so far (a hit at exactly `best` with a lower id still counts: <=)
        const float lim = ANY ? tmax : best;
        okL = (nL <= fL) & (nL <= lim) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= lim) & (fR >= tmin);
    }
    // a candidate triangle: inside the window, and (closest) before the best so far or as far and of a lower id
    // ((uint32_t) btri: -1 is the largest, so the first hit inside the window always counts)
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(a.tri48, tri, o, d, t, u, v) && t >= tmin && (t < best || (t == best && (uint32_t)tri < (uint32_t)btri))) {
            found = true;
            if (!ANY) { best = t; bu = u; bv = v; btri = tri; }
        }
    }
    PSM_D bool done() const { return ANY && found; }   // any hit: the lane retires at its first hit
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (ANY) a.occluded[i] = found ? 1 : 0;
        else a.hits[i] = found ? make_float4(bu, bv, best, __int_as_float(btri)) : miss_hit();
    }
};

// the point queries: closest point (WITHIN = false) and within radius (WITHIN = true)
template <bool WITHIN>
struct PointBody {
    const QueryArgs& a;
    const PointBound B;
    v3 p;
    float rmax, best, bu, bv;   // best: the pruning bound -- the best d2 so far, the rmax bound until one is found
    int btri;
    bool found;
    PointImage P;

    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(a.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        rmax = q.w;
        const bool valid = alive && finite3(p) && rmax >= 0.f;   // NaN or negative rmax: a miss; +inf: no limit
        best = (rmax * rmax) * 1.00000095367431640625f + 0x1p-126f;   // fl(rmax^2) (1 + 2^-20) + 2^-126
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        found = false;
        float M[16];
        #pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        P.set(M, p);
        return valid;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        P.children(B, n0, n1, best, okL, okR, kL, kR);
    }
    // a candidate: within rmax, and (closest) nearer than the best so far or as near and of a lower id
    // ((uint32_t) btri: -1 is the largest; before the first, best is the rmax bound, >= every d2 that counts)
    PSM_D void leaf(int tri) {
        const float4 A = a.tri48[(size_t)3 * tri + 0], Bv = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        float u, v;
        const float d2 = closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(C.x, C.y, C.z), p, u, v);
        if (sqrtf(d2) <= rmax && (d2 < best || (d2 == best && (uint32_t)tri < (uint32_t)btri))) {
            found = true;
            if (!WITHIN) { best = d2; bu = u; bv = v; btri = tri; }
        }
    }
    PSM_D bool done() const { return WITHIN && found; }   // within: the lane retires at its first counting candidate
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (WITHIN) a.occluded[i] = found ? 1 : 0;
        else a.hits[i] = found ? make_float4(bu, bv, sqrtf(best), __int_as_float(btri)) : miss_hit();
    }
};

template <bool ANY>
PSM_D void query_body(const QueryArgs& a) {
    RayBody<ANY> q{a};
    query_walk(a, q);
}

template <bool WITHIN>
PSM_D void point_body(const QueryArgs& a) {
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
    PointBody<WITHIN> q{a, point_bound(M)};
    query_walk(a, q);
}

// ---- hit count, inside / outside, signed distance (include/psm_hip.h) ------------------------------------------

// The ray every one of these walks: all candidates with tri_query's acceptance and tmin <= t <= tmax are counted -- the any-hit
// predicate, asked "how many?". Against the any-hit body: a child box is kept against [tmin, tmax] only (there is no best t to
// prune by) and the lane never retires early. The count is a sum of integers: it does not depend on the traversal order, so the
// children's order key (the near distance, as the other ray bodies) is only a matter of memory locality.
struct CountRay {
    const QueryArgs& a;
    v3 o, d;
    float tmin, tmax;
    uint32_t count;
    Axis X, Y, Z;

    // aim the ray (dir: as given, normalised here as every query ray's) and clear the count; false: the ray is invalid (RayBody)
    PSM_D bool aim(v3 orig, v3 dir, float lo, float hi) {
        o = orig;
        d = normalize3(dir);
        tmin = lo;
        tmax = hi;
        count = 0u;
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        X = ray_axis(M, 0, o, d);
        Y = ray_axis(M, 1, o, d);
        Z = ray_axis(M, 2, o, d);
        return finite3(o) && finite3(d) && tmin <= tmax;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        okL = (nL <= fL) & (nL <= tmax) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= tmax) & (fR >= tmin);
    }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(a.tri48, tri, o, d, t, u, v) && t >= tmin && t <= tmax) count++;
    }
    PSM_D bool done() const { return false; }   // every crossing counts: the walk ends when the stack is empty
};

// hit count of a ray (psm_bvh_count_hits_dev)
struct CountBody : CountRay {
    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = a.rays[2 * i]; r1 = a.rays[2 * i + 1]; }
        return aim(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), r0.w, r1.w) && alive;
    }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const { a.count[i] = count; }
};

// inside / outside of a point (SIGN = false: psm_bvh_inside_dev) and the sign of a closest-point result (SIGN = true: the second
// kernel of psm_bvh_signed_distance_dev, after bvh_query_point has written hits[i]). One point per lane; its `samples` rays are
// walked one after the other (again()), so at any moment every lane of the wave follows the same direction from nearby origins.
// A ray votes "inside" iff its count is odd; the point is inside iff more than half of the rays vote so.
// SIGN: a point whose closest-point result is a miss (no triangle within rmax, an invalid query) walks nothing and keeps its
// record; the others get the sign bit of t set when inside (a distance of 0 becomes -0).
template <bool SIGN>
struct InsideBody : CountRay {
    v3 p;
    uint32_t k, votes;
    float dist;
    bool valid;

    PSM_D bool shoot() {
        const int r = __builtin_amdgcn_readfirstlane((int)k);   // (the same k in every lane that walks: the row by scalar loads)
        return aim(p, mk3(INSIDE_DIR[r][0], INSIDE_DIR[r][1], INSIDE_DIR[r][2]), 0.f, __builtin_inff());
    }
    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(a.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        k = 0u;
        votes = 0u;
        dist = 0.f;
        valid = alive;
        if (SIGN) {
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (alive) h = a.hits[i];
            dist = h.z;
            valid = __float_as_int(h.w) >= 0;
        }
        valid = shoot() && valid;   // (a non-finite p: outside)
        return valid;
    }
    PSM_D bool again() {
        votes += count & 1u;
        k++;
        if (!valid || k >= a.samples) return false;
        shoot();
        return true;
    }
    PSM_D void finish(size_t i) const {
        const bool in = 2u * votes > a.samples;
        if (!SIGN) a.occluded[i] = in ? 1 : 0;
        else if (in) ((float*)(a.hits + i))[2] = __uint_as_float(__float_as_uint(dist) | 0x80000000u);
    }
};

PSM_D void count_body(const QueryArgs& a) {
    CountBody q{{a}};
    query_walk(a, q);
}

template <bool SIGN>
PSM_D void inside_body(const QueryArgs& a) {
    InsideBody<SIGN> q{{a}};
    query_walk(a, q);
}

}  // namespace

// the kernels, under names of their own (profiles and the codegen tests find them by these)
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_closest(QueryArgs a) { query_body<false>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_any(QueryArgs a) { query_body<true>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_point(QueryArgs a) { point_body<false>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_within(QueryArgs a) { point_body<true>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_count(QueryArgs a) { count_body(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_inside(QueryArgs a) { inside_body<false>(a); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void bvh_query_sign(QueryArgs a) { inside_body<true>(a); }

// ---- scene queries: the seven queries over several hierarchies at once (include/psm_hip.h "scene queries") ------

// One geometry of a scene as a kernel reads it: QueryArgs' four hierarchy pointers. The table of a launch travels in the
// kernel-argument segment (PSM_SCENE_MAX_GEOMETRIES x 32 B = 1 KB): no device allocation, nothing that could go stale.
struct SceneGeom {
    const uint4* node32;
    const float4* tri48;
    const uint32_t* sm;
    const int32_t* sorted_tri;
};
struct SceneArgs {
    const float4* rays;      // as QueryArgs
    size_t n;
    int* spill;
    float4* hits;
    uint8_t* occluded;
    uint32_t* count;
    int32_t* geom;           // closest hit / closest point / signed distance: the winning geometry per query, -1 on a miss
    uint32_t samples;
    uint32_t geoms;          // G: 1 .. PSM_SCENE_MAX_GEOMETRIES
    SceneGeom g[PSM_SCENE_MAX_GEOMETRIES];
};

namespace {

// query_walk over a scene, as a walk of its own (the seven single-hierarchy kernels keep theirs, and with it their code): per
// query the geometries one after the other, geometry 0 first, each walked as query_walk walks its hierarchy. The geometry index
// is the same in every lane of the wave, so the four pointers, the root and the leaf count of a geometry are scalar loads from
// the kernel-argument table. The body carries its running state (best, count, parity, found) from one geometry to the next:
//   bool begin(i, alive)     load query i and clear the running state; false: the query misses without a walk
//   void enter(gm, g)        the per-geometry set-up (the ray's axes / the point's bound from that geometry's fit transform)
//   children, leaf, done, again, finish: as query_walk's; a lane that is done() skips the remaining geometries
//   again(): every geometry is walked again (the inside queries' next ray: its parity is summed over the whole scene)
// Args: SceneArgs, or the instanced queries' InstArgs (below): the same walk over a table whose entries also carry a pose. A
// body whose enter() returns bool says whether the query is valid in that entry (the instanced queries: validity is judged
// per instance, on the moved query); one that returns void is valid everywhere (the scene bodies, whose code this leaves as it was).
template <class Args, class Body>
PSM_D void scene_walk(const Args& s, Body& q) {
    __shared__ int stack[QSTACK_LDS][QUERY_BLOCK];
    const int lane = (int)threadIdx.x;
    __builtin_assume(lane >= 0 && lane < QUERY_BLOCK);
    const size_t spill_stride = (size_t)gridDim.x * QUERY_BLOCK;
    int* __restrict__ spill = s.spill + (size_t)blockIdx.x * QUERY_BLOCK + lane;
    for (size_t i = (size_t)blockIdx.x * QUERY_BLOCK + (size_t)lane; i - (size_t)lane < s.n; i += spill_stride) {
        const bool alive = i < s.n;
        const bool valid = q.begin(i, alive);
        do {
            for (uint32_t g = 0; g < s.geoms; g++) {
                const auto gm = s.g[g];
                const uint4* __restrict__ node32 = gm.node32;
                const int root = (int)gm.sm[SM_ROOT];
                const uint32_t count = gm.sm[SM_COUNT];
                const int lone = (count == 1u) ? gm.sorted_tri[0] : -1;
                bool here = true;
                if constexpr (std::is_void_v<decltype(q.enter(gm, (int)g))>) q.enter(gm, (int)g);
                else here = q.enter(gm, (int)g);
                const bool go = valid && here && !q.done();
                if (go && lone >= 0) q.leaf(lone);
                int cur = root, sp = 0;
                bool walking = go && root >= 0;
                while (walking) {
                    const uint4* np = (const uint4*)((const char*)node32 + ((uint32_t)cur << 5));
                    const uint4 n0 = np[0], n1 = np[1];
                    const int lkx = (int)n1.z, lky = (int)n1.w;
                    bool okL, okR;
                    float kL, kR;
                    q.children(n0, n1, okL, okR, kL, kR);
                    const bool leafL = okL && lkx < 0, leafR = okR && lky < 0;
                    int t0 = leafL ? ~lkx : (leafR ? ~lky : -1);
                    int t1 = (leafL && leafR) ? ~lky : -1;
                    while (t0 >= 0) {
                        q.leaf(t0);
                        t0 = t1;
                        t1 = -1;
                    }
                    if (q.done()) break;
                    const bool intL = okL && !leafL, intR = okR && !leafR;
                    const bool leftFirst = intL && (!intR || kL <= kR);
                    const int first = leftFirst ? lkx : lky, second = leftFirst ? lky : lkx;
                    if (intL && intR) {
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
            }
        } while (q.again());
        if (alive) q.finish(i);
    }
}

// The tie rule across geometries (closest hit and closest point; `best` is t or d2). The winner is the smallest value, on a
// bit-equal value the lexicographically lowest (geom, tri). The geometries are walked in ascending order, so at a candidate
// (g, tri) with value x every earlier record is of a geometry <= g:
//   x <  best                                   wins, whatever the ids
//   x == best, the record is of geometry g      wins iff tri < btri: `<` on the id, as inside one hierarchy
//   x == best, the record is of a geometry < g  loses: (geom, tri) of the record is lower whatever tri is
//   x == best, no record yet                    wins (best is the window's / the radius' own bound): any id is below "none"
// One unsigned key `tie` holds all of it as "tri < tie": 0xffffffff while there is no record, 0 from enter() on when the record
// is of an earlier geometry (no id is below 0), the record's tri once it is of this geometry. The same hierarchy twice
// therefore answers with the lower index. Boxes are kept with `<=` against best in every case: inside geometry g a candidate at
// exactly best with a lower id must still be reached, and best may have become this geometry's at any leaf. For a best that is
// still an earlier geometry's, `<` would be enough (an equal value loses); keeping `<=` there visits, and rejects at the leaf,
// only candidates at exactly the earlier best -- never a wrong answer, and no second compare in the node loop.
struct SceneBest {
    float best, bu, bv;
    int btri, bgeom, cur;
    uint32_t tie;
    PSM_D void clear(float bound) {
        best = bound;
        bu = 0.f;
        bv = 0.f;
        btri = -1;
        bgeom = -1;
        tie = 0xffffffffu;
    }
    PSM_D void enter_geom(int g) {
        cur = g;
        if (bgeom >= 0) tie = 0u;
    }
    PSM_D bool wins(float x, int tri) const { return x < best || (x == best && (uint32_t)tri < tie); }
    PSM_D void take(float x, float u, float v, int tri) {
        best = x;
        bu = u;
        bv = v;
        btri = tri;
        bgeom = cur;
        tie = (uint32_t)tri;
    }
};

// a ray in a scene: RayBody's / CountRay's ray, with the axes redone per geometry (each has a fit transform of its own)
struct SceneRay {
    SceneGeom gm;
    v3 o, d;
    float tmin, tmax;
    Axis X, Y, Z;

    PSM_D bool aim(v3 orig, v3 dir, float lo, float hi) {
        o = orig;
        d = normalize3(dir);
        tmin = lo;
        tmax = hi;
        return finite3(o) && finite3(d) && tmin <= tmax;
    }
    template <class Args>
    PSM_D bool load(const Args& s, size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 1.f), r1 = make_float4(1.f, 0.f, 0.f, -1.f);
        if (alive) { r0 = s.rays[2 * i]; r1 = s.rays[2 * i + 1]; }
        return aim(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), r0.w, r1.w) && alive;
    }
    PSM_D void axes(const SceneGeom& g) {
        gm = g;
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
        X = ray_axis(M, 0, o, d);
        Y = ray_axis(M, 1, o, d);
        Z = ray_axis(M, 2, o, d);
    }
    PSM_D void boxes(uint4 n0, uint4 n1, float lim, bool& okL, bool& okR, float& nL, float& nR) const {
        float fL, fR;
        slab(X, Y, Z, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z), nL, fL);
        slab(X, Y, Z, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y), nR, fR);
        okL = (nL <= fL) & (nL <= lim) & (fL >= tmin);
        okR = (nR <= fR) & (nR <= lim) & (fR >= tmin);
    }
};

// closest hit (ANY = false) and any hit (ANY = true) of a scene: RayBody with the best carried across the geometries
// (Args: SceneArgs; the instanced bodies below derive from these over InstArgs and replace begin() and enter())
template <bool ANY, class Args = SceneArgs>
struct SceneRayBody : SceneRay {
    const Args& s;
    SceneBest b;
    bool found;

    PSM_D SceneRayBody(const Args& a) : s(a) {}
    PSM_D bool begin(size_t i, bool alive) {
        const bool valid = load(s, i, alive);
        b.clear(tmax);
        found = false;
        return valid;
    }
    PSM_D void enter(const SceneGeom& g, int gi) {
        axes(g);
        b.enter_geom(gi);
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        boxes(n0, n1, ANY ? tmax : b.best, okL, okR, nL, nR);   // (<=: see SceneBest)
    }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(gm.tri48, tri, o, d, t, u, v) && t >= tmin && b.wins(t, tri)) {
            found = true;
            if (!ANY) b.take(t, u, v, tri);
        }
    }
    PSM_D bool done() const { return ANY && found; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (ANY) {
            s.occluded[i] = found ? 1 : 0;
        } else {
            s.hits[i] = found ? make_float4(b.bu, b.bv, b.best, __int_as_float(b.btri)) : miss_hit();
            s.geom[i] = b.bgeom;
        }
    }
};

// closest point (WITHIN = false) and within radius (WITHIN = true) of a scene: PointBody with the best d2 carried across the
// geometries; the point's normalised image and the bound's factors are redone per geometry (point_bound: per fit transform)
template <bool WITHIN, class Args = SceneArgs>
struct ScenePointBody {
    const Args& s;
    SceneGeom gm;
    PointBound B;
    v3 p;
    float rmax;
    SceneBest b;
    bool found;
    PointImage P;

    PSM_D ScenePointBody(const Args& a) : s(a) {}
    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(s.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        rmax = q.w;
        b.clear((rmax * rmax) * 1.00000095367431640625f + 0x1p-126f);   // (PointBody::begin)
        found = false;
        return alive && finite3(p) && rmax >= 0.f;
    }
    PSM_D void enter(const SceneGeom& g, int gi) {
        gm = g;
        float M[16];
        #pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(g.sm[SM_M + k]);
        B = point_bound(M);
        P.set(M, p);
        b.enter_geom(gi);
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        // (<=: see SceneBest; LB^2 is a world distance, comparable across the geometries' transforms)
        P.children(B, n0, n1, b.best, okL, okR, kL, kR);
    }
    PSM_D void leaf(int tri) {
        const float4 A = gm.tri48[(size_t)3 * tri + 0], Bv = gm.tri48[(size_t)3 * tri + 1], Cv = gm.tri48[(size_t)3 * tri + 2];
        float u, v;
        const float d2 = closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(Cv.x, Cv.y, Cv.z), p, u, v);
        if (sqrtf(d2) <= rmax && b.wins(d2, tri)) {
            found = true;
            if (!WITHIN) b.take(d2, u, v, tri);
        }
    }
    PSM_D bool done() const { return WITHIN && found; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (WITHIN) {
            s.occluded[i] = found ? 1 : 0;
        } else {
            s.hits[i] = found ? make_float4(b.bu, b.bv, sqrtf(b.best), __int_as_float(b.btri)) : miss_hit();
            s.geom[i] = b.bgeom;
        }
    }
};

// the counting ray of a scene (CountRay): the count runs on across the geometries
struct SceneCountRay : SceneRay {
    uint32_t count;
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const { boxes(n0, n1, tmax, okL, okR, nL, nR); }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(gm.tri48, tri, o, d, t, u, v) && t >= tmin && t <= tmax) count++;
    }
    PSM_D bool done() const { return false; }
};

template <class Args = SceneArgs>
struct SceneCountBody : SceneCountRay {
    const Args& s;
    PSM_D SceneCountBody(const Args& a) : s(a) {}
    PSM_D bool begin(size_t i, bool alive) {
        count = 0u;
        return load(s, i, alive);
    }
    PSM_D void enter(const SceneGeom& g, int) { axes(g); }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const { s.count[i] = count; }
};

// inside / outside of a point against a scene (SIGN = false) and the sign of a scene closest-point result (SIGN = true):
// InsideBody, with ray k's crossings summed over all geometries before it votes (again() comes after the last geometry)
template <bool SIGN, class Args = SceneArgs>
struct SceneInsideBody : SceneCountRay {
    const Args& s;
    v3 p;
    uint32_t k, votes;
    float dist;
    bool valid;

    PSM_D SceneInsideBody(const Args& a) : s(a) {}
    PSM_D bool shoot() {
        const int r = __builtin_amdgcn_readfirstlane((int)k);
        count = 0u;
        return aim(p, mk3(INSIDE_DIR[r][0], INSIDE_DIR[r][1], INSIDE_DIR[r][2]), 0.f, __builtin_inff());
    }
    PSM_D bool begin(size_t i, bool alive) {
        const float4 q = load_point(s.rays, i, alive);
        p = mk3(q.x, q.y, q.z);
        k = 0u;
        votes = 0u;
        dist = 0.f;
        valid = alive;
        if (SIGN) {
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (alive) h = s.hits[i];
            dist = h.z;
            valid = __float_as_int(h.w) >= 0;
        }
        valid = shoot() && valid;
        return valid;
    }
    PSM_D void enter(const SceneGeom& g, int) { axes(g); }
    PSM_D bool again() {
        votes += count & 1u;
        k++;
        if (!valid || k >= s.samples) return false;
        shoot();
        return true;
    }
    PSM_D void finish(size_t i) const {
        const bool in = 2u * votes > s.samples;
        if (!SIGN) s.occluded[i] = in ? 1 : 0;
        else if (in) ((float*)(s.hits + i))[2] = __uint_as_float(__float_as_uint(dist) | 0x80000000u);
    }
};

template <class Body, class Args>
PSM_D void scene_body(const Args& s) {
    Body q(s);
    scene_walk(s, q);
}

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_closest(SceneArgs s) { scene_body<SceneRayBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_any(SceneArgs s) { scene_body<SceneRayBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_point(SceneArgs s) { scene_body<ScenePointBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_within(SceneArgs s) { scene_body<ScenePointBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_count(SceneArgs s) { scene_body<SceneCountBody<>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_inside(SceneArgs s) { scene_body<SceneInsideBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void scene_query_sign(SceneArgs s) { scene_body<SceneInsideBody<true>>(s); }

// ---- instanced scene queries: a rigid transform per entry (include/psm_hip.h "instanced scene queries") ---------

// One instance as a kernel reads it: a geometry of a scene and its pose, the 12 floats of psm_instance.world_from_object
// (row-major 3 x 4 [R | T]). The table travels in the kernel-argument segment as SceneArgs' does (32 x 80 B = 2560 B): a pose
// changed on the host is the next launch's, and nothing on the device can go stale. The instance index is the same in every
// lane of a wave, so the matrix is read by scalar loads and never leaves the scalar registers.
struct InstGeom : SceneGeom {
    float m[12];
};
struct InstArgs {
    const float4* rays;      // as SceneArgs
    size_t n;
    int* spill;
    float4* hits;
    uint8_t* occluded;
    uint32_t* count;
    int32_t* geom;           // the winning INSTANCE per query, -1 on a miss
    uint32_t samples;
    uint32_t geoms;          // instances: 1 .. PSM_SCENE_MAX_GEOMETRIES
    InstGeom g[PSM_SCENE_MAX_GEOMETRIES];
};
static_assert(sizeof(InstGeom) == 80 && sizeof(InstArgs) <= 4096, "the instance table must fit the kernel-argument segment");

namespace {

// The instanced bodies are the scene bodies over InstArgs with begin() and enter() replaced. begin() keeps what passes through
// unchanged (the window, rmax) and the query's index; enter() reads the query again from memory (16 or 32 B, resident in L2),
// moves it into the instance's object space, then does the scene body's per-geometry set-up. The world query is therefore never
// live across the walk, which would cost the registers the scene kernels do not have to spare. enter() returns whether the moved
// query is valid in this instance (NaN and infinity propagate through the move; a finite query can overflow in it).

// enter() of the ray bodies: the ray aimed as SceneRay::aim aims it (the direction rotated as given, then normalised)
PSM_D bool inst_ray(SceneRay& r, const float4* __restrict__ rays, const InstGeom& g, size_t i, bool alive) {
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(1.f, 0.f, 0.f, 0.f);
    if (alive) { r0 = rays[2 * i]; r1 = rays[2 * i + 1]; }
    r.o = inst_point(g.m, mk3(r0.x, r0.y, r0.z));
    r.d = normalize3(inst_rotate(g.m, mk3(r1.x, r1.y, r1.z)));
    r.axes(g);
    return finite3(r.o) && finite3(r.d);
}
// begin() of the ray bodies: the window alone
PSM_D bool inst_window(SceneRay& r, const float4* __restrict__ rays, size_t i, bool alive) {
    r.tmin = 0.f;
    r.tmax = -1.f;
    if (alive) { r.tmin = rays[2 * i].w; r.tmax = rays[2 * i + 1].w; }
    return alive && r.tmin <= r.tmax;
}

// closest hit / any hit over instances. t is the distance along the moved unit direction: an object-space value, comparable
// across instances because the move is rigid (to 1e-5 relative: psm_hip.h)
template <bool ANY>
struct InstRayBody : SceneRayBody<ANY, InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstRayBody(const InstArgs& a) : SceneRayBody<ANY, InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        const bool valid = inst_window(*this, this->s.rays, i, al);
        this->b.clear(this->tmax);
        this->found = false;
        return valid;
    }
    PSM_D bool enter(const InstGeom& g, int gi) {
        const bool here = inst_ray(*this, this->s.rays, g, idx, alive);   // the move, then the axes; then the tie key
        this->b.enter_geom(gi);
        return here;
    }
};

struct InstCountBody : SceneCountBody<InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstCountBody(const InstArgs& a) : SceneCountBody<InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        count = 0u;
        return inst_window(*this, s.rays, i, al);
    }
    PSM_D bool enter(const InstGeom& g, int) { return inst_ray(*this, s.rays, g, idx, alive); }
};

// closest point / within over instances: p is the point in the instance's object space; rmax passes through, d2 is an
// object-space value (see InstRayBody)
template <bool WITHIN>
struct InstPointBody : ScenePointBody<WITHIN, InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstPointBody(const InstArgs& a) : ScenePointBody<WITHIN, InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        const float4 q = load_point(this->s.rays, i, al);
        this->rmax = q.w;
        this->b.clear((q.w * q.w) * 1.00000095367431640625f + 0x1p-126f);   // (PointBody::begin)
        this->found = false;
        return al && finite3(mk3(q.x, q.y, q.z)) && q.w >= 0.f;   // (a non-finite world point is non-finite in every instance)
    }
    PSM_D bool enter(const InstGeom& g, int gi) {
        const float4 q = load_point(this->s.rays, idx, alive);
        this->p = inst_point(g.m, mk3(q.x, q.y, q.z));
        ScenePointBody<WITHIN, InstArgs>::enter(g, gi);
        return finite3(this->p);
    }
};

// inside / the sign of a closest-point result over instances: ray k is the WORLD ray {p, 0, PSM_INSIDE_DIRECTIONS[k], +inf},
// moved per instance; its crossings are summed over all instances before it votes
template <bool SIGN>
struct InstInsideBody : SceneInsideBody<SIGN, InstArgs> {
    size_t idx;
    bool alive;
    PSM_D InstInsideBody(const InstArgs& a) : SceneInsideBody<SIGN, InstArgs>(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
        if (al) q = this->s.rays[i];
        this->k = 0u;
        this->votes = 0u;
        this->count = 0u;
        this->dist = 0.f;
        this->tmin = 0.f;
        this->tmax = __builtin_inff();
        this->valid = al;
        if (SIGN) {
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (al) h = this->s.hits[i];
            this->dist = h.z;
            this->valid = __float_as_int(h.w) >= 0;
        }
        this->valid = finite3(mk3(q.x, q.y, q.z)) && this->valid;   // (a non-finite p: outside)
        return this->valid;
    }
    PSM_D bool enter(const InstGeom& g, int) {
        float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
        if (alive) q = this->s.rays[idx];
        const int r = __builtin_amdgcn_readfirstlane((int)this->k);
        this->o = inst_point(g.m, mk3(q.x, q.y, q.z));
        this->d = normalize3(inst_rotate(g.m, mk3(INSIDE_DIR[r][0], INSIDE_DIR[r][1], INSIDE_DIR[r][2])));
        this->axes(g);
        return finite3(this->o) && finite3(this->d);
    }
    PSM_D bool again() {
        this->votes += this->count & 1u;
        this->k++;
        if (!this->valid || this->k >= this->s.samples) return false;
        this->count = 0u;
        return true;
    }
};

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_closest(InstArgs s) { scene_body<InstRayBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_any(InstArgs s) { scene_body<InstRayBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_point(InstArgs s) { scene_body<InstPointBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_within(InstArgs s) { scene_body<InstPointBody<true>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_count(InstArgs s) { scene_body<InstCountBody>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_inside(InstArgs s) { scene_body<InstInsideBody<false>>(s); }
__global__ __launch_bounds__(QUERY_BLOCK, 8) void inst_query_sign(InstArgs s) { scene_body<InstInsideBody<true>>(s); }

namespace {

// the stack entries beyond the LDS part, per context, shared by every query kind (all run on the context's stream, never at
// once; the world queries' launches use the same grid cap): one column per lane of a launch (allocated on the context's first query)
constexpr size_t SPILL_BYTES = (size_t)(QSTACK_MAX - QSTACK_LDS) * QUERY_GRID_CAP * QUERY_BLOCK * sizeof(int);
std::mutex spill_mu;
std::unordered_map<const psm_ctx*, void*> spill_area;

}  // namespace

int spill_for(psm_ctx* c, void** out) {
    std::lock_guard<std::mutex> lk(spill_mu);
    void*& p = spill_area[c];
    if (!p) PSM_HIP(c, hipMalloc(&p, SPILL_BYTES));
    *out = p;
    return PSM_OK;
}

// ceil(log2(n)) for n >= 1
int ceil_log2(size_t n) {
    int k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

// the builder's height bound of a hierarchy (QSTACK_MAX)
int depth_bound(const psm_bvh* b) { return 63 + ceil_log2(b->cap); }

const QueryDesc QUERY_DESC[] = {{"psm_bvh_intersect_dev", "rays", "hits", 16, false},
                                {"psm_bvh_occluded_dev", "rays", nullptr, 1, false},
                                {"psm_bvh_closest_point_dev", "points", "hits", 16, true},
                                {"psm_bvh_within_dev", "points", nullptr, 1, true},
                                {"psm_bvh_count_hits_dev", "rays", "counts", 4, false},
                                {"psm_bvh_inside_dev", "points", nullptr, 1, true},
                                {"psm_bvh_signed_distance_dev", "points", "hits", 16, true},
                                {"psm_bvh_first_hits_dev", "rays", "hits", 16, false},
                                {"psm_bvh_nearest_dev", "points", "hits", 16, true},
                                {"psm_bvh_box_overlaps_dev", "boxes", nullptr, 1, false},
                                {"psm_bvh_box_count_dev", "boxes", "counts", 4, false},
                                {"psm_bvh_box_triangles_dev", "boxes", "tris", 4, false},
                                {"psm_bvh_sweep_sphere_dev", "sweeps", "hits", 16, false},
                                {"psm_bvh_sweep_occluded_dev", "sweeps", nullptr, 1, false},
                                {"psm_bvh_tri_overlaps_dev", "triangles", nullptr, 1, false},
                                {"psm_bvh_tri_count_dev", "triangles", "counts", 4, false},
                                {"psm_bvh_tri_triangles_dev", "triangles", "tris", 4, false},
                                {"psm_bvh_tri_closest_dev", "triangles", "hits", 16, false},
                                {"psm_bvh_tri_within_dev", "triangles", nullptr, 1, false}};

// The data checks every query shares, under the entry point's name: in / out must be non-NULL, in 16-byte aligned, out as its
// kind asks (a psm_hit 16 bytes, a count 4); samples (the inside kinds only): 1, 3 or 5; the k-best kinds' k travels as
// samples: 1 .. PSM_QUERY_K_MAX. index: what the per-query index array (d_geom: the kinds with a psm_hit output only; the
// k-best kinds' and the box and triangle families' triangles queries' d_count) is called in the messages, NULL for a query that has none. A batch that passes makes the context's
// device the current one.
int check_data(psm_ctx* c, const char* name, const char* index, QueryKind kind, const void* d_in, const void* d_out, const int32_t* d_geom,
               uint32_t samples) {
    const QueryDesc& k = QUERY_DESC[kind];
    char msg[128];
    const bool with_geom = index && (k.out_align == 16 || kind == Q_BOX_TRIS || kind == Q_TRI_TRIS);   // (the triangles queries: int32 rows and counts)
    if (!d_in || !d_out || (with_geom && !d_geom)) {
        snprintf(msg, sizeof msg, "%s: NULL pointer", name);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    const bool in_bad = ((uintptr_t)d_in & 15u) != 0, out_bad = ((uintptr_t)d_out & (uintptr_t)(k.out_align - 1)) != 0;
    if (in_bad || out_bad) {
        if (k.out_align == 16) snprintf(msg, sizeof msg, "%s: %s or %s not 16-byte aligned", name, k.in, k.out);
        else if (in_bad) snprintf(msg, sizeof msg, "%s: %s not 16-byte aligned", name, k.in);
        else snprintf(msg, sizeof msg, "%s: %s not %u-byte aligned", name, k.out, k.out_align);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    if (with_geom && ((uintptr_t)d_geom & 3u) != 0) {
        snprintf(msg, sizeof msg, "%s: %s not 4-byte aligned", name, index);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    if ((kind == Q_INSIDE || kind == Q_SIGNED) && samples != 1 && samples != 3 && samples != 5) {
        snprintf(msg, sizeof msg, "%s: samples must be 1, 3 or 5", name);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    if ((kind == Q_FIRST_HITS || kind == Q_NEAREST || kind == Q_BOX_TRIS || kind == Q_TRI_TRIS) && (samples == 0 || samples > PSM_QUERY_K_MAX)) {
        snprintf(msg, sizeof msg, "%s: k must be 1 .. %d", name, PSM_QUERY_K_MAX);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    (void)hipSetDevice(c->device);
    return PSM_OK;
}

// Why a pose is refused, or NULL (psm_hip.h): in double, on the host. A rigid motion or a reflection has R^T R = 1; the bound
// leaves room for a matrix that was composed in float32 and refuses every scale or shear a user could mean.
const char* pose_fault(const float* m) {
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(m[k])) return "has a non-finite transform";
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            double dot = 0.0;
            for (int i = 0; i < 3; i++) dot += (double)m[4 * i + a] * (double)m[4 * i + b];
            if (std::fabs(dot - (a == b ? 1.0 : 0.0)) > 1e-5) return "has a transform that is not rigid (R^T R differs from 1 by more than 1e-5)";
        }
    return nullptr;
}

namespace {

const char* const SCENE_NAME[] = {"psm_scene_intersect_dev", "psm_scene_occluded_dev", "psm_scene_closest_point_dev",
                                  "psm_scene_within_dev", "psm_scene_count_hits_dev", "psm_scene_inside_dev",
                                  "psm_scene_signed_distance_dev"};
const char* const INST_NAME[] = {"psm_instances_intersect_dev", "psm_instances_occluded_dev", "psm_instances_closest_point_dev",
                                 "psm_instances_within_dev", "psm_instances_count_hits_dev", "psm_instances_inside_dev",
                                 "psm_instances_signed_distance_dev"};

const Kernels<QueryArgs> BVH_KERNELS = {{bvh_query_closest, bvh_query_any, bvh_query_point, bvh_query_within, bvh_query_count,
                                         bvh_query_inside, bvh_query_sign}};
const Kernels<SceneArgs> SCENE_KERNELS = {{scene_query_closest, scene_query_any, scene_query_point, scene_query_within,
                                           scene_query_count, scene_query_inside, scene_query_sign}};
const Kernels<InstArgs> INST_KERNELS = {{inst_query_closest, inst_query_any, inst_query_point, inst_query_within, inst_query_count,
                                         inst_query_inside, inst_query_sign}};

bool too_deep(const psm_bvh* b) { return depth_bound(b) > QSTACK_MAX; }

// A query of one hierarchy: n == 0 is answered before anything else is looked at; then the data, the state, the depth.
// The k-best kinds (kbest.hip) come through here too: samples is their k, d_out their [n][k] records, d_count their counts;
// and the box kinds (box.hip): d_in the boxes, and for the triangles query samples = k, d_out the [n][k] ids, d_count the counts;
// and the sweep kinds (sweep.hip): d_in the sweeps; and the triangle kinds (tri.hip): d_in the query triangles, the rest as the box
// kinds; and the clearance kinds (tri_dist.hip): d_in the query triangles with their rmax, d_out two float4 per query or a byte.
int query(psm_bvh* b, QueryKind kind, const void* d_in, size_t n, void* d_out, uint32_t samples = 0, uint32_t* d_count = nullptr) {
    if (!b) return PSM_ERR_INVALID;
    if (n == 0) return PSM_OK;
    psm_ctx* c = b->ctx;
    const bool points = QUERY_DESC[kind].points, kbest = kind == Q_FIRST_HITS || kind == Q_NEAREST;
    const bool box = kind >= Q_BOX_ANY && kind <= Q_BOX_TRIS, sweep = kind == Q_SWEEP || kind == Q_SWEEP_ANY;
    const bool tri = kind >= Q_TRI_ANY && kind <= Q_TRI_TRIS;
    const bool clear = kind == Q_TRI_CLOSEST || kind == Q_TRI_WITHIN;
    const bool counted = kbest || kind == Q_BOX_TRIS || kind == Q_TRI_TRIS;
    int rc = check_data(c, QUERY_DESC[kind].name, counted ? "counts" : nullptr, kind, d_in, d_out, (const int32_t*)d_count, samples);
    if (rc != PSM_OK) return rc;
    if (!b->built)
        return set_err(c, PSM_ERR_STATE, box ? "box query before build" : clear ? "clearance query before build" : tri ? "triangle query before build" : sweep ? "sweep query before build" : points ? "point query before build" : "ray query before build");
    if (too_deep(b))
        return set_err(c, PSM_ERR_CAPACITY, box      ? "box query: hierarchy deeper than the query stack"
                                            : clear  ? "clearance query: hierarchy deeper than the query stack"
                                            : tri    ? "triangle query: hierarchy deeper than the query stack"
                                            : sweep  ? "sweep query: hierarchy deeper than the query stack"
                                            : points ? "point query: hierarchy deeper than the query stack"
                                                     : "ray query: hierarchy deeper than the query stack");
    QueryArgs qa = {};
    uint32_t grid = 0;
    rc = batch_args(c, d_in, n, d_out, samples, qa, grid);
    if (rc != PSM_OK) return rc;
    qa.node32 = b->d_node32; qa.tri48 = b->d_tri48; qa.sm = b->d_small; qa.sorted_tri = b->d_sorted_tri;
    if (kbest) {
        qa.count = d_count;
        return kbest_launch(c, points, grid, qa);
    }
    if (box) {   // (box.hip; the triangles query's rows are d_out, its counts d_count)
        if (kind == Q_BOX_TRIS) qa.count = d_count;
        return box_launch(c, (int)kind - (int)Q_BOX_ANY, grid, qa);
    }
    if (sweep) return sweep_launch(c, kind == Q_SWEEP_ANY, grid, qa);   // (sweep.hip)
    if (tri) {   // (tri.hip; the triangles query's rows are d_out, its counts d_count)
        if (kind == Q_TRI_TRIS) qa.count = d_count;
        return tri_launch(c, (int)kind - (int)Q_TRI_ANY, grid, qa);
    }
    if (clear) return tri_dist_launch(c, kind == Q_TRI_WITHIN, grid, qa);   // (tri_dist.hip)
    return launch(c, BVH_KERNELS, kind, grid, qa);
}

// An entry of a list as the list queries read it: a scene's psm_bvh*, or a psm_instance (a hierarchy and its pose). noun: what
// the messages call it; fault: why the entry itself is refused, or NULL; fill: its row of the kernel-argument table.
struct SceneEntry {
    using Args = SceneArgs;
    static constexpr const char* noun = "geometry";
    static psm_bvh* bvh(psm_bvh* e) { return e; }
    static const char* fault(psm_bvh*) { return nullptr; }
    static void fill(SceneGeom& t, psm_bvh* b) { t = SceneGeom{b->d_node32, b->d_tri48, b->d_small, b->d_sorted_tri}; }
};
struct InstEntry {
    using Args = InstArgs;
    static constexpr const char* noun = "instance";
    static psm_bvh* bvh(const psm_instance& e) { return e.bvh; }
    static const char* fault(const psm_instance& e) { return pose_fault(e.world_from_object); }
    static void fill(InstGeom& t, const psm_instance& e) {
        SceneEntry::fill(t, e.bvh);
        for (int k = 0; k < 12; k++) t.m[k] = e.world_from_object[k];
    }
};

// The per-entry checks of a list against its context c, the message naming the first failing index: every entry's handle
// (NULL, another context than c), every entry's own fault (the poses), every entry's state (not built, too deep for the stack).
template <class E, class Entry>
int check_entries(psm_ctx* c, const Entry* list, uint32_t count, const char* name) {
    char msg[160];
    for (uint32_t g = 0; g < count; g++) {
        if (!E::bvh(list[g])) {
            snprintf(msg, sizeof msg, "%s: %s %u is NULL", name, E::noun, g);
            return set_err(c, PSM_ERR_INVALID, msg);
        }
        if (E::bvh(list[g])->ctx != c) {
            snprintf(msg, sizeof msg, "%s: %s %u belongs to another context", name, E::noun, g);
            return set_err(c, PSM_ERR_INVALID, msg);
        }
    }
    for (uint32_t g = 0; g < count; g++)
        if (const char* why = E::fault(list[g])) {
            snprintf(msg, sizeof msg, "%s: %s %u %s", name, E::noun, g, why);
            return set_err(c, PSM_ERR_INVALID, msg);
        }
    for (uint32_t g = 0; g < count; g++) {
        if (!E::bvh(list[g])->built) {
            snprintf(msg, sizeof msg, "%s: %s %u is not built", name, E::noun, g);
            return set_err(c, PSM_ERR_STATE, msg);
        }
        if (too_deep(E::bvh(list[g]))) {
            snprintf(msg, sizeof msg, "%s: %s %u is deeper than the query stack", name, E::noun, g);
            return set_err(c, PSM_ERR_CAPACITY, msg);
        }
    }
    return PSM_OK;
}

// The list of a scene or an instanced query, checked first and whole, also for n == 0, all of it on the host before any device
// is touched: its length, then its entries (check_entries). The message goes to the context of the first non-NULL entry, *ctx
// (a list of NULLs only has no context to tell: the return code alone).
template <class E, class Entry>
int check_list(const Entry* list, uint32_t count, const char* name, psm_ctx** ctx) {
    if (!list || count == 0 || count > PSM_SCENE_MAX_GEOMETRIES) return PSM_ERR_INVALID;
    psm_ctx* c = nullptr;
    for (uint32_t g = 0; g < count && !c; g++)
        if (E::bvh(list[g])) c = E::bvh(list[g])->ctx;
    if (!c) return PSM_ERR_INVALID;
    *ctx = c;
    return check_entries<E>(c, list, count, name);
}

// A query of a list (E: SceneEntry or InstEntry): the list, n == 0, the data, the table, the launch. index: what d_geom is
// called in the messages ("geom" / "inst").
template <class E, class Entry>
int list_query(const Entry* list, uint32_t count, const char* name, const char* index, const Kernels<typename E::Args>& kernels,
               QueryKind kind, const void* d_in, size_t n, void* d_out, int32_t* d_geom, uint32_t samples) {
    psm_ctx* c = nullptr;
    int rc = check_list<E>(list, count, name, &c);
    if (rc != PSM_OK || n == 0) return rc;
    rc = check_data(c, name, index, kind, d_in, d_out, d_geom, samples);
    if (rc != PSM_OK) return rc;
    typename E::Args a = {};
    uint32_t grid = 0;
    rc = batch_args(c, d_in, n, d_out, samples, a, grid);
    if (rc != PSM_OK) return rc;
    a.geom = d_geom;
    a.geoms = count;
    for (uint32_t g = 0; g < count; g++) E::fill(a.g[g], list[g]);
    return launch(c, kernels, kind, grid, a);
}

int scene_query(psm_bvh* const* geoms, uint32_t count, QueryKind kind, const void* d_in, size_t n, void* d_out, int32_t* d_geom,
                uint32_t samples = 0) {
    return list_query<SceneEntry>(geoms, count, SCENE_NAME[kind], "geom", SCENE_KERNELS, kind, d_in, n, d_out, d_geom, samples);
}

int inst_query(const psm_instance* insts, uint32_t count, QueryKind kind, const void* d_in, size_t n, void* d_out, int32_t* d_inst,
               uint32_t samples = 0) {
    return list_query<InstEntry>(insts, count, INST_NAME[kind], "inst", INST_KERNELS, kind, d_in, n, d_out, d_inst, samples);
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

// psm_world_set_instances (world.hip): the instanced queries' per-entry checks, against the world's context
int check_instances(psm_ctx* c, const psm_instance* list, uint32_t count, const char* name) {
    return check_entries<InstEntry>(c, list, count, name);
}

// psm_grid_signed_distance_dev (grid_dist.hip): the second kernel of psm_bvh_signed_distance_dev alone, over n points and the
// closest-point records a grid walk wrote for them. The caller has made every check (the hierarchy is built, samples is 1, 3 or 5)
int sign_launch(psm_bvh* b, const void* d_points, size_t n, uint32_t samples, void* d_hits) {
    QueryArgs qa = {};
    uint32_t grid = 0;
    const int rc = batch_args(b->ctx, d_points, n, d_hits, samples, qa, grid);
    if (rc != PSM_OK) return rc;
    qa.node32 = b->d_node32; qa.tri48 = b->d_tri48; qa.sm = b->d_small; qa.sorted_tri = b->d_sorted_tri;
    bvh_query_sign<<<grid, QUERY_BLOCK, 0, b->ctx->stream>>>(qa);
    PSM_HIP(b->ctx, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm

int psm_bvh_intersect_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits) {
    return psm::query(bvh, psm::Q_CLOSEST, d_rays, n, d_hits);
}

int psm_bvh_occluded_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::query(bvh, psm::Q_ANY, d_rays, n, d_hit);
}

int psm_bvh_closest_point_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, psm_hit* d_hits) {
    return psm::query(bvh, psm::Q_POINT, d_points, n, d_hits);
}

int psm_bvh_within_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint8_t* d_hit) {
    return psm::query(bvh, psm::Q_WITHIN, d_points, n, d_hit);
}

int psm_bvh_count_hits_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_COUNT, d_rays, n, d_count);
}

int psm_bvh_inside_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t samples, uint8_t* d_inside) {
    return psm::query(bvh, psm::Q_INSIDE, d_points, n, d_inside, samples);
}

int psm_bvh_signed_distance_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t samples, psm_hit* d_hits) {
    return psm::query(bvh, psm::Q_SIGNED, d_points, n, d_hits, samples);
}

int psm_bvh_first_hits_dev(psm_bvh* bvh, const psm_query_ray* d_rays, size_t n, uint32_t k, psm_hit* d_hits, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_FIRST_HITS, d_rays, n, d_hits, k, d_count);
}

int psm_bvh_nearest_dev(psm_bvh* bvh, const psm_point_query* d_points, size_t n, uint32_t k, psm_hit* d_hits, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_NEAREST, d_points, n, d_hits, k, d_count);
}

int psm_bvh_box_overlaps_dev(psm_bvh* bvh, const psm_box_query* d_boxes, size_t n, uint8_t* d_hit) {
    return psm::query(bvh, psm::Q_BOX_ANY, d_boxes, n, d_hit);
}

int psm_bvh_box_count_dev(psm_bvh* bvh, const psm_box_query* d_boxes, size_t n, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_BOX_COUNT, d_boxes, n, d_count);
}

int psm_bvh_box_triangles_dev(psm_bvh* bvh, const psm_box_query* d_boxes, size_t n, uint32_t k, int32_t* d_tris, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_BOX_TRIS, d_boxes, n, d_tris, k, d_count);
}

int psm_bvh_tri_overlaps_dev(psm_bvh* bvh, const psm_tri_query* d_tris, size_t n, uint8_t* d_hit) {
    return psm::query(bvh, psm::Q_TRI_ANY, d_tris, n, d_hit);
}

int psm_bvh_tri_count_dev(psm_bvh* bvh, const psm_tri_query* d_tris, size_t n, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_TRI_COUNT, d_tris, n, d_count);
}

int psm_bvh_tri_triangles_dev(psm_bvh* bvh, const psm_tri_query* d_tris, size_t n, uint32_t k, int32_t* d_ids, uint32_t* d_count) {
    return psm::query(bvh, psm::Q_TRI_TRIS, d_tris, n, d_ids, k, d_count);
}

int psm_bvh_tri_closest_dev(psm_bvh* bvh, const psm_tri_dist_query* d_queries, size_t n, psm_tri_hit* d_hits) {
    return psm::query(bvh, psm::Q_TRI_CLOSEST, d_queries, n, d_hits);
}

int psm_bvh_tri_within_dev(psm_bvh* bvh, const psm_tri_dist_query* d_queries, size_t n, uint8_t* d_flag) {
    return psm::query(bvh, psm::Q_TRI_WITHIN, d_queries, n, d_flag);
}

int psm_bvh_sweep_sphere_dev(psm_bvh* bvh, const psm_sweep_query* d_sweeps, size_t n, psm_hit* d_hits) {
    return psm::query(bvh, psm::Q_SWEEP, d_sweeps, n, d_hits);
}

int psm_bvh_sweep_occluded_dev(psm_bvh* bvh, const psm_sweep_query* d_sweeps, size_t n, uint8_t* d_hit) {
    return psm::query(bvh, psm::Q_SWEEP_ANY, d_sweeps, n, d_hit);
}

int psm_scene_intersect_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits, int32_t* d_geom) {
    return psm::scene_query(geoms, count, psm::Q_CLOSEST, d_rays, n, d_hits, d_geom);
}

int psm_scene_occluded_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::scene_query(geoms, count, psm::Q_ANY, d_rays, n, d_hit, nullptr);
}

int psm_scene_closest_point_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, psm_hit* d_hits,
                                int32_t* d_geom) {
    return psm::scene_query(geoms, count, psm::Q_POINT, d_points, n, d_hits, d_geom);
}

int psm_scene_within_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint8_t* d_hit) {
    return psm::scene_query(geoms, count, psm::Q_WITHIN, d_points, n, d_hit, nullptr);
}

int psm_scene_count_hits_dev(psm_bvh* const* geoms, uint32_t count, const psm_query_ray* d_rays, size_t n, uint32_t* d_count) {
    return psm::scene_query(geoms, count, psm::Q_COUNT, d_rays, n, d_count, nullptr);
}

int psm_scene_inside_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                         uint8_t* d_inside) {
    return psm::scene_query(geoms, count, psm::Q_INSIDE, d_points, n, d_inside, nullptr, samples);
}

int psm_scene_signed_distance_dev(psm_bvh* const* geoms, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                                  psm_hit* d_hits, int32_t* d_geom) {
    return psm::scene_query(geoms, count, psm::Q_SIGNED, d_points, n, d_hits, d_geom, samples);
}

int psm_instances_intersect_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits,
                                int32_t* d_inst) {
    return psm::inst_query(insts, count, psm::Q_CLOSEST, d_rays, n, d_hits, d_inst);
}

int psm_instances_occluded_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::inst_query(insts, count, psm::Q_ANY, d_rays, n, d_hit, nullptr);
}

int psm_instances_closest_point_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, psm_hit* d_hits,
                                    int32_t* d_inst) {
    return psm::inst_query(insts, count, psm::Q_POINT, d_points, n, d_hits, d_inst);
}

int psm_instances_within_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, uint8_t* d_hit) {
    return psm::inst_query(insts, count, psm::Q_WITHIN, d_points, n, d_hit, nullptr);
}

int psm_instances_count_hits_dev(const psm_instance* insts, uint32_t count, const psm_query_ray* d_rays, size_t n, uint32_t* d_count) {
    return psm::inst_query(insts, count, psm::Q_COUNT, d_rays, n, d_count, nullptr);
}

int psm_instances_inside_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n, uint32_t samples,
                             uint8_t* d_inside) {
    return psm::inst_query(insts, count, psm::Q_INSIDE, d_points, n, d_inside, nullptr, samples);
}

int psm_instances_signed_distance_dev(const psm_instance* insts, uint32_t count, const psm_point_query* d_points, size_t n,
                                      uint32_t samples, psm_hit* d_hits, int32_t* d_inst) {
    return psm::inst_query(insts, count, psm::Q_SIGNED, d_points, n, d_hits, d_inst, samples);
}
