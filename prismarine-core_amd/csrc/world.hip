// world.hip -- instance worlds: the seven queries of query.hip over a top-level tree of posed instances (new; no reference
// counterpart; include/psm_hip.h "instance worlds").
//
// A world is a handle that owns, on the device, a table of instances (a hierarchy's four pointers and a rigid pose: the row of
// query.hip's InstGeom, now in memory) and a binary tree over the instances' padded world-space boxes. A world of N instances
// answers every query exactly as psm_instances_*_dev would over the same ordered list if that list could be N long: the tree
// only decides which instances a query enters, and every box test is padded and slackened so that it never drops an instance
// that holds a counting candidate (the bounds: WORLD_PAD below). What a query does inside an instance is what the instanced
// bodies of query.hip do, from the same pieces: the tests, the move and the constants of psm_query_dev.h, the checks and the
// launch of psm_query_host.h. This file holds what is a world's own: rows, tree, walk, stale check, depth rule.
// The k-best queries of a world (a ray's first k hits, a point's k nearest triangles over all instances) are
// here too: two more bodies for the same walk, with the sorted list of psm_world_klist.h in the place of the one best record.
// So are the host functions of every other query family over a world (psm_world is private to this file); those of the posed
// meshes and of the grids are sequences of the pieces mesh.hip and grid.hip define once, and all of them
// take how a walk starts from world_start().
//
// The walk is one loop over one stack ([depth][lane] in LDS, the rest in the context's spill area). A stack entry is a link:
//   link < 0               instance ~link of the world: the lane enters it (loads its row, moves the query, sets up)
//   link & WORLD_TOP       node (link & ~WORLD_TOP) of the tree over the instances
//   otherwise              an internal node of the hierarchy the lane is in (query.hip's links; leaves are never pushed)
// A lane is "inside an instance" exactly while its current link is of the third kind; when its pop brings up a link of the first
// two kinds it is back at the top level -- the tag does what a marker entry would, without the entry (the host still budgets
// one). Lanes of a wave may be at different levels: the loop body holds the three steps under one branch each.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"    // the constants, the triangle / box / point tests, inst_point / inst_rotate, INSIDE_DIR
#include "psm_query_host.h"   // QueryKind, check_data / check_instances, batch_args / launch; mesh.hip's and grid.hip's shared host pieces
#include "psm_world_dev.h"    // WorldRow / WorldNode / WorldArgs, the WORLD_* constants, world_walk, load_row / load_pose,
                              // WorldBest, WorldRay
#define PSM_KLIST_FN PSM_D
#include "psm_world_klist.h"  // WorldKList: the sorted list of the k-best queries (also compiled for the host by a test)

namespace psm {

namespace {

// closest hit (ANY = false) and any hit (ANY = true)
template <bool ANY>
struct WorldRayBody : WorldRay {
    const WorldArgs& w;
    WorldBest b;
    bool found, alive;
    size_t idx;

    PSM_D WorldRayBody(const WorldArgs& a) : w(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        begin_ray(w, i, al);
        b.clear(tmax);
        found = false;
        return al && tmin <= tmax;
    }
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& nL, float& nR) const {
        top_boxes(w0, w1, w2, ANY ? tmax : b.best, okL, okR, nL, nR);
    }
    PSM_D int enter(int in) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(1.f, 0.f, 0.f, 0.f);
        if (alive) { r0 = w.rays[2 * idx]; r1 = w.rays[2 * idx + 1]; }
        const int32_t* st;
        uint32_t count;
        const int r = enter_ray(w, in, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), st, count);
        if (r != -1 && count == 1u) leaf(st[0]);
        return r;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const {
        boxes(n0, n1, ANY ? tmax : b.best, okL, okR, nL, nR);
    }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(tri48, tri, o, d, t, u, v) && t >= tmin && b.wins(t, inst, tri)) {
            found = true;
            if (!ANY) b.take(t, u, v, inst, tri);
        }
    }
    PSM_D bool done() const { return ANY && found; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (ANY) {
            w.occluded[i] = found ? 1 : 0;
        } else {
            w.hits[i] = found ? make_float4(b.bu, b.bv, b.best, __int_as_float(b.btri)) : miss_hit();
            w.geom[i] = b.binst;
        }
    }
};

// the counting ray (query.hip's CountRay): every candidate inside the window, summed over the instances entered
struct WorldCountRay : WorldRay {
    uint32_t count;
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& nL, float& nR) const {
        top_boxes(w0, w1, w2, tmax, okL, okR, nL, nR);
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const { boxes(n0, n1, tmax, okL, okR, nL, nR); }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(tri48, tri, o, d, t, u, v) && t >= tmin && t <= tmax) count++;
    }
    PSM_D bool done() const { return false; }
};

struct WorldCountBody : WorldCountRay {
    const WorldArgs& w;
    bool alive;
    size_t idx;
    PSM_D WorldCountBody(const WorldArgs& a) : w(a) {}
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        begin_ray(w, i, al);
        count = 0u;
        return al && tmin <= tmax;
    }
    PSM_D int enter(int in) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(1.f, 0.f, 0.f, 0.f);
        if (alive) { r0 = w.rays[2 * idx]; r1 = w.rays[2 * idx + 1]; }
        const int32_t* st;
        uint32_t cnt;
        const int r = enter_ray(w, in, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), st, cnt);
        if (r != -1 && cnt == 1u) leaf(st[0]);
        return r;
    }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const { w.count[i] = count; }
};

// inside / the sign of a closest-point result: ray k is the WORLD ray {p, 0, PSM_INSIDE_DIRECTIONS[k], +inf}; its crossings are
// summed over every instance it reaches before it votes; again() restarts the top-level walk for the next direction
template <bool SIGN>
struct WorldInsideBody : WorldCountRay {
    const WorldArgs& w;
    uint32_t k, votes;
    float dist;
    bool valid, alive;
    size_t idx;

    PSM_D WorldInsideBody(const WorldArgs& a) : w(a) {}
    PSM_D v3 dir() const {
        const int r = __builtin_amdgcn_readfirstlane((int)k);   // (every lane of the wave is at the same k)
        return mk3(INSIDE_DIR[r][0], INSIDE_DIR[r][1], INSIDE_DIR[r][2]);
    }
    PSM_D float4 point() const {
        float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
        if (alive) q = w.rays[idx];
        return q;
    }
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        const float4 q = point();
        k = 0u;
        votes = 0u;
        count = 0u;
        dist = 0.f;
        tmin = 0.f;
        tmax = __builtin_inff();
        valid = al;
        if (SIGN) {
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (al) h = w.hits[i];
            dist = h.z;
            valid = __float_as_int(h.w) >= 0;
        }
        valid = finite3(mk3(q.x, q.y, q.z)) && valid;   // (a non-finite p: outside)
        world_ray(mk3(q.x, q.y, q.z), dir());
        return valid;
    }
    PSM_D int enter(int in) {
        const float4 q = point();
        const int32_t* st;
        uint32_t cnt;
        const int r = enter_ray(w, in, mk3(q.x, q.y, q.z), dir(), st, cnt);
        if (r != -1 && cnt == 1u) leaf(st[0]);
        return r;
    }
    PSM_D bool again() {
        votes += count & 1u;
        k++;
        if (!valid || k >= w.samples) return false;
        count = 0u;
        const float4 q = point();
        world_ray(mk3(q.x, q.y, q.z), dir());
        return true;
    }
    PSM_D void finish(size_t i) const {
        const bool in = 2u * votes > w.samples;
        if (!SIGN) w.occluded[i] = in ? 1 : 0;
        else if (in) ((float*)(w.hits + i))[2] = __uint_as_float(__float_as_uint(dist) | 0x80000000u);
    }
};

// closest point (WITHIN = false) and within radius (WITHIN = true): query.hip's InstPointBody; the top level tests the WORLD
// point's squared distance to a box grown by qpad against the best d2 (an object-space value: equal to the world one to 3e-5)
template <bool WITHIN>
struct WorldPointBody {
    const WorldArgs& w;
    const uint4* node32;
    const float4* tri48;
    int inst;
    PointBound B;
    v3 p, wp;
    float rmax, qpad;
    WorldBest b;
    bool found, alive;
    size_t idx;
    PointImage P;

    PSM_D WorldPointBody(const WorldArgs& a) : w(a) {}
    PSM_D float4 point() const {
        float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
        if (alive) q = w.rays[idx];
        return q;
    }
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        const float4 q = point();
        wp = mk3(q.x, q.y, q.z);
        qpad = WORLD_QSLACK * smaxf(smaxf(pabs(q.x), pabs(q.y)), pabs(q.z));
        rmax = q.w;
        b.clear((q.w * q.w) * 1.00000095367431640625f + 0x1p-126f);   // (query.hip PointBody::begin)
        found = false;
        return al && finite3(wp) && q.w >= 0.f;
    }
    PSM_D float gap2(float lx, float ly, float lz, float hx, float hy, float hz) const {
        const float tx = smaxf(smaxf((lx - qpad) - wp.x, wp.x - (hx + qpad)), 0.f);
        const float ty = smaxf(smaxf((ly - qpad) - wp.y, wp.y - (hy + qpad)), 0.f);
        const float tz = smaxf(smaxf((lz - qpad) - wp.z, wp.z - (hz + qpad)), 0.f);
        return (tx * tx + ty * ty) + tz * tz;
    }
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = gap2(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y);
        kR = gap2(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w);
        const float lim = b.best + WORLD_PSLACK * b.best;
        okL = !(kL > lim);
        okR = !(kR > lim);
    }
    PSM_D int enter(int in) {
        const float4 q = point();
        const RowLoad r = load_row(w, in, *this);
        p = inst_point(r.m, mk3(q.x, q.y, q.z));
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(r.sm[SM_M + k]);
        B = point_bound(M);
        P.set(M, p);
        if (!finite3(p)) return -1;
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        P.children(B, n0, n1, b.best, okL, okR, kL, kR);
    }
    PSM_D void leaf(int tri) {
        const float4 A = tri48[(size_t)3 * tri + 0], Bv = tri48[(size_t)3 * tri + 1], Cv = tri48[(size_t)3 * tri + 2];
        float u, v;
        const float d2 = closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(Cv.x, Cv.y, Cv.z), p, u, v);
        if (sqrtf(d2) <= rmax && b.wins(d2, inst, tri)) {
            found = true;
            if (!WITHIN) b.take(d2, u, v, inst, tri);
        }
    }
    PSM_D bool done() const { return WITHIN && found; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        if (WITHIN) {
            w.occluded[i] = found ? 1 : 0;
        } else {
            w.hits[i] = found ? make_float4(b.bu, b.bv, sqrtf(b.best), __int_as_float(b.btri)) : miss_hit();
            w.geom[i] = b.binst;
        }
    }
};

template <class Body>
PSM_D void world_body(const WorldArgs& w) {
    Body q(w);
    world_walk(w, q);
}

// ---- k-best: a ray's first k hits, a point's k nearest triangles, over the whole world ------------------------

// The sorted list of one query (psm_world_klist.h: kbest.hip's KList with a third key word), its two columns in the wave's
// dynamic LDS: the k x 64 keys {value bits, tri}, then the k x 64 instances, both [slot][lane]
struct WorldList : WorldKList<uint2, QUERY_BLOCK> {
    PSM_D static uint2* keys() {
        extern __shared__ uint2 world_list[];
        return world_list;
    }
    PSM_D WorldList(uint32_t slots)
        : WorldKList<uint2, QUERY_BLOCK>(keys() + threadIdx.x, (uint32_t*)(keys() + (size_t)slots * QUERY_BLOCK) + threadIdx.x, slots) {}
};

// the first k hits of a ray over the world: WorldRayBody<false> with the list in the place of its one best record. lim: the
// bound of both levels of boxes -- tmax until the list is full, then the last slot's t (kept with <=, and at the top level
// slackened: a candidate at the last slot's t of a lower (inst, tri) must still be reached)
struct WorldFirstHitsBody : WorldRay {
    const WorldArgs& w;
    WorldList L;
    float lim;
    bool alive;
    size_t idx;

    PSM_D WorldFirstHitsBody(const WorldArgs& a) : w(a), L(a.samples) {}
    PSM_D void ray(float4& r0, float4& r1) const {
        r0 = make_float4(0.f, 0.f, 0.f, 0.f);
        r1 = make_float4(1.f, 0.f, 0.f, 0.f);
        if (alive) { r0 = w.rays[2 * idx]; r1 = w.rays[2 * idx + 1]; }
    }
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        begin_ray(w, i, al);
        lim = tmax;
        L.clear();   // per query: the grid-stride loop comes here again
        return al && tmin <= tmax;
    }
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& nL, float& nR) const {
        top_boxes(w0, w1, w2, lim, okL, okR, nL, nR);
    }
    PSM_D int enter(int in) {
        float4 r0, r1;
        ray(r0, r1);
        const int32_t* st;
        uint32_t count;
        const int r = enter_ray(w, in, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), st, count);
        if (r != -1 && count == 1u) leaf(st[0]);
        return r;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& nL, float& nR) const { boxes(n0, n1, lim, okL, okR, nL, nR); }
    PSM_D void leaf(int tri) {
        float t, u, v;
        if (tri_query(tri48, tri, o, d, t, u, v) && t >= tmin && t <= tmax) lim = L.offer(t, (uint32_t)inst, (uint32_t)tri, lim);
    }
    PSM_D bool done() const { return false; }
    PSM_D bool again() const { return false; }
    // u, v are not kept: per stored (inst, tri) the ray is re-read and moved exactly as enter() moves it and the same test is
    // run again -- the same function on the same inputs gives the same bits (-ffp-contract=off)
    PSM_D void finish(size_t i) const {
        float4 r0, r1;
        ray(r0, r1);
        float4* __restrict__ row = w.hits + i * L.k;
        int32_t* __restrict__ irow = w.geom + i * L.k;
        for (uint32_t s = 0; s < L.k; s++) {
            float4 h = miss_hit();
            int32_t hin = -1;
            if (s < L.cnt) {
                const uint2 e = L.key[(size_t)s * QUERY_BLOCK];
                const uint32_t in = L.ins[(size_t)s * QUERY_BLOCK];
                float m[12];
                const float4* tris = load_pose(w, in, m);
                const v3 oo = inst_point(m, mk3(r0.x, r0.y, r0.z));
                const v3 dd = normalize3(inst_rotate(m, mk3(r1.x, r1.y, r1.z)));
                float t = 0.f, u = 0.f, v = 0.f;
                (void)tri_query(tris, (int)e.y, oo, dd, t, u, v);
                h = make_float4(u, v, __uint_as_float(e.x), __uint_as_float(e.y));
                hin = (int32_t)in;
            }
            row[s] = h;
            irow[s] = hin;
        }
        w.count[i] = L.cnt;
    }
};

// the k nearest triangles of a point over the world: WorldPointBody<false> with the list in the place of its one best record.
// best: the bound of both levels of boxes -- the rmax bound until the list is full, then the last slot's d2. The key is d2, each
// instance's own value for its own moved point (not the distance: two d2 may share a sqrtf)
struct WorldNearestBody {
    const WorldArgs& w;
    const uint4* node32;
    const float4* tri48;
    int inst;
    PointBound B;
    v3 p, wp;
    float rmax, qpad, best;
    WorldList L;
    bool alive;
    size_t idx;
    PointImage P;

    PSM_D WorldNearestBody(const WorldArgs& a) : w(a), L(a.samples) {}
    PSM_D float4 point() const {
        float4 q = make_float4(0.f, 0.f, 0.f, -1.f);
        if (alive) q = w.rays[idx];
        return q;
    }
    PSM_D bool begin(size_t i, bool al) {
        idx = i;
        alive = al;
        const float4 q = point();
        wp = mk3(q.x, q.y, q.z);
        qpad = WORLD_QSLACK * smaxf(smaxf(pabs(q.x), pabs(q.y)), pabs(q.z));
        rmax = q.w;
        best = (q.w * q.w) * 1.00000095367431640625f + 0x1p-126f;   // (query.hip PointBody::begin)
        L.clear();
        return al && finite3(wp) && q.w >= 0.f;
    }
    PSM_D float gap2(float lx, float ly, float lz, float hx, float hy, float hz) const {
        const float tx = smaxf(smaxf((lx - qpad) - wp.x, wp.x - (hx + qpad)), 0.f);
        const float ty = smaxf(smaxf((ly - qpad) - wp.y, wp.y - (hy + qpad)), 0.f);
        const float tz = smaxf(smaxf((lz - qpad) - wp.z, wp.z - (hz + qpad)), 0.f);
        return (tx * tx + ty * ty) + tz * tz;
    }
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = gap2(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y);
        kR = gap2(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w);
        const float lim = best + WORLD_PSLACK * best;
        okL = !(kL > lim);
        okR = !(kR > lim);
    }
    PSM_D int enter(int in) {
        const float4 q = point();
        const RowLoad r = load_row(w, in, *this);
        p = inst_point(r.m, mk3(q.x, q.y, q.z));
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(r.sm[SM_M + k]);
        B = point_bound(M);
        P.set(M, p);
        if (!finite3(p)) return -1;
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;
    }
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        P.children(B, n0, n1, best, okL, okR, kL, kR);
    }
    PSM_D static float test(const float4* tris, int tri, v3 at, float& u, float& v) {
        const float4 A = tris[(size_t)3 * tri + 0], Bv = tris[(size_t)3 * tri + 1], Cv = tris[(size_t)3 * tri + 2];
        return closest_on_tri(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(Cv.x, Cv.y, Cv.z), at, u, v);
    }
    PSM_D void leaf(int tri) {
        float u, v;
        const float d2 = test(tri48, tri, p, u, v);
        if (sqrtf(d2) <= rmax) best = L.offer(d2, (uint32_t)inst, (uint32_t)tri, best);
    }
    PSM_D bool done() const { return false; }
    PSM_D bool again() const { return false; }
    PSM_D void finish(size_t i) const {
        const float4 q = point();
        float4* __restrict__ row = w.hits + i * L.k;
        int32_t* __restrict__ irow = w.geom + i * L.k;
        for (uint32_t s = 0; s < L.k; s++) {
            float4 h = miss_hit();
            int32_t hin = -1;
            if (s < L.cnt) {
                const uint2 e = L.key[(size_t)s * QUERY_BLOCK];
                const uint32_t in = L.ins[(size_t)s * QUERY_BLOCK];
                float m[12];
                const float4* tris = load_pose(w, in, m);
                float u, v;
                (void)test(tris, (int)e.y, inst_point(m, mk3(q.x, q.y, q.z)), u, v);
                h = make_float4(u, v, sqrtf(__uint_as_float(e.x)), __uint_as_float(e.y));
                hin = (int32_t)in;
            }
            row[s] = h;
            irow[s] = hin;
        }
        w.count[i] = L.cnt;
    }
};

}  // namespace

// The lane's two hierarchy pointers, its instance index and the world ray beside the object ray do not fit 64 VGPRs: the
// kernels are built for 4 waves per SIMD (128 VGPRs), without spills or scratch (tests/test_world_query_cpu.py holds the counts).
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_closest(WorldArgs w) { world_body<WorldRayBody<false>>(w); }
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_any(WorldArgs w) { world_body<WorldRayBody<true>>(w); }
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_point(WorldArgs w) { world_body<WorldPointBody<false>>(w); }
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_within(WorldArgs w) { world_body<WorldPointBody<true>>(w); }
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_count(WorldArgs w) { world_body<WorldCountBody>(w); }
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_inside(WorldArgs w) { world_body<WorldInsideBody<false>>(w); }
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_sign(WorldArgs w) { world_body<WorldInsideBody<true>>(w); }

// WorldArgs as the closest-hit / closest-point kernels read it, and: hits and geom [n][k], count [n], samples = k; the launch
// gives k x 64 x 12 B of dynamic LDS beside the stack (DESIGN.md 4.14 has the budget and the register counts)
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_first_hits(WorldArgs w) { world_body<WorldFirstHitsBody>(w); }
__global__ __launch_bounds__(QUERY_BLOCK, 4) void world_query_nearest(WorldArgs w) { world_body<WorldNearestBody>(w); }

// ---- set-up kernels: boxes, Morton keys, the tree, its boxes (correct and free of host round trips; not tuned) -----------------

struct WorldSrc {   // a distinct hierarchy of a world: its triangles as the candidate tests read them
    const float4* tri48;
    uint32_t tris;
    uint32_t pad;
};

// the object-space box of each distinct hierarchy: min / max over v0, v0 + e1, v0 + e2 of ALL its loaded triangles -- a superset
// of the kept ones (a triangle the build dropped only widens the box); a NaN coordinate is ignored (fminf / fmaxf)
__global__ __launch_bounds__(256) void world_obj_boxes(const WorldSrc* __restrict__ src, float4* __restrict__ obox) {
    __shared__ float red[6][256];
    const WorldSrc s = src[blockIdx.x];
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (uint32_t t = threadIdx.x; t < s.tris; t += 256u) {
        const float4 a = s.tri48[(size_t)3 * t], b = s.tri48[(size_t)3 * t + 1], c = s.tri48[(size_t)3 * t + 2];
        const float v[3][3] = {{a.x, a.y, a.z}, {a.x + b.x, a.y + b.y, a.z + b.z}, {a.x + c.x, a.y + c.y, a.z + c.z}};
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) { lo[j] = fminf(lo[j], v[k][j]); hi[j] = fmaxf(hi[j], v[k][j]); }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) { red[j][threadIdx.x] = lo[j]; red[3 + j][threadIdx.x] = hi[j]; }
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if ((int)threadIdx.x < s2)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                red[j][threadIdx.x] = fminf(red[j][threadIdx.x], red[j][threadIdx.x + s2]);
                red[3 + j][threadIdx.x] = fmaxf(red[3 + j][threadIdx.x], red[3 + j][threadIdx.x + s2]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        obox[2 * blockIdx.x] = make_float4(red[0][0], red[1][0], red[2][0], 0.f);
        obox[2 * blockIdx.x + 1] = make_float4(red[3][0], red[4][0], red[5][0], 0.f);
    }
}

// the padded world box of each instance: centre R c + T, half extent |R| e, grown by WORLD_PAD * S + WORLD_FLOOR. A hierarchy
// without triangles (lo = +inf, hi = -inf) gets an inverted box that no query passes.
__global__ __launch_bounds__(256) void world_inst_boxes(const WorldRow* __restrict__ rows, const uint32_t* __restrict__ slot,
                                                        const float4* __restrict__ obox, uint32_t n, float4* __restrict__ box) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 lo = obox[2 * slot[i]], hi = obox[2 * slot[i] + 1];
    const float* m = rows[i].m;
    if (!(lo.x <= hi.x && lo.y <= hi.y && lo.z <= hi.z)) {
        box[2 * i] = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.f);
        box[2 * i + 1] = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), 0.f);
        return;
    }
    const float c[3] = {0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z};
    const float e[3] = {0.5f * hi.x - 0.5f * lo.x, 0.5f * hi.y - 0.5f * lo.y, 0.5f * hi.z - 0.5f * lo.z};
    float S = fmaxf(fmaxf(fmaxf(pabs(lo.x), pabs(hi.x)), fmaxf(pabs(lo.y), pabs(hi.y))), fmaxf(pabs(lo.z), pabs(hi.z)));
    S = fmaxf(S, fmaxf(fmaxf(pabs(m[3]), pabs(m[7])), pabs(m[11])));
    float cw[3], ew[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        cw[k] = ((m[4 * k] * c[0] + m[4 * k + 1] * c[1]) + m[4 * k + 2] * c[2]) + m[4 * k + 3];
        ew[k] = (pabs(m[4 * k]) * e[0] + pabs(m[4 * k + 1]) * e[1]) + pabs(m[4 * k + 2]) * e[2];
        S = fmaxf(S, pabs(cw[k]) + ew[k]);
    }
    const float pad = WORLD_PAD * S + WORLD_FLOOR;
    box[2 * i] = make_float4((cw[0] - ew[0]) - pad, (cw[1] - ew[1]) - pad, (cw[2] - ew[2]) - pad, 0.f);
    box[2 * i + 1] = make_float4((cw[0] + ew[0]) + pad, (cw[1] + ew[1]) + pad, (cw[2] + ew[2]) + pad, 0.f);
}

PSM_D float finite_or(float x, float y) { return __builtin_isfinite(x) ? x : y; }

// the bounds of the finite box centres (one workgroup; at most 65 536 instances)
__global__ __launch_bounds__(1024) void world_centre_bounds(const float4* __restrict__ box, uint32_t n, float4* __restrict__ bounds) {
    __shared__ float red[6][1024];
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (uint32_t i = threadIdx.x; i < n; i += 1024u) {
        const float4 a = box[2 * i], b = box[2 * i + 1];
        const float c[3] = {0.5f * a.x + 0.5f * b.x, 0.5f * a.y + 0.5f * b.y, 0.5f * a.z + 0.5f * b.z};
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (__builtin_isfinite(c[j])) { lo[j] = fminf(lo[j], c[j]); hi[j] = fmaxf(hi[j], c[j]); }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) { red[j][threadIdx.x] = lo[j]; red[3 + j][threadIdx.x] = hi[j]; }
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                red[j][threadIdx.x] = fminf(red[j][threadIdx.x], red[j][threadIdx.x + s]);
                red[3 + j][threadIdx.x] = fmaxf(red[3 + j][threadIdx.x], red[3 + j][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        bounds[0] = make_float4(red[0][0], red[1][0], red[2][0], 0.f);
        bounds[1] = make_float4(red[3][0], red[4][0], red[5][0], 0.f);
    }
}

// key = the 48-bit Morton code of the box centre (16 bits per axis over the centres' bounds) << 16 | the instance index: the
// keys are distinct, the index breaks ties, and the tree over them is at most 64 levels deep
__global__ __launch_bounds__(256) void world_morton(const float4* __restrict__ box, const float4* __restrict__ bounds, uint32_t n,
                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = box[2 * i], b = box[2 * i + 1], lo = bounds[0], hi = bounds[1];
    const float c[3] = {0.5f * a.x + 0.5f * b.x, 0.5f * a.y + 0.5f * b.y, 0.5f * a.z + 0.5f * b.z};
    const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
    uint32_t q[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float ext = h[j] - l[j];
        float f = (ext > 0.f && __builtin_isfinite(ext)) ? (finite_or(c[j], l[j]) - l[j]) / ext : 0.f;
        f = f > 0.f ? f : 0.f;   // (NaN: 0)
        f = f < 1.f ? f : 1.f;
        const uint32_t v = (uint32_t)(f * 65536.0f);
        q[j] = v < 65535u ? v : 65535u;
    }
    keys[i] = (morton3_64(q[0], q[1], q[2]) << 16) | (uint64_t)i;
    idx[i] = i;
}

// the radix tree over the sorted distinct keys (Karras 2012): thread i makes internal node i; node 0 is the root. parent[]:
// (node << 1 | side) for every internal node (entry i) and every leaf position (entry n - 1 + p); the root's is -1
PSM_D int key_delta(const uint64_t* __restrict__ keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    return __builtin_clzll(keys[i] ^ keys[j]);
}
__global__ __launch_bounds__(256) void world_emit(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint32_t n,
                                                  WorldNode* __restrict__ nodes, int* __restrict__ parent) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x), N = (int)n;
    if (i >= N - 1) return;
    const int d = key_delta(keys, N, i, i + 1) - key_delta(keys, N, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = key_delta(keys, N, i, i - d);
    int lmax = 2;
    while (lmax < 2 * N && key_delta(keys, N, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (key_delta(keys, N, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = key_delta(keys, N, i, j);
    int s = 0;
    for (int t = l; t > 1;) {
        t = (t + 1) >> 1;
        if (key_delta(keys, N, i, i + (s + t) * d) > dnode) s += t;
    }
    const int gamma = i + s * d + (d < 0 ? -1 : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const bool leafL = lo == gamma, leafR = hi == gamma + 1;
    nodes[i].w3 = make_int4(leafL ? ~(int)idx[gamma] : gamma, leafR ? ~(int)idx[gamma + 1] : gamma + 1, 0, 0);
    parent[leafL ? N - 1 + gamma : gamma] = i << 1;
    parent[leafR ? N - 1 + gamma + 1 : gamma + 1] = (i << 1) | 1;
    if (i == 0) parent[0] = -1;
}

// The boxes, bottom-up: a thread per leaf position carries its subtree's box (and height) to the parent's record; the first
// of a node's two children to arrive stops there, the second reads its sibling's half (written before the sibling's fence and
// counter increment; read with agent-scope atomic loads, past this CU's vector cache) and carries the exact min / max union
// further. Nobody waits for anybody: a thread leaves or goes on. Bounded by the tree's height.
PSM_D float load_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__global__ __launch_bounds__(256) void world_fit(const float4* __restrict__ box, const uint32_t* __restrict__ idx, uint32_t n,
                                                 WorldNode* nodes, const int* __restrict__ parent, uint32_t* arrived, int* height,
                                                 int* depth) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const float4 a = box[2 * idx[p]], b = box[2 * idx[p] + 1];
    float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z};
    int h = 0;
    int par = parent[n - 1 + p];
    while (par >= 0) {
        const int node = par >> 1, side = par & 1;
        float* rec = (float*)(nodes + node);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            __hip_atomic_store(rec + 6 * side + j, lo[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(rec + 6 * side + 3 + j, hi[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(height + 2 * node + side, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        if (atomicAdd(arrived + node, 1u) == 0u) return;
        __threadfence();
        const int other = side ^ 1;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            lo[j] = fminf(lo[j], load_agent(rec + 6 * other + j));
            hi[j] = fmaxf(hi[j], load_agent(rec + 6 * other + 3 + j));
        }
        const int ho = __hip_atomic_load(height + 2 * node + other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        h = (h > ho ? h : ho) + 1;
        if (node == 0) *depth = h;
        par = parent[node];
    }
}

// a query of an empty world: every record a miss
__global__ __launch_bounds__(256) void world_fill_miss(float4* hits, int32_t* geom, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    hits[i] = make_float4(0.f, 0.f, __builtin_inff(), __int_as_float(-1));
    geom[i] = -1;
}

}  // namespace psm

// ---- host side ---------------------------------------------------------------------------------------------------------------

struct psm_world {
    psm_ctx* ctx = nullptr;
    uint32_t cap = 0, count = 0;
    int depth = 0;                          // of the tree over the instances (internal nodes on the longest root-to-leaf path)
    std::vector<psm_instance> insts;        // the list as set
    std::vector<uint32_t> slot;             // per instance: its hierarchy's index in `distinct`
    std::vector<psm_bvh*> distinct;         // the hierarchies of the list, each once, in order of first appearance
    std::vector<uint64_t> gens;             // ... and the generation each had at psm_world_set_instances
    std::vector<uint32_t> first_of;         // ... and the first instance that uses it
    std::vector<psm::WorldRow> rows;        // staging of d_rows
    std::vector<psm::WorldSrc> srcs;        // staging of d_src
    psm::WorldRow* d_rows = nullptr;
    uint32_t* d_slot = nullptr;
    psm::WorldSrc* d_src = nullptr;
    float4* d_obox = nullptr;               // 2 per distinct hierarchy
    float4* d_box = nullptr;                // 2 per instance: the padded world box
    float4* d_bounds = nullptr;             // 2
    uint64_t* d_keys = nullptr;
    uint32_t* d_idx = nullptr;
    psm::WorldNode* d_nodes = nullptr;
    int* d_parent = nullptr;                // 2 cap
    uint32_t* d_arrived = nullptr;
    int* d_height = nullptr;                // 2 cap
    int* d_depth = nullptr;
};

namespace psm {
namespace {

const char* const WORLD_NAME[19] = {"psm_world_intersect_dev", "psm_world_occluded_dev", "psm_world_closest_point_dev",
                                    "psm_world_within_dev", "psm_world_count_hits_dev", "psm_world_inside_dev",
                                    "psm_world_signed_distance_dev", "psm_world_first_hits_dev", "psm_world_nearest_dev",
                                    "psm_world_box_overlaps_dev", "psm_world_box_count_dev", "psm_world_box_triangles_dev",
                                    "psm_world_sweep_sphere_dev", "psm_world_sweep_occluded_dev",
                                    "psm_world_tri_overlaps_dev", "psm_world_tri_count_dev", "psm_world_tri_triangles_dev",
                                    "psm_world_tri_closest_dev", "psm_world_tri_within_dev"};
const Kernels<WorldArgs> WORLD_KERNELS = {{world_query_closest, world_query_any, world_query_point, world_query_within,
                                           world_query_count, world_query_inside, world_query_sign}};

// what a walk of the hierarchy can hold on the stack: the builder's bound (depth_bound), and never more than its internal nodes
int hier_depth(const psm_bvh* b) {
    const int bound = depth_bound(b);
    const int nodes = b->tri_count > 0 ? (int)(b->tri_count < (1u << 30) ? b->tri_count : (1u << 30)) - 1 : 0;
    return nodes < bound ? nodes : bound;
}

// the first instance whose hierarchy is no longer what the world recorded, or -1
int first_stale(const psm_world* w) {
    int first = -1;
    for (size_t h = 0; h < w->distinct.size(); h++)
        if ((bvh_generation(w->distinct[h]) != w->gens[h] || !w->distinct[h]->built) && (first < 0 || (int)w->first_of[h] < first))
            first = (int)w->first_of[h];
    return first;
}
int refuse_stale(const psm_world* w, const char* name, int inst) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: instance %d's hierarchy was rebuilt, or reloaded and not refitted, after psm_world_set_instances (set the instances again)", name, inst);
    return set_err(w->ctx, PSM_ERR_STATE, msg);
}

void world_clear(psm_world* w) {
    w->count = 0;
    w->depth = 0;
    w->insts.clear(); w->slot.clear(); w->distinct.clear(); w->gens.clear(); w->first_of.clear(); w->rows.clear(); w->srcs.clear();
}

// boxes and tree from the table on the device (the context's stream); reads the tree's depth back (one synchronisation)
int world_rebuild(psm_world* w) {
    psm_ctx* c = w->ctx;
    const uint32_t n = w->count, nh = (uint32_t)w->distinct.size();
    w->depth = 0;
    if (n < 2) return PSM_OK;   // a world of one: no tree, the instance is entered by every query
    const uint32_t grid = (n + 255u) / 256u;
    world_obj_boxes<<<nh, 256, 0, c->stream>>>(w->d_src, w->d_obox);
    world_inst_boxes<<<grid, 256, 0, c->stream>>>(w->d_rows, w->d_slot, w->d_obox, n, w->d_box);
    world_centre_bounds<<<1, 1024, 0, c->stream>>>(w->d_box, n, w->d_bounds);
    world_morton<<<grid, 256, 0, c->stream>>>(w->d_box, w->d_bounds, n, w->d_keys, w->d_idx);
    PSM_HIP(c, hipGetLastError());
    int rc = launch_sort(c, w->d_keys, w->d_idx, n, nullptr, 64);
    if (rc != PSM_OK) return rc;
    PSM_HIP(c, hipMemsetAsync(w->d_arrived, 0, (size_t)n * sizeof(uint32_t), c->stream));
    world_emit<<<grid, 256, 0, c->stream>>>(w->d_keys, w->d_idx, n, w->d_nodes, w->d_parent);
    world_fit<<<grid, 256, 0, c->stream>>>(w->d_box, w->d_idx, n, w->d_nodes, w->d_parent, w->d_arrived, w->d_height, w->d_depth);
    PSM_HIP(c, hipGetLastError());
    int depth = 0;
    PSM_HIP(c, hipMemcpyAsync(&depth, w->d_depth, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    rc = sort_check(c);
    if (rc != PSM_OK) return rc;
    w->depth = depth;
    return PSM_OK;
}

// the depth rule: the tree's depth, one entry for the way back, the deepest hierarchy's bound
int check_depth(psm_world* w, const char* name) {
    int deepest = 0;
    uint32_t which = 0;
    for (size_t h = 0; h < w->distinct.size(); h++)
        if (hier_depth(w->distinct[h]) > deepest) { deepest = hier_depth(w->distinct[h]); which = w->first_of[h]; }
    if (w->depth + deepest + 1 <= QSTACK_MAX) return PSM_OK;
    char msg[200];
    snprintf(msg, sizeof msg, "%s: the tree over the instances (depth %d) and instance %u's hierarchy (depth bound %d) are together deeper than the query stack (%d); the world is left empty",
             name, w->depth, which, deepest, QSTACK_MAX);
    world_clear(w);
    return set_err(w->ctx, PSM_ERR_CAPACITY, msg);
}

int world_upload_and_build(psm_world* w, const char* name) {
    psm_ctx* c = w->ctx;
    (void)hipSetDevice(c->device);
    const uint32_t n = w->count;
    PSM_HIP(c, hipMemcpyAsync(w->d_rows, w->rows.data(), (size_t)n * sizeof(WorldRow), hipMemcpyHostToDevice, c->stream));
    PSM_HIP(c, hipMemcpyAsync(w->d_slot, w->slot.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    PSM_HIP(c, hipMemcpyAsync(w->d_src, w->srcs.data(), w->srcs.size() * sizeof(WorldSrc), hipMemcpyHostToDevice, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));   // (the staging vectors are pageable and the caller's to change)
    int rc = world_rebuild(w);
    if (rc != PSM_OK) { world_clear(w); return rc; }
    return check_depth(w, name);
}

// How a walk of the world starts, the rest zero: the tree's root or the one instance of a world of one, the table, the tree
WorldArgs world_start(const psm_world* w) {
    WorldArgs a = {};
    a.root = w->count == 1 ? ~0 : 0;
    a.rows = w->d_rows;
    a.nodes = w->d_nodes;
    return a;
}

// the grid's nine numbers, its bricks and the world's root as the kernels take them (the twin of psm_grid_dev.h's grid_args)
WorldGridArgs world_grid_args(const psm_grid* grid, const GridShape& s, const psm_world* w) {
    WorldGridArgs g = {};
    g.ox = grid->origin[0]; g.oy = grid->origin[1]; g.oz = grid->origin[2];
    g.cx = grid->cell[0]; g.cy = grid->cell[1]; g.cz = grid->cell[2];
    g.nx = grid->dims[0]; g.ny = grid->dims[1]; g.nz = grid->dims[2];
    g.nbx = s.nb[0]; g.nby = s.nb[1];
    g.bricks = (uint32_t)s.bricks;
    g.root = world_start(w).root;
    return g;
}

// A query of a world: the data (check_data, as every query's), the empty world's answer, the stale check, the launch. The
// k-best kinds come through here too: samples is their k, d_out and d_inst their [n][k] rows, d_count their counts (which go
// through check_data's index slot as "counts", as in query.hip's query(); d_inst is then checked here). And the box kinds
// (world_box.hip): d_in the world boxes; the triangles query as a k-best kind with int32 rows: d_out the [n][k] triangles,
// d_inst the [n][k] instances, d_count the counts. And the sweep kinds (world_sweep.hip): d_in the sweeps, a 16-byte record and
// d_inst, or a byte, as the closest-hit and the any-hit kinds. And the triangle kinds (world_tri.hip): d_in the world triangles
// (psm_tri_query), everything else as the box kinds. And the clearance kinds (world_tri_dist.hip): d_in the world triangles with
// their rmax (psm_tri_dist_query), d_out two float4 per query and d_inst, or a byte
int world_query(psm_world* w, QueryKind kind, const void* d_in, size_t n, void* d_out, int32_t* d_inst, uint32_t samples = 0,
                uint32_t* d_count = nullptr) {
    if (!w) return PSM_ERR_INVALID;
    if (n == 0) return PSM_OK;
    psm_ctx* c = w->ctx;
    const char* name = WORLD_NAME[kind];
    const bool box = kind >= Q_BOX_ANY && kind <= Q_BOX_TRIS, sweep = kind == Q_SWEEP || kind == Q_SWEEP_ANY;
    const bool tri = kind >= Q_TRI_ANY && kind <= Q_TRI_TRIS;
    const bool clear = kind == Q_TRI_CLOSEST || kind == Q_TRI_WITHIN;
    const bool kbest = kind == Q_FIRST_HITS || kind == Q_NEAREST || kind == Q_BOX_TRIS || kind == Q_TRI_TRIS;   // (the kinds with rows and counts)
    int rc = kbest ? check_data(c, name, "counts", kind, d_in, d_out, (const int32_t*)d_count, samples)
                   : check_data(c, name, "inst", kind, d_in, d_out, d_inst, samples);
    if (rc != PSM_OK) return rc;
    if (kbest && (!d_inst || ((uintptr_t)d_inst & 3u) != 0)) {
        char msg[128];
        snprintf(msg, sizeof msg, d_inst ? "%s: inst not 4-byte aligned" : "%s: NULL pointer", name);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    const size_t rows = kbest ? n * samples : n;   // (samples <= PSM_QUERY_K_MAX here)
    if (w->count == 0) {   // an empty world: every query misses, no query kernel runs
        const unsigned per = QUERY_DESC[kind].out_align;
        if (kind == Q_BOX_TRIS || kind == Q_TRI_TRIS) {   // rows of -1 in both arrays
            PSM_HIP(c, hipMemsetAsync(d_out, 0xFF, rows * sizeof(int32_t), c->stream));
            PSM_HIP(c, hipMemsetAsync(d_inst, 0xFF, rows * sizeof(int32_t), c->stream));
        } else if (kind == Q_TRI_CLOSEST) {   // (a psm_tri_hit is two float4: world_tri_dist.hip writes the miss records)
            WorldArgs e = {};
            e.n = n;
            e.hits = (float4*)d_out;
            e.geom = d_inst;
            return world_tri_dist_launch(c, false, 0, e);
        } else if (per == 16) world_fill_miss<<<(unsigned)((rows + 255) / 256), 256, 0, c->stream>>>((float4*)d_out, d_inst, rows);
        else PSM_HIP(c, hipMemsetAsync(d_out, 0, n * per, c->stream));
        PSM_HIP(c, hipGetLastError());
        if (kbest) PSM_HIP(c, hipMemsetAsync(d_count, 0, n * sizeof(uint32_t), c->stream));
        return PSM_OK;
    }
    const int stale = first_stale(w);
    if (stale >= 0) return refuse_stale(w, name, stale);
    WorldArgs a = world_start(w);
    uint32_t grid = 0;
    rc = batch_args(c, d_in, n, d_out, samples, a, grid);
    if (rc != PSM_OK) return rc;
    a.geom = d_inst;
    if (box) {   // (world_box.hip; the triangles query's list: k x 64 x 8 B of dynamic LDS, the launch's)
        if (kind == Q_BOX_TRIS) a.count = d_count;
        return world_box_launch(c, (int)kind - (int)Q_BOX_ANY, grid, a);
    }
    if (sweep) return world_sweep_launch(c, kind == Q_SWEEP_ANY, grid, a);   // (world_sweep.hip)
    if (tri) {   // (world_tri.hip; rows, counts and the list's LDS as the box kinds')
        if (kind == Q_TRI_TRIS) a.count = d_count;
        return world_tri_launch(c, (int)kind - (int)Q_TRI_ANY, grid, a);
    }
    if (clear) return world_tri_dist_launch(c, kind == Q_TRI_WITHIN, grid, a);   // (world_tri_dist.hip)
    if (kbest) {   // the list: k x 64 x (8 + 4) B of dynamic LDS per wave, beside the stack
        a.count = d_count;
        const size_t lds = (size_t)samples * QUERY_BLOCK * (sizeof(uint2) + sizeof(uint32_t));
        if (kind == Q_NEAREST) world_query_nearest<<<grid, QUERY_BLOCK, lds, c->stream>>>(a);
        else world_query_first_hits<<<grid, QUERY_BLOCK, lds, c->stream>>>(a);
        PSM_HIP(c, hipGetLastError());
        return PSM_OK;
    }
    return launch(c, WORLD_KERNELS, kind, grid, a);
}

const char* const WORLD_MESH_NAME[] = {"psm_world_mesh_overlaps_dev", "psm_world_mesh_count_dev", "psm_world_mesh_triangles_dev"};

// A world's skip argument: an instance index, or -1
int world_mesh_skip_ok(const psm_world* w, const char* name, int32_t skip) {
    if (skip >= -1 && (skip < 0 || (uint32_t)skip < w->count)) return PSM_OK;
    return mesh_refuse(w->ctx, PSM_ERR_INVALID, "%s: skip %d of a world of %u (-1: no instance is left out)", name, (int)skip, w->count);
}

// A mesh query of a world (world_mesh.hip): mesh.hip's mesh_query() with a world where the queried hierarchy was,
// of the same shared pieces (psm_query_host.h). The NULL world and p == 0 are answered before anything else is
// looked at; then the data, k, the other hierarchy's state and context, the stale check (every world query's), the poses, skip,
// the number of answers -- all on the host, before any launch, the outputs untouched. Then the upload (one synchronisation),
// the outputs are cleared in stream order, and one kernel runs unless the world is empty or the other hierarchy has no leaf.
// mode: 0 overlaps, 1 count, 2 triangles
int world_mesh_query(psm_world* w, psm_bvh* o, const float* poses, size_t p, int32_t skip, int mode, uint32_t k, void* d_out,
                     int32_t* d_inst, uint32_t* d_count) {
    if (!w) return PSM_ERR_INVALID;
    if (p == 0) return PSM_OK;
    psm_ctx* c = w->ctx;
    const char* name = WORLD_MESH_NAME[mode];
    const bool rows = mode == 2;
    int rc = mesh_pointers(c, name, o && poses && d_out && (!rows || (d_inst && d_count)));
    if (rc == PSM_OK && mode != 0) rc = mesh_aligned(c, name, rows ? "tris" : "counts", d_out, 4);
    if (rc == PSM_OK && rows) rc = mesh_aligned(c, name, "inst", d_inst, 4);
    if (rc == PSM_OK && rows) rc = mesh_aligned(c, name, "counts", d_count, 4);
    if (rc != PSM_OK) return rc;
    if (rows && (k == 0 || k > PSM_QUERY_K_MAX)) return mesh_refuse(c, PSM_ERR_INVALID, "%s: k must be 1 .. %d", name, PSM_QUERY_K_MAX);
    if (!o->built) return set_err(c, PSM_ERR_STATE, "mesh query before build");
    if (o->ctx != c) return mesh_refuse(c, PSM_ERR_INVALID, "%s: the world and the other hierarchy are of different contexts", name);
    const int stale = first_stale(w);
    if (stale >= 0) return refuse_stale(w, name, stale);
    const uint32_t T = o->tri_count;
    rc = mesh_poses_rigid(c, name, poses, p);
    if (rc == PSM_OK) rc = world_mesh_skip_ok(w, name, skip);
    if (rc == PSM_OK) rc = mesh_answers_fit(c, name, p, T);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    uint32_t L = 0;
    void* d_poses = nullptr;
    WorldMeshArgs m = {};
    m.w = world_start(w);
    uint32_t grid = 0;
    if (w->count != 0) {   // (an empty world: no query kernel, nothing to upload; the clears alone)
        rc = mesh_upload(c, o, poses, p, &d_poses, nullptr, &L);
        if (rc != PSM_OK) return rc;
        // (the context's stack area is allocated here, on its first query: the last thing that can fail before the outputs change)
        rc = batch_args(c, nullptr, p * (size_t)L, d_out, k, m.w, grid);
        if (rc != PSM_OK) return rc;
    }
    // the outputs, cleared in stream order: a dropped triangle's entries and an unset flag read 0 / -1
    const size_t cells = p * (size_t)T;
    if (mode == 0) PSM_HIP(c, hipMemsetAsync(d_out, 0, p, c->stream));
    if (mode == 1) PSM_HIP(c, hipMemsetAsync(d_out, 0, cells * sizeof(uint32_t), c->stream));
    if (rows) {
        PSM_HIP(c, hipMemsetAsync(d_out, 0xff, cells * k * sizeof(int32_t), c->stream));
        PSM_HIP(c, hipMemsetAsync(d_inst, 0xff, cells * k * sizeof(int32_t), c->stream));
        PSM_HIP(c, hipMemsetAsync(d_count, 0, cells * sizeof(uint32_t), c->stream));
    }
    if (w->count == 0 || L == 0) return PSM_OK;
    m.w.geom = d_inst;
    if (rows) m.w.count = d_count;
    m.tri48 = o->d_tri48; m.leaf_tri = o->d_leaftri; m.poses = (const float4*)d_poses;
    m.L = L; m.T = T; m.skip = skip;
    m.flags = mesh_skip(p * (size_t)L) ? WORLD_MESH_FLAG_SKIP : 0u;   // (read by the flag kernel alone)
    return world_mesh_launch(c, mode, grid, m);
}

const char* const WORLD_MESH_DIST_NAME[] = {"psm_world_mesh_closest_dev", "psm_world_mesh_within_dev", "psm_world_mesh_clearance_dev"};

// A mesh clearance query of a world (world_mesh_dist.hip): world_mesh_query()'s sequence with the records'
// alignment where its k was; all on the host, before any launch, the outputs untouched. Then the upload (one synchronisation),
// every word of the clearance query is set to "none" in stream order, and the kernels run -- unless the world is empty or the
// other hierarchy has no leaf: then the miss records are written without a walk. mode: WMD_CLOSEST, WMD_WITHIN, WMD_CLEAR
int world_mesh_dist_query(psm_world* w, psm_bvh* o, const float* poses, size_t p, int32_t skip, int mode, float rmax, void* d_out,
                          int32_t* d_inst) {
    if (!w) return PSM_ERR_INVALID;
    if (p == 0) return PSM_OK;
    psm_ctx* c = w->ctx;
    const char* name = WORLD_MESH_DIST_NAME[mode];
    const bool records = mode != WMD_WITHIN;
    int rc = mesh_pointers(c, name, o && poses && d_out && (!records || d_inst));
    if (rc == PSM_OK && records) rc = mesh_aligned(c, name, "hits", d_out, 16);
    if (rc == PSM_OK && records) rc = mesh_aligned(c, name, "inst", d_inst, 4);
    if (rc != PSM_OK) return rc;
    if (!o->built) return set_err(c, PSM_ERR_STATE, "mesh query before build");
    if (o->ctx != c) return mesh_refuse(c, PSM_ERR_INVALID, "%s: the world and the other hierarchy are of different contexts", name);
    const int stale = first_stale(w);
    if (stale >= 0) return refuse_stale(w, name, stale);
    const uint32_t T = o->tri_count;
    rc = mesh_poses_rigid(c, name, poses, p);
    if (rc == PSM_OK) rc = world_mesh_skip_ok(w, name, skip);
    if (rc == PSM_OK) rc = mesh_answers_fit(c, name, p, T);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    uint32_t L = 0;
    void *d_poses = nullptr, *d_keys = nullptr;
    WorldMeshDistArgs a = {};
    a.m.w = world_start(w);
    uint32_t grid = 0;
    if (w->count != 0) {   // (an empty world: no query kernel, nothing to upload; the miss records alone)
        rc = mesh_upload(c, o, poses, p, &d_poses, mode == WMD_CLEAR ? &d_keys : nullptr, &L);
        if (rc != PSM_OK) return rc;
        // (the context's stack area is allocated here, on its first query: the last thing that can fail before the outputs change)
        rc = batch_args(c, nullptr, p * (size_t)L, d_out, 0, a.m.w, grid);
        if (rc != PSM_OK) return rc;
    }
    const bool walk = w->count != 0 && L != 0;
    if (mode == WMD_WITHIN) PSM_HIP(c, hipMemsetAsync(d_out, 0, p, c->stream));
    else if (!walk || (mode == WMD_CLOSEST && L < T)) {   // the miss records: no walk, or a dropped triangle's cells
        WorldMeshDistArgs f = {};
        f.m.w.n = mode == WMD_CLOSEST ? p * (size_t)T : p;
        f.m.w.hits = (float4*)d_out;
        f.m.w.geom = d_inst;
        rc = world_mesh_dist_launch(c, WMD_FILL, 0, mode == WMD_CLEAR, 0, f);
        if (rc != PSM_OK) return rc;
    }
    if (!walk) return PSM_OK;
    a.m.w.geom = d_inst;
    a.m.tri48 = o->d_tri48; a.m.leaf_tri = o->d_leaftri; a.m.poses = (const float4*)d_poses;
    a.m.L = L; a.m.T = T; a.m.skip = skip;
    a.keys = (unsigned long long*)d_keys;
    a.rmax = rmax;
    if (mode == WMD_CLOSEST) return world_mesh_dist_launch(c, WMD_CLOSEST, 0, false, grid, a);
    if (mode == WMD_WITHIN) {
        a.m.flags = mesh_skip(p * (size_t)L) ? WORLD_MESH_FLAG_SKIP : 0u;
        return world_mesh_dist_launch(c, WMD_WITHIN, 0, false, grid, a);
    }
    // every word: "none"; the clearance kernel (mesh_bound(): the study knob, the same answer under each letter); then one lane
    // per pose walks the winner again and writes the record (a word left at "none": the miss)
    PSM_HIP(c, hipMemsetAsync(d_keys, 0xff, p * sizeof(uint64_t), c->stream));
    rc = world_mesh_dist_launch(c, WMD_CLEAR, mesh_bound(), false, grid, a);
    if (rc != PSM_OK) return rc;
    WorldMeshDistArgs pick = a;
    rc = batch_args(c, nullptr, p, d_out, 0, pick.m.w, grid);
    if (rc != PSM_OK) return rc;
    return world_mesh_dist_launch(c, WMD_PICK, 0, true, grid, pick);
}

const char* const WORLD_GRID_NAME[] = {"psm_grid_world_surface_dev", "psm_grid_world_counts_dev", "psm_grid_world_instances_dev",
                                       "psm_grid_world_solid_dev"};
enum { WGRID_SOLID = 3 };   // (beside psm_world_dev.h's WGRID_SURFACE, WGRID_COUNTS, WGRID_INSTANCES: the surface launch, then the fill)

// A grid over a world (world_grid.hip): grid.hip's grid_query() with a world where the hierarchy was, of the same
// shared pieces (psm_query_host.h). The NULL world is answered before anything else is looked at; then the front
// every grid call shares (grid_front: the pointers, the grid, the alignment, samples) -- all on the host, before any launch, the
// output untouched. An empty world is answered in stream order without a query kernel, BEFORE the stale refusal (every world
// query's; the mesh queries above have the two the other way round). The depth rule is psm_world_set_instances': the wave's one
// stack holds depth + deepest + 1 links. Solid: the surface launch, then the shared slab loop with psm_world_inside_dev where the
// hierarchy's inside query was
int world_grid_query(psm_world* w, const psm_grid* grid, int call, uint32_t samples, void* d_out) {
    if (!w) return PSM_ERR_INVALID;
    psm_ctx* c = w->ctx;
    const char* name = WORLD_GRID_NAME[call];
    const bool words = call == WGRID_SURFACE || call == WGRID_SOLID;
    GridShape s;
    int rc = grid_front(c, name, grid, d_out, s, words ? "bricks" : (call == WGRID_COUNTS ? "counts" : "inst"), d_out, words ? 8u : 4u,
                        nullptr, call == WGRID_SOLID ? &samples : nullptr);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    if (w->count == 0) {   // an empty world: no voxel is set, no query kernel runs
        const size_t voxels = (size_t)grid->dims[0] * grid->dims[1] * grid->dims[2];   // (a valid grid: below 2^37)
        if (words) PSM_HIP(c, hipMemsetAsync(d_out, 0, (size_t)s.bricks * sizeof(uint64_t), c->stream));
        else PSM_HIP(c, hipMemsetAsync(d_out, call == WGRID_COUNTS ? 0 : 0xFF, voxels * sizeof(uint32_t), c->stream));
        return PSM_OK;
    }
    const int stale = first_stale(w);
    if (stale >= 0) return refuse_stale(w, name, stale);
    const WorldGridArgs g = world_grid_args(grid, s, w);
    GridSlabs a;
    if (call == WGRID_SOLID) {   // (the last thing that can fail before the output changes)
        rc = slabs_for(c, s.bricks, false, a);
        if (rc != PSM_OK) return rc;
    }
    const uint32_t blocks = (uint32_t)(s.bricks < QUERY_GRID_CAP ? s.bricks : QUERY_GRID_CAP);
    rc = world_grid_launch(c, call == WGRID_SOLID ? (int)WGRID_SURFACE : call, blocks, g, w->d_rows, w->d_nodes, d_out);
    if (rc != PSM_OK || call != WGRID_SOLID) return rc;
    // the inside of the surface, a slab of bricks at a time, all in stream order: the centres, the world's inside query over
    // them, the flags' ballots ORed into the words
    return grid_slabs(s.bricks, a.slab, [&](uint32_t first, uint32_t bricks) {
        int rc = grid_centres_launch(c, grid, s, first, bricks, a.points);
        if (rc == PSM_OK) rc = psm_world_inside_dev(w, (const psm_point_query*)a.points, (size_t)bricks * QUERY_BLOCK, samples, a.flags);
        if (rc == PSM_OK) rc = grid_fill_launch(c, grid, s, first, bricks, a.flags, (uint64_t*)d_out);
        return rc;
    });
}

// psm_world_signed_distance_dev's second kernel alone, over n points and the closest-point records a grid walk wrote for them:
// the twin of query.hip's sign_launch. The caller has made every check (the world is not empty and not stale, samples is 1, 3 or 5)
int world_sign_launch(psm_world* w, const void* d_points, size_t n, uint32_t samples, void* d_hits) {
    WorldArgs a = world_start(w);
    uint32_t grid = 0;
    const int rc = batch_args(w->ctx, d_points, n, d_hits, samples, a, grid);
    if (rc != PSM_OK) return rc;
    world_query_sign<<<grid, QUERY_BLOCK, 0, w->ctx->stream>>>(a);
    PSM_HIP(w->ctx, hipGetLastError());
    return PSM_OK;
}

// A distance-field grid over a world (world_grid_dist.hip): grid_dist.hip's dist_query() with a world where the
// hierarchy was, of the same shared pieces. The NULL world is answered before anything else is looked at; then grid_front (the
// pointers, the grid, the alignment, rmax, samples) -- all on the host, before any launch, the outputs untouched. An empty world is
// answered in stream order by fills alone; then the stale refusal (every world query's). The depth rule is
// psm_world_set_instances'. Signed: the shared slab loop over slabs_for()'s scratch -- the centres, the walk's records beside them,
// the world's sign kernel over both, the records into the dense arrays --, the instances written by the walk itself
int world_grid_dist_query(psm_world* w, const psm_grid* grid, float rmax, bool sign, uint32_t samples, float* d_dist, int32_t* d_tri,
                          int32_t* d_inst) {
    if (!w) return PSM_ERR_INVALID;
    psm_ctx* c = w->ctx;
    const char* name = sign ? "psm_grid_world_signed_distance_dev" : "psm_grid_world_distance_dev";
    GridShape s;
    int rc = grid_front(c, name, grid, d_dist, s, "dist, tri or inst", (const void*)((uintptr_t)d_dist | (uintptr_t)d_tri | (uintptr_t)d_inst),
                        4, &rmax, sign ? &samples : nullptr);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    if (w->count == 0) {   // an empty world: every voxel misses, no query kernel runs
        const size_t voxels = (size_t)grid->dims[0] * grid->dims[1] * grid->dims[2];   // (a valid grid: below 2^37)
        PSM_HIP(c, hipMemsetD32Async((hipDeviceptr_t)d_dist, 0x7F800000, voxels, c->stream));   // +inf
        if (d_tri) PSM_HIP(c, hipMemsetAsync(d_tri, 0xFF, voxels * sizeof(int32_t), c->stream));
        if (d_inst) PSM_HIP(c, hipMemsetAsync(d_inst, 0xFF, voxels * sizeof(int32_t), c->stream));
        return PSM_OK;
    }
    const int stale = first_stale(w);
    if (stale >= 0) return refuse_stale(w, name, stale);
    WorldGridDistArgs a = {world_grid_args(grid, s, w), 0u, rmax};
    if (!sign) {
        const uint32_t blocks = (uint32_t)(s.bricks < QUERY_GRID_CAP ? s.bricks : QUERY_GRID_CAP);
        return world_grid_dist_launch(c, blocks, a, w->d_rows, w->d_nodes, d_dist, d_tri, d_inst, nullptr);
    }
    // signed, a slab of bricks at a time, all in stream order. The scratch and the context's stack area, which the sign launches
    // use, are the last things that can fail before the outputs change
    GridSlabs sl;
    void* spill = nullptr;
    rc = slabs_for(c, s.bricks, true, sl);
    if (rc == PSM_OK) rc = spill_for(c, &spill);
    if (rc != PSM_OK) return rc;
    return grid_slabs(s.bricks, sl.slab, [&](uint32_t first, uint32_t bricks) {
        int rc = grid_centres_launch(c, grid, s, first, bricks, sl.points);
        a.first = first; a.g.bricks = bricks;
        const uint32_t blocks = bricks < QUERY_GRID_CAP ? bricks : QUERY_GRID_CAP;
        if (rc == PSM_OK) rc = world_grid_dist_launch(c, blocks, a, w->d_rows, w->d_nodes, nullptr, nullptr, d_inst, sl.hits);
        if (rc == PSM_OK) rc = world_sign_launch(w, sl.points, (size_t)bricks * QUERY_BLOCK, samples, sl.hits);
        if (rc == PSM_OK) rc = grid_dist_scatter_launch(c, grid, s, first, bricks, sl.hits, d_dist, d_tri);
        return rc;
    });
}

template <class T>
int world_alloc(psm_ctx* c, T** p, size_t n) {
    PSM_HIP(c, hipMalloc((void**)p, (n ? n : 1) * sizeof(T)));
    return PSM_OK;
}

}  // namespace
}  // namespace psm

psm_world* psm_world_create(psm_ctx* c, uint32_t capacity) {
    using namespace psm;
    if (!c) return nullptr;
    if (capacity == 0 || capacity > PSM_WORLD_MAX_INSTANCES) {
        set_err(c, PSM_ERR_INVALID, "psm_world_create: capacity must be 1 .. PSM_WORLD_MAX_INSTANCES");
        return nullptr;
    }
    (void)hipSetDevice(c->device);
    psm_world* w = new (std::nothrow) psm_world();
    if (!w) return nullptr;
    w->ctx = c;
    w->cap = capacity;
    const size_t n = capacity;
    int rc = PSM_OK;
    auto A = [&](int r) { if (rc == PSM_OK) rc = r; };
    A(world_alloc(c, &w->d_rows, n)); A(world_alloc(c, &w->d_slot, n)); A(world_alloc(c, &w->d_src, n));
    A(world_alloc(c, &w->d_obox, 2 * n)); A(world_alloc(c, &w->d_box, 2 * n)); A(world_alloc(c, &w->d_bounds, 2));
    A(world_alloc(c, &w->d_keys, n)); A(world_alloc(c, &w->d_idx, n)); A(world_alloc(c, &w->d_nodes, n));
    A(world_alloc(c, &w->d_parent, 2 * n)); A(world_alloc(c, &w->d_arrived, n)); A(world_alloc(c, &w->d_height, 2 * n));
    A(world_alloc(c, &w->d_depth, 1));
    if (rc != PSM_OK) { psm_world_destroy(w); return nullptr; }
    return w;
}

int psm_world_destroy(psm_world* w) {
    if (!w) return PSM_ERR_INVALID;
    (void)hipSetDevice(w->ctx->device);
    (void)hipStreamSynchronize(w->ctx->stream);
    void* all[] = {w->d_rows, w->d_slot, w->d_src, w->d_obox, w->d_box, w->d_bounds, w->d_keys, w->d_idx, w->d_nodes, w->d_parent,
                   w->d_arrived, w->d_height, w->d_depth};
    for (void* p : all)
        if (p) (void)hipFree(p);
    delete w;
    return PSM_OK;
}

uint32_t psm_world_count(const psm_world* w) { return w ? w->count : 0u; }

int psm_world_set_instances(psm_world* w, const psm_instance* insts, uint32_t count) {
    using namespace psm;
    if (!w) return PSM_ERR_INVALID;
    psm_ctx* c = w->ctx;
    const char* name = "psm_world_set_instances";
    char msg[160];
    if (count == 0) { world_clear(w); return PSM_OK; }
    if (!insts) return set_err(c, PSM_ERR_INVALID, "psm_world_set_instances: NULL list");
    if (count > w->cap) {
        snprintf(msg, sizeof msg, "%s: %u instances exceed the world's capacity of %u", name, count, w->cap);
        return set_err(c, PSM_ERR_CAPACITY, msg);
    }
    // the per-entry checks of the instanced queries, in their order, all before any device work
    const int rc = check_instances(c, insts, count, name);
    if (rc != PSM_OK) return rc;
    world_clear(w);
    w->count = count;
    w->insts.assign(insts, insts + count);
    w->rows.resize(count);
    w->slot.resize(count);
    std::unordered_map<const psm_bvh*, uint32_t> seen;
    for (uint32_t g = 0; g < count; g++) {
        psm_bvh* b = insts[g].bvh;
        auto it = seen.find(b);
        if (it == seen.end()) {
            it = seen.emplace(b, (uint32_t)w->distinct.size()).first;
            w->distinct.push_back(b);
            w->gens.push_back(bvh_generation(b));
            w->first_of.push_back(g);
            w->srcs.push_back(WorldSrc{b->d_tri48, b->tri_count, 0u});
        }
        w->slot[g] = it->second;
        WorldRow& r = w->rows[g];
        r.node32 = b->d_node32; r.tri48 = b->d_tri48; r.sm = b->d_small; r.sorted_tri = b->d_sorted_tri;
        memcpy(r.m, insts[g].world_from_object, sizeof r.m);
    }
    return world_upload_and_build(w, name);
}

int psm_world_set_transforms(psm_world* w, uint32_t first, uint32_t count, const float* m12) {
    using namespace psm;
    if (!w) return PSM_ERR_INVALID;
    psm_ctx* c = w->ctx;
    const char* name = "psm_world_set_transforms";
    char msg[160];
    if ((uint64_t)first + count > w->count) {
        snprintf(msg, sizeof msg, "%s: instances %u .. %llu of a world of %u", name, first, (unsigned long long)first + count, w->count);
        return set_err(c, PSM_ERR_INVALID, msg);
    }
    if (count == 0) return PSM_OK;
    if (!m12) return set_err(c, PSM_ERR_INVALID, "psm_world_set_transforms: NULL matrices");
    for (uint32_t k = 0; k < count; k++)
        if (const char* why = pose_fault(m12 + 12 * (size_t)k)) {
            snprintf(msg, sizeof msg, "%s: instance %u %s", name, first + k, why);
            return set_err(c, PSM_ERR_INVALID, msg);
        }
    const int stale = first_stale(w);
    if (stale >= 0) return refuse_stale(w, name, stale);
    for (uint32_t k = 0; k < count; k++) {
        memcpy(w->insts[first + k].world_from_object, m12 + 12 * (size_t)k, 12 * sizeof(float));
        memcpy(w->rows[first + k].m, m12 + 12 * (size_t)k, 12 * sizeof(float));
    }
    for (size_t h = 0; h < w->distinct.size(); h++) w->srcs[h].tris = w->distinct[h]->tri_count;
    return world_upload_and_build(w, name);
}

int psm_world_intersect_dev(psm_world* w, const psm_query_ray* d_rays, size_t n, psm_hit* d_hits, int32_t* d_inst) {
    return psm::world_query(w, psm::Q_CLOSEST, d_rays, n, d_hits, d_inst);
}
int psm_world_occluded_dev(psm_world* w, const psm_query_ray* d_rays, size_t n, uint8_t* d_hit) {
    return psm::world_query(w, psm::Q_ANY, d_rays, n, d_hit, nullptr);
}
int psm_world_count_hits_dev(psm_world* w, const psm_query_ray* d_rays, size_t n, uint32_t* d_count) {
    return psm::world_query(w, psm::Q_COUNT, d_rays, n, d_count, nullptr);
}
int psm_world_closest_point_dev(psm_world* w, const psm_point_query* d_points, size_t n, psm_hit* d_hits, int32_t* d_inst) {
    return psm::world_query(w, psm::Q_POINT, d_points, n, d_hits, d_inst);
}
int psm_world_within_dev(psm_world* w, const psm_point_query* d_points, size_t n, uint8_t* d_hit) {
    return psm::world_query(w, psm::Q_WITHIN, d_points, n, d_hit, nullptr);
}
int psm_world_inside_dev(psm_world* w, const psm_point_query* d_points, size_t n, uint32_t samples, uint8_t* d_inside) {
    return psm::world_query(w, psm::Q_INSIDE, d_points, n, d_inside, nullptr, samples);
}
int psm_world_signed_distance_dev(psm_world* w, const psm_point_query* d_points, size_t n, uint32_t samples, psm_hit* d_hits,
                                  int32_t* d_inst) {
    return psm::world_query(w, psm::Q_SIGNED, d_points, n, d_hits, d_inst, samples);
}
int psm_world_first_hits_dev(psm_world* w, const psm_query_ray* d_rays, size_t n, uint32_t k, psm_hit* d_hits, int32_t* d_inst,
                             uint32_t* d_count) {
    return psm::world_query(w, psm::Q_FIRST_HITS, d_rays, n, d_hits, d_inst, k, d_count);
}
int psm_world_nearest_dev(psm_world* w, const psm_point_query* d_points, size_t n, uint32_t k, psm_hit* d_hits, int32_t* d_inst,
                          uint32_t* d_count) {
    return psm::world_query(w, psm::Q_NEAREST, d_points, n, d_hits, d_inst, k, d_count);
}
int psm_world_box_overlaps_dev(psm_world* w, const psm_box_query* d_boxes, size_t n, uint8_t* d_hit) {
    return psm::world_query(w, psm::Q_BOX_ANY, d_boxes, n, d_hit, nullptr);
}
int psm_world_box_count_dev(psm_world* w, const psm_box_query* d_boxes, size_t n, uint32_t* d_count) {
    return psm::world_query(w, psm::Q_BOX_COUNT, d_boxes, n, d_count, nullptr);
}
int psm_world_box_triangles_dev(psm_world* w, const psm_box_query* d_boxes, size_t n, uint32_t k, int32_t* d_tri, int32_t* d_inst,
                                uint32_t* d_count) {
    return psm::world_query(w, psm::Q_BOX_TRIS, d_boxes, n, d_tri, d_inst, k, d_count);
}
int psm_world_tri_overlaps_dev(psm_world* w, const psm_tri_query* d_tris, size_t n, uint8_t* d_hit) {
    return psm::world_query(w, psm::Q_TRI_ANY, d_tris, n, d_hit, nullptr);
}
int psm_world_tri_count_dev(psm_world* w, const psm_tri_query* d_tris, size_t n, uint32_t* d_count) {
    return psm::world_query(w, psm::Q_TRI_COUNT, d_tris, n, d_count, nullptr);
}
int psm_world_tri_triangles_dev(psm_world* w, const psm_tri_query* d_tris, size_t n, uint32_t k, int32_t* d_tri, int32_t* d_inst,
                                uint32_t* d_count) {
    return psm::world_query(w, psm::Q_TRI_TRIS, d_tris, n, d_tri, d_inst, k, d_count);
}
int psm_world_tri_closest_dev(psm_world* w, const psm_tri_dist_query* d_tris, size_t n, psm_tri_hit* d_hits, int32_t* d_inst) {
    return psm::world_query(w, psm::Q_TRI_CLOSEST, d_tris, n, d_hits, d_inst);
}
int psm_world_tri_within_dev(psm_world* w, const psm_tri_dist_query* d_tris, size_t n, uint8_t* d_hit) {
    return psm::world_query(w, psm::Q_TRI_WITHIN, d_tris, n, d_hit, nullptr);
}
int psm_world_sweep_sphere_dev(psm_world* w, const psm_sweep_query* d_sweeps, size_t n, psm_hit* d_hits, int32_t* d_inst) {
    return psm::world_query(w, psm::Q_SWEEP, d_sweeps, n, d_hits, d_inst);
}
int psm_world_sweep_occluded_dev(psm_world* w, const psm_sweep_query* d_sweeps, size_t n, uint8_t* d_hit) {
    return psm::world_query(w, psm::Q_SWEEP_ANY, d_sweeps, n, d_hit, nullptr);
}
int psm_world_mesh_overlaps_dev(psm_world* w, psm_bvh* other, const float* poses, size_t p, int32_t skip, uint8_t* d_hit) {
    return psm::world_mesh_query(w, other, poses, p, skip, 0, 0, d_hit, nullptr, nullptr);
}
int psm_world_mesh_count_dev(psm_world* w, psm_bvh* other, const float* poses, size_t p, int32_t skip, uint32_t* d_count) {
    return psm::world_mesh_query(w, other, poses, p, skip, 1, 0, d_count, nullptr, nullptr);
}
int psm_world_mesh_triangles_dev(psm_world* w, psm_bvh* other, const float* poses, size_t p, int32_t skip, uint32_t k, int32_t* d_tri,
                                 int32_t* d_inst, uint32_t* d_count) {
    return psm::world_mesh_query(w, other, poses, p, skip, 2, k, d_tri, d_inst, d_count);
}
int psm_world_mesh_closest_dev(psm_world* w, psm_bvh* other, const float* poses, size_t p, int32_t skip, float rmax, psm_tri_hit* d_hits,
                               int32_t* d_inst) {
    return psm::world_mesh_dist_query(w, other, poses, p, skip, psm::WMD_CLOSEST, rmax, d_hits, d_inst);
}
int psm_world_mesh_within_dev(psm_world* w, psm_bvh* other, const float* poses, size_t p, int32_t skip, float r, uint8_t* d_flag) {
    return psm::world_mesh_dist_query(w, other, poses, p, skip, psm::WMD_WITHIN, r, d_flag, nullptr);
}
int psm_world_mesh_clearance_dev(psm_world* w, psm_bvh* other, const float* poses, size_t p, int32_t skip, float rmax, psm_mesh_hit* d_hits,
                                 int32_t* d_inst) {
    return psm::world_mesh_dist_query(w, other, poses, p, skip, psm::WMD_CLEAR, rmax, d_hits, d_inst);
}
int psm_grid_world_surface_dev(psm_world* w, const psm_grid* grid, uint64_t* d_bricks) {
    return psm::world_grid_query(w, grid, psm::WGRID_SURFACE, 0, d_bricks);
}
int psm_grid_world_counts_dev(psm_world* w, const psm_grid* grid, uint32_t* d_counts) {
    return psm::world_grid_query(w, grid, psm::WGRID_COUNTS, 0, d_counts);
}
int psm_grid_world_instances_dev(psm_world* w, const psm_grid* grid, int32_t* d_inst) {
    return psm::world_grid_query(w, grid, psm::WGRID_INSTANCES, 0, d_inst);
}
int psm_grid_world_solid_dev(psm_world* w, const psm_grid* grid, uint32_t samples, uint64_t* d_bricks) {
    return psm::world_grid_query(w, grid, psm::WGRID_SOLID, samples, d_bricks);
}
int psm_grid_world_distance_dev(psm_world* w, const psm_grid* grid, float rmax, float* d_dist, int32_t* d_tri, int32_t* d_inst) {
    return psm::world_grid_dist_query(w, grid, rmax, false, 0, d_dist, d_tri, d_inst);
}
int psm_grid_world_signed_distance_dev(psm_world* w, const psm_grid* grid, float rmax, uint32_t samples, float* d_dist, int32_t* d_tri,
                                       int32_t* d_inst) {
    return psm::world_grid_dist_query(w, grid, rmax, true, samples, d_dist, d_tri, d_inst);
}
