// world_mesh_dist.hip -- mesh clearance over an instance world (new; no reference counterpart; include/psm_hip.h "mesh clearance
// over a world"): how close each stored triangle of ANOTHER built hierarchy comes to the (instance, triangle)
// pairs of a world at each of p rigid poses (world_query_mesh_closest), whether any comes within a radius
// (world_query_mesh_within), and the one nearest pair of each pose (world_query_mesh_clearance, then world_query_mesh_pick).
//
// Three proven pieces joined (the bodies are restated: sharing them through a header would move the pinned kernels of
// world_tri_dist.hip and mesh_dist.hip, DESIGN.md 4.10 has the precedent):
//   * begin() is world_mesh.hip's / mesh_dist.hip's: query i is pose q = i / L and the other's leaf j = i % L in slot order
//     (mesh_split), the query triangle is mesh_query_tri of the stored record and the pose, its bounding box by selections
//   * top() / enter() / children() / leaf() are world_tri_dist.hip's WorldTriDistBody: gap2 at the top level, tri_dist_lb2 on
//     the per-instance point_bound inside, both against best (1 + WORLD_PSLACK), the candidate posed forward and judged by
//     tri_dist. The instance left out (skip) is refused in enter(), as world_mesh.hip has it
//   * the shared word of a pose is mesh_dist.hip's MeshDistBody: take / read_word / publish and the FLAGS template. The word
//     carries (dist, t), t the triangle of OTHER -- never the queried side's pair. The pair (instance, triangle) of the world is
//     found by the pick kernel, one lane per pose, which walks posed triangle t* again with Dmin for rmax through the closest
//     body with the same skip: that walk returns the lowest (instance, triangle) at the smallest d2 by itself
// mesh_dist.hip's argument carries over with "pair of the world" where it has "pair of the hierarchy": every published value is
// the dist of a real pair that counts (its instance is not the skipped one: that one is never entered), so D >= Dmin at every
// read; both prunes are closed against best (1 + WORLD_PSLACK) >= best and the acceptance is closed, so a lane whose minimum
// is Dmin never loses it, and the final word is (Dmin, t*) under every schedule.
#include <cstdio>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_dev.h"
#include "psm_world_dev.h"       // world_walk, WorldArgs, WorldMeshDistArgs, load_pose
#include "psm_world_box_dev.h"   // fwd_point, fwd_vec, absmax3, WorldBoxPrune (enter_row)
#include "psm_tri_dist_dev.h"    // tri_dist, tri_dist_lb2; tri_min3 / tri_max3 through psm_tri_dev.h
#include "psm_mesh_dev.h"        // mesh_split, mesh_query_tri
#include "psm_mesh_dist_key.h"   // mesh_key

namespace psm {

namespace {

constexpr uint32_t WMD_FLAG_BOUND = 2u;    // clearance: lanes read the shared word (off: every lane walks with rmax alone)
constexpr uint32_t WMD_FLAG_REREAD = 4u;   // ... before every leaf too, not in begin() alone
constexpr uint32_t WMD_FLAG_EARLY = 8u;    // ... and publish whenever their best improves, not at finish() alone
constexpr uint32_t WMD_SHARED = WMD_FLAG_BOUND | WMD_FLAG_REREAD | WMD_FLAG_EARLY;   // the default

// Waves per SIMD the kernels are bounded for (DESIGN.md 4.26 has the table as compiled): what the bodies take unforced. Nothing
// is spilled.
constexpr int WMD_CLOSEST_WAVES = 3, WMD_WITHIN_WAVES = 2, WMD_CLEAR_WAVES = 2, WMD_PICK_WAVES = 3;

// MODE: WMD_CLOSEST / _WITHIN / _CLEAR / _PICK. FLAGS: the clearance kernel's WMD_FLAG_*, fixed per instance
template <int MODE, uint32_t FLAGS>
struct WorldMeshDistBody : WorldBoxPrune {
    const WorldMeshDistArgs& a;
    const WorldMeshArgs& m;
    const WorldArgs& w;
    PointBound B;          // of the fit matrix of the instance the lane is in
    v3 qa, qb, qc;         // the posed triangle in world space; WorldBoxPrune's lo, hi are its bounding box
    float rmax, best, bu, bv, bs, bt;   // best: the pruning bound -- the best d2 so far, the rmax bound until one is found
    int btri, binst;
    bool found, over;      // over: the lane cannot lower its pose's key any more (within: its pose's flag reads 1)
    uint32_t t, out;       // the other's triangle; where the answer goes: the pose, else (closest) q * T + t
    uint64_t seen;         // clearance: the lowest key this lane has read or published

    PSM_D WorldMeshDistBody(const WorldMeshDistArgs& x) : a(x), m(x.m), w(x.m.w) {}

    // fl(r^2) (1 + 2^-20) + 2^-126: the prune bound of an acceptance radius r (psm_query_dev.h "rmax")
    PSM_D static float bound_of(float r) { return (r * r) * 1.00000095367431640625f + 0x1p-126f; }

    // A key read from the shared word, as MeshDistBody::take has it: its dist is a smaller rmax; a best of this lane's beyond
    // its bound is given up; (0, t') with t' < t ends the lane. "none" reads as a NaN dist, which is below no rmax
    PSM_D void take(uint64_t key) {
        const float D = mesh_key_dist(key);
        rmax = D < rmax ? D : rmax;
        const float nb = bound_of(rmax);
        const bool cut = nb < best;
        best = cut ? nb : best;
        found = found && !cut;
        over = over || ((uint32_t)(key >> 32) == 0u && mesh_key_tri(key) < t);
    }
    PSM_D unsigned long long* word() const { return a.keys + out; }
    PSM_D uint64_t read_word() const { return __hip_atomic_load(word(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    // the lane's own (dist, t), if it is below the last key it read; what was there before is a read like any other
    PSM_D void publish(bool go_on) {
        const uint64_t own = mesh_key(sqrtf(best), t);
        if (!(own < seen)) return;
        const uint64_t old = atomicMin(word(), (unsigned long long)own);
        seen = old < own ? old : own;
        if (go_on) take(seen);
    }

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, p0 = r0, p1 = r0, p2 = r0;
        uint64_t q = 0;
        float R = a.rmax;
        bool has = true;
        t = 0u;
        if (alive) {
            if (MODE == WMD_PICK) {   // (the word is final: the clearance kernel is in stream order before this one)
                q = i;
                const uint64_t key = a.keys[i];
                has = key != MESH_KEY_NONE && mesh_key_tri(key) < m.T;
                if (has) { t = mesh_key_tri(key); R = mesh_key_dist(key); }
            } else {
                uint32_t j;
                mesh_split(i, m.L, m.magic, q, j);
                t = (uint32_t)m.leaf_tri[j];
            }
            r0 = m.tri48[(size_t)3 * t]; r1 = m.tri48[(size_t)3 * t + 1]; r2 = m.tri48[(size_t)3 * t + 2];
            p0 = m.poses[3 * q]; p1 = m.poses[3 * q + 1]; p2 = m.poses[3 * q + 2];
        }
        out = MODE == WMD_CLOSEST ? (uint32_t)q * m.T + t : (uint32_t)q;
        const float pose[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
        mesh_query_tri(pose, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), mk3(r2.x, r2.y, r2.z), qa, qb, qc);
        rmax = R;
        bool valid = alive && has && finite3(qa) && finite3(qb) && finite3(qc) && rmax >= 0.f;   // NaN or negative rmax: a miss
        // the bounding box, exact: selections of the coordinates
        lo = mk3(tri_min3(qa.x, qb.x, qc.x), tri_min3(qa.y, qb.y, qc.y), tri_min3(qa.z, qb.z, qc.z));
        hi = mk3(tri_max3(qa.x, qb.x, qc.x), tri_max3(qa.y, qb.y, qc.y), tri_max3(qa.z, qb.z, qc.z));
        qmax = smaxf(absmax3(lo), absmax3(hi));   // the largest |coordinate| of the nine
        best = bound_of(rmax);
        bu = 0.f; bv = 0.f; bs = 0.f; bt = 0.f;   // per query: the grid-stride loop comes here again
        btri = -1; binst = -1;
        found = false;
        over = false;
        seen = MESH_KEY_NONE;
        // The flag of a pose is the OR over its leaves and a 1 is final: a lane that reads one has nothing to add (world_mesh.hip's
        // skip). The load is atomic (relaxed): made here, at every query, never hoisted.
        if (MODE == WMD_WITHIN && (m.flags & WORLD_MESH_FLAG_SKIP) && valid) valid = __atomic_load_n(w.occluded + out, __ATOMIC_RELAXED) == 0;
        if (MODE == WMD_CLEAR && (FLAGS & WMD_FLAG_BOUND) && valid) {
            seen = read_word();
            take(seen);
            valid = !over;
        }
        return valid;
    }
    // closest, pick: a record at d2 == 0 is held: only a lexicographically lower pair, also at 0, can replace it
    PSM_D bool settled() const { return (MODE == WMD_CLOSEST || MODE == WMD_PICK) && found && best == 0.f; }
    PSM_D bool lower(int in, int tri) const { return (uint32_t)in < (uint32_t)binst || (in == binst && (uint32_t)tri < (uint32_t)btri); }
    // WorldTriDistBody::gap2: the squared gap between the bounding box and a top-level child box grown by the query's slack
    PSM_D float gap2(float lx, float ly, float lz, float hx, float hy, float hz) const {
        const float pad = WORLD_QSLACK * qmax;
        const float tx = smaxf(smaxf((lx - pad) - hi.x, lo.x - (hx + pad)), 0.f);
        const float ty = smaxf(smaxf((ly - pad) - hi.y, lo.y - (hy + pad)), 0.f);
        const float tz = smaxf(smaxf((lz - pad) - hi.z, lo.z - (hz + pad)), 0.f);
        return (tx * tx + ty * ty) + tz * tz;
    }
    // kept iff the gap is not above best (1 + WORLD_PSLACK) (negations: a NaN keeps the box); the order key is the gap
    PSM_D void top(float4 w0, float4 w1, float4 w2, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = gap2(w0.x, w0.y, w0.z, w0.w, w1.x, w1.y);
        kR = gap2(w1.z, w1.w, w2.x, w2.y, w2.z, w2.w);
        const float lim = best + WORLD_PSLACK * best;
        okL = !(kL > lim);
        okR = !(kR > lim);
    }
    // The instance left out is never entered: neither its row nor its lone leaf is read (the lone-leaf shortcut and a world of one
    // come through here). Nor is any instance once the lane is over. Otherwise WorldTriDistBody::enter()
    PSM_D int enter(int in) {
        if (in == m.skip) return -1;
        if ((MODE == WMD_WITHIN || MODE == WMD_CLEAR) && over) return -1;
        if (settled() && (uint32_t)in > (uint32_t)binst) return -1;   // (no pair of it can replace the record)
        const RowLoad r = enter_row(w, in);
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(r.sm[SM_M + k]);
        B = point_bound(M);
        if (r.sm[SM_COUNT] == 1u) leaf(r.sorted_tri[0]);
        const int root = (int)r.sm[SM_ROOT];
        return root >= 0 ? root : -2;   // -2: no tree (0 or 1 leaves)
    }
    // tri_dist.hip's LB^2 on the gaps between a child's fp16 box and the grown intervals; kept iff LB^2 <= best (1 + WORLD_PSLACK)
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = tri_dist_lb2(B, glx, gly, glz, ghx, ghy, ghz, half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        kR = tri_dist_lb2(B, glx, gly, glz, ghx, ghy, ghz, half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        const float lim = best + WORLD_PSLACK * best;
        okL = kL <= lim;
        okR = kR <= lim;
    }
    // The candidate posed forward (the pose re-read: 12 floats are not kept live over the walk), then tri_dist, unchanged.
    // closest, pick: WorldTriDistBody::leaf(). within: the first pair that counts. clearance: MeshDistBody::leaf() -- neither the
    // pair nor the weights are kept: a candidate improves its lane iff it is the first that counts or its d2 is smaller
    PSM_D void leaf(int tri) {
        if (settled() && !lower(inst, tri)) return;
        if (MODE == WMD_CLEAR) {
            if (FLAGS & WMD_FLAG_REREAD) {
                const uint64_t key = read_word();
                seen = key < seen ? key : seen;   // (the word only falls; an older value read late changes nothing in take())
                take(key);
            }
            if (over || (found && best == 0.f)) return;
        }
        // within: the skip again before every leaf -- a lane that began before its pose's flag was set stops at the next one
        if (MODE == WMD_WITHIN && (m.flags & WORLD_MESH_FLAG_SKIP) && __atomic_load_n(w.occluded + out, __ATOMIC_RELAXED) != 0) {
            over = true;
            return;
        }
        float p[12];
        (void)load_pose(w, (uint32_t)inst, p);
        const float4 A = tri48[(size_t)3 * tri + 0], Bv = tri48[(size_t)3 * tri + 1], C = tri48[(size_t)3 * tri + 2];
        const v3 v0 = fwd_point(p, mk3(A.x, A.y, A.z)), e1 = fwd_vec(p, mk3(Bv.x, Bv.y, Bv.z)), e2 = fwd_vec(p, mk3(C.x, C.y, C.z));
        const TriDist d = tri_dist(v0, e1, e2, qa, qb, qc);
        if (MODE == WMD_CLOSEST || MODE == WMD_PICK) {
            if (sqrtf(d.d2) <= rmax && (d.d2 < best || (d.d2 == best && lower(inst, tri)))) {
                found = true;
                best = d.d2; bu = d.u; bv = d.v; bs = d.s; bt = d.t; btri = tri; binst = inst;
            }
        } else if (MODE == WMD_WITHIN) {
            if (sqrtf(d.d2) <= rmax && d.d2 <= best) found = true;
        } else if (sqrtf(d.d2) <= rmax && (!found || d.d2 < best)) {
            found = true;
            best = d.d2;
            if (FLAGS & WMD_FLAG_EARLY) publish(true);
        }
    }
    // within: the lane retires at its first counting candidate, or when its pose's flag reads 1 (over); clearance: at a pair at
    // d2 == 0, or when a lower (0, t') is there
    PSM_D bool done() const { return (MODE == WMD_WITHIN && (found || over)) || (MODE == WMD_CLEAR && (over || (found && best == 0.f))); }
    PSM_D bool again() const { return false; }
    // (the flag: the host path cleared it, and only a 1 is ever stored -- by as many lanes as find one, the same byte value)
    PSM_D void finish(size_t i) {
        if (MODE == WMD_WITHIN) {
            if (found) w.occluded[out] = 1;
        } else if (MODE == WMD_CLEAR) {
            if (found) publish(false);
        } else {   // psm_tri_hit / psm_mesh_hit: two float4 stores, and the instance
            const size_t at = MODE == WMD_CLOSEST ? (size_t)out : i;
            w.hits[2 * at] = found ? make_float4(bu, bv, sqrtf(best), __int_as_float(btri)) : miss_hit();
            w.hits[2 * at + 1] = make_float4(bs, bt, MODE == WMD_PICK ? __int_as_float(found ? (int)t : -1) : 0.f, 0.f);
            w.geom[at] = binst;
        }
    }
};

template <int MODE, uint32_t FLAGS = 0u>
PSM_D void world_mesh_dist_body(const WorldMeshDistArgs& a) {
    WorldMeshDistBody<MODE, FLAGS> q(a);
    world_walk(a.m.w, q);
}

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, WMD_CLOSEST_WAVES) void world_query_mesh_closest(WorldMeshDistArgs a) { world_mesh_dist_body<WMD_CLOSEST>(a); }

__global__ __launch_bounds__(QUERY_BLOCK, WMD_WITHIN_WAVES) void world_query_mesh_within(WorldMeshDistArgs a) { world_mesh_dist_body<WMD_WITHIN>(a); }

// (FLAGS = 0: every lane walks with rmax alone and publishes at finish(); the others: WMD_FLAG_*)
template <uint32_t FLAGS>
__global__ __launch_bounds__(QUERY_BLOCK, WMD_CLEAR_WAVES) void world_query_mesh_clearance(WorldMeshDistArgs a) { world_mesh_dist_body<WMD_CLEAR, FLAGS>(a); }

__global__ __launch_bounds__(QUERY_BLOCK, WMD_PICK_WAVES) void world_query_mesh_pick(WorldMeshDistArgs a) { world_mesh_dist_body<WMD_PICK>(a); }

// The miss record in every cell of an output and -1 for its instance: a byte memset cannot write +inf and -1 side by side, and
// the closest kernel writes the cells of other's leaves only. z: the word after s, t (psm_mesh_hit's `other`: -1; psm_tri_hit: 0)
__global__ __launch_bounds__(256) void world_mesh_dist_fill(float4* hits, int32_t* geom, size_t cells, float z) {
    const float4 miss = make_float4(0.f, 0.f, __builtin_inff(), __int_as_float(-1)), tail = make_float4(0.f, 0.f, z, 0.f);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
        hits[2 * i] = miss;
        hits[2 * i + 1] = tail;
        geom[i] = -1;
    }
}

// world.hip's host path (world_mesh_dist_query(): the stale refusal, the fill, the words' reset, the grid and, shared with the
// other posed-mesh entry points through mesh.hip, the checks and the upload) launches through this (psm_world_dev.h has the modes)
int world_mesh_dist_launch(psm_ctx* c, int mode, char bound, bool pick, uint32_t grid, WorldMeshDistArgs a) {
    a.m.magic = mesh_magic(a.m.L);
    if (mode == WMD_FILL) {
        const size_t cells = a.m.w.n, blocks = (cells + 255) / 256;
        world_mesh_dist_fill<<<(uint32_t)(blocks < 4096 ? blocks : 4096), 256, 0, c->stream>>>(a.m.w.hits, a.m.w.geom, cells, pick ? __builtin_bit_cast(float, -1) : 0.f);
    } else if (mode == WMD_CLOSEST) world_query_mesh_closest<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (mode == WMD_WITHIN) world_query_mesh_within<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (mode == WMD_PICK) world_query_mesh_pick<<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (bound == '0') world_query_mesh_clearance<0u><<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (bound == '2') world_query_mesh_clearance<WMD_FLAG_BOUND><<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else if (bound == '3') world_query_mesh_clearance<WMD_FLAG_BOUND | WMD_FLAG_REREAD><<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    else world_query_mesh_clearance<WMD_SHARED><<<grid, QUERY_BLOCK, 0, c->stream>>>(a);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace psm
