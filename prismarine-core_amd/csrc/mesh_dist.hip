// mesh_dist.hip -- mesh clearance against a built hierarchy (new; no reference counterpart; include/psm_hip.h "mesh clearance",
// DESIGN.md 4.24): how close each stored triangle of ANOTHER built hierarchy comes to the hierarchy's triangles at each of p
// rigid poses (bvh_query_mesh_closest), whether any comes within a radius (bvh_query_mesh_within), and the one nearest pair of
// each pose (bvh_query_mesh_clearance, then bvh_query_mesh_pick) -- the clearance queries (tri_dist.hip) with the query
// triangles taken from the other hierarchy's stored leaves, as the mesh queries (mesh.hip) take them.
//
// The walk is query.hip's (query_walk, psm_query_dev.h) over n = p x L queries in slot order, exactly mesh.hip's: query i is pose
// q = i / L and the other's leaf j = i % L, its leaves by ascending load-order id. begin() makes the posed triangle as MeshBody
// does (mesh_query_tri); the candidate test, the bound and the child order are TriDistBody's, restated here: sharing the body
// through a header moved tri_dist.hip's two kernels (DESIGN.md 4.10 has the precedent), and they are pinned.
//
// The clearance kernel is the first in the project whose lanes share a bound that is decided inside the launch. Per pose there
// is one 64-bit word in device memory, key = (bits(dist) << 32) | t (psm_mesh_dist_key.h): unsigned order is (dist, t) order and
// all-ones, which the host sets in stream order, is "none". The protocol:
//   * reading: a lane reads its pose's key with a relaxed, agent-scope atomic load in begin() and, by default, before every
//     leaf. The address is the lane's own (a vector load, never hoisted). The dist part D acts as a smaller rmax: the prune bound
//     becomes fl(D^2) (1 + 2^-20) + 2^-126 and acceptance sqrtf(d2) <= D -- the arithmetic triClosest has for rmax, so the
//     argument of psm_query_dev.h for that bound holds word for word with D in rmax's place
//   * publishing: a lane publishes (dist, t) of its own best with atomicMin on the word, at finish() and, by default, whenever
//     its best improves -- only if its key is below the last key it read. What atomicMin returns is a fresh read
//   * nobody waits: no spin, no fence, no hand-off. The word carries nothing but itself; a stale read only means more work
//   * why the answer is fixed: every published value is the dist of a real pair of that pose that counts, so D >= Dmin, the
//     pose's smallest dist, at every read. A lane whose own minimum is Dmin therefore never loses it: the prune is closed (a box
//     is dropped only when every point of it is farther than D) and the acceptance is closed (dist <= D). A lane that discards
//     a best of its own does so only when that best's d2 exceeds the bound of a D it read, i.e. its dist > D >= Dmin. So every
//     lane whose minimum is Dmin publishes (Dmin, t) unless a lower key is already there, no key below (Dmin, t*) is ever
//     published, and the final word is (Dmin, t*), t* the lowest such t -- whatever the order, the timing or either tree
//   * early exit: a key (0, t') with t' < t cannot be beaten by lane t, which retires: TriDistBody's d2 == 0 shortcut across
//     lanes. A lane that holds a pair at d2 == 0 itself retires too: only dist and t leave this kernel
//   * the weights never travel through the word: a second, tiny launch of p lanes (bvh_query_mesh_pick) reads t* from each word
//     and walks that one posed triangle as the closest kernel would, with Dmin for rmax (the same record: the winner of the
//     walk with rmax counts under Dmin too), and writes the psm_mesh_hit. A word that still reads "none" gives the miss record
#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_host.h"     // batch_args, depth_bound, mesh.hip's shared host pieces; psm_query_dev.h through it
#include "psm_mesh_dev.h"       // mesh_split, mesh_query_tri
#include "psm_tri_dist_dev.h"   // tri_dist; box_row through psm_tri_dev.h
#include "psm_mesh_dist_key.h"  // mesh_key

namespace psm {

// QueryArgs keeps its layout; what a mesh clearance query adds travels beside it. q: the queried hierarchy's records, spill,
// outputs (closest: psm_tri_hit [p][T]; within: the flag per pose; pick: psm_mesh_hit [p]), n = p x L (pick: p)
struct MeshDistArgs {
    QueryArgs q;
    const float4* tri48;        // the other hierarchy's v0, e1, e2 per triangle
    const int32_t* leaf_tri;    // ... and its leaves in slot order: leaf j is triangle leaf_tri[j], ascending
    const float4* poses;        // [p] x three float4: the rows of [R | T]
    unsigned long long* keys;   // [p]: the poses' shared words (clearance, pick)
    uint64_t magic;             // mesh_magic(L)
    uint32_t L, T;              // the other's leaf count and loaded triangle count
    uint32_t flags;             // MD_FLAG_SKIP
    float rmax;                 // one per call
};

namespace {

enum { MD_CLOSEST = 0, MD_WITHIN = 1, MD_CLEAR = 2, MD_PICK = 3 };
constexpr uint32_t MD_FLAG_SKIP = 1u;     // within: a lane whose pose's flag already reads 1 does not walk
constexpr uint32_t MD_FLAG_BOUND = 2u;    // clearance: lanes read the shared word (off: every lane walks with rmax alone)
constexpr uint32_t MD_FLAG_REREAD = 4u;   // ... before every leaf too, not in begin() alone
constexpr uint32_t MD_FLAG_EARLY = 8u;    // ... and publish whenever their best improves, not at finish() alone
constexpr uint32_t MD_SHARED = MD_FLAG_BOUND | MD_FLAG_REREAD | MD_FLAG_EARLY;   // the default

// Waves per SIMD the kernels are bounded for (DESIGN.md 4.24 has the table): what the bodies take unforced. The closest and the
// pick kernel carry the winner's weights as tri_dist.hip's closest kernel does; the within and the clearance kernel carry none
// and have the fifteen features scheduled side by side, as its within kernel. Nothing is spilled.
constexpr int MD_CLOSEST_WAVES = 4, MD_WITHIN_WAVES = 3, MD_CLEAR_WAVES = 3, MD_PICK_WAVES = 4;

// FLAGS: the clearance kernel's MD_FLAG_BOUND / _REREAD / _EARLY, fixed per instance (held in the launch's arguments they cost the
// kernel two SGPR spills)
template <int MODE, uint32_t FLAGS>
struct MeshDistBody {
    const MeshDistArgs& m;
    const QueryArgs& a;
    const PointBound B;
    v3 qa, qb, qc;
    float glx, gly, glz, ghx, ghy, ghz;   // the grown image interval of the query's bounding box per normalised axis
    float rmax, best, bu, bv, bs, bt;     // best: the pruning bound -- the best d2 so far, the rmax bound until one is found
    int btri;
    bool found, over;                     // over: the lane cannot lower its pose's key any more (within: its pose's flag reads 1)
    uint32_t t, out;                      // the other's triangle; where the answer goes: the pose, else (closest) q * T + t
    uint64_t seen;                        // clearance: the lowest key this lane has read or published

    // fl(r^2) (1 + 2^-20) + 2^-126: the prune bound of an acceptance radius r (psm_query_dev.h "rmax")
    PSM_D static float bound_of(float r) { return (r * r) * 1.00000095367431640625f + 0x1p-126f; }

    // A key read from the shared word: its dist is a smaller rmax; a best of this lane's beyond its bound is given up (its dist
    // is above the key's: it cannot be the pose's); (0, t') with t' < t ends the lane.
    // Without a branch: "none" reads as a NaN dist, which is below no rmax, and its high half is not 0; best never exceeds
    // bound_of(rmax) (it is that bound, or the d2 of a pair within rmax), so the bound of an unchanged rmax cuts nothing.
    PSM_D void take(uint64_t key) {
        const float D = mesh_key_dist(key);
        rmax = D < rmax ? D : rmax;
        const float nb = bound_of(rmax);
        const bool cut = nb < best;
        best = cut ? nb : best;
        found = found && !cut;
        over = over || ((uint32_t)(key >> 32) == 0u && mesh_key_tri(key) < t);
    }
    PSM_D unsigned long long* word() const { return m.keys + out; }
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
        float R = m.rmax;
        bool has = true;
        t = 0u;
        if (alive) {
            if (MODE == MD_PICK) {   // (the word is final: the clearance kernel is in stream order before this one)
                q = i;
                const uint64_t key = m.keys[i];
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
        out = MODE == MD_CLOSEST ? (uint32_t)q * m.T + t : (uint32_t)q;
        const float pose[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
        mesh_query_tri(pose, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), mk3(r2.x, r2.y, r2.z), qa, qb, qc);
        rmax = R;
        bool valid = alive && has && finite3(qa) && finite3(qb) && finite3(qc) && rmax >= 0.f;   // NaN or negative rmax: a miss
        best = bound_of(rmax);
        bu = 0.f; bv = 0.f; bs = 0.f; bt = 0.f;   // per query: the grid-stride loop comes here again
        btri = -1;
        found = false;
        over = false;
        seen = MESH_KEY_NONE;
        // the bounding box, exact: selections of the coordinates
        const v3 lo = mk3(tri_min3(qa.x, qb.x, qc.x), tri_min3(qa.y, qb.y, qc.y), tri_min3(qa.z, qb.z, qc.z));
        const v3 hi = mk3(tri_max3(qa.x, qb.x, qc.x), tri_max3(qa.y, qb.y, qc.y), tri_max3(qa.z, qb.z, qc.z));
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        box_row(M, 0, lo, hi, glx, ghx);
        box_row(M, 1, lo, hi, gly, ghy);
        box_row(M, 2, lo, hi, glz, ghz);
        // The flag of a pose is the OR over its leaves and a 1 is final: a lane that reads one has nothing to add (mesh.hip's
        // skip). The load is atomic (relaxed): made here, at every query, never hoisted.
        if (MODE == MD_WITHIN && (m.flags & MD_FLAG_SKIP) && valid) valid = __atomic_load_n(a.occluded + out, __ATOMIC_RELAXED) == 0;
        if (MODE == MD_CLEAR && (FLAGS & MD_FLAG_BOUND) && valid) {
            seen = read_word();
            take(seen);
            valid = !over;
        }
        return valid;
    }
    // LB^2 of one child box (mn / mx: its fp16 corners): PointImage::lb2 with the gap to an interval (a NaN gap is 0: kept)
    PSM_D float lb2(float mnx, float mny, float mnz, float mxx, float mxy, float mxz) const {
        const float tx = smaxf(smaxf(mnx - ghx, glx - mxx), 0.f) * B.il0;
        const float ty = smaxf(smaxf(mny - ghy, gly - mxy), 0.f) * B.il1;
        const float tz = smaxf(smaxf(mnz - ghz, glz - mxz), 0.f) * B.il2;
        const float mm = smaxf(smaxf(tx, ty), tz);
        return (B.orth ? ((tx * tx + ty * ty) + tz * tz) : mm * mm) * B.wf;
    }
    // kept iff LB^2 <= best (<=: a triangle as near as the best and of a lower id still counts); the order key is LB^2
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        kL = lb2(half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        kR = lb2(half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        okL = kL <= best;
        okR = kR <= best;
    }
    // A candidate, as TriDistBody has it: within rmax, and (closest, pick) nearer than the best so far or as near and of a lower
    // id, with its shortcut at d2 == 0. The clearance kernel keeps no id of bvh and no weights: a candidate improves its lane
    // iff it is the first that counts or its d2 is smaller (before the first, best is the rmax bound, >= every d2 that counts).
    PSM_D void leaf(int tri) {
        const bool record = MODE == MD_CLOSEST || MODE == MD_PICK;
        if (record && found && best == 0.f && (uint32_t)tri > (uint32_t)btri) return;
        if (MODE == MD_CLEAR) {
            if (FLAGS & MD_FLAG_REREAD) {
                const uint64_t key = read_word();
                seen = key < seen ? key : seen;   // (the word only falls; an older value read late changes nothing in take())
                take(key);
            }
            if (over || (found && best == 0.f)) return;
        }
        // within: the skip again before every leaf -- a lane that began before its pose's flag was set stops at the next one
        if (MODE == MD_WITHIN && (m.flags & MD_FLAG_SKIP) && __atomic_load_n(a.occluded + out, __ATOMIC_RELAXED) != 0) {
            over = true;
            return;
        }
        const float4 A = a.tri48[(size_t)3 * tri + 0], Bv = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        const TriDist w = tri_dist(mk3(A.x, A.y, A.z), mk3(Bv.x, Bv.y, Bv.z), mk3(C.x, C.y, C.z), qa, qb, qc);
        if (record) {
            if (sqrtf(w.d2) <= rmax && (w.d2 < best || (w.d2 == best && (uint32_t)tri < (uint32_t)btri))) {
                found = true;
                best = w.d2; bu = w.u; bv = w.v; bs = w.s; bt = w.t; btri = tri;
            }
        } else if (MODE == MD_WITHIN) {
            if (sqrtf(w.d2) <= rmax && w.d2 <= best) found = true;
        } else if (sqrtf(w.d2) <= rmax && (!found || w.d2 < best)) {
            found = true;
            best = w.d2;
            if (FLAGS & MD_FLAG_EARLY) publish(true);
        }
    }
    // within: the lane retires at its first counting candidate, or when its pose's flag reads 1 (over); clearance: at a pair at d2 == 0, or when a lower (0, t') is there
    PSM_D bool done() const { return (MODE == MD_WITHIN && (found || over)) || (MODE == MD_CLEAR && (over || (found && best == 0.f))); }
    PSM_D bool again() const { return false; }
    // (the flag: the host path cleared it, and only a 1 is ever stored -- by as many lanes as find one, the same byte value)
    PSM_D void finish(size_t i) {
        if (MODE == MD_WITHIN) {
            if (found) a.occluded[out] = 1;
        } else if (MODE == MD_CLEAR) {
            if (found) publish(false);
        } else {   // psm_tri_hit / psm_mesh_hit: two float4 stores
            const size_t at = MODE == MD_CLOSEST ? (size_t)out : i;
            a.hits[2 * at] = found ? make_float4(bu, bv, sqrtf(best), __int_as_float(btri)) : miss_hit();
            a.hits[2 * at + 1] = make_float4(bs, bt, MODE == MD_PICK ? __int_as_float(found ? (int)t : -1) : 0.f, 0.f);
        }
    }
};

template <int MODE, uint32_t FLAGS = 0u>
PSM_D void mesh_dist_body(const MeshDistArgs& m) {
    float M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = u2f(m.q.sm[SM_M + k]);
    MeshDistBody<MODE, FLAGS> q{m, m.q, point_bound(M)};
    query_walk(m.q, q);
}

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, MD_CLOSEST_WAVES) void bvh_query_mesh_closest(MeshDistArgs m) { mesh_dist_body<MD_CLOSEST>(m); }

__global__ __launch_bounds__(QUERY_BLOCK, MD_WITHIN_WAVES) void bvh_query_mesh_within(MeshDistArgs m) { mesh_dist_body<MD_WITHIN>(m); }

// (FLAGS = 0: every lane walks with rmax alone and publishes at finish(); the others: MD_FLAG_*)
template <uint32_t FLAGS>
__global__ __launch_bounds__(QUERY_BLOCK, MD_CLEAR_WAVES) void bvh_query_mesh_clearance(MeshDistArgs m) { mesh_dist_body<MD_CLEAR, FLAGS>(m); }

__global__ __launch_bounds__(QUERY_BLOCK, MD_PICK_WAVES) void bvh_query_mesh_pick(MeshDistArgs m) { mesh_dist_body<MD_PICK>(m); }

// The miss record in every cell of a closest call's output: a byte memset cannot write +inf and -1 side by side, and the query
// kernel writes the cells of other's leaves only. Launched only where other's build dropped a triangle (L < T).
__global__ __launch_bounds__(256) void mesh_dist_fill(float4* hits, size_t cells) {
    const float4 miss = make_float4(0.f, 0.f, __builtin_inff(), __int_as_float(-1)), zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
        hits[2 * i] = miss;
        hits[2 * i + 1] = zero;
    }
}

namespace {

const char* const MESH_DIST_NAME[] = {"psm_bvh_mesh_closest_dev", "psm_bvh_mesh_within_dev", "psm_bvh_mesh_clearance_dev"};

// A mesh clearance query, of mesh.hip's shared pieces (psm_query_host.h) in mesh_query()'s order: NULL handles and p == 0 are
// answered before anything else is looked at; then the data, the state, the depth, the contexts, the poses, the number of
// answers, all on the host, before any launch, the outputs untouched. Then the upload: one copy, one synchronisation, no graph
// capture.
int mesh_dist_query(psm_bvh* b, psm_bvh* o, const float* poses, size_t p, int mode, float rmax, void* d_out) {
    if (!b || !o) return PSM_ERR_INVALID;
    if (p == 0) return PSM_OK;
    psm_ctx* c = b->ctx;
    const char* name = MESH_DIST_NAME[mode];
    int rc = mesh_pointers(c, name, poses && d_out);
    if (rc == PSM_OK && mode != MD_WITHIN) rc = mesh_aligned(c, name, "hits", d_out, 16);
    if (rc != PSM_OK) return rc;
    if (!b->built || !o->built) return set_err(c, PSM_ERR_STATE, "mesh query before build");
    if (depth_bound(b) > QSTACK_MAX) return set_err(c, PSM_ERR_CAPACITY, "mesh query: hierarchy deeper than the query stack");
    if (o->ctx != c) return mesh_refuse(c, PSM_ERR_INVALID, "%s: the two hierarchies are of different contexts", name);
    const uint32_t T = o->tri_count;
    rc = mesh_poses_rigid(c, name, poses, p);
    if (rc == PSM_OK) rc = mesh_answers_fit(c, name, p, T);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    void *d_poses = nullptr, *d_keys = nullptr;
    uint32_t L = 0;
    rc = mesh_upload(c, o, poses, p, &d_poses, mode == MD_CLEAR ? &d_keys : nullptr, &L);
    if (rc != PSM_OK) return rc;
    // (the context's stack area is allocated here, on its first query: the last thing that can fail before the outputs change)
    MeshDistArgs m = {};
    uint32_t grid = 0;
    rc = batch_args(c, nullptr, p * (size_t)L, d_out, 0, m.q, grid);
    if (rc != PSM_OK) return rc;
    m.q.node32 = b->d_node32; m.q.tri48 = b->d_tri48; m.q.sm = b->d_small; m.q.sorted_tri = b->d_sorted_tri;
    m.tri48 = o->d_tri48; m.leaf_tri = o->d_leaftri; m.poses = (const float4*)d_poses; m.keys = (unsigned long long*)d_keys;
    m.magic = mesh_magic(L); m.L = L; m.T = T; m.rmax = rmax;
    if (mode == MD_CLOSEST) {
        const size_t cells = p * (size_t)T;
        if (L < T) {   // a dropped triangle's cells read the miss record
            const size_t blocks = (cells + 255) / 256;
            mesh_dist_fill<<<(uint32_t)(blocks < 4096 ? blocks : 4096), 256, 0, c->stream>>>((float4*)d_out, cells);
            PSM_HIP(c, hipGetLastError());
        }
        if (L == 0) return PSM_OK;
        bvh_query_mesh_closest<<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
    } else if (mode == MD_WITHIN) {
        PSM_HIP(c, hipMemsetAsync(d_out, 0, p, c->stream));
        if (L == 0) return PSM_OK;
        m.flags = mesh_skip(p * (size_t)L) ? MD_FLAG_SKIP : 0u;   // (the flag read in begin() and before every leaf)
        bvh_query_mesh_within<<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
    } else {
        PSM_HIP(c, hipMemsetAsync(d_keys, 0xff, p * sizeof(uint64_t), c->stream));   // every word: "none"
        if (L != 0) {
            const char how = mesh_bound();   // (the study knob: the same answer under each letter)
            if (how == '0') bvh_query_mesh_clearance<0u><<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
            else if (how == '2') bvh_query_mesh_clearance<MD_FLAG_BOUND><<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
            else if (how == '3') bvh_query_mesh_clearance<MD_FLAG_BOUND | MD_FLAG_REREAD><<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
            else bvh_query_mesh_clearance<MD_SHARED><<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
            PSM_HIP(c, hipGetLastError());
        }
        // the second launch: one lane per pose walks the winner again and writes the record (a word left at "none": the miss)
        MeshDistArgs pick = m;
        pick.flags = 0u;
        rc = batch_args(c, nullptr, p, d_out, 0, pick.q, grid);
        if (rc != PSM_OK) return rc;
        bvh_query_mesh_pick<<<grid, QUERY_BLOCK, 0, c->stream>>>(pick);
    }
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace

}  // namespace psm

int psm_bvh_mesh_closest_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, float rmax, psm_tri_hit* d_hits) {
    return psm::mesh_dist_query(bvh, other, poses, p, psm::MD_CLOSEST, rmax, d_hits);
}

int psm_bvh_mesh_within_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, float r, uint8_t* d_flag) {
    return psm::mesh_dist_query(bvh, other, poses, p, psm::MD_WITHIN, r, d_flag);
}

int psm_bvh_mesh_clearance_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, float rmax, psm_mesh_hit* d_hits) {
    return psm::mesh_dist_query(bvh, other, poses, p, psm::MD_CLEAR, rmax, d_hits);
}
