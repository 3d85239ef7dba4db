// mesh.hip -- mesh queries against a built hierarchy (new; no reference counterpart; include/psm_hip.h "mesh queries",
// DESIGN.md 4.21): whether, how many and which of the hierarchy's triangles meet each triangle of ANOTHER built hierarchy at each
// of p rigid poses -- the triangle queries (tri.hip) with the query triangles taken from the other hierarchy's stored leaves.
//
// The walk is query.hip's (query_walk, psm_query_dev.h) over n = p x L queries, L the other hierarchy's leaf count: query i is
// pose q = i / L and the other's leaf j = i % L in SLOT order (its leaves by ascending load-order id, the build's leaf_tri), so
// a launch walks exactly the queries, in exactly the order, that the triangle queries walk for the same posed triangles packed
// in load order. (The other's Morton order was measured and is slower for this walk: DESIGN.md 4.21.) The query triangle is
// made in begin() from the other's stored record and the pose (mesh_query_tri, psm_mesh_dev.h); no psm_tri_query record exists
// anywhere. From there the body is tri.hip's TriBody restated: tri_tri, the box family's prune on the query triangle's bounding
// box, the list of the k lowest ids. Results go to [q][t], t the leaf's load-order triangle id; the host path clears the
// outputs first, so a triangle the other's build dropped reads 0 / -1.
//
// This file also holds the host pieces all twelve posed-mesh entry points share (psm_query_host.h): the
// refusals they have in common, the contexts' pose and key areas with the one upload, and the two study knobs.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#include "psm_common.h"
#include "psm_internal.h"
#include "psm_query_host.h"   // batch_args, depth_bound, pose_fault; psm_query_dev.h through it
#include "psm_mesh_dev.h"     // mesh_split, mesh_query_tri; tri_tri, box_row, fwd_point / fwd_vec through it

#define PSM_BOX_LIST_FN PSM_D
#include "psm_box_list.h"

namespace psm {

// QueryArgs keeps its layout; what a mesh query adds travels beside it. q: the queried hierarchy's records, spill, outputs
// (occluded: the flag per pose; count: [p][T]; hits: the int32 [p][T][k] rows), samples = k, n = p x L.
struct MeshArgs {
    QueryArgs q;
    const float4* tri48;        // the other hierarchy's v0, e1, e2 per triangle
    const int32_t* leaf_tri;    // ... and its leaves in slot order: leaf j is triangle leaf_tri[j], ascending
    const float4* poses;        // [p] x three float4: the rows of [R | T]
    uint64_t magic;             // mesh_magic(L)
    uint32_t L, T;              // the other's leaf count and loaded triangle count
    uint32_t flags;             // MESH_FLAG_*
};

namespace {

enum { MESH_ANY = 0, MESH_COUNT = 1, MESH_TRIS = 2 };
constexpr uint32_t MESH_FLAG_SKIP = 1u;   // the flag kernel: a lane whose pose's flag already reads 1 does not walk

// a lane's column of the wave's id list: slot s of this lane is col[s * QUERY_BLOCK]
PSM_D uint32_t* mesh_id_column() {
    extern __shared__ uint32_t mesh_ids[];
    return mesh_ids + threadIdx.x;
}

// Waves per SIMD the kernels are bounded for (DESIGN.md 4.21 has the table): tri.hip's, whose body this is. The flag and the
// count kernel fit 7 waves' 72 registers (72 and 71), the list kernel takes 79 (80 allocated: 6 waves); nothing is spilled.
// The output index is 32 bits wide for that: with 64 the count kernel takes 74 and spills when held to 72.
constexpr int MESH_ANY_WAVES = 7, MESH_COUNT_WAVES = 7, MESH_LIST_WAVES = 6;

// MODE: what is kept of the candidates that count -- a flag per pose (the walk ends at the first), their number, the k lowest ids
template <int MODE>
struct MeshBody {
    const MeshArgs& m;
    const QueryArgs& a;
    BoxIdList<QUERY_BLOCK> L;
    v3 qa, qb, qc;
    float glx, gly, glz, ghx, ghy, ghz;   // the grown image interval of the query's bounding box per normalised axis
    uint32_t cnt;
    uint32_t out;                         // where the answer goes: the pose (flag), else q * T + t (below 2^32: the host checks)

    PSM_D bool begin(size_t i, bool alive) {
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, p0 = r0, p1 = r0, p2 = r0;
        uint64_t q = 0;
        uint32_t t = 0u;
        if (alive) {
            uint32_t j;
            mesh_split(i, m.L, m.magic, q, j);
            t = (uint32_t)m.leaf_tri[j];
            r0 = m.tri48[(size_t)3 * t]; r1 = m.tri48[(size_t)3 * t + 1]; r2 = m.tri48[(size_t)3 * t + 2];
            p0 = m.poses[3 * q]; p1 = m.poses[3 * q + 1]; p2 = m.poses[3 * q + 2];
        }
        out = MODE == MESH_ANY ? (uint32_t)q : (uint32_t)q * m.T + t;
        const float pose[12] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x, p2.y, p2.z, p2.w};
        mesh_query_tri(pose, mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), mk3(r2.x, r2.y, r2.z), qa, qb, qc);
        bool valid = alive && finite3(qa) && finite3(qb) && finite3(qc);
        cnt = 0u;
        L.clear();   // per query: the grid-stride loop comes here again
        // the bounding box, exact: selections of the coordinates
        const v3 lo = mk3(tri_min3(qa.x, qb.x, qc.x), tri_min3(qa.y, qb.y, qc.y), tri_min3(qa.z, qb.z, qc.z));
        const v3 hi = mk3(tri_max3(qa.x, qb.x, qc.x), tri_max3(qa.y, qb.y, qc.y), tri_max3(qa.z, qb.z, qc.z));
        float M[16];
#pragma unroll
        for (int k = 0; k < 16; k++) M[k] = u2f(a.sm[SM_M + k]);
        box_row(M, 0, lo, hi, glx, ghx);
        box_row(M, 1, lo, hi, gly, ghy);
        box_row(M, 2, lo, hi, glz, ghz);
        // The flag of a pose is the OR over its leaves and a 1 is final: a lane that reads one has nothing to add. The load is
        // atomic (relaxed): made here, at every query, never hoisted; whether it sees another wave's store changes the work only.
        if (MODE == MESH_ANY && (m.flags & MESH_FLAG_SKIP) && valid) valid = __atomic_load_n(a.occluded + out, __ATOMIC_RELAXED) == 0;
        return valid;
    }
    // a child box [mn, mx] is kept iff it meets the grown interval on all three axes (negations: a NaN keeps the box)
    PSM_D bool keep(float mnx, float mny, float mnz, float mxx, float mxy, float mxz) const {
        bool o = mxx < glx;
        o |= mnx > ghx;
        o |= mxy < gly;
        o |= mny > ghy;
        o |= mxz < glz;
        o |= mnz > ghz;
        return !o;
    }
    // (the record's fp16 corners in the order the slab and the point tests read them: mn.xyz, mx.xyz)
    PSM_D void children(uint4 n0, uint4 n1, bool& okL, bool& okR, float& kL, float& kR) const {
        okL = keep(half_lo(n0.x), half_hi(n0.x), half_lo(n0.y), half_hi(n0.y), half_lo(n0.z), half_hi(n0.z));
        okR = keep(half_lo(n0.w), half_hi(n0.w), half_lo(n1.x), half_hi(n1.x), half_lo(n1.y), half_hi(n1.y));
        kL = 0.f;
        kR = 0.f;
    }
    PSM_D void leaf(int tri) {
        const float4 A = a.tri48[(size_t)3 * tri + 0], B = a.tri48[(size_t)3 * tri + 1], C = a.tri48[(size_t)3 * tri + 2];
        if (!tri_tri(mk3(A.x, A.y, A.z), mk3(B.x, B.y, B.z), mk3(C.x, C.y, C.z), qa, qb, qc)) return;
        if (MODE == MESH_TRIS) L.offer((uint32_t)tri);
        else cnt++;
    }
    PSM_D bool done() const { return MODE == MESH_ANY && cnt != 0u; }
    PSM_D bool again() const { return false; }
    // (the flag: the host path cleared it, and only a 1 is ever stored -- by as many lanes as find one, the same byte value)
    PSM_D void finish(size_t) const {
        if (MODE == MESH_ANY) {
            if (cnt != 0u) a.occluded[out] = 1;
        }
        if (MODE == MESH_COUNT) a.count[out] = cnt;
        if (MODE == MESH_TRIS) {
            int32_t* __restrict__ row = (int32_t*)a.hits + (size_t)out * L.k;
            for (uint32_t s = 0; s < L.k; s++) row[s] = s < L.cnt ? (int32_t)L.id[(size_t)s * QUERY_BLOCK] : -1;
            a.count[out] = L.cnt;
        }
    }
};

}  // namespace

__global__ __launch_bounds__(QUERY_BLOCK, MESH_ANY_WAVES) void bvh_query_mesh_any(MeshArgs m) {
    MeshBody<MESH_ANY> q{m, m.q, BoxIdList<QUERY_BLOCK>(nullptr, 0u)};
    query_walk(m.q, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, MESH_COUNT_WAVES) void bvh_query_mesh_count(MeshArgs m) {
    MeshBody<MESH_COUNT> q{m, m.q, BoxIdList<QUERY_BLOCK>(nullptr, 0u)};
    query_walk(m.q, q);
}

__global__ __launch_bounds__(QUERY_BLOCK, MESH_LIST_WAVES) void bvh_query_mesh_tris(MeshArgs m) {
    MeshBody<MESH_TRIS> q{m, m.q, BoxIdList<QUERY_BLOCK>(mesh_id_column(), m.q.samples)};
    query_walk(m.q, q);
}

namespace {

// the device copy of a call's poses, per context (grown on demand; every call runs on the context's stream, never two at once),
// and beside it the words the poses of a mesh clearance call share (mesh_dist.hip)
struct PoseArea {
    void* ptr = nullptr;
    size_t bytes = 0;
};
struct PoseAreas {
    PoseArea poses, keys;
};
std::mutex pose_mu;
std::unordered_map<const psm_ctx*, PoseAreas> pose_area;

int area_for(psm_ctx* c, PoseArea& a, size_t bytes, void** out) {
    if (a.bytes < bytes) {
        // (the stream is idle wherever this is reached after a call: every call ends its upload with a synchronisation, and a
        // kernel that read the old area is in stream order before the free)
        if (a.ptr) PSM_HIP(c, hipStreamSynchronize(c->stream));
        if (a.ptr) PSM_HIP(c, hipFree(a.ptr));
        a = PoseArea();
        size_t want = 4096;
        while (want < bytes) want *= 2;
        PSM_HIP(c, hipMalloc(&a.ptr, want));
        a.bytes = want;
    }
    *out = a.ptr;
    return PSM_OK;
}

}  // namespace

// ---- The host pieces every posed-mesh entry point shares (psm_query_host.h): mesh_query() below, mesh_dist.hip's
// mesh_dist_query(), world.hip's world_mesh_query() and world_mesh_dist_query() are sequences of these and of what is their own.
// Each check answers PSM_OK or refuses under the entry point's name, on the host, nothing launched and no output byte changed.

int mesh_refuse(psm_ctx* c, int code, const char* format, ...) {
    char msg[192];
    va_list args;
    va_start(args, format);
    vsnprintf(msg, sizeof msg, format, args);
    va_end(args);
    return set_err(c, code, msg);
}

int mesh_pointers(psm_ctx* c, const char* name, bool all) {
    return all ? PSM_OK : mesh_refuse(c, PSM_ERR_INVALID, "%s: NULL pointer", name);
}

int mesh_aligned(psm_ctx* c, const char* name, const char* what, const void* ptr, unsigned align) {
    return ((uintptr_t)ptr & (align - 1u)) == 0 ? PSM_OK : mesh_refuse(c, PSM_ERR_INVALID, "%s: %s not %u-byte aligned", name, what, align);
}

int mesh_poses_rigid(psm_ctx* c, const char* name, const float* poses, size_t p) {
    for (size_t q = 0; q < p; q++)
        if (const char* why = pose_fault(poses + 12 * q)) return mesh_refuse(c, PSM_ERR_INVALID, "%s: pose %zu %s", name, q, why);
    return PSM_OK;
}

int mesh_answers_fit(psm_ctx* c, const char* name, size_t p, uint32_t T) {
    if ((uint64_t)p * T < MESH_QUERIES_MAX) return PSM_OK;
    return mesh_refuse(c, PSM_ERR_CAPACITY, "%s: %zu poses of %u triangles are more than 2^32 answers", name, p, T);
}

// The upload: the poses go to the device as a world's do (psm_world_set_transforms: a copy on the context's stream and a
// synchronisation, the caller's memory being pageable and the caller's to change), with the other hierarchy's leaf count coming
// back in the same wait -- the one synchronisation of a call.
int mesh_upload(psm_ctx* c, const psm_bvh* o, const float* poses, size_t p, void** d_poses, void** d_keys, uint32_t* L) {
    {
        std::lock_guard<std::mutex> lk(pose_mu);
        PoseAreas& a = pose_area[c];
        int rc = area_for(c, a.poses, p * 12 * sizeof(float), d_poses);
        if (rc == PSM_OK && d_keys) rc = area_for(c, a.keys, p * sizeof(uint64_t), d_keys);
        if (rc != PSM_OK) return rc;
    }
    *L = 0;
    PSM_HIP(c, hipMemcpyAsync(*d_poses, poses, p * 12 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    PSM_HIP(c, hipMemcpyAsync(L, o->d_small + SM_COUNT, sizeof *L, hipMemcpyDeviceToHost, c->stream));
    PSM_HIP(c, hipStreamSynchronize(c->stream));
    if (*L > o->tri_count) return set_err(c, PSM_ERR_STATE, "mesh query: the other hierarchy's leaf count exceeds its triangle count");
    return PSM_OK;
}

// The flag kernels' skip pays where workgroups start after others have finished: a launch that takes the grid-stride loop. The
// overlaps kernels read the flag in begin() (measured: 7 to 22 % faster at 1 024 poses; without a second trip every wave starts
// at once, nothing is skipped and the load alone cost up to 8 % at one pose -- DESIGN.md 4.21); the within kernels read it before
// every leaf too, a leaf costing far more than the load (measured at 1 024 poses: 6.5 against 27 ms, 64 against 191 ms --
// DESIGN.md 4.24). PSM_MESH_SKIP = 0 / 1 forces it off / on (a study knob: psm_hip.h).
bool mesh_skip(size_t queries) {
    const char* knob = getenv("PSM_MESH_SKIP");
    return knob ? knob[0] != '0' : (queries + QUERY_BLOCK - 1) / QUERY_BLOCK > QUERY_GRID_CAP;
}

// PSM_MESH_BOUND = 0 / 1 forces the clearance kernels' shared bound off / on (a study knob: psm_hip.h); 2 and 3 are the
// alternatives DESIGN.md 4.24 measures: the word read in begin() alone and published at finish() alone; re-read before every
// leaf but published at finish() alone. The answer is the same under each. On by default at every launch size (measured, the
// torus of 2 304 triangles against the Sponza-class / the stress scene: 0.71 against 3.3 ms and 1.3 against 17 ms at one pose,
// 29 against 238 ms and 81 against 961 ms at 1 024; read in begin() alone 3.2 / 17 / 133 / 573 ms, published late 1.3 / 3.7 /
// 47 / 273 ms).
char mesh_bound() {
    const char* knob = getenv("PSM_MESH_BOUND");
    return knob ? knob[0] : '1';
}

namespace {

const char* const MESH_NAME[] = {"psm_bvh_mesh_overlaps_dev", "psm_bvh_mesh_count_dev", "psm_bvh_mesh_triangles_dev"};

// A mesh query: NULL handles and p == 0 are answered before anything else is looked at; then the data, k, the state, the depth,
// the contexts, the poses, the number of answers -- all on the host, before any launch, the outputs untouched. Then the upload.
int mesh_query(psm_bvh* b, psm_bvh* o, const float* poses, size_t p, int mode, uint32_t k, void* d_out, uint32_t* d_count) {
    if (!b || !o) return PSM_ERR_INVALID;
    if (p == 0) return PSM_OK;
    psm_ctx* c = b->ctx;
    const char* name = MESH_NAME[mode];
    const bool rows = mode == MESH_TRIS;
    int rc = mesh_pointers(c, name, poses && d_out && (!rows || d_count));
    if (rc == PSM_OK && mode != MESH_ANY) rc = mesh_aligned(c, name, rows ? "tris" : "counts", d_out, 4);
    if (rc == PSM_OK && rows) rc = mesh_aligned(c, name, "counts", d_count, 4);
    if (rc != PSM_OK) return rc;
    if (rows && (k == 0 || k > PSM_QUERY_K_MAX)) return mesh_refuse(c, PSM_ERR_INVALID, "%s: k must be 1 .. %d", name, PSM_QUERY_K_MAX);
    if (!b->built || !o->built) return set_err(c, PSM_ERR_STATE, "mesh query before build");
    if (depth_bound(b) > QSTACK_MAX) return set_err(c, PSM_ERR_CAPACITY, "mesh query: hierarchy deeper than the query stack");
    if (o->ctx != c) return mesh_refuse(c, PSM_ERR_INVALID, "%s: the two hierarchies are of different contexts", name);
    const uint32_t T = o->tri_count;
    rc = mesh_poses_rigid(c, name, poses, p);
    if (rc == PSM_OK) rc = mesh_answers_fit(c, name, p, T);
    if (rc != PSM_OK) return rc;
    (void)hipSetDevice(c->device);
    void* d_poses = nullptr;
    uint32_t L = 0;
    rc = mesh_upload(c, o, poses, p, &d_poses, nullptr, &L);
    if (rc != PSM_OK) return rc;
    // (the context's stack area is allocated here, on its first query: the last thing that can fail before the outputs change)
    MeshArgs m = {};
    uint32_t grid = 0;
    rc = batch_args(c, nullptr, p * (size_t)L, d_out, k, m.q, grid);
    if (rc != PSM_OK) return rc;
    // the outputs, cleared in stream order: a dropped triangle's entries and an unset flag read 0 / -1
    const size_t cells = p * (size_t)T;
    if (mode == MESH_ANY) PSM_HIP(c, hipMemsetAsync(d_out, 0, p, c->stream));
    if (mode == MESH_COUNT) PSM_HIP(c, hipMemsetAsync(d_out, 0, cells * sizeof(uint32_t), c->stream));
    if (rows) {
        PSM_HIP(c, hipMemsetAsync(d_out, 0xff, cells * k * sizeof(int32_t), c->stream));
        PSM_HIP(c, hipMemsetAsync(d_count, 0, cells * sizeof(uint32_t), c->stream));
    }
    if (L == 0) return PSM_OK;
    m.q.node32 = b->d_node32; m.q.tri48 = b->d_tri48; m.q.sm = b->d_small; m.q.sorted_tri = b->d_sorted_tri;
    if (rows) m.q.count = d_count;
    m.tri48 = o->d_tri48; m.leaf_tri = o->d_leaftri; m.poses = (const float4*)d_poses;
    m.magic = mesh_magic(L); m.L = L; m.T = T;
    m.flags = mesh_skip(p * (size_t)L) ? MESH_FLAG_SKIP : 0u;   // (read by the flag kernel alone)
    if (mode == MESH_ANY) bvh_query_mesh_any<<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
    else if (mode == MESH_COUNT) bvh_query_mesh_count<<<grid, QUERY_BLOCK, 0, c->stream>>>(m);
    else bvh_query_mesh_tris<<<grid, QUERY_BLOCK, (size_t)k * QUERY_BLOCK * sizeof(uint32_t), c->stream>>>(m);
    PSM_HIP(c, hipGetLastError());
    return PSM_OK;
}

}  // namespace

// for psm_ctx_destroy: the context's pose area and its key words go with it
void mesh_release(psm_ctx* c) {
    std::lock_guard<std::mutex> lk(pose_mu);
    auto it = pose_area.find(c);
    if (it == pose_area.end()) return;
    if (it->second.poses.ptr) (void)hipFree(it->second.poses.ptr);
    if (it->second.keys.ptr) (void)hipFree(it->second.keys.ptr);
    pose_area.erase(it);
}

}  // namespace psm

int psm_bvh_mesh_overlaps_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, uint8_t* d_hit) {
    return psm::mesh_query(bvh, other, poses, p, psm::MESH_ANY, 0, d_hit, nullptr);
}

int psm_bvh_mesh_count_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, uint32_t* d_count) {
    return psm::mesh_query(bvh, other, poses, p, psm::MESH_COUNT, 0, d_count, nullptr);
}

int psm_bvh_mesh_triangles_dev(psm_bvh* bvh, psm_bvh* other, const float* poses, size_t p, uint32_t k, int32_t* d_ids, uint32_t* d_count) {
    return psm::mesh_query(bvh, other, poses, p, psm::MESH_TRIS, k, d_ids, d_count);
}
