#!/usr/bin/env python3
"""Ray-query benchmark (psm_bvh_intersect_dev / psm_bvh_occluded_dev): Mrays/s of closest hit and any hit over the Sponza-class
scene's 1920 x 1080 camera rays, over as many bounce-like rays (origins at the primary hits, random directions in the hemisphere of
the hit triangle's face normal), and psm_rt_traverse WHOLE over the same primary rays for comparison. Each figure: the median of
REPS (5) device-synchronised calls after a warm-up call. Prints one JSON line.
`query_bench.py points`: the point queries (psm_bvh_closest_point_dev / psm_bvh_within_dev) on the same scene instead, NPTS (2^21)
points per set: (a) surface samples plus Gaussian noise of 1 % of the scene diagonal, closest point with rmax = inf; (b) uniform in
the scene's bounds, rmax = inf; (c) set (b) through within with a radius of 0.5 % of the diagonal.
`query_bench.py signed`: the hit count and the queries built on it (psm_bvh_count_hits_dev / psm_bvh_inside_dev /
psm_bvh_signed_distance_dev): (a) count beside closest and any on the ray mode's primary and bounce-like rays; (b) on a closed mesh
(a torus of TORUS_NU x TORUS_NV quads, 2 M triangles) and a regular grid of NPTS points over its bounds: inside with 1 / 3 / 5
rays, closest point, and signed distance with rmax = inf and with a band of 2 % of the diagonal.
`query_bench.py scene`: the scene queries (psm_scene_*_dev) on the ray mode's primary and bounce-like rays and the point mode's
uniform points: (a) a scene of ONE geometry against the plain query (the cost of the machinery); (b) the scene cut into 2, 8 and 32
spatially separate parts (slabs of equal triangle count along x): one scene launch against the merged hierarchy and against the sum
of G plain launches; (c) the static scene plus a small mesh that moves (MOVING_NU x MOVING_NV torus): rebuild of the small mesh +
a scene query against rebuild of the merged hierarchy + a plain query.
`query_bench.py instances`: the instanced scene queries (psm_instances_*_dev) on the scene mode's bounce-like rays and uniform
points: (a) identity instances against `scene` on the same hierarchies (the merged one; 8 slabs): the cost of the move; (b) ONE torus
hierarchy (MOVING_NU x MOVING_NV) at 2, 8 and 32 poses on a lattice inside the scene's bounds; (c) the static scene plus a moving
10 000-triangle torus: a pose update + an instanced query against a re-upload and rebuild of the small mesh + a scene query.
`query_bench.py world`: the instance worlds (psm_world_*) through the package's InstanceWorld, device arrays in and out:
(a) N = 32 separated tori, world against InstancedScene on the same library, interleaved A B A B; (b) one torus at 256, 4096
and 65 536 grid poses: absolute throughput of local rays and points; (c) a pose update plus a world query against re-baking the
posed triangles into one hierarchy (upload + build) plus a plain query. WORLD_N = queries per batch (default 2^18).
`query_bench.py kbest`: the k-best queries (psm_bvh_first_hits_dev / psm_bvh_nearest_dev) for k = 1, 4 and 16, every pair
alternated A B A B with medians of REPS: on the ray mode's primary and bounce-like rays firstHits against intersect, against
countHits, and against what a caller does without it -- k intersect launches, tmin moved past the last t between them (a torch
operation on the same stream; it loses hits at a bit-equal t); on the point mode's two sets nearest against closestPoint.
`query_bench.py worldkbest`: the k-best queries of an instance world (psm_world_first_hits_dev / psm_world_nearest_dev) on the world
mode's scenes (one torus at 32, 256, 4096 and 65 536 grid poses, local rays and points), k = 1, 4 and 16, every pair alternated
A B A B with medians of REPS: firstHits against intersect, and against k intersect launches with tmin moved past the last t
between them (it loses hits at a bit-equal t); nearest against closestPoint. WORLD_N = queries per batch (default 2^18).
`query_bench.py boxes`: the box queries (psm_bvh_box_overlaps_dev / psm_bvh_box_count_dev / psm_bvh_box_triangles_dev) on the
Sponza-class scene and the stress scene (STRESS_TRIS triangles, default 10 M): the three queries (triangles at k = 4 and 16) over
the cell boxes of a 64^3 and a 128^3 grid of the scene's bounds, each alternated A B A B (medians of REPS) with what a caller had
before them: psm_bvh_within_dev with the cell's half-diagonal as radius (a sphere around the cell: it over-reports); and
boxCount for ONE box around half the scene (the case an early acceptance of contained subtrees would serve).
`query_bench.py worldboxes`: the box queries of an instance world (psm_world_box_overlaps_dev / psm_world_box_count_dev /
psm_world_box_triangles_dev) on the world mode's torus at 256 and 4 096 grid poses: the three queries (triangles at k = 4 and 16)
over the cell boxes of a 64^3 grid of the world's bounds, each alternated A B A B (medians of REPS) with psm_world_within_dev at
the cell's half-diagonal -- the stand-in a caller had --; and countInBox for ONE box around half the world.
`query_bench.py worldsweeps`: the sphere sweeps of an instance world (psm_world_sweep_sphere_dev / psm_world_sweep_occluded_dev) on
the worldboxes mode's world, the torus at 256 and 4 096 turned grid poses: WORLD_SWEEP_N (262 144) sweeps along rays through the
world with radii of 0.1 %, 1 % and 5 % of the world's diagonal, alternated A B A B with the world's intersect / occluded on the same
rays; the fraction that touches and the fraction that touches at t = 0. No ratio is fixed in advance.

`query_bench.py sweeps`: the sphere sweeps (psm_bvh_sweep_sphere_dev / psm_bvh_sweep_occluded_dev) on the Sponza-class scene and
the stress scene (STRESS_TRIS triangles, default 10 M): SWEEP_N (2 M) sweeps along the camera's primary rays with radii of 0.1 %,
1 % and 5 % of the scene's diagonal, each alternated A B A B (medians of REPS) with psm_bvh_intersect_dev / psm_bvh_occluded_dev
on the same rays -- the floor a sweep cannot beat --, and the fractions that touch at all and that touch at t = 0.
`query_bench.py triangles`: the triangle queries (psm_bvh_tri_overlaps_dev / psm_bvh_tri_count_dev / psm_bvh_tri_triangles_dev) on the
Sponza-class scene and the stress scene (STRESS_TRIS triangles, default 10 M), the three queries (triangles at k = 4 and 16), each
alternated A B A B (medians of REPS) with boxCount / boxTriangles over the same triangles' bounding boxes -- the stand-in a caller
had, a superset -- on two query sets: a second mesh of small triangles, a torus (TRI_TORUS_NU x TRI_TORUS_NV quads) placed to cut
through the scene, and TRI_SLANTED (4 096) scene-sized slanted triangles, where the bounding box is a poor proxy; for each the
fraction of queries that report and the ratio of box count to triangle count. No ratio is fixed in advance.
`query_bench.py clearance`: the clearance queries (psm_bvh_tri_closest_dev / psm_bvh_tri_within_dev) on the Sponza-class scene and the
stress scene, on the triangles mode's two query sets (the torus of small triangles, the scene-sized slanted ones), at rmax = +inf and
at a small finite rmax (CLEAR_RMAX, default 1 % of the scene's diagonal): triClosest alternated A B A B (host-timed medians of REPS)
with triCount on the same triangles, triWithin with closestPoint on the queries' centroids at the same rmax -- context columns, not
bars: neither answers the clearance question --, and the fractions that find a triangle and that are at distance 0.
`query_bench.py worldtriangles`: the triangle queries of an instance world (psm_world_tri_overlaps_dev / psm_world_tri_count_dev /
psm_world_tri_triangles_dev) on the worldboxes mode's world, the torus at 256 and 4 096 turned grid poses, the three queries
(triangles at k = 4 and 16), each alternated A B A B (medians of REPS) with countInBox / trianglesInBox over the same triangles'
bounding boxes -- the one-launch stand-in a caller had, a superset: context, not a bar -- on two query sets: a second torus posed
WTRI_BODIES (64) times beside bodies of the world, so that the meshes cut, and WTRI_SLANTED (4 096) body-sized slanted triangles;
for each the fraction of queries that report and the ratio of box-reported to triangle-reported pairs. No ratio is fixed in advance.
`query_bench.py meshes`: the mesh queries (psm_bvh_mesh_overlaps_dev / psm_bvh_mesh_count_dev / psm_bvh_mesh_triangles_dev) on the
Sponza-class scene, cut by the worldboxes mode's torus (2 304 triangles) scaled to a quarter of its extent, and on that torus cut by
itself, at 1, 64 and 1 024 poses placed so that the meshes cut (the build of the other mesh excluded), the torus loaded as it is
made (in strips) and with its triangles shuffled. Per case, each pair alternated
A B A B (host-timed medians of REPS): (a) the mesh query, against (b) triCount / triTriangles (k = 16) over the same posed triangles
already resident on the device as psm_tri_query records in load order -- kernel for kernel --, the two B series of count giving
the spread between runs, and the call's own overhead (upload, wait, clears: a mesh query of a mesh without leaves) timed apart; (c) the path the call replaces: download of the other mesh's triangles, posing in numpy,
packing, upload, triCount (timed as a whole, alternated with (a)); and the flag query with its early-out skip forced on and off
(PSM_MESH_SKIP = 1 / 0; by itself a launch skips when it takes the grid-stride loop). No ratio is fixed in advance.
`query_bench.py worldmeshes`: the mesh queries of an instance world (psm_world_mesh_overlaps_dev / psm_world_mesh_count_dev /
psm_world_mesh_triangles_dev) on the worldtriangles mode's world of 4 096 torus poses and on the Sponza-class scene as a world of one,
the other mesh the torus (2 304 triangles; a quarter of the scene's extent across against the scene) at 1, 64 and 1 024 poses placed
so that the meshes cut. Per case and query, alternated A B A B (host-timed medians of REPS), twice: (a) the world mesh query, the
whole call, against (b) countOnTriangle / overlapsTriangle / trianglesOnTriangle (k = 16) over the same posed triangles already
resident on the device as psm_tri_query records in load order; the two (b) medians give the spread between runs; and the call's
own overhead (checks, upload, wait, clears: the same call on a mesh without leaves) timed apart. No ratio is fixed in advance.
`query_bench.py world-clearance`: the clearance queries of an instance world (psm_world_tri_closest_dev / psm_world_tri_within_dev) on
worlds of 1, 64 and 1 024 turned grid poses (WCLEAR_POSES) of the Sponza-class scene and of the worldboxes mode's torus
(WCLEAR_SCENES), WCLEAR_QUERIES (2^16) world triangles of a twentieth of a body's extent anywhere in the world's box, at rmax = +inf
and at a small one (WCLEAR_RMAX, default 1 % of a body's diagonal). closestToTriangle and withinOfTriangle (the whole numpy call:
upload, one launch, download), each alternated A B A B (host-timed medians of REPS; one timed call from 1 024 instances on) with what a caller
could do before: the queries moved into every instance on the host, TriangleHierarchy.triClosest once per instance, the minimum on
the host. Both times, the ratio, the fraction that finds a pair, and the largest difference between the two distances (they differ
by the rounding of the host's move). No ratio is fixed in advance.
`query_bench.py meshclearance`: mesh clearance (psm_bvh_mesh_closest_dev / psm_bvh_mesh_within_dev / psm_bvh_mesh_clearance_dev) on
the Sponza-class scene and the stress scene (CLEAR_SCENES), the other mesh the meshes mode's torus (2 304 triangles, a quarter of the
scene's extent across) and its hollow twin (as many triangles, none a leaf: the call's own overhead), at 1 and 1 024 poses whose
centres lie up to two torus radii off a vertex of the scene (some cut, most come near). Alternated A B A B (host-timed medians of
REPS, the whole call): meshClearance with the shared bound off and on (PSM_MESH_BOUND = 0 / 1), then on against its two variants
(2: the word read in begin() alone and published at finish() alone; 3: re-read before every leaf, published at finish() alone),
meshClearance against meshClosest plus a torch min over the device buffer (what a caller had), meshWithin at 1 % of the diagonal
against meshOverlaps (context: it answers less) and with its skip forced on and off (PSM_MESH_SKIP = 1 / 0). No ratio is fixed in advance.
`query_bench.py world-mesh-clearance`: mesh clearance over an instance world (psm_world_mesh_clearance_dev) on the world-clearance
mode's worlds -- 1, 64 and 1 024 turned grid poses (WMCLEAR_INSTANCES) of the Sponza-class scene and of the torus (WMCLEAR_SCENES) --,
the other mesh the 2 304-triangle torus at a quarter of a body's extent, at 1 and 1 024 poses (WMCLEAR_POSES) anywhere in the
world's box, at rmax = +inf and at 1 % of a body's diagonal. clearanceToMesh (the whole numpy call) alternated A B A B (host-timed
medians of REPS; one timed call where a side's warm-up call takes more than WMCLEAR_SLOW seconds) with (1) what a caller could do
before: the torus posed on the host, closestToTriangle over the p x T triangles, the minimum per pose on the host, and with (2)
the same call under PSM_MESH_BOUND=0. Both ratios and whether the two paths agree in (dist, tri, other, instance) at every pose.
Each case's figures are also appended to WMCLEAR_LOG as they come. No ratio is fixed in advance.
`query_bench.py worldgrids`: the voxel grids over a world (psm_grid_world_surface_dev / _counts_dev / _instances_dev / _solid_dev) on
the worldboxes mode's world, the torus at 256 and 4 096 turned grid poses (WORLD_GRID_POSES): 64^3, 128^3 and 256^3 grids over the
world's bounds (GRID_SIZES), per size surface, counts and instances alternated A B A B (host-timed medians of REPS) with overlapsBox /
countInBox / trianglesInBox(k = 1) over voxel_boxes() of the same grid, twice: launch against launch with the box records resident,
and the package's whole call from host memory (the records' packing and upload and the answers' read-back included). Also solid at
3 rays, the occupied voxels, and whether all three answers were the box queries' (same_answers).

`query_bench.py grids`: the voxel grids (psm_grid_surface_dev / psm_grid_counts_dev / psm_grid_solid_dev) on the Sponza-class scene:
64^3, 128^3 and 256^3 grids over its bounds (GRID_SIZES), per size the ms of surface, counts and solid (3 rays), the occupied voxels,
and surface alternated A B A B (host-timed medians of REPS) with the way a caller had to the same bits -- boxOverlaps over
voxel_boxes of the same grid: the kernel alone over resident records, the package's torch call over resident lo / hi, and the same
from host arrays (the box upload included) --, with a check that the bits are the same. No ratio is fixed in advance.
`query_bench.py distgrids`: the distance-field grids (psm_grid_distance_dev / psm_grid_signed_distance_dev) on the Sponza-class
scene: 64^3, 128^3 and 256^3 grids over its bounds (GRID_SIZES), rmax = +inf and a band of two cell diagonals, unsigned and signed
with 3 rays; per case the field alternated A B A B (host-timed medians of REPS) with the way a caller had to the same bits --
closestPoint / signedDistance over voxel_centres of the same grid: the entry point alone over resident records, the package's
torch call over resident centres, and the same from host arrays (the upload included) --, the fraction of voxels with a triangle
within rmax, and a check that dist and tri are the same bits (same_bits). No ratio is fixed in advance.
`query_bench.py sparsegrids`: the sparse grids (psm_grid_sparse_*_dev) on the Sponza-class scene: 128^3, 256^3, 512^3 and, sparse
only, 1024^3 grids over its bounds (SPARSE_SIZES; the dense side up to SPARSE_DENSE_MAX), the distance field with a band of two cell
diagonals and with rmax = +inf, and the surface. Per case the bricks listed and their fraction, the bytes of both outputs, the
listing with the coarse pass on and off (PSM_SPARSE_COARSE, alternated A B A B, host-timed medians of REPS, and whether both lists
agree), the fill, and list + fill alternated with the dense call of the same tree, after a check that the sparse answer scattered
back is the dense one bit for bit (same_bits); the dense call is also alternated with itself (the spread). Each case's figures are
also appended to SPARSE_LOG as they come. No ratio is fixed in advance.
`query_bench.py worlddistgrids`: the distance-field grids over a world (psm_grid_world_distance_dev /
psm_grid_world_signed_distance_dev) on the worldgrids mode's worlds, the torus at 256 and 4 096 turned grid poses
(WORLD_GRID_POSES): 64^3, 128^3 and 256^3 grids over the world's bounds (GRID_SIZES), rmax = +inf and a band of two cell diagonals,
unsigned and signed with 3 rays; per case the field alternated A B A B (host-timed medians of REPS, each call ending in a
synchronise) with the ways a caller had to the same bits -- the world's closestPoint / signedDistance over voxel_centres of the
same grid: the entry point alone over resident records, the package's torch call over resident centres, and the same from the
host array (the upload included) --, the fraction of voxels with a triangle within rmax, and a check that dist, tri and inst are
the same bits (same_bits). Each case's figures are also appended to WORLD_DIST_LOG as they come. No ratio is fixed in advance.
A kernel trace of its own: rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/query_bench.py [points | signed | scene | instances]"""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
psm = importlib.import_module("prismarine-core_amd")
scenes = importlib.import_module("prismarine-core_amd.scenes")

W, H = 1920, 1080
REPS = int(os.environ.get("REPS", "5"))
NPTS = int(os.environ.get("NPTS", str(1 << 21)))
TORUS_NU, TORUS_NV = int(os.environ.get("TORUS_NU", "1448")), int(os.environ.get("TORUS_NV", "724"))


def median_ms(ctx, fn):
    fn()
    ctx.sync()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def points():
    sc = scenes.sponza_like()
    ctx = psm.Context(0)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(sc["tris"].shape[0])
    th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
    th.build()
    tris = sc["tris"].reshape(-1, 3, 3)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.RandomState(7)
    n = NPTS
    w = rng.dirichlet([1, 1, 1], n).astype(np.float32)
    surf = np.einsum("ij,ijk->ik", w, tris[rng.randint(0, tris.shape[0], n)])
    sets = {"surface_noise": (surf + rng.normal(0, 0.01 * diag, (n, 3))).astype(np.float32),
            "uniform": rng.uniform(lo, hi, (n, 3)).astype(np.float32)}
    lib = psm.lib()
    h_pts, h_hits, h_in = ctx.buf_alloc(16 * n), ctx.buf_alloc(16 * n), ctx.buf_alloc(n)
    p_pts, p_hits, p_in = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in (h_pts, h_hits, h_in))

    def upload(p, r):
        q = np.empty((n, 4), np.float32)
        q[:, 0:3], q[:, 3] = p, r
        ctx.buf_upload(h_pts, q)

    def closest():
        ctx.check(lib.psm_bvh_closest_point_dev(th._h, p_pts, C.c_size_t(n), p_hits), "psm_bvh_closest_point_dev")

    def within():
        ctx.check(lib.psm_bvh_within_dev(th._h, p_pts, C.c_size_t(n), p_in), "psm_bvh_within_dev")

    radius = 0.005 * diag
    out = {"points": n, "reps": REPS, "tris": int(tris.shape[0]), "diag": round(diag, 3), "within_radius": round(radius, 4)}
    upload(sets["surface_noise"], np.inf)
    out["a_surface_noise_closest_ms"] = median_ms(ctx, closest)
    upload(sets["uniform"], np.inf)
    out["b_uniform_closest_ms"] = median_ms(ctx, closest)
    upload(sets["uniform"], radius)
    out["c_uniform_within_ms"] = median_ms(ctx, within)
    out["c_within_fraction"] = float(ctx.buf_download(h_in, np.uint8, n).mean())
    for k in ("a_surface_noise_closest", "b_uniform_closest", "c_uniform_within"):
        out[k + "_mpts_s"] = round(n / out[k + "_ms"] / 1e3, 1)
        out[k + "_ms"] = round(out[k + "_ms"], 4)
    out["lib"] = os.path.basename(psm.LIB_PATH)
    for h in (h_pts, h_hits, h_in):
        ctx.buf_free(h)
    th.close()
    ctx.close()
    print(json.dumps(out))


def bounce_rays(sc, o, d, hits):
    """bounce-like rays: from the primary hits (rays that missed start at their origin), a cosine-ish direction about the face
    normal turned towards the incoming ray"""
    n = o.shape[0]
    tri = hits.view(np.int32)[:, 3]
    rng = np.random.RandomState(7)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    hit = tri >= 0
    bo = np.where(hit[:, None], o + dn * np.where(hit, hits[:, 2], 0)[:, None], o).astype(np.float32)
    t3 = sc["tris"].reshape(-1, 3, 3)[np.maximum(tri, 0)]
    nrm = np.cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    nrm = np.where((np.sum(nrm * dn, axis=1) > 0)[:, None], -nrm, nrm)
    nrm = np.where(hit[:, None], nrm, dn)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return bo, (nrm + u).astype(np.float32)


def torus(nu, nv, R=1.0, r=0.4):
    """a closed mesh: a torus around the z axis, nu x nv quads split in two, vertices on the surface"""
    u, w = np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv)
    U, Wv = np.meshgrid(u, w, indexing="ij")
    vs = np.stack([(R + r * np.cos(Wv)) * np.cos(U), (R + r * np.cos(Wv)) * np.sin(U), r * np.sin(Wv)], -1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    a, b, c, d = vs[i, j], vs[i1, j], vs[i1, j1], vs[i, j1]
    return np.concatenate([np.stack([a, b, c], -2).reshape(-1, 9), np.stack([a, c, d], -2).reshape(-1, 9)]).astype(np.float32)


def signed():
    lib = psm.lib()
    out = {"reps": REPS}
    # (a) count beside closest and any: the ray mode's rays
    sc = scenes.sponza_like()
    ctx = psm.Context(0)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(sc["tris"].shape[0])
    th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
    th.build()
    rt = psm.Pipeline(ctx, seed=1000)
    rt.resizeBuffers(W, H)
    rt.resize(W, H)
    cam = scenes.camera_matrices(sc["eye"], sc["view"], W, H)
    rt.camera_matrices(cam[0], cam[1])
    prim = rt.download_rays()
    rt.close()
    n = prim.shape[0]
    o, d = prim["origin"].copy(), prim["direct"].copy()
    h_rays, h_hits, h_occ, h_cnt = ctx.buf_alloc(32 * n), ctx.buf_alloc(16 * n), ctx.buf_alloc(n), ctx.buf_alloc(4 * n)
    p_rays, p_hits, p_occ, p_cnt = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in (h_rays, h_hits, h_occ, h_cnt))

    def upload(o, d, tmin):
        r = np.zeros((n, 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, np.inf
        ctx.buf_upload(h_rays, r)

    def closest():
        ctx.check(lib.psm_bvh_intersect_dev(th._h, p_rays, C.c_size_t(n), p_hits), "psm_bvh_intersect_dev")

    def anyhit():
        ctx.check(lib.psm_bvh_occluded_dev(th._h, p_rays, C.c_size_t(n), p_occ), "psm_bvh_occluded_dev")

    def count():
        ctx.check(lib.psm_bvh_count_hits_dev(th._h, p_rays, C.c_size_t(n), p_cnt), "psm_bvh_count_hits_dev")

    out["rays"] = n
    upload(o, d, 0.0)
    for k, fn in (("closest", closest), ("any", anyhit), ("count", count)):
        out["primary_%s_ms" % k] = median_ms(ctx, fn)
    out["primary_mean_count"] = float(ctx.buf_download(h_cnt, np.uint32, n).mean())
    hits = ctx.buf_download(h_hits, np.float32, 4 * n).reshape(n, 4)
    upload(*bounce_rays(sc, o, d, hits), 1e-3)
    for k, fn in (("closest", closest), ("any", anyhit), ("count", count)):
        out["bounce_%s_ms" % k] = median_ms(ctx, fn)
    out["bounce_mean_count"] = float(ctx.buf_download(h_cnt, np.uint32, n).mean())
    for s in ("primary", "bounce"):
        out[s + "_count_over_closest"] = round(out[s + "_count_ms"] / out[s + "_closest_ms"], 3)
        out[s + "_count_over_any"] = round(out[s + "_count_ms"] / out[s + "_any_ms"], 3)
        for k in ("closest", "any", "count"):
            out["%s_%s_mrays_s" % (s, k)] = round(n / out["%s_%s_ms" % (s, k)] / 1e3, 1)
            out["%s_%s_ms" % (s, k)] = round(out["%s_%s_ms" % (s, k)], 4)
    for h in (h_rays, h_hits, h_occ, h_cnt):
        ctx.buf_free(h)
    th.close()

    # (b) a closed mesh and a regular grid over its bounds
    tris = torus(TORUS_NU, TORUS_NV)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tris.shape[0])
    th.loadTriangles(tris)
    th.build()
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diag = float(np.linalg.norm(hi - lo))
    g = int(round(NPTS ** (1.0 / 3.0)))
    m = g * g * g
    ax = [np.linspace(lo[k], hi[k], g, dtype=np.float32) for k in range(3)]
    grid = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    h_pts, h_hits, h_in = ctx.buf_alloc(16 * m), ctx.buf_alloc(16 * m), ctx.buf_alloc(m)
    p_pts, p_hits, p_in = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in (h_pts, h_hits, h_in))

    def upload_points(r):
        q = np.empty((m, 4), np.float32)
        q[:, 0:3], q[:, 3] = grid, r
        ctx.buf_upload(h_pts, q)

    def inside(s):
        return lambda: ctx.check(lib.psm_bvh_inside_dev(th._h, p_pts, C.c_size_t(m), C.c_uint32(s), p_in), "psm_bvh_inside_dev")

    def closest_point():
        ctx.check(lib.psm_bvh_closest_point_dev(th._h, p_pts, C.c_size_t(m), p_hits), "psm_bvh_closest_point_dev")

    def signed_distance():
        ctx.check(lib.psm_bvh_signed_distance_dev(th._h, p_pts, C.c_size_t(m), C.c_uint32(3), p_hits), "psm_bvh_signed_distance_dev")

    band = 0.02 * diag
    out.update({"points": m, "grid": g, "mesh_tris": int(tris.shape[0]), "diag": round(diag, 3), "band": round(band, 4)})
    upload_points(np.inf)
    times = {}
    for s in (1, 3, 5):
        times["inside_%d" % s] = median_ms(ctx, inside(s))
        out["inside_%d_fraction" % s] = float(ctx.buf_download(h_in, np.uint8, m).mean())
    times["closest_point"] = median_ms(ctx, closest_point)
    times["signed_distance_3"] = median_ms(ctx, signed_distance)
    upload_points(band)
    times["closest_point_band"] = median_ms(ctx, closest_point)
    times["signed_distance_3_band"] = median_ms(ctx, signed_distance)
    out["band_fraction"] = float((ctx.buf_download(h_hits, np.float32, 4 * m).view(np.int32)[3::4] >= 0).mean())
    for k, v in times.items():
        out[k + "_ms"] = round(v, 4)
        out[k + "_mpts_s"] = round(m / v / 1e3, 1)
    out["lib"] = os.path.basename(psm.LIB_PATH)
    for h in (h_pts, h_hits, h_in):
        ctx.buf_free(h)
    th.close()
    ctx.close()
    print(json.dumps(out))


def scene():
    lib = psm.lib()
    sc = scenes.sponza_like()
    tris = np.ascontiguousarray(sc["tris"], np.float32).reshape(-1, 9)
    ctx = psm.Context(0)

    def hier(t):
        th = psm.TriangleHierarchy(ctx)
        th.allocate(t.shape[0])
        th.loadTriangles(t)
        th.build()
        return th

    merged = hier(tris)
    rt = psm.Pipeline(ctx, seed=1000)
    rt.resizeBuffers(W, H)
    rt.resize(W, H)
    cam = scenes.camera_matrices(sc["eye"], sc["view"], W, H)
    rt.camera_matrices(cam[0], cam[1])
    prim = rt.download_rays()
    rt.close()
    n = prim.shape[0]
    o, d = prim["origin"].copy(), prim["direct"].copy()
    m = NPTS
    t3 = tris.reshape(-1, 3, 3)
    lo, hi = t3.reshape(-1, 3).min(0), t3.reshape(-1, 3).max(0)
    pts = np.empty((m, 4), np.float32)
    pts[:, 0:3], pts[:, 3] = np.random.RandomState(7).uniform(lo, hi, (m, 3)), np.inf
    k = max(n, m)
    h_rays, h_pts, h_hits, h_geom, h_occ = (ctx.buf_alloc(x) for x in (32 * n, 16 * m, 16 * k, 4 * k, k))
    p_rays, p_pts, p_hits, p_geom, p_occ = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in (h_rays, h_pts, h_hits, h_geom, h_occ))
    ctx.buf_upload(h_pts, pts)
    cn, cm = C.c_size_t(n), C.c_size_t(m)

    def upload(o, d, tmin):
        r = np.zeros((n, 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, np.inf
        ctx.buf_upload(h_rays, r)

    def handles(ths):
        return (C.c_void_p * len(ths))(*[t._h for t in ths]), C.c_uint32(len(ths))

    # the four workloads, plain (one hierarchy) and scene (a list)
    def plain(kind, th):
        if kind == "closest":
            return lambda: ctx.check(lib.psm_bvh_intersect_dev(th._h, p_rays, cn, p_hits), "psm_bvh_intersect_dev")
        if kind == "any":
            return lambda: ctx.check(lib.psm_bvh_occluded_dev(th._h, p_rays, cn, p_occ), "psm_bvh_occluded_dev")
        if kind == "point":
            return lambda: ctx.check(lib.psm_bvh_closest_point_dev(th._h, p_pts, cm, p_hits), "psm_bvh_closest_point_dev")
        return lambda: ctx.check(lib.psm_bvh_inside_dev(th._h, p_pts, cm, C.c_uint32(3), p_occ), "psm_bvh_inside_dev")

    def scene_of(kind, ths):
        g, c = handles(ths)
        if kind == "closest":
            return lambda: ctx.check(lib.psm_scene_intersect_dev(g, c, p_rays, cn, p_hits, p_geom), "psm_scene_intersect_dev")
        if kind == "any":
            return lambda: ctx.check(lib.psm_scene_occluded_dev(g, c, p_rays, cn, p_occ), "psm_scene_occluded_dev")
        if kind == "point":
            return lambda: ctx.check(lib.psm_scene_closest_point_dev(g, c, p_pts, cm, p_hits, p_geom), "psm_scene_closest_point_dev")
        return lambda: ctx.check(lib.psm_scene_inside_dev(g, c, p_pts, cm, C.c_uint32(3), p_occ), "psm_scene_inside_dev")

    def each(kind, ths):
        fns = [plain(kind, t) for t in ths]
        return lambda: [f() for f in fns]

    out = {"rays": n, "points": m, "reps": REPS, "tris": int(tris.shape[0])}
    upload(o, d, 0.0)
    plain("closest", merged)()
    hits = ctx.buf_download(h_hits, np.float32, 4 * n).reshape(n, 4)
    bounce = bounce_rays(sc, o, d, hits)
    # slabs of equal triangle count along x
    order = np.argsort(t3[:, :, 0].mean(axis=1), kind="stable")
    parts = {g: [hier(tris[np.sort(idx)]) for idx in np.array_split(order, g)] for g in (2, 8, 32)}
    workloads = (("primary_closest", "closest", (o, d, 0.0)), ("bounce_closest", "closest", (*bounce, 1e-3)),
                 ("bounce_any", "any", None), ("points_closest", "point", None), ("points_inside3", "inside", None))
    for name, kind, rays in workloads:
        if rays is not None:
            upload(*rays)
        # (a): plain, scene of one, plain again (the plain query's own spread beside the difference)
        out[name + "_plain_ms"] = [round(median_ms(ctx, plain(kind, merged)), 4)]
        out[name + "_g1_ms"] = round(median_ms(ctx, scene_of(kind, [merged])), 4)
        out[name + "_plain_ms"].append(round(median_ms(ctx, plain(kind, merged)), 4))
        # (b)
        for g, ths in parts.items():
            out["%s_g%d_scene_ms" % (name, g)] = round(median_ms(ctx, scene_of(kind, ths)), 4)
            out["%s_g%d_launches_ms" % (name, g)] = round(median_ms(ctx, each(kind, ths)), 4)
    # (c) the static scene and a small mesh that moves: a rebuild of what moved + a query
    small = (torus(int(os.environ.get("MOVING_NU", "100")), int(os.environ.get("MOVING_NV", "50"))) * np.float32(1.5)
             + np.tile(np.float32([0.0, 3.0, 0.0]), 3)).astype(np.float32)
    mover = hier(small)
    both = hier(np.concatenate([tris, small]))
    out["moving_tris"] = int(small.shape[0])
    upload(*bounce, 1e-3)
    for name, kind in (("bounce_closest", "closest"), ("points_closest", "point")):
        q_scene, q_plain = scene_of(kind, [merged, mover]), plain(kind, both)

        def frame_scene():
            mover.markDirty()
            mover.build()
            q_scene()

        def frame_merged():
            both.markDirty()
            both.build()
            q_plain()

        out["moving_%s_rebuild_small_plus_scene_ms" % name] = round(median_ms(ctx, frame_scene), 4)
        out["moving_%s_rebuild_merged_plus_plain_ms" % name] = round(median_ms(ctx, frame_merged), 4)
        out["moving_%s_scene_query_ms" % name] = round(median_ms(ctx, q_scene), 4)
        out["moving_%s_plain_query_ms" % name] = round(median_ms(ctx, q_plain), 4)
    out["lib"] = os.path.basename(psm.LIB_PATH)
    for h in (h_rays, h_pts, h_hits, h_geom, h_occ):
        ctx.buf_free(h)
    for th in [merged, mover, both] + [t for ths in parts.values() for t in ths]:
        th.close()
    ctx.close()
    print(json.dumps(out))


def instances():
    lib = psm.lib()
    sc = scenes.sponza_like()
    tris = np.ascontiguousarray(sc["tris"], np.float32).reshape(-1, 9)
    ctx = psm.Context(0)

    def hier(t):
        th = psm.TriangleHierarchy(ctx)
        th.allocate(t.shape[0])
        th.loadTriangles(t)
        th.build()
        return th

    merged = hier(tris)
    rt = psm.Pipeline(ctx, seed=1000)
    rt.resizeBuffers(W, H)
    rt.resize(W, H)
    cam = scenes.camera_matrices(sc["eye"], sc["view"], W, H)
    rt.camera_matrices(cam[0], cam[1])
    prim = rt.download_rays()
    rt.close()
    n = prim.shape[0]
    o, d = prim["origin"].copy(), prim["direct"].copy()
    m = NPTS
    t3 = tris.reshape(-1, 3, 3)
    lo, hi = t3.reshape(-1, 3).min(0), t3.reshape(-1, 3).max(0)
    pts = np.empty((m, 4), np.float32)
    pts[:, 0:3], pts[:, 3] = np.random.RandomState(7).uniform(lo, hi, (m, 3)), np.inf
    k = max(n, m)
    h_rays, h_pts, h_hits, h_geom, h_occ = (ctx.buf_alloc(x) for x in (32 * n, 16 * m, 16 * k, 4 * k, k))
    p_rays, p_pts, p_hits, p_geom, p_occ = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in (h_rays, h_pts, h_hits, h_geom, h_occ))
    ctx.buf_upload(h_pts, pts)
    cn, cm = C.c_size_t(n), C.c_size_t(m)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 4:7], r[:, 7] = o, d, np.inf
    ctx.buf_upload(h_rays, r)
    ctx.check(lib.psm_bvh_intersect_dev(merged._h, p_rays, cn, p_hits), "psm_bvh_intersect_dev")
    bo, bd = bounce_rays(sc, o, d, ctx.buf_download(h_hits, np.float32, 4 * n).reshape(n, 4))
    r[:, 0:3], r[:, 3], r[:, 4:7] = bo, 1e-3, bd
    ctx.buf_upload(h_rays, r)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)

    def turn(angle, at):      # a rotation about y and a translation
        c, s_ = np.cos(angle), np.sin(angle)
        return np.array([[c, 0, s_, at[0]], [0, 1, 0, at[1]], [-s_, 0, c, at[2]]], np.float32)

    def scene_of(kind, ths):
        g, c = (C.c_void_p * len(ths))(*[t._h for t in ths]), C.c_uint32(len(ths))
        if kind == "closest":
            return lambda: ctx.check(lib.psm_scene_intersect_dev(g, c, p_rays, cn, p_hits, p_geom), "psm_scene_intersect_dev")
        if kind == "point":
            return lambda: ctx.check(lib.psm_scene_closest_point_dev(g, c, p_pts, cm, p_hits, p_geom), "psm_scene_closest_point_dev")
        return lambda: ctx.check(lib.psm_scene_inside_dev(g, c, p_pts, cm, C.c_uint32(3), p_occ), "psm_scene_inside_dev")

    def inst_list(ths, poses):
        v = (psm.Instance * len(ths))()
        for i, (th, pose) in enumerate(zip(ths, poses)):
            v[i].bvh = th._h.value
            v[i].world_from_object[:] = np.asarray(pose, np.float32).reshape(12).tolist()
        return v

    def inst_of(kind, v):
        c = C.c_uint32(len(v))
        if kind == "closest":
            return lambda: ctx.check(lib.psm_instances_intersect_dev(v, c, p_rays, cn, p_hits, p_geom), "psm_instances_intersect_dev")
        if kind == "point":
            return lambda: ctx.check(lib.psm_instances_closest_point_dev(v, c, p_pts, cm, p_hits, p_geom), "psm_instances_closest_point_dev")
        return lambda: ctx.check(lib.psm_instances_inside_dev(v, c, p_pts, cm, C.c_uint32(3), p_occ), "psm_instances_inside_dev")

    kinds = (("bounce_closest", "closest"), ("points_closest", "point"), ("points_inside3", "inside"))
    out = {"rays": n, "points": m, "reps": REPS, "tris": int(tris.shape[0])}
    # (a) identity instances against the scene queries on the same hierarchies: scene, instances, scene again
    order = np.argsort(t3[:, :, 0].mean(axis=1), kind="stable")
    slabs = [hier(tris[np.sort(idx)]) for idx in np.array_split(order, 8)]
    for g, ths in ((1, [merged]), (8, slabs)):
        for name, kind in kinds:
            a0 = median_ms(ctx, scene_of(kind, ths))
            b = median_ms(ctx, inst_of(kind, inst_list(ths, [eye] * g)))
            a1 = median_ms(ctx, scene_of(kind, ths))
            out["identity_%s_g%d_scene_ms" % (name, g)] = [round(a0, 4), round(a1, 4)]
            out["identity_%s_g%d_instances_ms" % (name, g)] = round(b, 4)
            out["identity_%s_g%d_ratio" % (name, g)] = round(b / (0.5 * (a0 + a1)), 4)
    # (b) one torus at 2 / 8 / 32 poses, on a lattice across the scene's bounds
    small = torus(int(os.environ.get("MOVING_NU", "100")), int(os.environ.get("MOVING_NV", "50"))).astype(np.float32)
    mover = hier(small)
    out["torus_tris"] = int(small.shape[0])
    rng = np.random.RandomState(3)
    for g in (2, 8, 32):
        poses = [turn(rng.uniform(0, 6.28), lo + (hi - lo) * rng.uniform(0.1, 0.9, 3)) for _ in range(g)]
        for name, kind in kinds:
            out["torus_%s_p%d_ms" % (name, g)] = round(median_ms(ctx, inst_of(kind, inst_list([mover] * g, poses))), 4)
    # (c) the static scene and a torus that moves: a new pose + an instanced query, against a rebuild of the torus + a scene query
    step = [0]
    for name, kind in kinds[:2]:
        q_scene = scene_of(kind, [merged, mover])

        v = inst_list([merged, mover], [eye, eye])
        q_inst = inst_of(kind, v)

        def frame_instances():     # the new pose written into the host's list (12 floats), then the query
            step[0] += 1
            v[1].world_from_object[:] = turn(0.01 * step[0], [0.0, 3.0, 0.0]).reshape(12).tolist()
            q_inst()

        def frame_rebuild():       # what a moved body costs without poses: its triangles uploaded again, rebuilt, then the query
            mover.clearTribuffer()
            mover.loadTriangles(small)
            mover.build()
            q_scene()

        a0 = median_ms(ctx, frame_rebuild)
        b = median_ms(ctx, frame_instances)
        a1 = median_ms(ctx, frame_rebuild)
        out["moving_%s_rebuild_small_plus_scene_ms" % name] = [round(a0, 4), round(a1, 4)]
        out["moving_%s_pose_plus_instances_ms" % name] = round(b, 4)
        out["moving_%s_ratio" % name] = round(b / (0.5 * (a0 + a1)), 4)
    out["lib"] = os.path.basename(psm.LIB_PATH)
    for h in (h_rays, h_pts, h_hits, h_geom, h_occ):
        ctx.buf_free(h)
    for th in [merged, mover] + slabs:
        th.close()
    ctx.close()
    print(json.dumps(out))


def world():
    import torch
    n = int(os.environ.get("WORLD_N", str(1 << 18)))
    ctx = psm.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    tor = torus(48, 24, 0.7, 0.25)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tor.shape[0])
    th.loadTriangles(tor)
    th.build()
    rng = np.random.RandomState(1)
    dev = torch.device("cuda", 0)
    out = {"mode": "world", "queries": n, "torus_triangles": int(tor.shape[0]), "reps": REPS}

    def grid_poses(count):
        side = int(np.ceil(np.sqrt(count)))
        m = np.zeros((count, 3, 4), np.float32)
        m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = 1.0
        k = np.arange(count)
        m[:, 0, 3], m[:, 1, 3] = 2.5 * (k % side), 2.5 * (k // side)
        return m

    def local_queries(poses):
        c = poses[rng.randint(0, poses.shape[0], n), :, 3]
        o = (c + rng.uniform(-1.5, 1.5, (n, 3))).astype(np.float32)
        d = (c + rng.uniform(-0.6, 0.6, (n, 3)) - o).astype(np.float32)
        p = (c + rng.uniform(-1.2, 1.2, (n, 3))).astype(np.float32)
        return [torch.from_numpy(a).to(dev) for a in (o, d, p)]

    # (a) 32 separated bodies: the world against the flat list, A B A B
    poses = grid_poses(32)
    o, d, p = local_queries(poses)
    flat = psm.InstancedScene(ctx, [(th, m) for m in poses])
    wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
    for name, fa, fb in (("intersect", lambda: flat.intersect(o, d), lambda: wd.intersect(o, d)),
                         ("closest_point", lambda: flat.closestPoint(p), lambda: wd.closestPoint(p)),
                         ("inside", lambda: flat.inside(p, 3), lambda: wd.inside(p, 3))):
        a1, b1, a2, b2 = median_ms(ctx, fa), median_ms(ctx, fb), median_ms(ctx, fa), median_ms(ctx, fb)
        out["n32_%s_instanced_ms" % name] = [round(a1, 4), round(a2, 4)]
        out["n32_%s_world_ms" % name] = [round(b1, 4), round(b2, 4)]
        out["n32_%s_world_over_instanced" % name] = round((b1 + b2) / (a1 + a2), 3)
    wd.close()
    # (b) one torus at many poses
    for count in (256, 4096, 65536):
        poses = grid_poses(count)
        o, d, p = local_queries(poses)
        t0 = time.perf_counter()
        wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
        ctx.sync()
        out["poses%d_set_instances_ms" % count] = round((time.perf_counter() - t0) * 1e3, 3)
        out["poses%d_set_transforms_ms" % count] = round(median_ms(ctx, wd.refresh), 3)
        for name, fn in (("intersect", lambda: wd.intersect(o, d)), ("closest_point", lambda: wd.closestPoint(p)), ("inside", lambda: wd.inside(p, 3))):
            ms = median_ms(ctx, fn)
            out["poses%d_%s_ms" % (count, name)] = round(ms, 4)
            out["poses%d_%s_Mq_per_s" % (count, name)] = round(n / ms / 1e3, 2)
        if count == 256:
            # (c) a body moves: pose update + world query against re-bake (posed triangles, upload, build) + plain query
            baked = psm.TriangleHierarchy(ctx)
            baked.allocate(count * tor.shape[0])

            def rebake():
                tris = (tor[None] + poses[:, None, None, :, 3]).reshape(-1, 3, 3)
                baked.clearTribuffer()
                baked.loadTriangles(tris)
                baked.build()
                return baked.intersect(o, d)

            def move():
                wd.setTransform(7, poses[7])
                return wd.intersect(o, d)
            a1, b1, a2, b2 = median_ms(ctx, rebake), median_ms(ctx, move), median_ms(ctx, rebake), median_ms(ctx, move)
            out["moving_rebake_plus_query_ms"] = [round(a1, 3), round(a2, 3)]
            out["moving_pose_plus_world_query_ms"] = [round(b1, 3), round(b2, 3)]
            baked.close()
        wd.close()
    th.close()
    print(json.dumps(out))


def abab(ctx, fa, fb):
    """medians (ms) of fa and fb, alternated A B A B after a warm-up call of each"""
    fa()
    fb()
    ctx.sync()
    ta, tb = [], []
    for _ in range(REPS):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ta)), 4), round(float(np.median(tb)), 4)


def worldkbest():
    import torch   # (before the library loads its HIP runtime)
    n = int(os.environ.get("WORLD_N", str(1 << 18)))
    dev = torch.device("cuda", 0)
    ctx = psm.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)   # torch's tmin update and the launches: one stream
    tor = torus(48, 24, 0.7, 0.25)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tor.shape[0])
    th.loadTriangles(tor)
    th.build()
    rng = np.random.RandomState(1)
    lib = psm.lib()
    size = C.c_size_t(n)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    pts = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    geom = torch.zeros((n,), dtype=torch.int32, device=dev)
    rows = torch.zeros((n, 16, 4), dtype=torch.float32, device=dev)
    inst = torch.zeros((n, 16), dtype=torch.int32, device=dev)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    p_rays, p_pts, p_hits, p_geom, p_rows, p_inst, p_count = (C.c_void_p(x.data_ptr()) for x in (rays, pts, hits, geom, rows, inst, count))
    inf = torch.tensor(float("inf"), device=dev)
    out = {"mode": "worldkbest", "queries": n, "torus_triangles": int(tor.shape[0]), "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    for poses_n in (32, 256, 4096, 65536):
        side = int(np.ceil(np.sqrt(poses_n)))      # the world mode's grid of poses and its local queries
        poses = np.zeros((poses_n, 3, 4), np.float32)
        poses[:, 0, 0] = poses[:, 1, 1] = poses[:, 2, 2] = 1.0
        k_ = np.arange(poses_n)
        poses[:, 0, 3], poses[:, 1, 3] = 2.5 * (k_ % side), 2.5 * (k_ // side)
        c = poses[rng.randint(0, poses_n, n), :, 3]
        o = (c + rng.uniform(-1.5, 1.5, (n, 3))).astype(np.float32)
        r = np.zeros((n, 8), np.float32)
        r[:, 0:3], r[:, 4:7], r[:, 7] = o, (c + rng.uniform(-0.6, 0.6, (n, 3)) - o).astype(np.float32), np.inf
        rays.copy_(torch.from_numpy(r))
        q = np.empty((n, 4), np.float32)
        q[:, 0:3], q[:, 3] = (c + rng.uniform(-1.2, 1.2, (n, 3))).astype(np.float32), np.inf
        pts.copy_(torch.from_numpy(q))
        wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
        w = wd._w

        def closest():
            ctx.check(lib.psm_world_intersect_dev(w, p_rays, size, p_hits, p_geom), "psm_world_intersect_dev")

        def point():
            ctx.check(lib.psm_world_closest_point_dev(w, p_pts, size, p_hits, p_geom), "psm_world_closest_point_dev")

        def first(k):
            return lambda: ctx.check(lib.psm_world_first_hits_dev(w, p_rays, size, C.c_uint32(k), p_rows, p_inst, p_count), "psm_world_first_hits_dev")

        def near(k):
            return lambda: ctx.check(lib.psm_world_nearest_dev(w, p_pts, size, C.c_uint32(k), p_rows, p_inst, p_count), "psm_world_nearest_dev")

        def emulation(k):
            def run():
                for j in range(k):
                    closest()
                    if j + 1 < k:
                        rays[:, 3] = torch.nextafter(hits[:, 2], inf)
                rays[:, 3] = 0.0
            return run

        tag = "poses%d" % poses_n
        ctx.check(lib.psm_world_count_hits_dev(w, p_rays, size, p_count), "psm_world_count_hits_dev")
        out[tag + "_mean_hits"] = round(float(count.float().mean().item()), 2)
        for k in (1, 4, 16):
            a, b = abab(ctx, first(k), closest)
            out["%s_first_hits_k%d_ms" % (tag, k)], out["%s_intersect_beside_k%d_ms" % (tag, k)] = a, b
            a, b = abab(ctx, first(k), emulation(k))
            out["%s_first_hits_k%d_again_ms" % (tag, k)], out["%s_%dx_intersect_ms" % (tag, k)] = a, b
            a, b = abab(ctx, near(k), point)
            out["%s_nearest_k%d_ms" % (tag, k)], out["%s_closest_point_beside_k%d_ms" % (tag, k)] = a, b
        wd.close()
    th.close()
    ctx.close()
    print(json.dumps(out))


def kbest():
    import torch   # (before the library loads its HIP runtime)
    dev = torch.device("cuda", 0)
    sc = scenes.sponza_like()
    ctx = psm.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)   # torch's tmin update and the launches: one stream
    th = psm.TriangleHierarchy(ctx)
    th.allocate(sc["tris"].shape[0])
    th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
    th.build()
    rt = psm.Pipeline(ctx, seed=1000)
    rt.resizeBuffers(W, H)
    rt.resize(W, H)
    cam = scenes.camera_matrices(sc["eye"], sc["view"], W, H)
    rt.camera_matrices(cam[0], cam[1])
    prim = rt.download_rays()
    rt.close()
    n = prim.shape[0]
    o, d = prim["origin"].copy(), prim["direct"].copy()
    lib = psm.lib()
    size = C.c_size_t(n)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    hits = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    rows = torch.zeros((n, 16, 4), dtype=torch.float32, device=dev)
    count = torch.zeros((n,), dtype=torch.int32, device=dev)
    p_rays, p_hits, p_rows, p_count = (C.c_void_p(x.data_ptr()) for x in (rays, hits, rows, count))
    inf = torch.tensor(float("inf"), device=dev)

    def pack(o, d, tmin):
        r = np.zeros((n, 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, np.inf
        rays.copy_(torch.from_numpy(r))

    def closest():
        ctx.check(lib.psm_bvh_intersect_dev(th._h, p_rays, size, p_hits), "psm_bvh_intersect_dev")

    def counting():
        ctx.check(lib.psm_bvh_count_hits_dev(th._h, p_rays, size, p_count), "psm_bvh_count_hits_dev")

    def first(k):
        return lambda: ctx.check(lib.psm_bvh_first_hits_dev(th._h, p_rays, size, C.c_uint32(k), p_rows, p_count), "psm_bvh_first_hits_dev")

    def emulation(k, tmin0):
        def run():
            for j in range(k):
                closest()
                if j + 1 < k:
                    rays[:, 3] = torch.nextafter(hits[:, 2], inf)
            rays[:, 3] = tmin0
        return run

    out = {"rays": n, "points": NPTS, "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    pack(o, d, 0.0)
    closest()
    ctx.sync()
    bo, bd = bounce_rays(sc, o, d, hits.cpu().numpy())
    for name, (ro, rd, tmin0) in (("primary", (o, d, 0.0)), ("bounce", (bo, bd, 1e-3))):
        pack(ro, rd, tmin0)
        out[name + "_intersect_ms"], out[name + "_count_hits_ms"] = abab(ctx, closest, counting)
        out[name + "_mean_hits"] = round(float(count.float().mean().item()), 2)
        for k in (1, 4, 16):
            a, b = abab(ctx, first(k), closest)
            out["%s_first_hits_k%d_ms" % (name, k)], out["%s_intersect_beside_k%d_ms" % (name, k)] = a, b
            a, b = abab(ctx, first(k), emulation(k, tmin0))
            out["%s_first_hits_k%d_again_ms" % (name, k)], out["%s_%dx_intersect_ms" % (name, k, )] = a, b

    tris = sc["tris"].reshape(-1, 3, 3)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.RandomState(7)
    m = min(NPTS, n)
    w = rng.dirichlet([1, 1, 1], m).astype(np.float32)
    surf = np.einsum("ij,ijk->ik", w, tris[rng.randint(0, tris.shape[0], m)])
    sets = {"surface_noise": (surf + rng.normal(0, 0.01 * diag, (m, 3))).astype(np.float32),
            "uniform": rng.uniform(lo, hi, (m, 3)).astype(np.float32)}
    msize = C.c_size_t(m)
    out["points"] = m
    for name, pts in sets.items():
        q = np.empty((m, 4), np.float32)
        q[:, 0:3], q[:, 3] = pts, np.inf
        rays.view(-1, 4)[:m].copy_(torch.from_numpy(q))

        def point():
            ctx.check(lib.psm_bvh_closest_point_dev(th._h, p_rays, msize, p_hits), "psm_bvh_closest_point_dev")
        for k in (1, 4, 16):
            a, b = abab(ctx, lambda: ctx.check(lib.psm_bvh_nearest_dev(th._h, p_rays, msize, C.c_uint32(k), p_rows, p_count),
                                               "psm_bvh_nearest_dev"), point)
            out["%s_nearest_k%d_ms" % (name, k)], out["%s_closest_point_beside_k%d_ms" % (name, k)] = a, b
    th.close()
    ctx.close()
    print(json.dumps(out))


def boxes():
    lib = psm.lib()
    out = {"reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    stress_tris = int(os.environ.get("STRESS_TRIS", "10000000"))
    for scene_name, sc in (("sponza", scenes.sponza_like()), ("stress", scenes.stress(stress_tris))):
        ctx = psm.Context(0)
        th = psm.TriangleHierarchy(ctx)
        th.allocate(sc["tris"].shape[0])
        th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
        th.build()
        v = sc["tris"].reshape(-1, 3)
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        out[scene_name + "_tris"] = int(th.info().leaf_count)
        for g in (64, 128):
            n = g ** 3
            idx = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)
            cell = (hi - lo) / g
            b = np.zeros((n, 8), np.float32)
            b[:, 0:3], b[:, 4:7] = lo + idx * cell, lo + (idx + 1) * cell
            q = np.zeros((n, 4), np.float32)
            q[:, 0:3], q[:, 3] = lo + (idx + 0.5) * cell, 0.5 * float(np.linalg.norm(cell))
            hs = [ctx.buf_alloc(x) for x in (32 * n, 16 * n, n, 4 * n, 4 * 16 * n)]
            p_box, p_pts, p_flag, p_count, p_rows = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
            ctx.buf_upload(hs[0], b)
            ctx.buf_upload(hs[1], q)
            size = C.c_size_t(n)

            def within():
                ctx.check(lib.psm_bvh_within_dev(th._h, p_pts, size, p_flag), "psm_bvh_within_dev")

            def overlaps():
                ctx.check(lib.psm_bvh_box_overlaps_dev(th._h, p_box, size, p_flag), "psm_bvh_box_overlaps_dev")

            def count():
                ctx.check(lib.psm_bvh_box_count_dev(th._h, p_box, size, p_count), "psm_bvh_box_count_dev")

            def triangles(k):
                return lambda: ctx.check(lib.psm_bvh_box_triangles_dev(th._h, p_box, size, C.c_uint32(k), p_rows, p_count),
                                         "psm_bvh_box_triangles_dev")
            key = "%s_%d_" % (scene_name, g)
            for name, fn in (("overlaps", overlaps), ("count", count), ("triangles_k4", triangles(4)), ("triangles_k16", triangles(16))):
                out[key + name + "_ms"], out[key + "within_beside_" + name + "_ms"] = abab(ctx, fn, within)
            within()
            sphere = float(ctx.buf_download(hs[2], np.uint8, n).mean())
            overlaps()
            out[key + "within_fraction"], out[key + "overlaps_fraction"] = round(sphere, 4), round(float(ctx.buf_download(hs[2], np.uint8, n).mean()), 4)
            count()
            out[key + "mean_count"] = round(float(ctx.buf_download(hs[3], np.uint32, n).mean()), 2)
            for h in hs:
                ctx.buf_free(h)
        # one box around half the scene (the lower half along x)
        hb, hc = ctx.buf_alloc(32), ctx.buf_alloc(16)
        b = np.zeros((1, 8), np.float32)
        b[0, 0:3], b[0, 4:7] = lo, [0.5 * (lo[0] + hi[0]), hi[1], hi[2]]
        ctx.buf_upload(hb, b)
        p_b, p_c = C.c_void_p(ctx.buf_ptr(hb)[0]), C.c_void_p(ctx.buf_ptr(hc)[0])
        out[scene_name + "_half_scene_count_ms"] = round(median_ms(ctx, lambda: ctx.check(lib.psm_bvh_box_count_dev(th._h, p_b, C.c_size_t(1), p_c),
                                                                                        "psm_bvh_box_count_dev")), 4)
        out[scene_name + "_half_scene_count"] = int(ctx.buf_download(hc, np.uint32, 1)[0])
        ctx.buf_free(hb)
        ctx.buf_free(hc)
        th.close()
        ctx.close()
    print(json.dumps(out))


def triangles():
    lib = psm.lib()
    out = {"mode": "triangles", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    stress_tris = int(os.environ.get("STRESS_TRIS", "10000000"))
    nu, nv = int(os.environ.get("TRI_TORUS_NU", "512")), int(os.environ.get("TRI_TORUS_NV", "256"))
    slanted = int(os.environ.get("TRI_SLANTED", "4096"))
    for scene_name, sc in (("sponza", scenes.sponza_like()), ("stress", scenes.stress(stress_tris))):
        ctx = psm.Context(0)
        th = psm.TriangleHierarchy(ctx)
        th.allocate(sc["tris"].shape[0])
        th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
        th.build()
        v = sc["tris"].reshape(-1, 3)
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        centre, ext = 0.5 * (lo + hi), hi - lo
        out[scene_name + "_tris"] = int(th.info().leaf_count)
        rng = np.random.RandomState(11)
        # a second mesh cutting through the scene: a torus around the vertical axis through the centre, tilted
        R = 0.25 * float(ext.max())
        t = torus(nu, nv, R, 0.4 * R).reshape(-1, 3).astype(np.float64)
        tilt = np.array([[1, 0, 0], [0, np.cos(0.5), -np.sin(0.5)], [0, np.sin(0.5), np.cos(0.5)]])
        mesh = (t @ tilt.T + centre).reshape(-1, 3, 3)
        # scene-sized slanted triangles: the vertices anywhere within a fifth of the extent of a point of the scene
        big = rng.uniform(lo, hi, (slanted, 1, 3)) + rng.uniform(-0.2, 0.2, (slanted, 3, 3)) * ext
        for set_name, q in (("torus", mesh), ("slanted", big)):
            q = q.astype(np.float32)
            n = q.shape[0]
            rec = np.zeros((n, 3, 4), np.float32)
            rec[:, :, 0:3] = q
            b = np.zeros((n, 8), np.float32)
            b[:, 0:3], b[:, 4:7] = q.min(axis=1), q.max(axis=1)
            hs = [ctx.buf_alloc(x) for x in (48 * n, 32 * n, n, 4 * n, 4 * 16 * n)]
            p_tri, p_box, p_flag, p_count, p_rows = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
            ctx.buf_upload(hs[0], rec.reshape(n, 12))
            ctx.buf_upload(hs[1], b)
            size = C.c_size_t(n)

            def overlaps():
                ctx.check(lib.psm_bvh_tri_overlaps_dev(th._h, p_tri, size, p_flag), "psm_bvh_tri_overlaps_dev")

            def count():
                ctx.check(lib.psm_bvh_tri_count_dev(th._h, p_tri, size, p_count), "psm_bvh_tri_count_dev")

            def tri_rows(k):
                return lambda: ctx.check(lib.psm_bvh_tri_triangles_dev(th._h, p_tri, size, C.c_uint32(k), p_rows, p_count),
                                         "psm_bvh_tri_triangles_dev")

            def box_count():
                ctx.check(lib.psm_bvh_box_count_dev(th._h, p_box, size, p_count), "psm_bvh_box_count_dev")

            def box_rows(k):
                return lambda: ctx.check(lib.psm_bvh_box_triangles_dev(th._h, p_box, size, C.c_uint32(k), p_rows, p_count),
                                         "psm_bvh_box_triangles_dev")
            key = "%s_%s_" % (scene_name, set_name)
            out[key + "queries"] = n
            for name, fn, beside, other in (("overlaps", overlaps, "box_count", box_count), ("count", count, "box_count", box_count),
                                            ("triangles_k4", tri_rows(4), "box_triangles_k4", box_rows(4)),
                                            ("triangles_k16", tri_rows(16), "box_triangles_k16", box_rows(16))):
                out[key + name + "_ms"], out[key + beside + "_beside_" + name + "_ms"] = abab(ctx, fn, other)
            overlaps()
            out[key + "overlaps_fraction"] = round(float(ctx.buf_download(hs[2], np.uint8, n).mean()), 4)
            count()
            tri_total = float(ctx.buf_download(hs[3], np.uint32, n).astype(np.float64).sum())
            box_count()
            box_counts = ctx.buf_download(hs[3], np.uint32, n)
            out[key + "box_reports_fraction"] = round(float((box_counts > 0).mean()), 4)
            out[key + "mean_count"], out[key + "box_mean_count"] = round(tri_total / n, 3), round(float(box_counts.mean()), 3)
            out[key + "box_count_over_count"] = round(float(box_counts.astype(np.float64).sum()) / max(tri_total, 1.0), 2)
            for h in hs:
                ctx.buf_free(h)
        th.close()
        ctx.close()
    print(json.dumps(out))


def clearance():
    lib = psm.lib()
    out = {"mode": "clearance", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    stress_tris = int(os.environ.get("STRESS_TRIS", "10000000"))
    nu, nv = int(os.environ.get("TRI_TORUS_NU", "512")), int(os.environ.get("TRI_TORUS_NV", "256"))
    slanted = int(os.environ.get("TRI_SLANTED", "4096"))
    small = float(os.environ.get("CLEAR_RMAX", "0.01"))
    names = os.environ.get("CLEAR_SCENES", "sponza,stress").split(",")
    for scene_name in names:
        sc = scenes.sponza_like() if scene_name == "sponza" else scenes.stress(stress_tris)
        ctx = psm.Context(0)
        th = psm.TriangleHierarchy(ctx)
        th.allocate(sc["tris"].shape[0])
        th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
        th.build()
        v = sc["tris"].reshape(-1, 3)
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        centre, ext = 0.5 * (lo + hi), hi - lo
        out[scene_name + "_tris"] = int(th.info().leaf_count)
        rng = np.random.RandomState(11)
        R = 0.25 * float(ext.max())                                   # the triangles mode's two query sets
        t = torus(nu, nv, R, 0.4 * R).reshape(-1, 3).astype(np.float64)
        tilt = np.array([[1, 0, 0], [0, np.cos(0.5), -np.sin(0.5)], [0, np.sin(0.5), np.cos(0.5)]])
        mesh = (t @ tilt.T + centre).reshape(-1, 3, 3)
        big = rng.uniform(lo, hi, (slanted, 1, 3)) + rng.uniform(-0.2, 0.2, (slanted, 3, 3)) * ext
        for set_name, q in (("torus", mesh), ("slanted", big)):
            q = q.astype(np.float32)
            n = q.shape[0]
            hs = [ctx.buf_alloc(x) for x in (48 * n, 16 * n, 32 * n, n, 4 * n)]
            p_tri, p_pts, p_hits, p_flag, p_count = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
            size = C.c_size_t(n)

            def closest():
                ctx.check(lib.psm_bvh_tri_closest_dev(th._h, p_tri, size, p_hits), "psm_bvh_tri_closest_dev")

            def within():
                ctx.check(lib.psm_bvh_tri_within_dev(th._h, p_tri, size, p_flag), "psm_bvh_tri_within_dev")

            def count():   # (reads the same records: rmax lies where psm_tri_query has a pad)
                ctx.check(lib.psm_bvh_tri_count_dev(th._h, p_tri, size, p_count), "psm_bvh_tri_count_dev")

            def point():
                ctx.check(lib.psm_bvh_closest_point_dev(th._h, p_pts, size, p_hits), "psm_bvh_closest_point_dev")
            for r_name, rmax in (("inf", np.inf), ("small", small * float(np.linalg.norm(ext)))):
                rec = np.zeros((n, 3, 4), np.float32)
                rec[:, :, 0:3] = q
                rec[:, 0, 3] = rmax
                pts = np.empty((n, 4), np.float32)
                pts[:, 0:3], pts[:, 3] = q.mean(axis=1), rmax
                ctx.buf_upload(hs[0], rec.reshape(n, 12))
                ctx.buf_upload(hs[1], pts)
                key = "%s_%s_rmax_%s_" % (scene_name, set_name, r_name)
                out[key + "queries"], out[key + "rmax"] = n, (None if np.isinf(rmax) else round(float(rmax), 5))
                out[key + "closest_ms"], out[key + "tri_count_beside_closest_ms"] = abab(ctx, closest, count)
                out[key + "within_ms"], out[key + "closest_point_beside_within_ms"] = abab(ctx, within, point)
                closest()
                hits = ctx.buf_download(hs[2], np.float32, 8 * n).reshape(n, 8)
                found = hits.view(np.int32)[:, 3] >= 0
                out[key + "found_fraction"] = round(float(found.mean()), 4)
                out[key + "at_distance_0_fraction"] = round(float((hits[:, 2] == 0).mean()), 4)
                out[key + "mean_dist_over_diagonal"] = round(float(hits[found, 2].mean() / np.linalg.norm(ext)), 5) if found.any() else None
                within()
                assert np.array_equal(ctx.buf_download(hs[3], np.uint8, n).astype(bool), found)
            for h in hs:
                ctx.buf_free(h)
        th.close()
        ctx.close()
    print(json.dumps(out))


def meshclearance():
    import torch
    lib = psm.lib()
    out = {"mode": "meshclearance", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    stress_tris = int(os.environ.get("STRESS_TRIS", "10000000"))
    tor = torus(48, 24, 0.7, 0.25).reshape(-1, 3, 3)
    rng = np.random.RandomState(17)

    def hier(ctx, tris):
        th = psm.TriangleHierarchy(ctx)
        th.allocate(tris.shape[0])
        th.loadTriangles(np.ascontiguousarray(tris, np.float32).reshape(-1, 9))
        th.build()
        return th

    def rotation():
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    for scene_name in os.environ.get("CLEAR_SCENES", "sponza,stress").split(","):
        sc = scenes.sponza_like() if scene_name == "sponza" else scenes.stress(stress_tris)
        tris = sc["tris"].reshape(-1, 3, 3)
        ctx = psm.Context(0)
        v = tris.reshape(-1, 3)
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        ext = hi - lo
        scale = 0.25 * float(ext.max()) / 1.9
        otris = (tor.astype(np.float64) * scale).astype(np.float32)
        th = hier(ctx, tris)
        out[scene_name + "_tris"] = int(th.info().leaf_count)
        r_small = 0.01 * float(np.linalg.norm(ext))
        t = otris.shape[0]
        for other_name, other in (("torus", hier(ctx, otris)), ("hollow", hier(ctx, np.repeat(otris[:, :1], 3, axis=1)))):
            for p in (1, 1024):
                rng.seed(2000 + p)
                at = v[rng.choice(v.shape[0], p)].astype(np.float64)
                off = rng.normal(size=(p, 3))
                off *= (rng.uniform(0, 2 * 0.95 * scale, p) / np.linalg.norm(off, axis=1))[:, None]
                poses = np.stack([np.concatenate([rotation(), c.reshape(3, 1)], axis=1) for c in at + off]).astype(np.float32)
                m12 = np.ascontiguousarray(poses.reshape(p, 12))
                hs = [ctx.buf_alloc(x) for x in (32 * p, max(p, 16), max(p, 16))]
                p_pair, p_flag, p_cut = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
                all_hits = torch.empty((p, t, 8), dtype=torch.float32, device=torch.device("cuda", ctx.device))
                np_, pm, inf = C.c_size_t(p), m12.ctypes.data_as(C.c_void_p), C.c_float(np.inf)

                def clearance(bound=None):
                    def run():
                        if bound is not None:
                            os.environ["PSM_MESH_BOUND"] = bound
                        try:
                            ctx.check(lib.psm_bvh_mesh_clearance_dev(th._h, other._h, pm, np_, inf, p_pair), "psm_bvh_mesh_clearance_dev")
                        finally:
                            if bound is not None:
                                del os.environ["PSM_MESH_BOUND"]
                    return run

                def closest_min():
                    ctx.check(lib.psm_bvh_mesh_closest_dev(th._h, other._h, pm, np_, inf, C.c_void_p(all_hits.data_ptr())), "psm_bvh_mesh_closest_dev")
                    ctx.sync()
                    least = all_hits[:, :, 2].min(dim=1)
                    torch.cuda.synchronize()
                    return least

                def within():
                    ctx.check(lib.psm_bvh_mesh_within_dev(th._h, other._h, pm, np_, C.c_float(r_small), p_flag), "psm_bvh_mesh_within_dev")

                def overlaps():
                    ctx.check(lib.psm_bvh_mesh_overlaps_dev(th._h, other._h, pm, np_, p_cut), "psm_bvh_mesh_overlaps_dev")

                def within_forced(skip):
                    def run():
                        os.environ["PSM_MESH_SKIP"] = skip
                        try:
                            within()
                        finally:
                            del os.environ["PSM_MESH_SKIP"]
                    return run
                key = "%s_%s_p%d_" % (scene_name, other_name, p)
                out[key + "queries"] = p * int(other.info().leaf_count)
                out[key + "clearance_bound_off_ms"], out[key + "clearance_bound_on_ms"] = abab(ctx, clearance("0"), clearance("1"))
                if other_name == "torus":
                    out[key + "clearance_on_again_ms"], out[key + "clearance_begin_only_ms"] = abab(ctx, clearance("1"), clearance("2"))
                    out[key + "clearance_on_third_ms"], out[key + "clearance_publish_late_ms"] = abab(ctx, clearance("1"), clearance("3"))
                out[key + "clearance_ms"], out[key + "closest_plus_torch_min_ms"] = abab(ctx, clearance(), closest_min)
                out[key + "within_1pct_ms"], out[key + "overlaps_ms"] = abab(ctx, within, overlaps)
                if other_name == "torus":
                    out[key + "within_skip_ms"], out[key + "within_no_skip_ms"] = abab(ctx, within_forced("1"), within_forced("0"))
                clearance()()
                ctx.sync()
                pair = ctx.buf_download(hs[0], np.float32, 8 * p).reshape(p, 8)
                least = closest_min()
                out[key + "equal"] = bool(np.array_equal(pair[:, 2], least.values.cpu().numpy()))   # (the tests hold the whole record)
                out[key + "at_distance_0_fraction"] = round(float((pair[:, 2] == 0).mean()), 4)
                out[key + "mean_dist_over_diagonal"] = round(float(pair[:, 2].mean() / np.linalg.norm(ext)), 5) if np.isfinite(pair[:, 2]).all() else None
                within()
                ctx.sync()
                out[key + "within_fraction"] = round(float(ctx.buf_download(hs[1], np.uint8, p).mean()), 4)
                del all_hits
                for h in hs:
                    ctx.buf_free(h)
            other.close()
        th.close()
        ctx.close()
    print(json.dumps(out))


def posed(src, poses):
    """the query triangles [p, t, 3, 3] of the stored (v0, e1, e2) of src [t, 3, 3] at poses [p, 3, 4], in float32 in the
    library's operation order (psm_hip.h "mesh queries"): (b) and (c) then ask exactly what (a) asks"""
    m = poses[:, None]
    v0, e1, e2 = src[None, :, 0], (src[:, 1] - src[:, 0])[None], (src[:, 2] - src[:, 0])[None]

    def vec(d):
        return np.stack([(m[..., k, 0] * d[..., 0] + m[..., k, 1] * d[..., 1]) + m[..., k, 2] * d[..., 2] for k in range(3)], axis=-1)
    a = vec(v0) + m[..., 3]
    return np.stack([a, a + vec(e1), a + vec(e2)], axis=2)


def meshes():
    lib = psm.lib()
    out = {"mode": "meshes", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    tor = torus(48, 24, 0.7, 0.25).reshape(-1, 3, 3)
    sp = scenes.sponza_like()
    rng = np.random.RandomState(13)

    def hier(ctx, tris):
        th = psm.TriangleHierarchy(ctx)
        th.allocate(tris.shape[0])
        th.loadTriangles(np.ascontiguousarray(tris, np.float32).reshape(-1, 9))
        th.build()
        return th

    def rotation():
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    for scene_name, tris in (("sponza", sp["tris"].reshape(-1, 3, 3)), ("torus", tor)):
        ctx = psm.Context(0)
        v = tris.reshape(-1, 3)
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        ext = hi - lo
        # the other mesh: the torus, a quarter of the scene's extent across (the torus against itself: as it is)
        scale = 1.0 if scene_name == "torus" else 0.25 * float(ext.max()) / 1.9
        otris = (tor.astype(np.float64) * scale).astype(np.float32)
        th = hier(ctx, tris)
        out[scene_name + "_tris"] = int(th.info().leaf_count)
        # the other mesh as the torus is made (strips: a load order that is already coherent), and with its triangles shuffled (a
        # load order that says nothing about place: what the Morton order of the lane mapping is there for)
        for order, otris in (("", otris), ("shuffled_", otris[np.random.RandomState(14).permutation(otris.shape[0])])):
            other = hier(ctx, otris)
            t = otris.shape[0]
            # as many triangles, none a leaf: a mesh query of it uploads, waits and clears as the real one does and launches no
            # kernel -- what a call costs beside the triangle queries on records that are already packed and resident
            hollow = hier(ctx, np.repeat(otris[:, :1], 3, axis=1))
            out[scene_name + "_other_tris"] = int(other.info().leaf_count)
            for p in (1, 64, 1024):
                # poses at which the meshes cut: the other mesh turned at random, its centre on a vertex of the queried mesh
                # (the same poses for either load order of the other mesh)
                rng.seed(1000 + p)
                at = v[rng.choice(v.shape[0], p)].astype(np.float64)
                poses = np.stack([np.concatenate([rotation(), c.reshape(3, 1)], axis=1) for c in at]).astype(np.float32)
                m12 = np.ascontiguousarray(poses.reshape(p, 12))
                n = p * t
                hs = [ctx.buf_alloc(x) for x in (48 * n, max(p, 16), 4 * n, 4 * 16 * n, 4 * n)]
                p_tri, p_flag, p_count, p_rows, p_count2 = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
                size, np_, pm = C.c_size_t(n), C.c_size_t(p), m12.ctypes.data_as(C.c_void_p)

                def pack():
                    src = other.download(psm.BVH_POSITIONS, np.float32, 9 * t).reshape(t, 3, 3)   # the other mesh, from the device
                    rec = np.zeros((p, t, 3, 4), np.float32)
                    rec[:, :, :, 0:3] = posed(src, poses)
                    return rec.reshape(n, 12)
                ctx.buf_upload(hs[0], pack())

                def mesh_overlaps():
                    ctx.check(lib.psm_bvh_mesh_overlaps_dev(th._h, other._h, pm, np_, p_flag), "psm_bvh_mesh_overlaps_dev")

                def forced(skip):
                    def run():
                        os.environ["PSM_MESH_SKIP"] = skip
                        try:
                            mesh_overlaps()
                        finally:
                            del os.environ["PSM_MESH_SKIP"]
                    return run

                def mesh_count():
                    ctx.check(lib.psm_bvh_mesh_count_dev(th._h, other._h, pm, np_, p_count), "psm_bvh_mesh_count_dev")

                def mesh_rows():
                    ctx.check(lib.psm_bvh_mesh_triangles_dev(th._h, other._h, pm, np_, C.c_uint32(16), p_rows, p_count), "psm_bvh_mesh_triangles_dev")

                def count_overhead():
                    ctx.check(lib.psm_bvh_mesh_count_dev(th._h, hollow._h, pm, np_, p_count), "psm_bvh_mesh_count_dev")

                def tri_overlaps():
                    ctx.check(lib.psm_bvh_tri_overlaps_dev(th._h, p_tri, size, p_count2), "psm_bvh_tri_overlaps_dev")

                def tri_count():
                    ctx.check(lib.psm_bvh_tri_count_dev(th._h, p_tri, size, p_count2), "psm_bvh_tri_count_dev")

                def tri_rows():
                    ctx.check(lib.psm_bvh_tri_triangles_dev(th._h, p_tri, size, C.c_uint32(16), p_rows, p_count2), "psm_bvh_tri_triangles_dev")

                def full_path():
                    ctx.buf_upload(hs[0], pack())
                    tri_count()
                key = "%s_%sp%d_" % (scene_name, order, p)
                out[key + "queries"] = n
                # (overlaps: the per-triangle flags of (b) are n bytes, the per-pose flags of (a) p bytes: (b) answers more)
                for name, fa, beside, fb in (("mesh_count", mesh_count, "tri_count", tri_count), ("mesh_overlaps", mesh_overlaps, "tri_overlaps", tri_overlaps),
                                             ("mesh_triangles_k16", mesh_rows, "tri_triangles_k16", tri_rows),
                                             ("mesh_count_again", mesh_count, "tri_count_again", tri_count),
                                             ("mesh_overlaps_skip", forced("1"), "mesh_overlaps_no_skip", forced("0"))):
                    out[key + name + "_ms"], out[key + beside + "_ms"] = abab(ctx, fa, fb)
                out[key + "mesh_count_overhead_ms"] = round(median_ms(ctx, count_overhead), 4)
                if n <= 64 * 2304 and not order:   # (the numpy posing of 2.4 M triangles takes seconds: the point is made at 1 and 64 poses)
                    out[key + "mesh_count_beside_full_path_ms"], out[key + "full_path_ms"] = abab(ctx, mesh_count, full_path)
                mesh_count()
                mine = ctx.buf_download(hs[2], np.uint32, n)
                tri_count()
                theirs = ctx.buf_download(hs[4], np.uint32, n)
                out[key + "equal"] = bool(np.array_equal(mine, theirs))
                mesh_overlaps()
                out[key + "poses_that_cut"] = round(float(ctx.buf_download(hs[1], np.uint8, p).mean()), 4)
                out[key + "triangles_that_meet"], out[key + "mean_count"] = round(float((mine > 0).mean()), 4), round(float(mine.mean()), 3)
                for h in hs:
                    ctx.buf_free(h)
            other.close()
            hollow.close()
        th.close()
        ctx.close()
    print(json.dumps(out))


def sweeps():
    lib = psm.lib()
    out = {"mode": "sweeps", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    stress_tris = int(os.environ.get("STRESS_TRIS", "10000000"))
    want = int(os.environ.get("SWEEP_N", "2000000"))
    for scene_name, sc in (("sponza", scenes.sponza_like()), ("stress", scenes.stress(stress_tris))):
        ctx = psm.Context(0)
        th = psm.TriangleHierarchy(ctx)
        th.allocate(sc["tris"].shape[0])
        th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
        th.build()
        rt = psm.Pipeline(ctx, seed=1000)
        rt.resizeBuffers(W, H)
        rt.resize(W, H)
        cam = scenes.camera_matrices(sc["eye"], sc["view"], W, H)
        rt.camera_matrices(cam[0], cam[1])
        prim = rt.download_rays()
        rt.close()
        n = min(want, prim.shape[0])
        pick = np.linspace(0, prim.shape[0] - 1, n).astype(np.int64)     # spread over the image, in order
        v = sc["tris"].reshape(-1, 3)
        diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0).astype(np.float64)))
        out[scene_name + "_tris"], out[scene_name + "_sweeps"], out[scene_name + "_diagonal"] = int(th.info().leaf_count), n, round(diag, 3)
        q = np.zeros((n, 8), np.float32)
        q[:, 0:3], q[:, 4:7], q[:, 7] = prim["origin"][pick], prim["direct"][pick], np.inf
        hs = [ctx.buf_alloc(x) for x in (32 * n, 32 * n, 16 * n, n)]
        p_rays, p_sweeps, p_hits, p_flag = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
        ctx.buf_upload(hs[0], q)                                         # the rays: tmin = 0 where the sweeps' radius is
        size = C.c_size_t(n)

        def intersect():
            ctx.check(lib.psm_bvh_intersect_dev(th._h, p_rays, size, p_hits), "psm_bvh_intersect_dev")

        def occluded():
            ctx.check(lib.psm_bvh_occluded_dev(th._h, p_rays, size, p_flag), "psm_bvh_occluded_dev")

        def sweep():
            ctx.check(lib.psm_bvh_sweep_sphere_dev(th._h, p_sweeps, size, p_hits), "psm_bvh_sweep_sphere_dev")

        def sweep_any():
            ctx.check(lib.psm_bvh_sweep_occluded_dev(th._h, p_sweeps, size, p_flag), "psm_bvh_sweep_occluded_dev")
        intersect()
        out[scene_name + "_ray_hit_fraction"] = round(float(np.isfinite(ctx.buf_download(hs[2], np.float32, 4 * n).reshape(n, 4)[:, 2]).mean()), 4)
        for pct in (0.1, 1.0, 5.0):
            q[:, 3] = 0.01 * pct * diag
            ctx.buf_upload(hs[1], q)
            key = "%s_r%g_" % (scene_name, pct)
            out[key + "sweep_ms"], out[key + "intersect_ms"] = abab(ctx, sweep, intersect)
            out[key + "sweep_occluded_ms"], out[key + "occluded_ms"] = abab(ctx, sweep_any, occluded)
            out[key + "sweep_over_intersect"] = round(out[key + "sweep_ms"] / out[key + "intersect_ms"], 2)
            out[key + "sweep_occluded_over_occluded"] = round(out[key + "sweep_occluded_ms"] / out[key + "occluded_ms"], 2)
            sweep()
            t = ctx.buf_download(hs[2], np.float32, 4 * n).reshape(n, 4)[:, 2]
            out[key + "hit_fraction"], out[key + "t0_fraction"] = round(float(np.isfinite(t).mean()), 4), round(float((t == 0).mean()), 4)
        for h in hs:
            ctx.buf_free(h)
        th.close()
        ctx.close()
    print(json.dumps(out))


def worldboxes():
    lib = psm.lib()
    ctx = psm.Context(0)
    tor = torus(48, 24, 0.7, 0.25)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tor.shape[0])
    th.loadTriangles(tor)
    th.build()
    rng = np.random.RandomState(1)
    g = 64
    n = g ** 3
    idx = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)
    out = {"mode": "worldboxes", "grid": g, "queries": n, "torus_triangles": int(tor.shape[0]), "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    hs = [ctx.buf_alloc(x) for x in (32 * n, 16 * n, n, 4 * n, 4 * 16 * n, 4 * 16 * n)]
    p_box, p_pts, p_flag, p_count, p_rows, p_inst = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
    size = C.c_size_t(n)
    for poses_n in (256, 4096):
        side = int(np.ceil(np.sqrt(poses_n)))      # the world mode's grid of poses, each turned about a random axis
        poses = np.zeros((poses_n, 3, 4), np.float32)
        k_ = np.arange(poses_n)
        for j in range(poses_n):
            q, r = np.linalg.qr(rng.normal(size=(3, 3)))
            poses[j, :, :3] = q * np.sign(np.diag(r))
        poses[:, 0, 3], poses[:, 1, 3] = 2.5 * (k_ % side), 2.5 * (k_ // side)
        lo = np.array([-1.25, -1.25, -1.25])
        hi = np.array([2.5 * (side - 1) + 1.25, 2.5 * ((poses_n - 1) // side) + 1.25, 1.25])
        cell = (hi - lo) / g
        b = np.zeros((n, 8), np.float32)
        b[:, 0:3], b[:, 4:7] = lo + idx * cell, lo + (idx + 1) * cell
        q = np.zeros((n, 4), np.float32)
        q[:, 0:3], q[:, 3] = lo + (idx + 0.5) * cell, 0.5 * float(np.linalg.norm(cell))
        ctx.buf_upload(hs[0], b)
        ctx.buf_upload(hs[1], q)
        wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
        w = wd._w

        def within():
            ctx.check(lib.psm_world_within_dev(w, p_pts, size, p_flag), "psm_world_within_dev")

        def overlaps():
            ctx.check(lib.psm_world_box_overlaps_dev(w, p_box, size, p_flag), "psm_world_box_overlaps_dev")

        def count():
            ctx.check(lib.psm_world_box_count_dev(w, p_box, size, p_count), "psm_world_box_count_dev")

        def triangles(k):
            return lambda: ctx.check(lib.psm_world_box_triangles_dev(w, p_box, size, C.c_uint32(k), p_rows, p_inst, p_count),
                                     "psm_world_box_triangles_dev")
        key = "poses%d_" % poses_n
        for name, fn in (("overlaps", overlaps), ("count", count), ("triangles_k4", triangles(4)), ("triangles_k16", triangles(16))):
            out[key + name + "_ms"], out[key + "within_beside_" + name + "_ms"] = abab(ctx, fn, within)
        within()
        sphere = float(ctx.buf_download(hs[2], np.uint8, n).mean())
        overlaps()
        out[key + "within_fraction"], out[key + "overlaps_fraction"] = round(sphere, 4), round(float(ctx.buf_download(hs[2], np.uint8, n).mean()), 4)
        count()
        out[key + "mean_count"] = round(float(ctx.buf_download(hs[3], np.uint32, n).mean()), 2)
        # one box around half the world (the lower half along x)
        hb, hc = ctx.buf_alloc(32), ctx.buf_alloc(16)
        one = np.zeros((1, 8), np.float32)
        one[0, 0:3], one[0, 4:7] = lo, [0.5 * (lo[0] + hi[0]), hi[1], hi[2]]
        ctx.buf_upload(hb, one)
        p_b, p_c = C.c_void_p(ctx.buf_ptr(hb)[0]), C.c_void_p(ctx.buf_ptr(hc)[0])
        out[key + "half_world_count_ms"] = round(median_ms(ctx, lambda: ctx.check(lib.psm_world_box_count_dev(w, p_b, C.c_size_t(1), p_c),
                                                                                "psm_world_box_count_dev")), 4)
        out[key + "half_world_count"] = int(ctx.buf_download(hc, np.uint32, 1)[0])
        ctx.buf_free(hb)
        ctx.buf_free(hc)
        wd.close()
    for h in hs:
        ctx.buf_free(h)
    th.close()
    ctx.close()
    print(json.dumps(out))


def worldtriangles():
    lib = psm.lib()
    ctx = psm.Context(0)
    tor = torus(48, 24, 0.7, 0.25)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tor.shape[0])
    th.loadTriangles(tor)
    th.build()
    rng = np.random.RandomState(1)
    bodies, slanted = int(os.environ.get("WTRI_BODIES", "64")), int(os.environ.get("WTRI_SLANTED", "4096"))
    out = {"mode": "worldtriangles", "torus_triangles": int(tor.shape[0]), "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}

    def turn():
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        return q * np.sign(np.diag(r))
    for poses_n in (256, 4096):
        side = int(np.ceil(np.sqrt(poses_n)))      # the worldboxes mode's world: a grid of poses, each turned about a random axis
        poses = np.zeros((poses_n, 3, 4), np.float32)
        k_ = np.arange(poses_n)
        for j in range(poses_n):
            poses[j, :, :3] = turn()
        poses[:, 0, 3], poses[:, 1, 3] = 2.5 * (k_ % side), 2.5 * (k_ // side)
        lo = np.array([-1.25, -1.25, -1.25])
        hi = np.array([2.5 * (side - 1) + 1.25, 2.5 * ((poses_n - 1) // side) + 1.25, 1.25])
        wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
        w = wd._w
        # a second torus posed `bodies` times: turned, and set half a radius beside a body of the world, so the two meshes cut
        mesh = []
        for j in rng.choice(poses_n, bodies, replace=False):
            at = poses[j, :, 3].astype(np.float64) + rng.uniform(-0.5, 0.5, 3)
            mesh.append(tor.reshape(-1, 3).astype(np.float64) @ turn().T + at)
        mesh = np.concatenate(mesh).reshape(-1, 3, 3)
        # body-sized slanted triangles: the vertices anywhere within a body's radius of a point of the world
        big = rng.uniform(lo, hi, (slanted, 1, 3)) + rng.uniform(-1.0, 1.0, (slanted, 3, 3))
        for set_name, q in (("torus", mesh), ("slanted", big)):
            q = q.astype(np.float32)
            n = q.shape[0]
            rec = np.zeros((n, 3, 4), np.float32)
            rec[:, :, 0:3] = q
            b = np.zeros((n, 8), np.float32)
            b[:, 0:3], b[:, 4:7] = q.min(axis=1), q.max(axis=1)
            hs = [ctx.buf_alloc(x) for x in (48 * n, 32 * n, n, 4 * n, 4 * 16 * n, 4 * 16 * n)]
            p_tri, p_box, p_flag, p_count, p_rows, p_inst = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
            ctx.buf_upload(hs[0], rec.reshape(n, 12))
            ctx.buf_upload(hs[1], b)
            size = C.c_size_t(n)

            def overlaps():
                ctx.check(lib.psm_world_tri_overlaps_dev(w, p_tri, size, p_flag), "psm_world_tri_overlaps_dev")

            def count():
                ctx.check(lib.psm_world_tri_count_dev(w, p_tri, size, p_count), "psm_world_tri_count_dev")

            def tri_rows(k):
                return lambda: ctx.check(lib.psm_world_tri_triangles_dev(w, p_tri, size, C.c_uint32(k), p_rows, p_inst, p_count),
                                         "psm_world_tri_triangles_dev")

            def box_count():
                ctx.check(lib.psm_world_box_count_dev(w, p_box, size, p_count), "psm_world_box_count_dev")

            def box_rows(k):
                return lambda: ctx.check(lib.psm_world_box_triangles_dev(w, p_box, size, C.c_uint32(k), p_rows, p_inst, p_count),
                                         "psm_world_box_triangles_dev")
            key = "poses%d_%s_" % (poses_n, set_name)
            out[key + "queries"] = n
            for name, fn, beside, other in (("overlaps", overlaps, "box_count", box_count), ("count", count, "box_count", box_count),
                                            ("triangles_k4", tri_rows(4), "box_triangles_k4", box_rows(4)),
                                            ("triangles_k16", tri_rows(16), "box_triangles_k16", box_rows(16))):
                out[key + name + "_ms"], out[key + beside + "_beside_" + name + "_ms"] = abab(ctx, fn, other)
            overlaps()
            out[key + "overlaps_fraction"] = round(float(ctx.buf_download(hs[2], np.uint8, n).mean()), 4)
            count()
            tri_total = float(ctx.buf_download(hs[3], np.uint32, n).astype(np.float64).sum())
            box_count()
            box_counts = ctx.buf_download(hs[3], np.uint32, n)
            out[key + "box_reports_fraction"] = round(float((box_counts > 0).mean()), 4)
            out[key + "mean_count"], out[key + "box_mean_count"] = round(tri_total / n, 3), round(float(box_counts.mean()), 3)
            out[key + "box_count_over_count"] = round(float(box_counts.astype(np.float64).sum()) / max(tri_total, 1.0), 2)
            for h in hs:
                ctx.buf_free(h)
        wd.close()
    th.close()
    ctx.close()
    print(json.dumps(out))


def worldclearance():
    out = {"mode": "world-clearance", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    n = int(os.environ.get("WCLEAR_QUERIES", str(1 << 16)))
    small = float(os.environ.get("WCLEAR_RMAX", "0.01"))
    counts = [int(x) for x in os.environ.get("WCLEAR_POSES", "1,64,1024").split(",")]
    for scene_name in os.environ.get("WCLEAR_SCENES", "sponza,torus").split(","):
        tris = (scenes.sponza_like()["tris"] if scene_name == "sponza" else torus(48, 24, 0.7, 0.25)).reshape(-1, 3, 3).astype(np.float32)
        ctx = psm.Context(0)
        th = psm.TriangleHierarchy(ctx)
        th.allocate(tris.shape[0])
        th.loadTriangles(np.ascontiguousarray(tris.reshape(-1, 9)))
        th.build()
        out[scene_name + "_tris"] = int(th.info().leaf_count)
        v = tris.reshape(-1, 3).astype(np.float64)
        centre, radius = 0.5 * (v.min(0) + v.max(0)), 0.5 * float(np.linalg.norm(v.max(0) - v.min(0)))
        rng = np.random.RandomState(23)
        for poses_n in counts:
            side = int(np.ceil(np.sqrt(poses_n)))       # a grid of poses a body's diameter apart, each turned about a random axis
            poses = np.zeros((poses_n, 3, 4))
            for j in range(poses_n):
                q_, r_ = np.linalg.qr(rng.normal(size=(3, 3)))
                rot = q_ * np.sign(np.diag(r_))
                poses[j, :, :3] = rot
                poses[j, :, 3] = np.array([2.0 * radius * (j % side), 2.0 * radius * (j // side), 0.0]) - rot @ centre
            poses = poses.astype(np.float32)
            lo = np.array([-radius, -radius, -radius])
            hi = np.array([2.0 * radius * (side - 1) + radius, 2.0 * radius * ((poses_n - 1) // side) + radius, radius])
            q = (rng.uniform(lo, hi, (n, 1, 3)) + rng.uniform(-0.05, 0.05, (n, 3, 3)) * radius).astype(np.float32)
            wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
            reps = REPS if poses_n < 1024 else 1
            p64 = poses.astype(np.float64)

            def loop(rmax, flag):
                """what a caller had: per instance, the queries moved by R^T (x - T) on the host, triClosest, the host minimum"""
                best, who = np.full(n, np.inf, np.float32), np.full(n, -1, np.int32)
                for j in range(poses_n):
                    moved = ((q.astype(np.float64) - p64[j, :, 3]) @ p64[j, :, :3]).astype(np.float32)
                    d = th.triClosest(moved, rmax).dist
                    nearer = d < best
                    best, who = np.where(nearer, d, best), np.where(nearer, j, who).astype(np.int32)
                return (who >= 0) if flag else (best, who)

            def abab_n(fa, fb):
                """medians (ms) of the two whole calls, alternated A B A B after a warm-up call of each, and their last results"""
                ra, rb = fa(), fb()
                ta, tb = [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    ra = fa()
                    t1 = time.perf_counter()
                    rb = fb()
                    t2 = time.perf_counter()
                    ta.append((t1 - t0) * 1e3)
                    tb.append((t2 - t1) * 1e3)
                return round(float(np.median(ta)), 3), round(float(np.median(tb)), 3), ra, rb
            for rname, rmax in (("inf", np.inf), ("small", small * 2.0 * radius)):
                key = "%s_poses%d_rmax_%s_" % (scene_name, poses_n, rname)
                print("world-clearance: " + key[:-1], file=sys.stderr, flush=True)   # (a case of the loop takes minutes)
                a, b, got, (best, who) = abab_n(lambda: wd.closestToTriangle(q, rmax), lambda: loop(rmax, False))
                out[key + "closest_ms"], out[key + "loop_ms"], out[key + "loop_over_closest"] = a, b, round(b / a, 2)
                a, b, flags, loop_flags = abab_n(lambda: wd.withinOfTriangle(q, rmax), lambda: loop(rmax, True))
                out[key + "within_ms"], out[key + "within_loop_ms"], out[key + "loop_over_within"] = a, b, round(b / a, 2)
                both = (got.tri >= 0) & (who >= 0)
                out[key + "found_fraction"] = round(float((got.tri >= 0).mean()), 4)
                out[key + "found_by_one_alone"] = int(((got.tri >= 0) != (who >= 0)).sum())
                out[key + "within_differs"] = int((flags != loop_flags).sum())
                out[key + "largest_dist_difference"] = float(np.abs(got.dist[both] - best[both]).max()) if both.any() else 0.0
                out[key + "same_instance_fraction"] = round(float((got.geom[both] == who[both]).mean()), 4) if both.any() else 1.0
            out["%s_poses%d_reps" % (scene_name, poses_n)] = reps
            wd.close()
        th.close()
        ctx.close()
    print(json.dumps(out))


def worldmeshclearance():
    out = {"mode": "world-mesh-clearance", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    counts = [int(x) for x in os.environ.get("WMCLEAR_INSTANCES", "1,64,1024").split(",")]
    pose_counts = [int(x) for x in os.environ.get("WMCLEAR_POSES", "1,1024").split(",")]
    slow = float(os.environ.get("WMCLEAR_SLOW", "1.5"))
    log = os.environ.get("WMCLEAR_LOG")
    tor = torus(48, 24, 0.7, 0.25).reshape(-1, 3, 3)

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def abab_n(fa, fb):
        """medians (ms) of the two whole calls, alternated A B A B after a warm-up call of each -- the warm-up call alone where it
        took more than `slow` seconds on either side -- their last results and the timed calls per side"""
        (wa, ra), (wb, rb) = timed(fa), timed(fb)
        if max(wa, wb) > slow * 1e3:
            return round(wa, 3), round(wb, 3), ra, rb, 1
        ta, tb = [], []
        for _ in range(REPS):
            a, ra = timed(fa)
            b, rb = timed(fb)
            ta.append(a)
            tb.append(b)
        return round(float(np.median(ta)), 3), round(float(np.median(tb)), 3), ra, rb, REPS

    for scene_name in os.environ.get("WMCLEAR_SCENES", "torus,sponza").split(","):
        tris = (scenes.sponza_like()["tris"] if scene_name == "sponza" else tor).reshape(-1, 3, 3).astype(np.float32)
        ctx = psm.Context(0)

        def hier(t):
            th = psm.TriangleHierarchy(ctx)
            th.allocate(t.shape[0])
            th.loadTriangles(np.ascontiguousarray(t.reshape(-1, 9), np.float32))
            th.build()
            return th
        th = hier(tris)
        out[scene_name + "_tris"] = int(th.info().leaf_count)
        v = tris.reshape(-1, 3).astype(np.float64)
        centre, radius = 0.5 * (v.min(0) + v.max(0)), 0.5 * float(np.linalg.norm(v.max(0) - v.min(0)))
        otris = (tor.astype(np.float64) * (0.25 * 2.0 * radius / 1.9)).astype(np.float32)
        other = hier(otris)
        t = otris.shape[0]
        rng = np.random.RandomState(29)
        for insts_n in counts:
            side = int(np.ceil(np.sqrt(insts_n)))       # world-clearance's grid: a body's diameter apart, each turned about a random axis
            ip = np.zeros((insts_n, 3, 4))
            for j in range(insts_n):
                q_, r_ = np.linalg.qr(rng.normal(size=(3, 3)))
                rot = q_ * np.sign(np.diag(r_))
                ip[j, :, :3] = rot
                ip[j, :, 3] = np.array([2.0 * radius * (j % side), 2.0 * radius * (j // side), 0.0]) - rot @ centre
            wd = psm.InstanceWorld(ctx, [(th, m) for m in ip.astype(np.float32)])
            lo = np.array([-radius, -radius, -radius])
            hi = np.array([2.0 * radius * (side - 1) + radius, 2.0 * radius * ((insts_n - 1) // side) + radius, radius])
            for p in pose_counts:
                poses = np.zeros((p, 3, 4))
                for j in range(p):
                    q_, r_ = np.linalg.qr(rng.normal(size=(3, 3)))
                    poses[j, :, :3] = q_ * np.sign(np.diag(r_))
                    poses[j, :, 3] = rng.uniform(lo, hi)
                poses = poses.astype(np.float32)
                for rname, rmax in (("inf", np.inf), ("small", 0.01 * 2.0 * radius)):
                    key = "%s_inst%d_p%d_rmax_%s_" % (scene_name, insts_n, p, rname)
                    print("world-mesh-clearance: " + key[:-1], file=sys.stderr, flush=True)

                    def clearance(bound=None):
                        def run():
                            if bound is not None:
                                os.environ["PSM_MESH_BOUND"] = bound
                            try:
                                return wd.clearanceToMesh(other, poses, rmax)
                            finally:
                                if bound is not None:
                                    del os.environ["PSM_MESH_BOUND"]
                        return run

                    def before():
                        """the parent's path: pose on the host, closestToTriangle over p x T triangles, the minimum on the host"""
                        got = wd.closestToTriangle(posed(otris, poses).reshape(-1, 3, 3), rmax)
                        dist = got.dist.reshape(p, t)
                        best = np.argmin(dist, axis=1)          # (the first of equal minima: the lowest t)
                        r = np.arange(p)
                        return dist[r, best], got.tri.reshape(p, t)[r, best], np.where(np.isfinite(dist[r, best]), best, -1), got.geom.reshape(p, t)[r, best]
                    row = {}
                    a, b, got, (dist, tri, best, inst), n1 = abab_n(clearance(), before)
                    row["clearance_ms"], row["before_ms"], row["before_over_clearance"], row["timed_calls"] = a, b, round(b / a, 2), n1
                    a, b, _, off, n2 = abab_n(clearance(), clearance("0"))
                    row["clearance_again_ms"], row["bound_off_ms"], row["bound_off_over_clearance"], row["timed_calls_bound"] = a, b, round(b / a, 2), n2
                    row["agree"] = bool(np.array_equal(got.dist, dist) and np.array_equal(got.tri, tri) and np.array_equal(got.other, best)
                                        and np.array_equal(got.geom, inst) and np.array_equal(off.buffer.view(np.uint32), got.buffer.view(np.uint32))
                                        and np.array_equal(off.geom, got.geom))
                    row["found_fraction"] = round(float((got.tri >= 0).mean()), 4)
                    row["at_distance_0_fraction"] = round(float((got.dist == 0).mean()), 4)
                    for k_, x in row.items():
                        out[key + k_] = x
                    if log:
                        with open(log, "a") as fh:
                            fh.write(json.dumps({key[:-1]: row}) + "\n")
            wd.close()
        other.close()
        th.close()
        ctx.close()
    print(json.dumps(out))


def worldmeshes():
    lib = psm.lib()
    ctx = psm.Context(0)
    tor = torus(48, 24, 0.7, 0.25).reshape(-1, 3, 3)
    rng = np.random.RandomState(17)
    out = {"mode": "worldmeshes", "torus_triangles": int(tor.shape[0]), "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}

    def hier(tris):
        th = psm.TriangleHierarchy(ctx)
        th.allocate(tris.shape[0])
        th.loadTriangles(np.ascontiguousarray(tris, np.float32).reshape(-1, 9))
        th.build()
        return th

    def turn():
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        return q * np.sign(np.diag(r))
    # the worldtriangles mode's world (4 096 turned grid poses of the torus), and the Sponza-class scene as a world of one
    poses_n = 4096
    side = int(np.ceil(np.sqrt(poses_n)))
    grid = np.zeros((poses_n, 3, 4), np.float32)
    k_ = np.arange(poses_n)
    for j in range(poses_n):
        grid[j, :, :3] = turn()
    grid[:, 0, 3], grid[:, 1, 3] = 2.5 * (k_ % side), 2.5 * (k_ // side)
    sp = scenes.sponza_like()["tris"].reshape(-1, 3, 3)
    identity = np.eye(3, 4, dtype=np.float32)
    for world_name, tris, world_poses in (("torus4096", tor, grid), ("sponza", sp, identity[None])):
        member = hier(tris)
        wd = psm.InstanceWorld(ctx, [(member, m) for m in world_poses])
        w = wd._w
        v = tris.reshape(-1, 3)
        # the other mesh: the torus as it is against the world of tori, a quarter of the scene's extent across against the scene
        scale = 1.0 if world_name != "sponza" else 0.25 * float((v.max(0) - v.min(0)).max()) / 1.9
        otris = (tor.astype(np.float64) * scale).astype(np.float32)
        other = hier(otris)
        t = otris.shape[0]
        # as many triangles, none a leaf: a call on it checks, uploads, waits and clears as the real one does and launches no kernel
        hollow = hier(np.repeat(otris[:, :1], 3, axis=1))
        out[world_name + "_instances"], out[world_name + "_member_tris"] = len(wd), int(member.info().leaf_count)
        out[world_name + "_other_tris"] = int(other.info().leaf_count)
        src = other.download(psm.BVH_POSITIONS, np.float32, 9 * t).reshape(t, 3, 3)
        for p in (1, 64, 1024):
            # poses at which the meshes cut: the other mesh turned at random, its centre half a radius beside a body of the world
            # (the scene: on one of its vertices)
            rng.seed(2000 + p)
            if world_name == "sponza":
                at = v[rng.choice(v.shape[0], p)].astype(np.float64)
            else:
                at = world_poses[rng.choice(poses_n, p, replace=False), :, 3].astype(np.float64) + rng.uniform(-0.5, 0.5, (p, 3))
            poses = np.stack([np.concatenate([turn(), c.reshape(3, 1)], axis=1) for c in at]).astype(np.float32)
            m12 = np.ascontiguousarray(poses.reshape(p, 12))
            n = p * t
            hs = [ctx.buf_alloc(x) for x in (48 * n, max(p, 16), max(n, 16), 4 * n, 4 * 16 * n, 4 * 16 * n, 4 * n)]
            p_tri, p_flag, p_flags, p_count, p_rows, p_inst, p_count2 = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
            size, np_, pm, none = C.c_size_t(n), C.c_size_t(p), m12.ctypes.data_as(C.c_void_p), C.c_int32(-1)
            rec = np.zeros((p, t, 3, 4), np.float32)
            rec[:, :, :, 0:3] = posed(src, poses)
            ctx.buf_upload(hs[0], rec.reshape(n, 12))

            def mesh_overlaps():
                ctx.check(lib.psm_world_mesh_overlaps_dev(w, other._h, pm, np_, none, p_flag), "psm_world_mesh_overlaps_dev")

            def mesh_count():
                ctx.check(lib.psm_world_mesh_count_dev(w, other._h, pm, np_, none, p_count), "psm_world_mesh_count_dev")

            def mesh_rows():
                ctx.check(lib.psm_world_mesh_triangles_dev(w, other._h, pm, np_, none, C.c_uint32(16), p_rows, p_inst, p_count), "psm_world_mesh_triangles_dev")

            def overhead(fn_name, *outs):
                fn = getattr(lib, fn_name)
                return lambda: ctx.check(fn(w, hollow._h, pm, np_, none, *outs), fn_name)

            def tri_overlaps():
                ctx.check(lib.psm_world_tri_overlaps_dev(w, p_tri, size, p_flags), "psm_world_tri_overlaps_dev")

            def tri_count():
                ctx.check(lib.psm_world_tri_count_dev(w, p_tri, size, p_count2), "psm_world_tri_count_dev")

            def tri_rows():
                ctx.check(lib.psm_world_tri_triangles_dev(w, p_tri, size, C.c_uint32(16), p_rows, p_inst, p_count2), "psm_world_tri_triangles_dev")
            key = "%s_p%d_" % (world_name, p)
            out[key + "queries"] = n
            # (a) and (b) alternated A B A B, (b) twice per case: its two medians give the spread between runs
            for name, fa, fb, fo in (("count", mesh_count, tri_count, overhead("psm_world_mesh_count_dev", p_count)),
                                     ("overlaps", mesh_overlaps, tri_overlaps, overhead("psm_world_mesh_overlaps_dev", p_flag)),
                                     ("triangles_k16", mesh_rows, tri_rows, overhead("psm_world_mesh_triangles_dev", C.c_uint32(16), p_rows, p_inst, p_count))):
                a1, b1 = abab(ctx, fa, fb)
                a2, b2 = abab(ctx, fa, fb)
                out[key + name + "_a_ms"], out[key + name + "_b_ms"] = [a1, a2], [b1, b2]
                out[key + name + "_overhead_ms"] = round(median_ms(ctx, fo), 4)
            mesh_count()
            mine = ctx.buf_download(hs[3], np.uint32, n)
            tri_count()
            theirs = ctx.buf_download(hs[6], np.uint32, n)
            out[key + "equal"] = bool(np.array_equal(mine, theirs))
            mesh_overlaps()
            out[key + "poses_that_cut"] = round(float(ctx.buf_download(hs[1], np.uint8, p).mean()), 4)
            out[key + "triangles_that_meet"], out[key + "mean_count"] = round(float((mine > 0).mean()), 4), round(float(mine.mean()), 3)
            for h in hs:
                ctx.buf_free(h)
        wd.close()
        for th in (other, hollow, member):
            th.close()
    ctx.close()
    print(json.dumps(out))


def worldsweeps():
    lib = psm.lib()
    ctx = psm.Context(0)
    tor = torus(48, 24, 0.7, 0.25)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tor.shape[0])
    th.loadTriangles(tor)
    th.build()
    rng = np.random.RandomState(1)
    n = int(os.environ.get("WORLD_SWEEP_N", "262144"))
    out = {"mode": "worldsweeps", "queries": n, "torus_triangles": int(tor.shape[0]), "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    hs = [ctx.buf_alloc(x) for x in (32 * n, 32 * n, 16 * n, 4 * n, n)]
    p_rays, p_sweeps, p_hits, p_inst, p_flag = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
    size = C.c_size_t(n)
    for poses_n in (256, 4096):
        side = int(np.ceil(np.sqrt(poses_n)))      # the worldboxes mode's world: a grid of poses, each turned about a random axis
        poses = np.zeros((poses_n, 3, 4), np.float32)
        k_ = np.arange(poses_n)
        for j in range(poses_n):
            q, r = np.linalg.qr(rng.normal(size=(3, 3)))
            poses[j, :, :3] = q * np.sign(np.diag(r))
        poses[:, 0, 3], poses[:, 1, 3] = 2.5 * (k_ % side), 2.5 * (k_ // side)
        lo = np.array([-1.25, -1.25, -1.25])
        hi = np.array([2.5 * (side - 1) + 1.25, 2.5 * ((poses_n - 1) // side) + 1.25, 1.25])
        diag = float(np.linalg.norm(hi - lo))
        # rays through the world: from a point of its box grown by a fifth towards a point inside it
        grow = 0.2 * (hi - lo)
        start = rng.uniform(lo - grow, hi + grow, (n, 3))
        aim = rng.uniform(lo, hi, (n, 3))
        q = np.zeros((n, 8), np.float32)
        q[:, 0:3], q[:, 4:7], q[:, 7] = start, aim - start, np.inf
        ctx.buf_upload(hs[0], q)                   # the rays: tmin = 0 where the sweeps' radius is
        wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
        w = wd._w

        def intersect():
            ctx.check(lib.psm_world_intersect_dev(w, p_rays, size, p_hits, p_inst), "psm_world_intersect_dev")

        def occluded():
            ctx.check(lib.psm_world_occluded_dev(w, p_rays, size, p_flag), "psm_world_occluded_dev")

        def sweep():
            ctx.check(lib.psm_world_sweep_sphere_dev(w, p_sweeps, size, p_hits, p_inst), "psm_world_sweep_sphere_dev")

        def sweep_any():
            ctx.check(lib.psm_world_sweep_occluded_dev(w, p_sweeps, size, p_flag), "psm_world_sweep_occluded_dev")
        key = "poses%d_" % poses_n
        out[key + "diagonal"] = round(diag, 3)
        intersect()
        out[key + "ray_hit_fraction"] = round(float(np.isfinite(ctx.buf_download(hs[2], np.float32, 4 * n).reshape(n, 4)[:, 2]).mean()), 4)
        for pct in (0.1, 1.0, 5.0):
            q[:, 3] = 0.01 * pct * diag
            ctx.buf_upload(hs[1], q)
            kr = "%sr%g_" % (key, pct)
            out[kr + "sweep_ms"], out[kr + "intersect_ms"] = abab(ctx, sweep, intersect)
            out[kr + "sweep_occluded_ms"], out[kr + "occluded_ms"] = abab(ctx, sweep_any, occluded)
            out[kr + "sweep_over_intersect"] = round(out[kr + "sweep_ms"] / out[kr + "intersect_ms"], 2)
            out[kr + "sweep_occluded_over_occluded"] = round(out[kr + "sweep_occluded_ms"] / out[kr + "occluded_ms"], 2)
            sweep()
            t = ctx.buf_download(hs[2], np.float32, 4 * n).reshape(n, 4)[:, 2]
            out[kr + "hit_fraction"], out[kr + "t0_fraction"] = round(float(np.isfinite(t).mean()), 4), round(float((t == 0).mean()), 4)
        wd.close()
    for h in hs:
        ctx.buf_free(h)
    th.close()
    ctx.close()
    print(json.dumps(out))


def grids():
    import torch   # (before the library loads its HIP runtime)
    dev = torch.device("cuda", 0)
    lib = psm.lib()
    sc = scenes.sponza_like()
    ctx = psm.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)   # torch's packing and the launches: one stream
    th = psm.TriangleHierarchy(ctx)
    th.allocate(sc["tris"].shape[0])
    th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
    th.build()
    v = sc["tris"].reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    out = {"mode": "grids", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH), "tris": int(th.info().leaf_count)}
    for g in (int(x) for x in os.environ.get("GRID_SIZES", "64,128,256").split(",")):
        origin, cell, dims = lo, (hi - lo) / g, (g, g, g)
        n = g ** 3
        grid = psm._grid(origin, cell, dims)
        words = torch.zeros(((g + 3) // 4,) * 3, dtype=torch.int64, device=dev)
        counts = torch.zeros((g, g, g), dtype=torch.int32, device=dev)
        p_words, p_counts = C.c_void_p(words.data_ptr()), C.c_void_p(counts.data_ptr())

        def surface():
            ctx.check(lib.psm_grid_surface_dev(th._h, C.byref(grid), p_words), "psm_grid_surface_dev")

        def count():
            ctx.check(lib.psm_grid_counts_dev(th._h, C.byref(grid), p_counts), "psm_grid_counts_dev")

        def solid():
            ctx.check(lib.psm_grid_solid_dev(th._h, C.byref(grid), C.c_uint32(3), p_words), "psm_grid_solid_dev")

        # the parent's way to the same bits: boxOverlaps over the voxels' boxes -- (1) the kernel alone over records that are
        # resident, (2) the package's torch call over resident lo / hi (it packs the records on the device), (3) the same
        # from host arrays: the upload of 24 bytes per voxel included
        blo, bhi = psm.voxel_boxes(origin, cell, dims)
        tlo, thi = torch.from_numpy(blo).to(dev), torch.from_numpy(bhi).to(dev)
        records = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        records[:, 0:3], records[:, 4:7] = tlo, thi
        flags = torch.zeros((n,), dtype=torch.uint8, device=dev)
        p_rec, p_flags, size = C.c_void_p(records.data_ptr()), C.c_void_p(flags.data_ptr()), C.c_size_t(n)

        def box_kernel():
            ctx.check(lib.psm_bvh_box_overlaps_dev(th._h, p_rec, size, p_flags), "psm_bvh_box_overlaps_dev")

        def box_torch():
            return th.boxOverlaps(tlo, thi)

        def box_upload():
            return th.boxOverlaps(torch.from_numpy(blo).to(dev), torch.from_numpy(bhi).to(dev))

        key = "g%d_" % g
        out[key + "voxels"] = n
        out[key + "surface_ms"], out[key + "box_overlaps_kernel_ms"] = abab(ctx, surface, box_kernel)
        out[key + "surface_again_ms"], out[key + "box_overlaps_torch_ms"] = abab(ctx, surface, box_torch)
        out[key + "surface_third_ms"], out[key + "box_overlaps_with_upload_ms"] = abab(ctx, surface, box_upload)
        box_counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        p_box_counts = C.c_void_p(box_counts.data_ptr())

        def box_count_kernel():
            ctx.check(lib.psm_bvh_box_count_dev(th._h, p_rec, size, p_box_counts), "psm_bvh_box_count_dev")

        out[key + "counts_ms"], out[key + "box_count_kernel_ms"] = abab(ctx, count, box_count_kernel)
        surface()
        vg = psm.VoxelGrid(words.clone(), dims, tuple(grid.origin), tuple(grid.cell))
        out[key + "solid_ms"] = round(median_ms(ctx, solid), 4)
        filled = psm.VoxelGrid(words, dims, tuple(grid.origin), tuple(grid.cell))
        out[key + "occupied"], out[key + "occupied_solid"] = vg.occupied(), filled.occupied()
        box_kernel()
        out[key + "same_bits"] = bool(torch.equal(vg.dense().reshape(-1), flags.view(torch.bool)) and torch.equal(counts.reshape(-1), box_counts))
        out[key + "surface_over_box_kernel"] = round(out[key + "surface_ms"] / out[key + "box_overlaps_kernel_ms"], 3)
    th.close()
    ctx.close()
    print(json.dumps(out))


def distgrids():
    """the distance-field grids against the point queries over voxel_centres() of the same grid"""
    import torch   # (before the library loads its HIP runtime)
    dev = torch.device("cuda", 0)
    lib = psm.lib()
    sc = scenes.sponza_like()
    ctx = psm.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)   # torch's packing and the launches: one stream
    th = psm.TriangleHierarchy(ctx)
    th.allocate(sc["tris"].shape[0])
    th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
    th.build()
    v = sc["tris"].reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    out = {"mode": "distgrids", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH), "tris": int(th.info().leaf_count)}
    for g in (int(x) for x in os.environ.get("GRID_SIZES", "64,128,256").split(",")):
        origin, cell, dims = lo, (hi - lo) / g, (g, g, g)
        n = g ** 3
        grid = psm._grid(origin, cell, dims)
        dist = torch.zeros((g, g, g), dtype=torch.float32, device=dev)
        tri = torch.zeros((g, g, g), dtype=torch.int32, device=dev)
        p_dist, p_tri = C.c_void_p(dist.data_ptr()), C.c_void_p(tri.data_ptr())
        centres = psm.voxel_centres(origin, cell, dims)
        tcentres = torch.from_numpy(centres).to(dev)
        records = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        records[:, 0:3] = tcentres
        hits = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        p_rec, p_hits, size = C.c_void_p(records.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_size_t(n)
        out["g%d_voxels" % g] = n
        band = 2.0 * float(np.linalg.norm(np.array(grid.cell, np.float64)))
        for rname, rmax in (("inf", float("inf")), ("band", band)):
            records[:, 3] = rmax
            r32 = C.c_float(rmax)
            for sname, samples in (("dist", None), ("signed", 3)):

                def field():
                    if samples is None:
                        ctx.check(lib.psm_grid_distance_dev(th._h, C.byref(grid), r32, p_dist, p_tri), "psm_grid_distance_dev")
                    else:
                        ctx.check(lib.psm_grid_signed_distance_dev(th._h, C.byref(grid), r32, C.c_uint32(samples), p_dist, p_tri),
                                  "psm_grid_signed_distance_dev")

                # the parent's way to the same bits: the point query over the voxels' centres -- (1) the entry point alone over
                # records that are resident, (2) the package's torch call over resident centres (it packs the records on the
                # device), (3) the same from host arrays: the upload of 12 bytes per voxel included
                def point_kernel():
                    if samples is None:
                        ctx.check(lib.psm_bvh_closest_point_dev(th._h, p_rec, size, p_hits), "psm_bvh_closest_point_dev")
                    else:
                        ctx.check(lib.psm_bvh_signed_distance_dev(th._h, p_rec, size, C.c_uint32(samples), p_hits), "psm_bvh_signed_distance_dev")

                def point_torch(c=None):
                    c = tcentres if c is None else c
                    return th.closestPoint(c, rmax) if samples is None else th.signedDistance(c, rmax, samples)

                def point_upload():
                    return point_torch(torch.from_numpy(centres).to(dev))

                key = "g%d_%s_%s_" % (g, rname, sname)
                out[key + "field_ms"], out[key + "point_kernel_ms"] = abab(ctx, field, point_kernel)
                out[key + "field_again_ms"], out[key + "point_torch_ms"] = abab(ctx, field, point_torch)
                out[key + "field_third_ms"], out[key + "point_with_upload_ms"] = abab(ctx, field, point_upload)
                field()
                point_kernel()
                ctx.sync()
                out[key + "hit_fraction"] = round(float((tri >= 0).float().mean()), 4)
                out[key + "same_bits"] = bool(torch.equal(dist.reshape(-1).view(torch.int32), hits[:, 2].contiguous().view(torch.int32))
                                              and torch.equal(tri.reshape(-1), hits[:, 3].contiguous().view(torch.int32)))
                out[key + "field_over_point_kernel"] = round(out[key + "field_ms"] / out[key + "point_kernel_ms"], 3)
                out[key + "field_over_point_with_upload"] = round(out[key + "field_third_ms"] / out[key + "point_with_upload_ms"], 3)
        del dist, tri, tcentres, records, hits
    th.close()
    ctx.close()
    print(json.dumps(out))


def sparsegrids():
    """the sparse grids (list + fill) against the dense calls of the same tree, with the listing's coarse pass on and off"""
    import torch   # (before the library loads its HIP runtime)
    dev = torch.device("cuda", 0)
    lib = psm.lib()
    sc = scenes.sponza_like()
    ctx = psm.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)   # torch's compares and the launches: one stream
    th = psm.TriangleHierarchy(ctx)
    th.allocate(sc["tris"].shape[0])
    th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
    th.build()
    v = sc["tris"].reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    dense_max = int(os.environ.get("SPARSE_DENSE_MAX", "512"))
    log = os.environ.get("SPARSE_LOG")
    out = {"mode": "sparsegrids", "reps": REPS, "lib": os.path.basename(psm.LIB_PATH), "tris": int(th.info().leaf_count)}

    def coarse(on):
        os.environ["PSM_SPARSE_COARSE"] = "1" if on else "0"   # (read at each call)

    def note(key, values):
        for k, x in values.items():
            out[key + k] = x
        if log:
            with open(log, "a") as f:
                f.write(json.dumps({key + k: x for k, x in values.items()}) + "\n")

    for g in (int(x) for x in os.environ.get("SPARSE_SIZES", "128,256,512,1024").split(",")):
        origin, cell, dims = lo, (hi - lo) / g, (g, g, g)
        grid = psm._grid(origin, cell, dims)
        bricks = int(lib.psm_grid_brick_count(C.byref(grid)))
        count = torch.zeros(4, dtype=torch.int32, device=dev)
        p_count = C.c_void_p(count.data_ptr())
        band = 2.0 * float(np.linalg.norm(np.array(grid.cell, np.float64)))
        cases = [("band", band, False), ("inf", float("inf"), False), ("surface", None, True)]
        for rname, rmax, surface in cases:
            key = "g%d_%s_" % (g, rname)
            if rname == "inf" and g > dense_max:
                note(key, {"skipped": "every brick listed: the sparse output is the dense one plus the ids, %d bytes" % (bricks * 516)})
                continue
            r32 = C.c_float(rmax if rmax is not None else 0.0)

            def lister(capacity, p_ids):
                if surface:
                    ctx.check(lib.psm_grid_sparse_surface_bricks_dev(th._h, C.byref(grid), C.c_uint32(capacity), p_ids, p_count), "psm_grid_sparse_surface_bricks_dev")
                else:
                    ctx.check(lib.psm_grid_sparse_distance_bricks_dev(th._h, C.byref(grid), r32, C.c_uint32(capacity), p_ids, p_count),
                              "psm_grid_sparse_distance_bricks_dev")

            coarse(True)
            lister(0, None)
            ctx.sync()
            n = int(count.cpu()[0])
            ids = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            p_ids = C.c_void_p(ids.data_ptr())
            if surface:
                words = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
                p_a, p_b = C.c_void_p(words.data_ptr()), None
            else:
                sdist = torch.zeros((max(n, 1), 64), dtype=torch.float32, device=dev)
                stri = torch.zeros((max(n, 1), 64), dtype=torch.int32, device=dev)
                p_a, p_b = C.c_void_p(sdist.data_ptr()), C.c_void_p(stri.data_ptr())

            def list_on():
                coarse(True)
                lister(n, p_ids)

            def list_off():
                coarse(False)
                lister(n, p_ids)

            def fill():
                if surface:
                    ctx.check(lib.psm_grid_sparse_surface_dev(th._h, C.byref(grid), p_ids, C.c_uint32(n), p_a), "psm_grid_sparse_surface_dev")
                else:
                    ctx.check(lib.psm_grid_sparse_distance_dev(th._h, C.byref(grid), r32, p_ids, C.c_uint32(n), p_a, p_b), "psm_grid_sparse_distance_dev")

            def both():   # the library's default: the coarse pass on unless rmax = +inf
                list_on()
                fill()

            figures = {"bricks": bricks, "listed": n, "listed_fraction": round(n / bricks, 5),
                       "sparse_bytes": n * (12 if surface else 516), "dense_bytes": bricks * 8 if surface else 8 * g ** 3}
            list_off()
            ids_off = ids.clone()
            list_on()
            figures["same_list_coarse_on_off"] = bool(torch.equal(ids, ids_off))
            figures["list_coarse_ms"], figures["list_plain_ms"] = abab(ctx, list_on, list_off)
            figures["list_coarse_again_ms"], figures["fill_ms"] = abab(ctx, list_on, fill)
            if g <= dense_max:
                if surface:
                    dwords = torch.zeros(bricks, dtype=torch.int64, device=dev)
                    p_dense = C.c_void_p(dwords.data_ptr())

                    def dense():
                        ctx.check(lib.psm_grid_surface_dev(th._h, C.byref(grid), p_dense), "psm_grid_surface_dev")
                else:
                    ddist = torch.zeros((g, g, g), dtype=torch.float32, device=dev)
                    dtri = torch.zeros((g, g, g), dtype=torch.int32, device=dev)
                    p_dense, p_dtri = C.c_void_p(ddist.data_ptr()), C.c_void_p(dtri.data_ptr())

                    def dense():
                        ctx.check(lib.psm_grid_distance_dev(th._h, C.byref(grid), r32, p_dense, p_dtri), "psm_grid_distance_dev")

                # the same bits as the dense call, before any timing of the pair
                both()
                dense()
                ctx.sync()
                shape = (tuple(grid.dims), tuple(grid.origin), tuple(grid.cell))
                if surface:
                    back = psm.SparseVoxelGrid(ids[:n], words[:n], *shape).dense().bricks.reshape(-1)
                    same = bool(torch.equal(back, dwords)) and n == int((dwords != 0).sum())
                else:
                    back = psm.SparseDistanceGrid(ids[:n], sdist[:n].reshape(n, 4, 4, 4), stri[:n].reshape(n, 4, 4, 4), *shape).dense()
                    same = bool(torch.equal(back.dist.view(torch.int32), ddist.view(torch.int32)) and torch.equal(back.tri, dtri))
                    del back
                figures["same_bits"] = same
                figures["sparse_ms"], figures["dense_ms"] = abab(ctx, both, dense)
                figures["dense_again_ms"], figures["dense_third_ms"] = abab(ctx, dense, dense)   # the spread of one side against itself
                figures["sparse_over_dense"] = round(figures["sparse_ms"] / figures["dense_ms"], 3)
                if surface:
                    del dwords
                else:
                    del ddist, dtri
            else:
                figures["sparse_ms"] = round(median_ms(ctx, both), 4)
            note(key, figures)
            del ids
            if surface:
                del words
            else:
                del sdist, stri
            torch.cuda.empty_cache()
    os.environ.pop("PSM_SPARSE_COARSE", None)
    th.close()
    ctx.close()
    print(json.dumps(out))


def worldgrids():
    """the voxel grids over a world against the world's box queries over voxel_boxes() of the same grid"""
    lib = psm.lib()
    ctx = psm.Context(0)
    tor = torus(48, 24, 0.7, 0.25)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tor.shape[0])
    th.loadTriangles(tor)
    th.build()
    rng = np.random.RandomState(1)
    out = {"mode": "worldgrids", "torus_triangles": int(tor.shape[0]), "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    for poses_n in (int(x) for x in os.environ.get("WORLD_GRID_POSES", "256,4096").split(",")):
        side = int(np.ceil(np.sqrt(poses_n)))      # the worldboxes mode's world: a grid of poses, each turned about a random axis
        poses = np.zeros((poses_n, 3, 4), np.float32)
        k_ = np.arange(poses_n)
        for j in range(poses_n):
            q, r = np.linalg.qr(rng.normal(size=(3, 3)))
            poses[j, :, :3] = q * np.sign(np.diag(r))
        poses[:, 0, 3], poses[:, 1, 3] = 2.5 * (k_ % side), 2.5 * (k_ // side)
        lo = np.array([-1.25, -1.25, -1.25])
        hi = np.array([2.5 * (side - 1) + 1.25, 2.5 * ((poses_n - 1) // side) + 1.25, 1.25])
        wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
        w = wd._w
        for g in (int(x) for x in os.environ.get("GRID_SIZES", "64,128,256").split(",")):
            origin, cell, dims = lo, (hi - lo) / g, (g, g, g)
            n = g ** 3
            grid = psm._grid(origin, cell, dims)
            bricks = ((g + 3) // 4) ** 3
            blo, bhi = psm.voxel_boxes(origin, cell, dims)
            rec = np.zeros((n, 8), np.float32)
            rec[:, 0:3], rec[:, 4:7] = blo, bhi
            hs = [ctx.buf_alloc(x) for x in (32 * n, n, 4 * n, 4 * n, 4 * n, 8 * bricks, 4 * n, 4 * n)]
            p_rec, p_flag, p_count, p_row, p_rinst, p_words, p_cells, p_labels = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in hs)
            ctx.buf_upload(hs[0], rec)
            del rec
            size = C.c_size_t(n)

            def surface():
                ctx.check(lib.psm_grid_world_surface_dev(w, C.byref(grid), p_words), "psm_grid_world_surface_dev")

            def counts():
                ctx.check(lib.psm_grid_world_counts_dev(w, C.byref(grid), p_cells), "psm_grid_world_counts_dev")

            def owners():
                ctx.check(lib.psm_grid_world_instances_dev(w, C.byref(grid), p_labels), "psm_grid_world_instances_dev")

            def solid():
                ctx.check(lib.psm_grid_world_solid_dev(w, C.byref(grid), C.c_uint32(3), p_words), "psm_grid_world_solid_dev")

            def box_overlaps():
                ctx.check(lib.psm_world_box_overlaps_dev(w, p_rec, size, p_flag), "psm_world_box_overlaps_dev")

            def box_count():
                ctx.check(lib.psm_world_box_count_dev(w, p_rec, size, p_count), "psm_world_box_count_dev")

            def box_first():
                ctx.check(lib.psm_world_box_triangles_dev(w, p_rec, size, C.c_uint32(1), p_row, p_rinst, p_count), "psm_world_box_triangles_dev")

            key = "poses%d_g%d_" % (poses_n, g)
            out[key + "voxels"] = n
            # (1) the records resident: launch against launch. (2) the whole call from host memory: the grid's nine numbers and
            # the read-back of its answer against voxel_boxes()' records packed, uploaded, queried and read back
            out[key + "surface_ms"], out[key + "overlaps_resident_ms"] = abab(ctx, surface, box_overlaps)
            out[key + "counts_ms"], out[key + "count_resident_ms"] = abab(ctx, counts, box_count)
            out[key + "instances_ms"], out[key + "triangles_k1_resident_ms"] = abab(ctx, owners, box_first)
            out[key + "surface_call_ms"], out[key + "overlaps_with_upload_ms"] = abab(ctx, lambda: wd.voxelize(origin, cell, dims), lambda: wd.overlapsBox(blo, bhi))
            out[key + "counts_call_ms"], out[key + "count_with_upload_ms"] = abab(ctx, lambda: wd.voxelCounts(origin, cell, dims), lambda: wd.countInBox(blo, bhi))
            out[key + "instances_call_ms"], out[key + "triangles_k1_with_upload_ms"] = abab(ctx, lambda: wd.voxelInstances(origin, cell, dims),
                                                                                          lambda: wd.trianglesInBox(blo, bhi, 1))
            surface()
            ctx.sync()
            words = ctx.buf_download(hs[5], np.uint64, bricks).reshape(((g + 3) // 4,) * 3)
            vg = psm.VoxelGrid(words, dims, tuple(grid.origin), tuple(grid.cell))
            out[key + "solid_ms"] = round(median_ms(ctx, solid), 4)
            filled = psm.VoxelGrid(ctx.buf_download(hs[5], np.uint64, bricks).reshape(((g + 3) // 4,) * 3), dims, tuple(grid.origin), tuple(grid.cell))
            out[key + "occupied"], out[key + "occupied_solid"] = vg.occupied(), filled.occupied()
            box_overlaps(); box_count(); counts()
            ctx.sync()
            flags, cells = ctx.buf_download(hs[1], np.uint8, n), ctx.buf_download(hs[6], np.uint32, n)
            same = np.array_equal(vg.dense().reshape(-1), flags.view(np.bool_)) and np.array_equal(cells, ctx.buf_download(hs[2], np.uint32, n))
            box_first(); owners()
            ctx.sync()
            same = same and np.array_equal(ctx.buf_download(hs[7], np.int32, n), ctx.buf_download(hs[4], np.int32, n))
            out[key + "same_answers"] = bool(same)
            out[key + "mean_count"] = round(float(cells.mean()), 3)
            for h in hs:
                ctx.buf_free(h)
        wd.close()
    th.close()
    ctx.close()
    print(json.dumps(out))


def worlddistgrids():
    """the distance-field grids over a world against the world's point queries over voxel_centres() of the same grid"""
    import torch   # (before the library loads its HIP runtime)
    dev = torch.device("cuda", 0)
    lib = psm.lib()
    log = os.environ.get("WORLD_DIST_LOG")
    ctx = psm.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)   # torch's packing and the launches: one stream
    tor = torus(48, 24, 0.7, 0.25)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(tor.shape[0])
    th.loadTriangles(tor)
    th.build()
    rng = np.random.RandomState(1)
    out = {"mode": "worlddistgrids", "torus_triangles": int(tor.shape[0]), "reps": REPS, "lib": os.path.basename(psm.LIB_PATH)}
    for poses_n in (int(x) for x in os.environ.get("WORLD_GRID_POSES", "256,4096").split(",")):
        side = int(np.ceil(np.sqrt(poses_n)))      # the worldgrids mode's world: a grid of poses, each turned about a random axis
        poses = np.zeros((poses_n, 3, 4), np.float32)
        k_ = np.arange(poses_n)
        for j in range(poses_n):
            q, r = np.linalg.qr(rng.normal(size=(3, 3)))
            poses[j, :, :3] = q * np.sign(np.diag(r))
        poses[:, 0, 3], poses[:, 1, 3] = 2.5 * (k_ % side), 2.5 * (k_ // side)
        lo = np.array([-1.25, -1.25, -1.25])
        hi = np.array([2.5 * (side - 1) + 1.25, 2.5 * ((poses_n - 1) // side) + 1.25, 1.25])
        wd = psm.InstanceWorld(ctx, [(th, m) for m in poses])
        w = wd._w
        for g in (int(x) for x in os.environ.get("GRID_SIZES", "64,128,256").split(",")):
            origin, cell, dims = lo, (hi - lo) / g, (g, g, g)
            n = g ** 3
            grid = psm._grid(origin, cell, dims)
            dist = torch.zeros((g, g, g), dtype=torch.float32, device=dev)
            tri = torch.zeros((g, g, g), dtype=torch.int32, device=dev)
            inst = torch.zeros((g, g, g), dtype=torch.int32, device=dev)
            p_dist, p_tri, p_inst = (C.c_void_p(x.data_ptr()) for x in (dist, tri, inst))
            centres = psm.voxel_centres(origin, cell, dims)
            tcentres = torch.from_numpy(centres).to(dev)
            records = torch.zeros((n, 4), dtype=torch.float32, device=dev)
            records[:, 0:3] = tcentres
            hits = torch.zeros((n, 4), dtype=torch.float32, device=dev)
            geom = torch.zeros((n,), dtype=torch.int32, device=dev)
            p_rec, p_hits, p_geom, size = C.c_void_p(records.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(geom.data_ptr()), C.c_size_t(n)
            out["poses%d_g%d_voxels" % (poses_n, g)] = n
            band = 2.0 * float(np.linalg.norm(np.array(grid.cell, np.float64)))
            for rname, rmax in (("inf", float("inf")), ("band", band)):
                records[:, 3] = rmax
                r32 = C.c_float(rmax)
                for sname, samples in (("dist", None), ("signed", 3)):

                    def field():
                        if samples is None:
                            ctx.check(lib.psm_grid_world_distance_dev(w, C.byref(grid), r32, p_dist, p_tri, p_inst), "psm_grid_world_distance_dev")
                        else:
                            ctx.check(lib.psm_grid_world_signed_distance_dev(w, C.byref(grid), r32, C.c_uint32(samples), p_dist, p_tri, p_inst),
                                      "psm_grid_world_signed_distance_dev")

                    # the parent's ways to the same bits: the world's point query over the voxels' centres -- (1) the entry point
                    # alone over records that are resident, (2) the package's torch call over resident centres (it packs the
                    # records on the device), (3) the same from the host array: the upload of 12 bytes per voxel included
                    def point_kernel():
                        if samples is None:
                            ctx.check(lib.psm_world_closest_point_dev(w, p_rec, size, p_hits, p_geom), "psm_world_closest_point_dev")
                        else:
                            ctx.check(lib.psm_world_signed_distance_dev(w, p_rec, size, C.c_uint32(samples), p_hits, p_geom), "psm_world_signed_distance_dev")

                    def point_torch(c=None):
                        c = tcentres if c is None else c
                        return wd.closestPoint(c, rmax) if samples is None else wd.signedDistance(c, rmax, samples)

                    def point_upload():
                        return point_torch(torch.from_numpy(centres).to(dev))

                    key = "poses%d_g%d_%s_%s_" % (poses_n, g, rname, sname)
                    case = {}
                    case[key + "field_ms"], case[key + "point_kernel_ms"] = abab(ctx, field, point_kernel)
                    case[key + "field_again_ms"], case[key + "point_torch_ms"] = abab(ctx, field, point_torch)
                    case[key + "field_third_ms"], case[key + "point_with_upload_ms"] = abab(ctx, field, point_upload)
                    field()
                    point_kernel()
                    ctx.sync()
                    case[key + "hit_fraction"] = round(float((tri >= 0).float().mean()), 4)
                    case[key + "same_bits"] = bool(torch.equal(dist.reshape(-1).view(torch.int32), hits[:, 2].contiguous().view(torch.int32))
                                                   and torch.equal(tri.reshape(-1), hits[:, 3].contiguous().view(torch.int32))
                                                   and torch.equal(inst.reshape(-1), geom))
                    case[key + "field_over_point_kernel"] = round(case[key + "field_ms"] / case[key + "point_kernel_ms"], 3)
                    case[key + "field_over_point_torch"] = round(case[key + "field_again_ms"] / case[key + "point_torch_ms"], 3)
                    case[key + "field_over_point_with_upload"] = round(case[key + "field_third_ms"] / case[key + "point_with_upload_ms"], 3)
                    out.update(case)
                    if log:
                        with open(log, "a") as f:
                            f.write(json.dumps(case) + "\n")
            del dist, tri, inst, tcentres, records, hits, geom
        wd.close()
    th.close()
    ctx.close()
    print(json.dumps(out))


def main():
    sc = scenes.sponza_like()
    ctx = psm.Context(0)
    th = psm.TriangleHierarchy(ctx)
    th.allocate(sc["tris"].shape[0])
    th.loadTriangles(sc["tris"], sc["normals"], sc["mats"])
    th.build()
    rt = psm.Pipeline(ctx, seed=1000)
    rt.resizeBuffers(W, H)
    rt.resize(W, H)
    cam = scenes.camera_matrices(sc["eye"], sc["view"], W, H)
    rt.camera_matrices(cam[0], cam[1])
    prim = rt.download_rays()
    n = prim.shape[0]
    o, d = prim["origin"].copy(), prim["direct"].copy()

    lib = psm.lib()
    h_rays, h_hits, h_occ = ctx.buf_alloc(32 * n), ctx.buf_alloc(16 * n), ctx.buf_alloc(n)
    p_rays, p_hits, p_occ = (C.c_void_p(ctx.buf_ptr(h)[0]) for h in (h_rays, h_hits, h_occ))

    def upload(o, d, tmin):
        r = np.zeros((n, 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, np.inf
        ctx.buf_upload(h_rays, r)

    def closest():
        ctx.check(lib.psm_bvh_intersect_dev(th._h, p_rays, C.c_size_t(n), p_hits), "psm_bvh_intersect_dev")

    def anyhit():
        ctx.check(lib.psm_bvh_occluded_dev(th._h, p_rays, C.c_size_t(n), p_occ), "psm_bvh_occluded_dev")

    out = {"rays": n, "reps": REPS}
    upload(o, d, 0.0)
    out["primary_closest_ms"] = median_ms(ctx, closest)
    out["primary_any_ms"] = median_ms(ctx, anyhit)
    hits = ctx.buf_download(h_hits, np.float32, 4 * n).reshape(n, 4)
    tri = hits.view(np.int32)[:, 3]
    out["primary_hit_fraction"] = float((tri >= 0).mean())

    bo, bd = bounce_rays(sc, o, d, hits)
    upload(bo, bd, 1e-3)
    out["bounce_closest_ms"] = median_ms(ctx, closest)
    out["bounce_any_ms"] = median_ms(ctx, anyhit)

    # the pipeline's traversal of the same primary rays, one launch (WHOLE)
    rt.setTraverseMode("whole")
    rt.upload_rays(prim)

    def pipeline():
        rt.resetHits()
        rt.intersection(th, force=True)

    out["pipeline_whole_ms"] = median_ms(ctx, pipeline)
    for k in ("primary_closest", "primary_any", "bounce_closest", "bounce_any", "pipeline_whole"):
        out[k + "_mrays_s"] = round(n / out[k + "_ms"] / 1e3, 1)
        out[k + "_ms"] = round(out[k + "_ms"], 4)
    for h in (h_rays, h_hits, h_occ):
        ctx.buf_free(h)
    rt.close()
    th.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    {"points": points, "signed": signed, "scene": scene, "instances": instances, "world": world, "kbest": kbest, "worldkbest": worldkbest, "boxes": boxes, "worldboxes": worldboxes, "sweeps": sweeps, "worldsweeps": worldsweeps, "triangles": triangles, "clearance": clearance, "meshes": meshes, "meshclearance": meshclearance, "worldtriangles": worldtriangles, "world-clearance": worldclearance, "world-mesh-clearance": worldmeshclearance, "worldmeshes": worldmeshes, "grids": grids, "distgrids": distgrids, "sparsegrids": sparsegrids, "worldgrids": worldgrids, "worlddistgrids": worlddistgrids}.get(" ".join(sys.argv[1:]), main)()
