"""A numpy float32 restatement of the hit-count, inside / outside and signed-distance queries (psm_bvh_count_hits_dev /
psm_bvh_inside_dev / psm_bvh_signed_distance_dev, include/psm_hip.h; query.hip CountRay), built on the ray queries' model
(query_model: the unclamped triangle test, normalize3, the validity of a ray) and the point queries' (point_query_model), and the
closed meshes the tests ask "inside?" about, each with its analytic answer.

A count is a sum of integers over the candidates, so it is held to the kernels exactly, as are the votes made from it; the signed
hits are the closest-point model's bits with the sign of t set."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import point_query_model as PQ
from query_model import normalize3, ray_valid, tri_test

F = np.float32
# PSM_INSIDE_DIRECTIONS (include/psm_hip.h), restated: the normalised (1, sqrt 2, sqrt 3), (-sqrt 5, 1, sqrt 2), (sqrt 3, -sqrt 7, 1),
# (-sqrt 2, -sqrt 3, -sqrt 11), (sqrt 7, 1, -sqrt 5) as float32 literals. tests/test_inside_query_cpu.py holds the header's and the
# package's tables to this one.
INSIDE_DIRECTIONS = np.array([[0.4082483, 0.57735026, 0.70710677], [-0.7905694, 0.35355338, 0.5],
                              [0.52223295, -0.797724, 0.30151135], [-0.35355338, -0.4330127, -0.8291562],
                              [0.7337994, 0.2773501, -0.6201737]], F)


def _chunks(n_rays, n_tris, budget=1 << 20):
    step = max(1, budget // max(n_tris, 1))
    for a in range(0, n_rays, step):
        yield a, min(n_rays, a + step)


def count(tris, cand, origins, directs, tmin=0.0, tmax=np.inf):
    """psm_bvh_count_hits_dev over the candidate triangle ids `cand` (the hierarchy's leaves): per ray the number of candidates
    the unclamped test accepts with tmin <= t <= tmax as floats; an invalid ray (query_model.ray_valid) counts 0. uint32 [R]."""
    origins = np.asarray(origins, F).reshape(-1, 3)
    d = normalize3(np.asarray(directs, F).reshape(-1, 3))
    R = origins.shape[0]
    lo = np.broadcast_to(np.asarray(tmin, F), (R,)).astype(F)
    hi = np.broadcast_to(np.asarray(tmax, F), (R,)).astype(F)
    cand = np.asarray(cand, np.int64).reshape(-1)
    out = np.zeros(R, np.uint32)
    if cand.size == 0 or R == 0:
        return out
    tris = np.asarray(tris, F).reshape(-1, 3, 3)[cand]
    valid = ray_valid(origins, d, lo, hi)

    def chunk(ab):
        a, b = ab
        t, _, _, ok = tri_test(tris, origins[a:b], d[a:b], clamp=False)
        with np.errstate(invalid="ignore"):
            hit = ok & valid[a:b, None] & (t >= lo[a:b, None]) & (t <= hi[a:b, None])
        out[a:b] = hit.sum(axis=1)

    with ThreadPoolExecutor(max_workers=8) as pool:   # (numpy releases the GIL: ray chunks on a few threads)
        list(pool.map(chunk, _chunks(R, cand.size)))
    return out


def parities(tris, cand, points, samples=5):
    """the votes of psm_bvh_inside_dev one by one: [samples, R] bool, row k = "the count of ray {p, 0, INSIDE_DIRECTIONS[k], +inf}
    is odd" (a non-finite p is an invalid ray: count 0, even)"""
    p = np.asarray(points, F).reshape(-1, 3)
    out = np.zeros((samples, p.shape[0]), bool)
    for k in range(samples):
        d = np.broadcast_to(INSIDE_DIRECTIONS[k], p.shape)
        out[k] = (count(tris, cand, p, d, F(0), F(np.inf)) & 1) == 1
    return out


def vote(par, samples):
    """inside iff more than half of the first `samples` rays vote so"""
    return 2 * par[:samples].sum(axis=0) > samples


def inside(tris, cand, points, samples=3):
    """psm_bvh_inside_dev: bool [R]"""
    assert samples in (1, 3, 5)
    return vote(parities(tris, cand, points, samples), samples)


def signed_distance(tris, cand, points, rmax=np.inf, samples=3):
    """psm_bvh_signed_distance_dev: point_query_model.query's hits [R, 4] with the sign bit of t set where the point found a
    triangle and is inside; a miss stays (0, 0, +inf, -1) and casts no rays"""
    p = np.asarray(points, F).reshape(-1, 3)
    hits, _ = PQ.query(tris, cand, p, rmax)
    found = np.nonzero(hits.view(np.int32)[:, 3] >= 0)[0]
    ins = inside(tris, cand, p[found], samples)
    hits.view(np.uint32)[found[ins], 2] |= np.uint32(0x80000000)
    return hits


# ---- closed meshes with an analytic inside ------------------------------------------------------------------------------------

def icosphere(level=3, radius=1.0, centre=(0.0, 0.0, 0.0), flip=False):
    """an icosahedron subdivided `level` times, vertices on the sphere (20 * 4^level triangles, outward winding; flip: inward).
    float32 [T, 3, 3]; the mesh is watertight: a shared vertex has the same bits in every triangle that uses it."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        nf = []
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    vs = (np.array(v) * radius + np.array(centre, np.float64)).astype(F)
    f = np.array(f)
    if flip:
        f = f[:, ::-1]
    return vs[f]


def torus(nu=48, nv=24, R=1.0, r=0.4):
    """a torus around the z axis (centre circle of radius R, tube radius r), nu x nv quads split in two: 2 nu nv triangles with
    their vertices on the surface, watertight"""
    u = np.arange(nu) * (2 * np.pi / nu)
    w = np.arange(nv) * (2 * np.pi / nv)
    U, W = np.meshgrid(u, w, indexing="ij")
    vs = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).astype(F)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    a, b, c, d = vs[i, j], vs[i1, j], vs[i1, j1], vs[i, j1]
    return np.concatenate([np.stack([a, b, c], -2).reshape(-1, 3, 3), np.stack([a, c, d], -2).reshape(-1, 3, 3)]).astype(F)


def cube():
    """the unit cube [0, 1]^3 as 12 triangles, outward winding"""
    c = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F)   # index = 4 x + 2 y + z
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, cc, d in q:
        f += [(a, b, cc), (a, cc, d)]
    return c[np.array(f)]


def shell(flip_inner):
    """two nested icospheres (radii 1 and 0.5): a shell, where a point in the cavity is outside. Parity does not care which way
    the inner sphere is wound: both are given."""
    return np.concatenate([icosphere(3, 1.0), icosphere(2, 0.5, flip=flip_inner)])


def _sphere_gap(tris, radius):
    """how far an inscribed polyhedron stays inside its sphere: radius - the smallest distance of a face's plane from the centre"""
    t = np.asarray(tris, np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return float(radius - np.abs((n * t[:, 0]).sum(-1)).min())


def torus_distance(p, R=1.0, r=0.4):
    """signed distance of points to the smooth torus (negative inside), float64"""
    p = np.asarray(p, np.float64)
    return np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2) - r


def _torus_gap(tris):
    """the largest distance of the polyhedron's surface from the smooth torus, over a barycentric lattice of 66 points per
    triangle (corners, edges, interior); the faces are within ~(edge^2 / 8 r) of it, so the lattice sees it to a few percent"""
    k = 10
    w = np.array([(i, j, k - i - j) for i in range(k + 1) for j in range(k + 1 - i)], np.float64) / k
    pts = np.einsum("sw,twc->tsc", w, np.asarray(tris, np.float64))
    return float(np.abs(torus_distance(pts)).max())


def geometry_cases():
    """The closed meshes and seeded point sets of the geometric check: (name, tris, points, truth, clearance, gap). truth is the
    analytic inside of the smooth shape (sphere, torus, cube, shell); the points are kept farther than `clearance` from its surface,
    and `gap` -- the largest distance between the polyhedron and that shape -- is smaller than the clearance (the CPU test asserts
    it), so the truth is the polyhedron's too."""
    out = []
    rng = np.random.RandomState(20261)
    # icosphere: 1280 triangles, 20 000 points in [-1.3, 1.3]^3
    tris = icosphere(3)
    p = rng.uniform(-1.3, 1.3, (20000, 3)).astype(F)
    rad = np.linalg.norm(p.astype(np.float64), axis=1)
    clr = 0.01
    keep = np.abs(rad - 1.0) > clr
    out.append(("icosphere", tris, p[keep], (rad < 1.0)[keep], clr, _sphere_gap(tris, 1.0)))
    # torus: 2304 triangles, 20 000 points in its bounding box grown by 0.2
    tris = torus()
    p = rng.uniform([-1.6, -1.6, -0.6], [1.6, 1.6, 0.6], (20000, 3)).astype(F)
    sd = torus_distance(p)
    clr = 0.02
    keep = np.abs(sd) > clr
    out.append(("torus", tris, p[keep], (sd < 0)[keep], clr, _torus_gap(tris)))
    # the unit cube against a regular grid of 33^3 points, spacing 1/16 (the cube's vertices sit on the grid's planes), the whole
    # grid moved by 1/64 on every axis: no point nearer than 1/64 to a face
    g = (np.arange(33, dtype=np.float64) / 16.0 - 0.5 + 1.0 / 64.0).astype(F)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out.append(("cube_grid", cube(), p, ((p > 0) & (p < 1)).all(axis=1), 1.0 / 64.0, 0.0))
    # the shell, inner sphere wound either way: 1280 + 320 triangles, 8000 points
    for flip in (False, True):
        tris = shell(flip)
        p = rng.uniform(-1.2, 1.2, (8000, 3)).astype(F)
        rad = np.linalg.norm(p.astype(np.float64), axis=1)
        clr = 0.02
        keep = (np.abs(rad - 1.0) > clr) & (np.abs(rad - 0.5) > clr)
        gap = max(_sphere_gap(tris[:1280], 1.0), _sphere_gap(tris[1280:], 0.5))
        out.append(("shell_flipped" if flip else "shell", tris, p[keep], ((rad < 1.0) & (rad > 0.5))[keep], clr, gap))
    return out
