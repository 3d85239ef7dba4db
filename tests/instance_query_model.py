"""The instanced scene queries (psm_instances_*_dev, include/psm_hip.h "instanced scene queries") in numpy float32: the canonical
move of a query into an instance's object space, restated; the moved queries are fed to the single-hierarchy yardsticks as they
are (query_model, point_query_model, inside_query_model) and the answers combined by scene_query_model's rules.

An instance is (tris [T, 3, 3], cand, pose): the triangles of one hierarchy, the ids of its leaves, and world_from_object as a
[3, 4] float32 matrix [R | T]. The move, one operation order:
    d = x - T (per component);  x'_j = (R[0][j] d.x + R[1][j] d.y) + R[2][j] d.z
and a direction the same without the subtraction. move() takes the dtype to work in: float64 gives the same formulas evaluated
in double, which the tests use to measure how far float32 is from them."""
import numpy as np

import inside_query_model as IQ
import point_query_model as PQ
import query_model as Q
import scene_query_model as SQ

F = np.float32
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)


def rotate(pose, d, dtype=F):
    """a direction into object space: R^T d in the canonical order"""
    m = np.asarray(pose, dtype).reshape(3, 4)
    d = np.asarray(d, dtype).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(m[0, j] * d[:, 0] + m[1, j] * d[:, 1]) + m[2, j] * d[:, 2] for j in range(3)], axis=1).astype(dtype)


def move(pose, x, dtype=F):
    """a point into object space: R^T (x - T) in the canonical order"""
    m = np.asarray(pose, dtype).reshape(3, 4)
    x = np.asarray(x, dtype).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return rotate(m, (x - m[:, 3]).astype(dtype), dtype)


def to_world(pose, x, dtype=np.float64):
    """an object-space point in world space: R x + T (what a caller does with a result; no canonical order is needed)"""
    m = np.asarray(pose, dtype).reshape(3, 4)
    return np.asarray(x, dtype).reshape(-1, 3) @ m[:, :3].T + m[:, 3]


def random_pose(rng, reflect=False, shift=1.0):
    """a seeded rigid pose: a rotation from a random unit quaternion (composed in double, rounded to float32 once), mirrored in x
    when `reflect`, and a translation of up to `shift` per axis"""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    if reflect:
        r = r @ np.diag([-1.0, 1.0, 1.0])
    return np.concatenate([r, rng.uniform(-shift, shift, (3, 1))], axis=1).astype(F)


def posed(tris, pose):
    """the triangles of an instance in world space, float32 (the "baked" mesh: rounded once more, so only close to the instance)"""
    t = np.asarray(tris, F).reshape(-1, 3)
    return to_world(pose, t).astype(F).reshape(-1, 3, 3)


def intersect(insts, origins, directs, tmin=0.0, tmax=np.inf):
    """psm_instances_intersect_dev and _occluded_dev: (hits [R, 4], inst [R] int32, any [R] bool)"""
    res = [Q.query(t, c, move(m, origins), rotate(m, directs), tmin, tmax) for t, c, m in insts]
    hits, inst = SQ.combine_closest([r[0] for r in res])
    return hits, inst, np.logical_or.reduce([r[1] for r in res])


def count(insts, origins, directs, tmin=0.0, tmax=np.inf):
    """psm_instances_count_hits_dev: uint32 [R]"""
    return np.sum([IQ.count(t, c, move(m, origins), rotate(m, directs), tmin, tmax) for t, c, m in insts], axis=0, dtype=np.uint32)


def closest_point(insts, points, rmax=np.inf):
    """psm_instances_closest_point_dev and _within_dev: (hits [R, 4], inst [R] int32, within [R] bool). The value compared
    across instances is each instance's own d2 of its own moved point."""
    moved = [move(m, points) for _, _, m in insts]
    res = [PQ.query(t, c, p, rmax) for (t, c, _), p in zip(insts, moved)]
    keys = [SQ.d2_of(t, p, r[0]) for (t, _, _), p, r in zip(insts, moved, res)]
    hits, inst = SQ.combine_closest([r[0] for r in res], keys)
    return hits, inst, np.logical_or.reduce([r[1] for r in res])


def parities(insts, points, samples=5):
    """[samples, R] bool: row k = "the crossings of the WORLD ray {p, 0, INSIDE_DIRECTIONS[k], +inf}, moved per instance and
    summed over all instances, are odd" """
    p = np.asarray(points, F).reshape(-1, 3)
    out = np.zeros((samples, p.shape[0]), bool)
    for k in range(samples):
        d = np.broadcast_to(IQ.INSIDE_DIRECTIONS[k], p.shape)
        out[k] = (count(insts, p, d, F(0), F(np.inf)) & 1) == 1
    return out


def inside(insts, points, samples=3):
    """psm_instances_inside_dev: bool [R]"""
    assert samples in (1, 3, 5)
    return IQ.vote(parities(insts, points, samples), samples)


def signed_distance(insts, points, rmax=np.inf, samples=3):
    """psm_instances_signed_distance_dev: (hits [R, 4], inst [R] int32)"""
    p = np.asarray(points, F).reshape(-1, 3)
    hits, inst, _ = closest_point(insts, p, rmax)
    found = np.nonzero(inst >= 0)[0]
    ins = inside(insts, p[found], samples)
    hits.view(np.uint32)[found[ins], 2] |= np.uint32(0x80000000)
    return hits, inst


# ---- instanced against baked: how decided an answer is, and how far float32 is from the same formulas in float64 -----------------
# The instanced queries work in object space, a scene over hierarchies built from posed() triangles in world space: two float32
# computations of the same geometric question, each rounded on its own. They must agree wherever the answer is decided by more than
# the rounding can move it. The decisions of a query are: which of two candidates is nearer (the gap between the best value and
# the runner-up's), whether a value lies inside the window or the radius (its distance to that edge) and -- for a ray -- whether
# it meets a triangle at all (the distance of its crossing point from the triangle's acceptance boundary, as a length). The
# margin of a query is the smallest of these over its candidates; the noise is measured, not assumed: deviation() below.

def _ray_values(insts, origins, directs, dtype):
    """per instance the moved ray against every triangle in `dtype`, by tri_test's formulas without the clamp: t and the signed
    distance e of the crossing point from the acceptance boundary (positive: accepted), as a length -- the smallest of u + 1e-5,
    1.00001 - u, v + 1e-5, 1.00001 - (u + v), times the triangle's smallest height. [R, T_total] each."""
    ts, es = [], []
    for tris, cand, m in insts:
        tri = np.asarray(tris, dtype).reshape(-1, 3, 3)[np.asarray(cand, np.int64)]
        o = move(m, origins, dtype)[:, None, :]
        d = rotate(m, directs, dtype)
        with np.errstate(all="ignore"):
            d = (d * (dtype(1.0) / np.sqrt(Q.dot3(d, d)))[:, None])[:, None, :]
            v0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
            pvec = Q.cross3(d, e2)
            inv = dtype(1.0) / Q.dot3(e1, pvec)
            tvec = o - v0
            u = Q.dot3(tvec, pvec) * inv
            qvec = Q.cross3(tvec, e1)
            v = Q.dot3(d, qvec) * inv
            t = Q.dot3(e2, qvec) * inv
            n = Q.cross3(e1, e2)
            longest = np.sqrt(np.maximum(np.maximum(Q.dot3(e1, e1), Q.dot3(e2, e2)), Q.dot3(e2 - e1, e2 - e1)))
            height = np.sqrt(Q.dot3(n, n)) / longest
            e = np.minimum(np.minimum(u + 1e-5, 1.00001 - u), np.minimum(v + 1e-5, 1.00001 - (u + v))) * height
        ts.append(np.asarray(t, np.float64))
        es.append(np.asarray(e, np.float64))
    return np.concatenate(ts, axis=1), np.concatenate(es, axis=1)


def _point_values(insts, points, dtype):
    """per instance the moved point's distance to every triangle in `dtype`, by closest_on_tris' formulas. [R, T_total]"""
    out = []
    for tris, cand, m in insts:
        tri = np.asarray(tris, dtype).reshape(-1, 3, 3)[np.asarray(cand, np.int64)]
        p = move(m, points, dtype)[:, None, :]
        v0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
        with np.errstate(all="ignore"):
            out.append(np.sqrt(np.asarray(PQ.closest_on_tris(v0, e1, e2, p)[2], np.float64)))
    return np.concatenate(out, axis=1)


def ray_margin_and_deviation(insts, origins, directs, tmin, tmax):
    """(margin [R], deviation): the margin of every ray's closest-hit, any-hit and hit-count answers in the float32 model, and the
    largest difference between the float32 and the float64 evaluation of a value a decision rests on (t and e of every candidate
    whose crossing point lies on or within a hundredth of the scene's size of its triangle, in either evaluation)."""
    t32, e32 = _ray_values(insts, origins, directs, F)
    t64, e64 = _ray_values(insts, origins, directs, np.float64)
    lo = np.broadcast_to(np.asarray(tmin, np.float64), (t32.shape[0],))[:, None]
    hi = np.broadcast_to(np.asarray(tmax, np.float64), (t32.shape[0],))[:, None]
    with np.errstate(invalid="ignore"):
        near = (np.maximum(e32, e64) > -0.01) & np.isfinite(t32) & np.isfinite(t64) & (np.maximum(t32, t64) > lo - 0.01) & (np.minimum(t32, t64) < hi + 0.01)
        dev = max(float(np.abs(t32 - t64)[near].max(initial=0.0)), float(np.abs(e32 - e64)[near].max(initial=0.0)))
        boundary = np.where(np.isfinite(e32), np.abs(e32), np.inf).min(axis=1)               # meets the triangle or not
        on = e32 > 0
        window = np.where(on & np.isfinite(t32), np.minimum(np.abs(t32 - lo), np.abs(t32 - hi)), np.inf).min(axis=1)
        hit = np.sort(np.where(on & (t32 >= lo) & (t32 <= hi), t32, np.inf), axis=1)
        gap = np.where(np.isfinite(hit[:, 1]), hit[:, 1] - hit[:, 0], np.inf) if hit.shape[1] > 1 else np.full(hit.shape[0], np.inf)
    return np.minimum(np.minimum(boundary, np.nan_to_num(window, nan=0.0)), gap), dev


def point_margin_and_deviation(insts, points, rmax):
    """(margin [R], deviation) of every point's closest-point and within answers: the gap between the two smallest distances and
    the smallest distance's to rmax; the largest float32 / float64 difference of a distance"""
    d32, d64 = _point_values(insts, points, F), _point_values(insts, points, np.float64)
    rm = np.broadcast_to(np.asarray(rmax, np.float64), (d32.shape[0],))
    s = np.sort(d32, axis=1)
    gap = s[:, 1] - s[:, 0] if s.shape[1] > 1 else np.full(s.shape[0], np.inf)
    with np.errstate(invalid="ignore"):
        return np.minimum(gap, np.abs(s[:, 0] - rm)), float(np.abs(d32 - d64).max())


def baked_case(seed, parts, tris_n=240, n=3000):
    """a seeded case of the instanced-against-baked comparison: a soup of separate triangles (no shared edges: a closest point on
    an edge has one owner) cut into `parts`, each with a rotation or reflection and a translation of its own; finite rays with
    random windows and points with random radii around the posed soup. Returns (pieces, poses, (o, d, tmin, tmax), (p, rmax))."""
    rng = np.random.RandomState(1000 + seed)
    c = rng.uniform(-1, 1, (tris_n, 1, 3))
    tris = (c + rng.uniform(-0.25, 0.25, (tris_n, 3, 3))).astype(F)
    pieces = SQ.split(tris, tuple([tris_n // (parts + 1)] * (parts - 1)))[0]
    poses = [random_pose(rng, reflect=bool(k & 1), shift=0.5) for k in range(parts)]
    o = rng.uniform(-2, 2, (n, 3)).astype(F)
    d = (rng.uniform(-1, 1, (n, 3)) - 0.5 * o).astype(F)
    tmin = rng.uniform(0, 1, n).astype(F)
    tmax = (tmin + rng.uniform(0.5, 4, n)).astype(F)
    p = rng.uniform(-1.8, 1.8, (n, 3)).astype(F)
    rmax = rng.uniform(0.05, 0.6, n).astype(F)
    return pieces, poses, (o, d, tmin, tmax), (p, rmax)
