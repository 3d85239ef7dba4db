"""A numpy restatement of the triangle queries (psm_bvh_tri_overlaps_dev / psm_bvh_tri_count_dev / psm_bvh_tri_triangles_dev,
include/psm_hip.h "triangle queries"; tri.hip, psm_tri_dev.h tri_tri).

tri_tri is written once over a float type: in float32 every operation is one numpy float32 operation in the order
psm_tri_dev.h writes it (the library builds with -ffp-contract=off, so each float32 operation rounds once, as numpy's do; there
is no division and no square root), and the selections are np.where on the comparisons the kernel makes. In float64 the same
formulas are the second reading tests/test_tri_query_cpu.py holds the float32 one against. The brute force here is the
yardstick of tests/test_tri_query_cpu.py and tests/test_gpu_tri_query.py."""
import numpy as np

from point_query_model import _split

F = np.float32
K_MAX = 16   # PSM_QUERY_K_MAX
AXES = 20


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross(x, y):
    """cross3 (psm_math.h)"""
    return [x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]]


def _max3(x, y, z):
    m = np.where(y > x, y, x)
    return np.where(z > m, z, m)


def _min3(x, y, z):
    m = np.where(y < x, y, x)
    return np.where(z < m, z, m)


def axes(v0, e1, e2, a, b, c, flags_only=False):
    """For every pair (broadcast over [..., 3]) and each of the 20 axes, in the order of include/psm_hip.h: (separates, gap,
    length) with `separates` the test as psm_tri_dev.h makes it, gap = max(qmin - tmax, tmin - qmax) and length the axis's
    Euclidean length (1 for the unit axes), each [20, ...]. The type is the inputs'. flags_only: no gaps and lengths are
    worked out and `separates` alone is returned, already reduced over the axes (the brute force's path)."""
    T = v0.dtype.type
    A, B, C = a - v0, b - v0, c - v0
    sep, gap, length = [], [], []

    def close(tmin, tmax, qmin, qmax, ln):
        if flags_only:
            s = ~((tmax >= qmin) & (qmax >= tmin))
            sep[:] = [sep[0] | s] if sep else [s]
            return
        sep.append(~((tmax >= qmin) & (qmax >= tmin)))
        gap.append(np.maximum(qmin - tmax, tmin - qmax))
        length.append(np.broadcast_to(ln, sep[-1].shape))

    for k in range(3):   # the unit axes, no product
        zero = np.zeros_like(e1[..., k] + A[..., k])
        close(_min3(zero, e1[..., k], e2[..., k]), _max3(zero, e1[..., k], e2[..., k]),
              _min3(A[..., k], B[..., k], C[..., k]), _max3(A[..., k], B[..., k], C[..., k]), T(1))
    E1, E2 = [e1[..., k] for k in range(3)], [e2[..., k] for k in range(3)]
    E3 = [E2[k] - E1[k] for k in range(3)]
    Av, Bv, Cv = ([x[..., k] for k in range(3)] for x in (A, B, C))
    G1, G2, G3 = [Bv[k] - Av[k] for k in range(3)], [Cv[k] - Av[k] for k in range(3)], [Cv[k] - Bv[k] for k in range(3)]
    n, m = _cross(E1, E2), _cross(G1, G2)
    general = [n, m]
    general += [_cross(e, g) for e in (E1, E2, E3) for g in (G1, G2, G3)]
    general += [_cross(n, e) for e in (E1, E2, E3)] + [_cross(m, g) for g in (G1, G2, G3)]
    for ax in general:
        p1, p2 = _dot(ax, E1), _dot(ax, E2)
        qa, qb, qc = _dot(ax, Av), _dot(ax, Bv), _dot(ax, Cv)
        zero = np.zeros_like(p1)
        close(_min3(zero, p1, p2), _max3(zero, p1, p2), _min3(qa, qb, qc), _max3(qa, qb, qc), None if flags_only else np.sqrt(_dot(ax, ax)))
    if flags_only:
        return sep[0]
    shape = np.broadcast(*sep).shape
    return (np.stack([np.broadcast_to(x, shape) for x in sep]), np.stack([np.broadcast_to(x, shape) for x in gap]),
            np.stack([np.broadcast_to(x, shape) for x in length]))


def tri_tri(v0, e1, e2, a, b, c):
    """tri_tri (psm_tri_dev.h) for every pair: v0 / e1 / e2 [..., 3] and a / b / c [..., 3] broadcast, all of one float type.
    True iff no axis separates."""
    with np.errstate(all="ignore"):
        return ~axes(v0, e1, e2, a, b, c, flags_only=True)


def _unit_pass(v0, e1, e2, a, b, c):
    """the pairs no unit axis separates (the first three axes of tri_tri alone): what the brute force sifts with"""
    A, B, C = a - v0, b - v0, c - v0
    zero = np.zeros_like(e1[..., 0] + A[..., 0])
    ok = np.ones(zero.shape, bool)
    for k in range(3):
        ok &= ((_max3(zero, e1[..., k], e2[..., k]) >= _min3(A[..., k], B[..., k], C[..., k])) &
               (_max3(A[..., k], B[..., k], C[..., k]) >= _min3(zero, e1[..., k], e2[..., k])))
    return ok


def tri_valid(q):
    """the query triangles [n, 3, 3] that can meet anything: nine finite numbers"""
    return np.isfinite(q.reshape(q.shape[0], -1)).all(axis=1)


def counts_matrix(tris, cand, q):
    """[queries, candidates] bool: which candidate (the ids `cand`, sorted) counts for which query triangle; and the sorted ids"""
    q = np.asarray(q, F).reshape(-1, 3, 3)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    v0, e1, e2 = _split(np.asarray(tris, F).reshape(-1, 3, 3)[cand])
    ok = np.zeros((q.shape[0], cand.size), bool)
    valid = tri_valid(q)
    step = max(1, (1 << 18) // max(cand.size, 1))
    with np.errstate(all="ignore"):
        for s in range(0, q.shape[0], step):   # the pairs that pass the unit axes, then tri_tri (all 20 axes) on those alone
            t = min(q.shape[0], s + step)
            ok[s:t] = _unit_pass(v0[None], e1[None], e2[None], q[s:t, None, 0, :], q[s:t, None, 1, :], q[s:t, None, 2, :]) & valid[s:t, None]
    r, c = np.nonzero(ok)
    for s in range(0, r.size, 1 << 18):
        i, j = r[s:s + (1 << 18)], c[s:s + (1 << 18)]
        ok[i, j] = tri_tri(v0[j], e1[j], e2[j], q[i, 0], q[i, 1], q[i, 2])
    return ok, cand


def query(tris, cand, q, k=K_MAX):
    """The three triangle queries over the candidate triangle ids `cand` (the hierarchy's leaves, PSM_BVH_LEAF_TRI) by brute
    force: (overlaps [R] bool, count [R] uint32 -- the full count --, rows [R, k] int32 -- the min(k, count) lowest ids that
    count, ascending, then -1 --, and the rows' count [R] uint32 = min(k, count))"""
    ok, cand = counts_matrix(tris, cand, q)
    count = ok.sum(axis=1).astype(np.uint32)
    rows = np.full((ok.shape[0], k), -1, np.int32)
    rank = np.cumsum(ok, axis=1) - 1                       # a counting candidate's slot (the candidates are sorted by id)
    r, c = np.nonzero(ok & (rank < k))
    rows[r, rank[r, c]] = cand[c]
    return count > 0, count, rows, np.minimum(count, np.uint32(k)).astype(np.uint32)
