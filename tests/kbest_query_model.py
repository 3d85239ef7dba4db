"""The k-best queries (psm_bvh_first_hits_dev / psm_bvh_nearest_dev, include/psm_hip.h; kbest.hip) as a brute force over the
leaves in numpy. The per-candidate values are query_model's and point_query_model's (tri_test / ray_valid, closest_on_tris /
point_valid): no float arithmetic is restated here. What this adds is the order: a stable lexicographic sort on (value, unsigned
triangle id) -- the value compared as a float, so -0 == +0 and the id decides -- cut at k."""
import numpy as np

import point_query_model as PQ
import query_model as Q

F = np.float32


def _rows(val, ok, cand, u, v, out_val, k):
    """rows [R, k, 4] (u, v, out_val, tri bits; misses 0, 0, +inf, -1) and count [R] from per-pair values [R, T]: the counting
    pairs (ok) sorted by (val, tri). cand is ascending, so a stable sort on val alone leaves equal values in id order."""
    R, T = val.shape
    key = np.where(ok, val, F(np.inf)).astype(F)                # (a counting pair is never a NaN: it passed its window)
    order = np.argsort(key, axis=1, kind="stable")              # by value as floats (-0 == +0); equal values keep id order
    # the counting pairs first (one may sit at +inf, where the others were put): stable again, so (value, id) order stays
    order = np.take_along_axis(order, np.argsort(~np.take_along_axis(ok, order, axis=1), axis=1, kind="stable"), axis=1)
    count = np.minimum(ok.sum(axis=1), k).astype(np.uint32)
    rows = np.zeros((R, k, 4), F)
    rows[:, :, 2] = np.inf
    rows.view(np.int32)[:, :, 3] = -1
    r = np.arange(R)
    for s in range(min(k, T)):
        col = order[:, s]
        live = s < count
        rows[:, s, 0] = np.where(live, u[r, col], F(0))
        rows[:, s, 1] = np.where(live, v[r, col], F(0))
        rows[:, s, 2] = np.where(live, out_val[r, col], F(np.inf))
        rows.view(np.int32)[:, s, 3] = np.where(live, cand[col], -1)
    return rows, count


def first_hits(tris, cand, origins, directs, k, tmin=0.0, tmax=np.inf):
    """psm_bvh_first_hits_dev over the candidate ids `cand`: rows [R, k, 4] float32 as the kernel writes them and count [R]"""
    origins = np.asarray(origins, F).reshape(-1, 3)
    d = Q.normalize3(np.asarray(directs, F).reshape(-1, 3))
    R = origins.shape[0]
    lo, hi = Q._window(R, tmin), Q._window(R, tmax)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    tris = np.asarray(tris, F).reshape(-1, 3, 3)[cand]
    valid = Q.ray_valid(origins, d, lo, hi)
    rows = np.zeros((R, k, 4), F)
    rows[:, :, 2] = np.inf
    rows.view(np.int32)[:, :, 3] = -1
    count = np.zeros(R, np.uint32)
    if cand.size == 0:
        return rows, count
    for a, b in Q._chunks(R, cand.size, 1 << 20):
        t, u, v, ok = Q.tri_test(tris, origins[a:b], d[a:b], clamp=False)
        with np.errstate(invalid="ignore"):
            hit = ok & valid[a:b, None] & (t >= lo[a:b, None]) & (t <= hi[a:b, None])
        rows[a:b], count[a:b] = _rows(t, hit, cand, u, v, t, k)
    return rows, count


def nearest(tris, cand, points, k, rmax=np.inf):
    """psm_bvh_nearest_dev over the candidate ids `cand`: rows [R, k, 4] (u, v, dist, tri) and count [R]; the key is d2"""
    p = np.asarray(points, F).reshape(-1, 3)
    R = p.shape[0]
    rm = np.broadcast_to(np.asarray(rmax, F), (R,)).astype(F)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    v0, e1, e2 = PQ._split(np.asarray(tris, F).reshape(-1, 3, 3)[cand])
    valid = PQ.point_valid(p, rm)
    rows = np.zeros((R, k, 4), F)
    rows[:, :, 2] = np.inf
    rows.view(np.int32)[:, :, 3] = -1
    count = np.zeros(R, np.uint32)
    if cand.size == 0:
        return rows, count
    for a, b in PQ._chunks(R, cand.size, 1 << 19):
        u, v, d2 = PQ.closest_on_tris(v0[None], e1[None], e2[None], p[a:b, None, :])
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(d2)
            ok = valid[a:b, None] & (dist <= rm[a:b, None])
        rows[a:b], count[a:b] = _rows(d2, ok, cand, u, v, dist, k)
    return rows, count
