"""A numpy restatement of the box queries (psm_bvh_box_overlaps_dev / psm_bvh_box_count_dev / psm_bvh_box_triangles_dev,
include/psm_hip.h "box queries"; box.hip, box_tri).

box_tri is written once over a float type: in float32 every operation is one numpy float32 operation in the order box.hip writes
it (the library builds with -ffp-contract=off, so each float32 operation rounds once, as numpy's do; there is no division and
no square root), and the selections are np.where on the comparisons the kernel makes. In float64 the same formulas are the
second reading tests/test_box_query_cpu.py holds the float32 one against. The brute force here is the yardstick of
tests/test_box_query_cpu.py and tests/test_gpu_box_query.py."""
import numpy as np

from point_query_model import _split

F = np.float32
K_MAX = 16   # PSM_QUERY_K_MAX


def _term(a, l, h):
    """one term of bmin(a): a >= 0 ? a L : a H (bmax: the same with L and H swapped)"""
    return np.where(a >= 0, a * l, a * h)


def _gap(pmx, pmn, bmin, bmax):
    """how far the axis is from not separating: the axis separates iff !(pmx >= bmin && pmn <= bmax); returned are the two
    differences whose signs say the same in exact arithmetic (bmin - pmx, pmn - bmax), for the float64 reading's margins"""
    return bmin - pmx, pmn - bmax


def axes(v0, e1, e2, lo, hi):
    """For every pair (broadcast over [..., 3]) and each of the 13 axes, in the order of include/psm_hip.h: (separates, gap,
    length) with `separates` the test as box.hip makes it, gap = max(bmin - max P, min P - bmax) and length the axis's
    Euclidean length (1 for the unit axes), each [13, ...]. The type is the inputs'."""
    T = v0.dtype.type
    zero = T(0)
    L, H = lo - v0, hi - v0
    f3 = e2 - e1
    sep, gap, length = [], [], []

    def close(pmx, pmn, bmin, bmax, ln):
        sep.append(~((pmx >= bmin) & (pmn <= bmax)))
        g0, g1 = _gap(pmx, pmn, bmin, bmax)
        gap.append(np.maximum(g0, g1))
        length.append(np.broadcast_to(ln, sep[-1].shape))

    for k in range(3):   # the unit axes: {0, e1_k, e2_k} against [L_k, H_k] directly
        a, b = e1[..., k], e2[..., k]
        pmx, pmn = np.where(a > 0, a, zero), np.where(a < 0, a, zero)
        pmx, pmn = np.where(b > pmx, b, pmx), np.where(b < pmn, b, pmn)
        close(pmx, pmn, L[..., k], H[..., k], T(1))
    for f, g in ((e1, e2), (e2, e1), (f3, e1)):   # the edge axes unit_k x f, g the edge that gives the projection
        for (i, j), (a1, a2) in (((1, 2), (-f[..., 2], f[..., 1])),       # k = x: (0, -fz, fy)
                                 ((0, 2), (f[..., 2], -f[..., 0])),       # k = y: (fz, 0, -fx)
                                 ((0, 1), (-f[..., 1], f[..., 0]))):      # k = z: (-fy, fx, 0)
            bmin = _term(a1, L[..., i], H[..., i]) + _term(a2, L[..., j], H[..., j])
            bmax = _term(a1, H[..., i], L[..., i]) + _term(a2, H[..., j], L[..., j])
            p = a1 * g[..., i] + a2 * g[..., j]
            close(np.where(p > 0, p, zero), np.where(p < 0, p, zero), bmin, bmax, np.sqrt(a1 * a1 + a2 * a2))
    n = [e1[..., 1] * e2[..., 2] - e2[..., 1] * e1[..., 2],               # cross3 (psm_math.h)
         e1[..., 2] * e2[..., 0] - e2[..., 2] * e1[..., 0],
         e1[..., 0] * e2[..., 1] - e2[..., 0] * e1[..., 1]]
    bmin = (_term(n[0], L[..., 0], H[..., 0]) + _term(n[1], L[..., 1], H[..., 1])) + _term(n[2], L[..., 2], H[..., 2])
    bmax = (_term(n[0], H[..., 0], L[..., 0]) + _term(n[1], H[..., 1], L[..., 1])) + _term(n[2], H[..., 2], L[..., 2])
    z = np.zeros_like(bmin)
    close(z, z, bmin, bmax, np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
    return np.stack(sep), np.stack(gap), np.stack(length)


def box_tri(v0, e1, e2, lo, hi):
    """box_tri (box.hip) for every pair: v0 / e1 / e2 [..., 3] and lo / hi [..., 3] broadcast, all of one float type. True iff
    no axis separates."""
    with np.errstate(all="ignore"):
        return ~axes(v0, e1, e2, lo, hi)[0].any(axis=0)


def box_valid(lo, hi):
    """the boxes that can overlap a triangle: six finite numbers, lo <= hi on every axis"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1)


def counts_matrix(tris, cand, lo, hi):
    """[boxes, candidates] bool: which candidate (the ids `cand`, sorted) counts for which box; and the sorted ids"""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    v0, e1, e2 = _split(np.asarray(tris, F).reshape(-1, 3, 3)[cand])
    ok = np.zeros((lo.shape[0], cand.size), bool)
    valid = box_valid(lo, hi)
    step = max(1, (1 << 19) // max(cand.size, 1))
    for a in range(0, lo.shape[0], step):
        b = min(lo.shape[0], a + step)
        ok[a:b] = box_tri(v0[None], e1[None], e2[None], lo[a:b, None, :], hi[a:b, None, :]) & valid[a:b, None]
    return ok, cand


def query(tris, cand, lo, hi, k=K_MAX):
    """The three box queries over the candidate triangle ids `cand` (the hierarchy's leaves, PSM_BVH_LEAF_TRI) by brute force:
    (overlaps [R] bool, count [R] uint32 -- the full count --, rows [R, k] int32 -- the min(k, count) lowest ids that count,
    ascending, then -1 --, and the rows' count [R] uint32 = min(k, count))"""
    ok, cand = counts_matrix(tris, cand, lo, hi)
    count = ok.sum(axis=1).astype(np.uint32)
    rows = np.full((ok.shape[0], k), -1, np.int32)
    rank = np.cumsum(ok, axis=1) - 1                       # a counting candidate's slot (the candidates are sorted by id)
    r, c = np.nonzero(ok & (rank < k))
    rows[r, rank[r, c]] = cand[c]
    return count > 0, count, rows, np.minimum(count, np.uint32(k)).astype(np.uint32)
