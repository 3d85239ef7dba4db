"""A numpy restatement of the clearance queries (psm_bvh_tri_closest_dev / psm_bvh_tri_within_dev, include/psm_hip.h "clearance
queries"; tri_dist.hip, psm_tri_dist_dev.h seg_seg and tri_dist).

seg_seg and tri_dist are written once over a float type: in float32 every operation is one numpy float32 operation in the order
psm_tri_dist_dev.h writes it (the library builds with -ffp-contract=off, so each float32 operation rounds once, as numpy's do;
division and sqrt are correctly rounded on both sides), and the selections are np.where on the comparisons the kernel makes. The
vertex features are point_query_model's closest_on_tris and the overlap test is tri_query_model's tri_tri, reused as they are
(closest_on_tris returns float32 weights whatever it is given: in float64 the six vertex features are therefore float64
arithmetic with weights rounded once). The brute force here is the yardstick of tests/test_tri_dist_query_cpu.py and
tests/test_gpu_tri_dist_query.py; the prune (box_row, point_bound, lb2) and a walk over a tree are restated for the CPU test."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import point_query_model as PQ
import tri_query_model as TQ
from point_query_model import _split
from query_model import dot3

F = np.float32
FEATURES = 15
PZERO = 0.0005


def _clamp01(x, T):
    """(x > 0 ? x : 0) then (x < 1 ? x : 1): NaN and -0 go to +0"""
    x = np.where(x > T(0), x, T(0))
    return np.where(x < T(1), x, T(1))


def seg_seg(p1, d1, p2, d2):
    """seg_seg (psm_tri_dist_dev.h) for every pair: the clamped closest points of p1 + x d1 and p2 + y d2; returns x, y"""
    T = np.result_type(p1, d1, p2, d2).type
    with np.errstate(all="ignore"):
        r = p1 - p2
        a, e, b = dot3(d1, d1), dot3(d2, d2), dot3(d1, d2)
        c, f = dot3(d1, r), dot3(d2, r)
        den = a * e - b * b
        skew = den > (a * e) * T(2.0 ** -16)
        x0 = _clamp01(np.where(skew, b * f - c * e, T(0)) / np.where(skew, den, T(1)), T)
        ye, xa = e > T(0), a > T(0)
        y = _clamp01(np.where(ye, b * x0 + f, T(0)) / np.where(ye, e, T(1)), T)
        x = _clamp01(np.where(xa, b * y - c, T(0)) / np.where(xa, a, T(1)), T)
    return x.astype(T), y.astype(T)


def d2_of(e1, e2, A, g1, g2, u, v, s, t):
    """tri_dist_d2: Q = (A + s g1) + t g2, P = u e1 + v e2, dot3(Q - P, Q - P)"""
    with np.errstate(all="ignore"):
        Q = (A + s[..., None] * g1) + t[..., None] * g2
        P = u[..., None] * e1 + v[..., None] * e2
        w = Q - P
        return dot3(w, w)


def features(v0, e1, e2, a, b, c):
    """The fifteen features of every pair (v0 / e1 / e2 and a / b / c [..., 3] broadcast, all of one float type), in the
    kernel's order: (d2, u, v, s, t), each [15, ...]"""
    T = np.result_type(v0, a).type
    with np.errstate(all="ignore"):
        A, B, C = a - v0, b - v0, c - v0
        g1, g2, g3 = B - A, C - A, C - B
        e3 = e2 - e1
        shape = np.broadcast(A[..., 0], e1[..., 0]).shape
        zero, one = np.zeros(shape, T), np.ones(shape, T)
        O = np.zeros(shape + (3,), T)
        rows = []
        for p, st in ((a, (zero, zero)), (b, (one, zero)), (c, (zero, one))):          # F0 - F2
            u, v, _ = PQ.closest_on_tris(v0, e1, e2, p)
            rows.append((u.astype(T) + zero, v.astype(T) + zero) + st)
        for p, uv in ((O, (zero, zero)), (e1 + O, (one, zero)), (e2 + O, (zero, one))):  # F3 - F5
            s, t, _ = PQ.closest_on_tris(A + O, g1 + O, g2 + O, p)
            rows.append(uv + (s.astype(T) + zero, t.astype(T) + zero))
        stored = ((O, e1, lambda x: (x, zero)), (O, e2, lambda x: (zero, x)), (e1, e3, lambda x: (one - x, x)))
        query = ((A, g1, lambda y: (y, zero)), (A, g2, lambda y: (zero, y)), (B, g3, lambda y: (one - y, y)))
        for p1, d1, uv in stored:                                                       # F6 - F14: i outer, j inner
            for p2, d2, st in query:
                x, y = seg_seg(p1 + O, d1 + O, p2 + O, d2 + O)
                rows.append(uv(x) + st(y))
        u, v, s, t = (np.stack([np.broadcast_to(r[k], shape) for r in rows]).astype(T) for k in range(4))
        d2 = np.stack([d2_of(e1, e2, A, g1, g2, u[k], v[k], s[k], t[k]) for k in range(FEATURES)])
    return d2, u, v, s, t


def tri_dist(v0, e1, e2, a, b, c, meet=None, detail=False):
    """tri_dist (psm_tri_dist_dev.h) for every pair: d2, u, v, s, t. The winner is the first feature; a later one replaces it iff
    its d2 is smaller (a NaN replaces nothing). Where tri_tri holds d2 is 0 and the weights stay the winner's. meet: tri_tri's
    answer if the caller has it. detail: also the winning feature's index and its own d2 (the fifteen features' minimum)."""
    d2, u, v, s, t = features(v0, e1, e2, a, b, c)
    T = d2.dtype.type
    best = d2[0].copy()
    k = np.zeros(best.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(1, FEATURES):
            take = d2[i] < best
            best = np.where(take, d2[i], best)
            k = np.where(take, i, k)
    pick = lambda x: np.take_along_axis(x, k[None], axis=0)[0]
    if meet is None:
        meet = TQ.tri_tri(v0, e1, e2, a, b, c)
    out = (np.where(meet, T(0), best), pick(u), pick(v), pick(s), pick(t))
    return out + (k, best) if detail else out


def query_valid(q, rmax):
    """the queries that can find a triangle: nine finite coordinates, rmax >= 0 (NaN and negative radii miss; -0 is 0)"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(q.reshape(q.shape[0], -1)).all(axis=1) & (rmax >= F(0))


def miss_records(n):
    hits = np.zeros((n, 8), F)
    hits[:, 2] = np.inf
    hits.view(np.int32)[:, 3] = -1
    return hits


def query(tris, cand, q, rmax=np.inf):
    """psm_bvh_tri_closest_dev and psm_bvh_tri_within_dev over the candidate triangle ids `cand` (the hierarchy's leaves,
    PSM_BVH_LEAF_TRI) by brute force: a candidate counts iff sqrt(d2) <= rmax; closest = the smallest d2, on a bit-equal d2 the
    lowest id. Returns (hits [R, 8] float32 as the kernel writes psm_tri_hit -- u, v, dist, tri bits, s, t, 0, 0; a miss is 0, 0,
    +inf, -1, 0, 0, 0, 0 --, within [R] bool)."""
    q = np.asarray(q, F).reshape(-1, 3, 3)
    R = q.shape[0]
    rm = np.broadcast_to(np.asarray(rmax, F), (R,)).astype(F)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    v0, e1, e2 = _split(np.asarray(tris, F).reshape(-1, 3, 3)[cand])
    hits = miss_records(R)
    within = np.zeros(R, bool)
    valid = query_valid(q, rm)
    if cand.size == 0:
        return hits, within

    def chunk(ab):
        lo, hi = ab
        qa, qb, qc = q[lo:hi, None, 0, :], q[lo:hi, None, 1, :], q[lo:hi, None, 2, :]
        with np.errstate(all="ignore"):
            # tri_tri on the pairs that pass its unit axes alone (the others it separates)
            meet = TQ._unit_pass(v0[None], e1[None], e2[None], qa, qb, qc)
            i, j = np.nonzero(meet)
            if i.size:
                meet[i, j] = TQ.tri_tri(v0[j], e1[j], e2[j], q[lo + i, 0], q[lo + i, 1], q[lo + i, 2])
            d2, u, v, s, t = tri_dist(v0[None], e1[None], e2[None], qa, qb, qc, meet=meet)
            dist = np.sqrt(d2)
            ok = valid[lo:hi, None] & (dist <= rm[lo:hi, None])
        found = ok.any(axis=1)
        best = np.where(ok, d2, F(np.inf)).min(axis=1)
        k = np.argmax(ok & (d2 == best[:, None]), axis=1)   # the lowest id of the smallest d2 (candidates sorted by id)
        r = np.arange(hi - lo)
        for col, x in ((0, u), (1, v), (4, s), (5, t)):
            hits[lo:hi, col] = np.where(found, x[r, k], F(0))
        hits[lo:hi, 2] = np.where(found, dist[r, k], F(np.inf))
        hits.view(np.int32)[lo:hi, 3] = np.where(found, cand[k], -1)
        within[lo:hi] = found

    with ThreadPoolExecutor(max_workers=8) as pool:   # (numpy releases the GIL: query chunks on a few threads)
        list(pool.map(chunk, PQ._chunks(R, cand.size, 1 << 16)))
    return hits, within


def points_of(tris, q, hits):
    """the two points of every record in float32: (v0 + u e1) + v e2 on the stored triangle and (a + s (b - a)) + t (c - a) on
    the query triangle (rows of misses are meaningless)"""
    tri = np.clip(hits.view(np.int32)[:, 3], 0, None)
    with np.errstate(all="ignore"):
        on_mesh = PQ.point_of(tris, tri, hits[:, 0], hits[:, 1])
        on_query = PQ.point_of(q, np.arange(hits.shape[0]), hits[:, 4], hits[:, 5])
    return on_mesh, on_query


# ---- the prune: box_row, point_bound and lb2 in float32, as tri_dist.hip computes them ---------------------------------------------

def box_rows(M, q):
    """box_row on the three normalised axes for query triangles q [..., 3, 3]: (gl, gh) [..., 3], the grown image interval of
    the bounding box. M: float32 [3 or 4, 4], row-major"""
    M = np.asarray(M, F)
    lo, hi = q.min(axis=-2), q.max(axis=-2)                          # exact: selections
    with np.errstate(all="ignore"):
        fa, fb = lo[..., None, :] * M[:3, :3], hi[..., None, :] * M[:3, :3]
        mn, mx, ab = np.fmin(fa, fb), np.fmax(fa, fb), np.fmax(np.abs(fa), np.abs(fb))
        ilo = ((mn[..., 0] + mn[..., 1]) + mn[..., 2]) + M[:3, 3]
        ihi = ((mx[..., 0] + mx[..., 1]) + mx[..., 2]) + M[:3, 3]
        h = (F(2) + (((ab[..., 0] + ab[..., 1]) + ab[..., 2]) + np.abs(M[:3, 3]))) * F(2.0 ** -16)
        gl, gh = ilo - h, ihi + h
    assert gl.dtype == F and gh.dtype == F
    return gl, gh


def point_bound(M):
    """point_bound (psm_query_dev.h): il [3], wf, orth"""
    M = np.asarray(M, F)
    rows = M[:3, :3]
    with np.errstate(all="ignore"):
        lam = np.sqrt(dot3(rows, rows))
        il = np.where(lam > 0, F(1) / np.where(lam > 0, lam, F(1)), F(0)).astype(F)
        c01 = np.abs(dot3(rows[0], rows[1])) * il[0] * il[1]
        c02 = np.abs(dot3(rows[0], rows[2])) * il[0] * il[2]
        c12 = np.abs(dot3(rows[1], rows[2])) * il[1] * il[2]
        cmax = np.fmax(np.fmax(c01, c02), c12) + F(2.0 ** -20)
        orth = bool(cmax <= F(2.0 ** -11) and (il > 0).all())
        wf = (F(1) - F(2.0 ** -18)) / (F(1) + F(2) * cmax) if orth else F(1) - F(2.0 ** -18)
    return il, F(wf), orth


def lb2(bound, gl, gh, mn, mx):
    """LB^2 of boxes [mn, mx] ([..., 3], float32) against the intervals [gl, gh]: tri_dist.hip's lb2"""
    il, wf, orth = bound
    with np.errstate(all="ignore"):
        t = np.fmax(np.fmax(mn - gh, gl - mx), F(0)) * il
        m = np.fmax(np.fmax(t[..., 0], t[..., 1]), t[..., 2])
        out = ((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]) if orth else m * m
        out = out * wf
    assert out.dtype == F
    return out


def rmax_bound(rmax):
    """the bound a query starts with: fl(rmax^2) (1 + 2^-20) + 2^-126"""
    with np.errstate(all="ignore"):
        r = np.asarray(rmax, F)
        return (r * r) * F(1.00000095367431640625) + F(2.0 ** -126)


def build_tree(M, tris, cand):
    """A real tree over the candidates for the walk below: median splits of the normalised centroids on the widest axis, a
    leaf's box its triangle's normalised bounding box (float32 image as the build takes it) padded by PZERO and rounded to
    fp16, an internal node's the union of its children's. Returns (nodes, root): a node is (mn, mx, left, right), a leaf
    (mn, mx, ~id, None); root None for no candidates."""
    M = np.asarray(M, F)
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    img = ((t[..., 0:1] * M[:3, 0] + t[..., 1:2] * M[:3, 1]) + t[..., 2:3] * M[:3, 2]) + M[:3, 3]
    mn = (img.min(axis=1) - F(PZERO)).astype(np.float16).astype(F)
    mx = (img.max(axis=1) + F(PZERO)).astype(np.float16).astype(F)
    cen = img.mean(axis=1)
    nodes = []

    def make(ids):
        if len(ids) == 1:
            nodes.append((mn[ids[0]], mx[ids[0]], ~int(ids[0]), None))
            return len(nodes) - 1
        axis = np.argmax(cen[ids].max(axis=0) - cen[ids].min(axis=0))
        ids = ids[np.argsort(cen[ids, axis], kind="stable")]
        l, r = make(ids[:len(ids) // 2]), make(ids[len(ids) // 2:])
        nodes.append((np.minimum(nodes[l][0], nodes[r][0]), np.maximum(nodes[l][1], nodes[r][1]), l, r))
        return len(nodes) - 1

    cand = np.asarray(cand, np.int64).reshape(-1)
    return nodes, (make(cand) if cand.size else None)


def walk(M, tris, tree, q, rmax, within=False):
    """query_walk with TriDistBody for ONE query triangle q [3, 3] over build_tree's tree: the record [8] (float32) or the flag,
    and the number of leaves tested"""
    nodes, root = tree
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    q = np.asarray(q, F).reshape(3, 3)
    rmax = F(rmax)
    rec = miss_records(1)[0]
    if root is None or not query_valid(q[None], np.asarray([rmax], F))[0]:
        return (False if within else rec), 0
    bound = point_bound(M)
    gl, gh = box_rows(M, q)
    best, btri, found, tested = rmax_bound(rmax), -1, False, 0
    bw = (F(0),) * 4
    stack = [root]
    while stack:
        mn, mx, left, right = nodes[stack.pop()]
        if right is None:
            kids = [(F(0), left)]
        else:
            kids = [(lb2(bound, gl, gh, nodes[k][0], nodes[k][1]), k) for k in (left, right)]
            kids = [(key, nodes[k][2] if nodes[k][3] is None else k, nodes[k][3] is None) for key, k in kids if key <= best]
            later = sorted([k for k in kids if not k[2]], key=lambda k: k[0], reverse=True)   # the nearer child is popped first
            stack.extend(k[1] for k in later)
            kids = [(k[0], k[1]) for k in kids if k[2]]
        for _, link in kids:
            tri = ~link
            if not within and found and best == 0 and tri > btri:   # (tri_dist.hip leaf(): it cannot replace the record)
                continue
            tested += 1
            v0, e1, e2 = _split(tris[tri:tri + 1])
            d2, u, v, s, t = (x[0] for x in tri_dist(v0, e1, e2, q[None, 0], q[None, 1], q[None, 2]))
            with np.errstate(invalid="ignore"):
                counts = np.sqrt(d2) <= rmax and (d2 < best or (d2 == best and (tri & 0xffffffff) < (btri & 0xffffffff)))
            if counts:
                found = True
                if within:
                    return True, tested
                best, btri, bw = d2, tri, (u, v, s, t)
    if within:
        return False, tested
    if found:
        rec[0], rec[1], rec[2], rec[4], rec[5] = bw[0], bw[1], np.sqrt(best), bw[2], bw[3]
        rec.view(np.int32)[3] = btri
    return rec, tested
