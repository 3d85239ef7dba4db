"""The triangle queries of an instance world (psm_world_tri_overlaps_dev / psm_world_tri_count_dev / psm_world_tri_triangles_dev,
include/psm_hip.h "triangle queries over a world"; world_tri.hip) in numpy, in two parts.

(a) The flat answer: tri_query_model's float32 tri_tri over the forward-posed leaves (world_box_query_model.posed_leaves) of every
    instance of the ordered list: a flag, the count summed over the instances, and the min(k, c) lowest (inst, tri) ascending. A
    world must answer exactly this.
(b) A float32 restatement of what world_tri.hip adds to that: world_box_query_model's top-level test, prune and walk, driven by
    the query's bounding box [min(a, b, c), max(a, b, c)] (selections: exact), with the prune applied to each leaf's own image box
    under the instance's fit transform with NO padding -- so (b) == (a) says that neither level ever cuts a candidate that counts.
    (b) also returns the instances each query entered.

An instance here is (tris [T, 3, 3], cand, pose [3, 4], M [3, 4]) as in world_box_query_model; (a) reads the first three alone."""
import numpy as np

import tri_query_model as TQ
import world_box_query_model as WB

F = np.float32
D = np.float64
U = np.uint32
K_MAX = TQ.K_MAX


def bounds(q):
    """the bounding box of every query triangle [n, 3, 3]: lo, hi [n, 3] float32 by tri_min3 / tri_max3's selections (a NaN
    coordinate leaves the box to the comparisons; such a query is invalid and never walks)"""
    q = np.asarray(q, F).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        return TQ._min3(q[:, 0], q[:, 1], q[:, 2]).astype(F), TQ._max3(q[:, 0], q[:, 1], q[:, 2]).astype(F)


# ---- (a) the flat answer ------------------------------------------------------------------------------------------------------------

def counts_matrix(inst, q, staged=True):
    """[queries, candidates] bool for one instance, and its sorted candidate ids. staged: tri_tri's three unit axes are evaluated
    for every pair first, in tri_tri's own float32 operations, and all 20 axes only for the pairs that pass them -- the same
    answer as tri_tri on every pair (test_world_tri_cpu holds the two against each other)"""
    tris, cand, pose = inst[0], inst[1], inst[2]
    q = np.asarray(q, F).reshape(-1, 3, 3)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    valid = TQ.tri_valid(q)
    ok = np.zeros((q.shape[0], cand.size), bool)
    if cand.size == 0 or q.shape[0] == 0:
        return ok, cand
    v0, e1, e2 = WB.posed_leaves(np.asarray(tris, F).reshape(-1, 3, 3)[cand], pose)
    step = max(1, (1 << 18) // cand.size)
    with np.errstate(all="ignore"):
        for s in range(0, q.shape[0], step):
            t = min(q.shape[0], s + step)
            a, b, c = q[s:t, None, 0, :], q[s:t, None, 1, :], q[s:t, None, 2, :]
            if staged:
                ok[s:t] = TQ._unit_pass(v0[None], e1[None], e2[None], a, b, c) & valid[s:t, None]
            else:
                ok[s:t] = TQ.tri_tri(v0[None], e1[None], e2[None], a, b, c) & valid[s:t, None]
    if staged:
        r, c = np.nonzero(ok)
        for s in range(0, r.size, 1 << 18):
            i, j = r[s:s + (1 << 18)], c[s:s + (1 << 18)]
            ok[i, j] = TQ.tri_tri(v0[j], e1[j], e2[j], q[i, 0], q[i, 1], q[i, 2])
    return ok, cand


def posed_world(insts):
    """every instance's sorted candidates posed forward, end to end: (v0, e1, e2 [L, 3] float32, tri [L], first [J], size [J])"""
    v0s, e1s, e2s, ts, size = [np.zeros((0, 3), F)], [np.zeros((0, 3), F)], [np.zeros((0, 3), F)], [np.zeros(0, np.int64)], []
    for inst in insts:
        cand = np.sort(np.asarray(inst[1], np.int64).reshape(-1))
        size.append(cand.size)
        if cand.size:
            v0, e1, e2 = WB.posed_leaves(np.asarray(inst[0], F).reshape(-1, 3, 3)[cand], inst[2])
            v0s.append(v0), e1s.append(e1), e2s.append(e2), ts.append(cand)
    size = np.array(size, np.int64).reshape(-1)
    return np.concatenate(v0s), np.concatenate(e1s), np.concatenate(e2s), np.concatenate(ts), np.cumsum(size) - size, size


def may_meet_all(posed, lo, hi):
    """[queries, instances] bool: WB.may_meet of every instance for the bounding boxes lo / hi, as one matrix (a world of
    thousands of instances pays for one pass per instance otherwise): the same bounds, the same 2^-18 slack"""
    v0, e1, e2, _, first, size = posed
    lo, hi = np.asarray(lo, F).reshape(-1, 3).astype(D), np.asarray(hi, F).reshape(-1, 3).astype(D)
    J = size.size
    blo, bhi, mag = np.full((J, 3), np.inf), np.full((J, 3), -np.inf), np.zeros(J)
    for j in np.nonzero(size)[0]:
        a, b, c = (x[first[j]:first[j] + size[j]].astype(D) for x in (v0, e1, e2))
        pts = np.concatenate([a, a + b, a + c])
        blo[j], bhi[j], mag[j] = pts.min(0), pts.max(0), np.abs(pts).max() + np.abs(b).max() + np.abs(c).max()
    out = np.zeros((lo.shape[0], J), bool)
    step = max(1, (1 << 21) // max(J, 1))
    with np.errstate(invalid="ignore"):
        qmag = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1)
        for s in range(0, lo.shape[0], step):
            t = min(lo.shape[0], s + step)
            slack = (2.0 ** -18 * (qmag[s:t, None] + mag[None, :]))[:, :, None]
            out[s:t] = ~((lo[s:t, None, :] > bhi[None] + slack) | (hi[s:t, None, :] < blo[None] - slack)).any(axis=-1)
    return out


def flat(insts, q, k=K_MAX):
    """(a): (overlaps [R] bool, count [R] uint32, tri [R, k] int32, inst [R, k] int32, rows' count [R] uint32). An instance is
    looked at only for the queries whose bounding box can pass the unit axes for some leaf of it (may_meet_all: tri_tri's unit axes
    are box_tri's for that box), and all 20 axes are evaluated only for the pairs that pass the unit axes -- shortcuts of the
    brute force alone, held against tri_tri on every pair by the CPU test"""
    q = np.asarray(q, F).reshape(-1, 3, 3)
    R = q.shape[0]
    valid = TQ.tri_valid(q)
    lo, hi = bounds(q)
    posed = posed_world(insts)
    v0, e1, e2, tri, first, size = posed
    zero = np.zeros_like(e1)
    tmin, tmax = TQ._min3(zero, e1, e2), TQ._max3(zero, e1, e2)               # the stored triangle's interval on the unit axes
    pr, pj = np.nonzero(may_meet_all(posed, lo, hi) & valid[:, None])        # the (query, instance) pairs to look at
    rs, ls = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    ends = np.cumsum(size[pj])
    at = 0
    with np.errstate(all="ignore"):
        while at < pr.size:                                                    # about 2^20 (query, leaf) pairs at a time
            to = max(at + 1, int(np.searchsorted(ends, (ends[at - 1] if at else 0) + (1 << 20), side="right")))
            n = size[pj[at:to]]
            r = np.repeat(pr[at:to], n)
            leaf = np.repeat(first[pj[at:to]] - (np.cumsum(n) - n), n) + np.arange(n.sum())
            for x in range(3):                                                 # tri_tri's unit axes, one at a time (TQ._unit_pass)
                A, B, C = (q[r, v, x] - v0[leaf, x] for v in range(3))
                ok = (tmax[leaf, x] >= TQ._min3(A, B, C)) & (TQ._max3(A, B, C) >= tmin[leaf, x])
                r, leaf = r[ok], leaf[ok]
            ok = TQ.tri_tri(v0[leaf], e1[leaf], e2[leaf], q[r, 0], q[r, 1], q[r, 2])
            rs.append(r[ok])
            ls.append(leaf[ok])
            at = to
    r, leaf = np.concatenate(rs), np.concatenate(ls)
    order = np.lexsort((leaf, r))                      # by query, then (inst, tri): the leaves lie in that order
    r, leaf = r[order], leaf[order]
    j, t = np.searchsorted(first + size, leaf, side="right"), tri[leaf]
    count = np.bincount(r, minlength=R).astype(np.int64)
    rank = np.arange(r.size) - (np.cumsum(count) - count)[r]
    trows, irows = np.full((R, k), -1, np.int32), np.full((R, k), -1, np.int32)
    keep = rank < k
    trows[r[keep], rank[keep]] = t[keep]
    irows[r[keep], rank[keep]] = j[keep]
    count = count.astype(U)
    return count > 0, count, trows, irows, np.minimum(count, U(k)).astype(U)


# ---- (b) the two tests and the walk ---------------------------------------------------------------------------------------------------

class TriWorld(WB.BoxWorld):
    """(b): world_query_model's boxes and tree, world_tri.hip's tests and walk: WorldBoxPrune on the query's bounding box"""

    def tris(self, q, k=K_MAX):
        """((overlaps, count, tri, inst, rows' count), (entered by the count / triangles walk, entered by the overlaps walk))"""
        q = np.asarray(q, F).reshape(-1, 3, 3)
        R = q.shape[0]
        valid = TQ.tri_valid(q)
        lo, hi = bounds(q)
        ent = ([], [])
        if not self.box_insts:
            return flat([], q, k), ([[] for _ in range(R)], [[] for _ in range(R)])
        pairs = [counts_matrix(inst, q) for inst in self.box_insts]
        sel = np.nonzero(valid)[0]
        keeps = []
        for inst in self.box_insts:                              # (the prune of a valid query alone: an invalid one never walks)
            kp = np.zeros_like(pairs[len(keeps)][0])
            kp[sel] = WB.prune_keeps(inst, lo[sel], hi[sel])
            keeps.append(kp)
        seen = [np.zeros_like(p[0]) for p in pairs]           # what the full walk reaches and counts
        flag = np.zeros(R, bool)
        for i in range(R):
            if not valid[i]:
                ent[0].append([])
                ent[1].append([])
                continue

            def keep(clo, chi):
                return WB.top_keep(clo, chi, lo[i], hi[i]), F(0)

            def visit_all(j):
                seen[j][i] = pairs[j][0][i] & keeps[j][i]
                return False

            def visit_any(j):
                flag[i] |= bool((pairs[j][0][i] & keeps[j][i]).any())
                return bool(flag[i])
            ent[0].append(self.tree.walk(keep, visit_all))
            ent[1].append(self.tree.walk(keep, visit_any))
        f, count, trows, irows, nrows = WB.rows_of(seen, [p[1] for p in pairs], k)
        return (flag, count, trows, irows, nrows), ent

    def reachable(self, q):
        """brute force: per query the set of instances whose padded world box meets the slack-grown bounding box"""
        q = np.asarray(q, F).reshape(-1, 3, 3)
        valid = TQ.tri_valid(q)
        lo, hi = bounds(q)
        return [sorted(j for j in range(len(self.box_insts)) if WB.top_keep(self.lo[j], self.hi[j], lo[i], hi[i])) if valid[i] else []
                for i in range(q.shape[0])]


# ---- the prune's chain, evaluated in float64 ---------------------------------------------------------------------

def prune_figures(inst, q):
    """world_box_query_model.prune_figures for the queries' bounding boxes, with the pairs that count under tri_tri in the place
    of those under box_tri: (counts [Q, C], the float32 interval keeps the leaf's exact unpadded image [Q, C], observed, bound,
    granted [Q, C, 3]). The chain's terms are 4.16's: the candidate test enters through its unit axes alone, which are box_tri's
    for [lo, hi]"""
    lo, hi = bounds(q)
    _, kept, observed, bound, granted = WB.prune_figures(inst, lo, hi)
    ok, _ = counts_matrix(inst, q)
    return ok, kept, observed, bound, granted
