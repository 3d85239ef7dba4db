"""The clearance queries of an instance world (psm_world_tri_closest_dev / psm_world_tri_within_dev, include/psm_hip.h "clearance
queries over a world"; world_tri_dist.hip) in numpy, in two parts.

(a) The flat answer: tri_dist_query_model's float32 tri_dist over the forward-posed leaves (world_box_query_model.posed_leaves) of
    every instance of the ordered list; of the pairs with sqrt(d2) <= rmax the smallest d2, on a bit-equal d2 the lowest
    (inst, tri). A world must answer exactly this.
(b) A float32 restatement of what world_tri_dist.hip adds to that: the top-level gap test against the padded world boxes of
    world_query_model's tree, world_box_query_model's prune_interval and tri_dist_query_model's lb2 inside an instance, both
    against best (1 + WORLD_PSLACK), the nearer child first, and the two shortcuts of a record at d2 == 0. The hierarchy of an
    instance is the builder's and is not restated: lb2 is applied to each leaf's own image box under the instance's fit
    transform with NO padding (a leaf the model keeps is kept by the kernel, whose leaf boxes are that image padded and whose
    inner boxes are unions), the leaves nearer first. (b) == (a) says that neither level cuts a pair that counts; (b) also
    returns the instances each query entered and the (instance, triangle) pairs it tested.

An instance here is (tris [T, 3, 3], cand, pose [3, 4], M [3, 4]) as in world_box_query_model; (a) reads the first three alone."""
import numpy as np

import tri_dist_query_model as TD
import tri_query_model as TQ
import world_box_query_model as WB
import world_query_model as WQ
import world_tri_query_model as WT

F = np.float32
D = np.float64
WORLD_QSLACK = WQ.WORLD_QSLACK
WORLD_PSLACK = WQ.WORLD_PSLACK


# ---- (a) the flat answer ------------------------------------------------------------------------------------------------------------

def pair_records(inst, q):
    """tri_dist of every (query, candidate) pair of one instance: (d2, u, v, s, t) [R, C] float32 and the sorted candidate ids;
    tri_tri is evaluated only for the pairs that pass its unit axes (the others it separates), as tri_dist_query_model.query"""
    tris, cand, pose = inst[0], inst[1], inst[2]
    q = np.asarray(q, F).reshape(-1, 3, 3)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    R, C = q.shape[0], cand.size
    out = [np.zeros((R, C), F) for _ in range(5)]
    if R == 0 or C == 0:
        return tuple(out) + (cand,)
    v0, e1, e2 = WB.posed_leaves(np.asarray(tris, F).reshape(-1, 3, 3)[cand], pose)
    step = max(1, (1 << 15) // C)
    with np.errstate(all="ignore"):
        for lo in range(0, R, step):
            hi = min(R, lo + step)
            qa, qb, qc = q[lo:hi, None, 0, :], q[lo:hi, None, 1, :], q[lo:hi, None, 2, :]
            meet = TQ._unit_pass(v0[None], e1[None], e2[None], qa, qb, qc)
            i, j = np.nonzero(meet)
            if i.size:
                meet[i, j] = TQ.tri_tri(v0[j], e1[j], e2[j], q[lo + i, 0], q[lo + i, 1], q[lo + i, 2])
            for k, x in enumerate(TD.tri_dist(v0[None], e1[None], e2[None], qa, qb, qc, meet=meet)):
                out[k][lo:hi] = x
    return tuple(out) + (cand,)


def flat(insts, q, rmax=np.inf, pairs=None):
    """(a): (hits [R, 8] float32 as the kernel writes psm_tri_hit, inst [R] int32, within [R] bool)"""
    q = np.asarray(q, F).reshape(-1, 3, 3)
    R = q.shape[0]
    rm = np.broadcast_to(np.asarray(rmax, F), (R,)).astype(F)
    valid = TD.query_valid(q, rm)
    hits, inst, within = TD.miss_records(R), np.full(R, -1, np.int32), np.zeros(R, bool)
    pairs = [pair_records(i, q) for i in insts] if pairs is None else pairs
    if not pairs or sum(p[5].size for p in pairs) == 0:
        return hits, inst, within
    d2, u, v, s, t = (np.concatenate([p[k] for p in pairs], axis=1) for k in range(5))   # columns ascend in (inst, tri)
    tri = np.concatenate([p[5] for p in pairs])
    owner = np.concatenate([np.full(p[5].size, j, np.int64) for j, p in enumerate(pairs)])
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2)
        ok = valid[:, None] & (dist <= rm[:, None])
    within = ok.any(axis=1)
    best = np.where(ok, d2, F(np.inf)).min(axis=1)
    k = np.argmax(ok & (d2 == best[:, None]), axis=1)
    r = np.arange(R)
    for col, x in ((0, u), (1, v), (4, s), (5, t)):
        hits[:, col] = np.where(within, x[r, k], F(0))
    hits[:, 2] = np.where(within, dist[r, k], F(np.inf))
    hits.view(np.int32)[:, 3] = np.where(within, tri[k], -1)
    inst = np.where(within, owner[k], -1).astype(np.int32)
    return hits, inst, within


def flat_near(insts, q, rmax=np.inf):
    """flat() for thousands of queries: an instance is looked at only for the queries it can hold the winner of. In float64,
    with [blo, bhi] the box of an instance's posed leaves: no pair of instance j is nearer to query i than the gap between that
    box and the query's bounding box. Every query first meets the instance of the smallest gap; the smallest distance found
    there bounds the winner's, and an instance whose gap exceeds it by more than a part in a thousand of it and of the
    coordinates' size (float32 distances differ from the real ones by parts in a million of that) cannot hold the smallest d2:
    its pairs are left out (NaN: they never count). A shortcut of the brute force alone, held against flat() by the CPU test."""
    q = np.asarray(q, F).reshape(-1, 3, 3)
    R, J = q.shape[0], len(insts)
    lo, hi = (x.astype(D) for x in WT.bounds(q))
    gap = np.full((R, J), np.inf)
    size = np.ones(R)
    with np.errstate(invalid="ignore"):
        for j, inst in enumerate(insts):
            cand = np.sort(np.asarray(inst[1], np.int64).reshape(-1))
            if cand.size:
                v0, e1, e2 = (x.astype(D) for x in WB.posed_leaves(np.asarray(inst[0], F).reshape(-1, 3, 3)[cand], inst[2]))
                pts = np.concatenate([v0, v0 + e1, v0 + e2])
                gap[:, j] = np.linalg.norm(np.maximum(np.maximum(pts.min(0) - hi, lo - pts.max(0)), 0.0), axis=1)
                size = np.maximum(size, np.abs(pts).max())
        size = np.maximum(size, np.maximum(np.abs(lo), np.abs(hi)).max(axis=1))
    gap = np.where(np.isnan(gap), np.inf, gap)                   # (an invalid query: it never counts, nothing is looked at)
    full = [[np.full((R, np.asarray(i[1]).size), np.nan, F) for _ in range(5)] for i in insts]
    cands = [np.sort(np.asarray(i[1], np.int64).reshape(-1)) for i in insts]

    def look(j, rows):
        if rows.size and cands[j].size:
            sub = pair_records(insts[j], q[rows])
            for k in range(5):
                full[j][k][rows] = sub[k]
    first = np.argmin(gap, axis=1) if J else np.zeros(R, np.int64)
    reached = np.isfinite(gap[np.arange(R), first]) if J else np.zeros(R, bool)
    found = np.full(R, np.inf)
    for j in range(J):
        rows = np.nonzero(reached & (first == j))[0]
        look(j, rows)
        if rows.size and cands[j].size:
            d2 = full[j][0][rows].astype(D)
            found[rows] = np.sqrt(np.where(np.isnan(d2), np.inf, d2).min(axis=1))
    limit = found * (1 + 1e-3) + 1e-3 * size
    for j in range(J):
        look(j, np.nonzero(reached & (first != j) & ~(gap[:, j] > limit))[0])
    return flat(insts, q, rmax, [tuple(full[j]) + (cands[j],) for j in range(J)])


# ---- (b) the two tests and the walk ---------------------------------------------------------------------------------------------------

def slackened(best):
    """best (1 + WORLD_PSLACK) as the kernel forms it: fl(best + fl(WORLD_PSLACK * best))"""
    with np.errstate(all="ignore"):
        return F(best + F(WORLD_PSLACK * best))


def top_gap2(clo, chi, lo, hi):
    """WorldTriDistBody::gap2: the squared gap between the bounding box [lo, hi] and the child box [clo, chi] grown by
    WORLD_QSLACK * |q|_inf (fmax: a NaN term is taken as 0)"""
    with np.errstate(all="ignore"):
        pad = F(WORLD_QSLACK * max(F(np.abs(lo).max()), F(np.abs(hi).max())))
        g = np.fmax(np.fmax(((clo - pad).astype(F) - hi).astype(F), (lo - (chi + pad).astype(F)).astype(F)), F(0))
        return F(F(g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])


def leaf_lb2(inst, lo, hi):
    """[queries, candidates] float32: lb2 of every leaf's own unpadded image box (float64, rounded to float32) against the grown
    intervals of each query's bounding box in that instance, and the sorted candidates"""
    tris, cand, pose, M = inst
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    if cand.size == 0:
        return np.zeros((lo.shape[0], 0), F), cand
    tmin, tmax = WB.leaf_images(np.asarray(tris, F).reshape(-1, 3, 3)[cand], M)
    gl, gh, _ = WB.prune_interval(M, pose, lo, hi)
    return TD.lb2(TD.point_bound(M), gl[:, None, :], gh[:, None, :], tmin.astype(F)[None], tmax.astype(F)[None]), cand


class TriDistWorld(WB.BoxWorld):
    """(b): world_query_model's boxes and tree, world_tri_dist.hip's tests and walk"""

    def closest(self, q, rmax=np.inf, within=False, pairs=None):
        """((hits, inst) or the flags, entered [R] lists of instances, tested [R] lists of (inst, tri))"""
        q = np.asarray(q, F).reshape(-1, 3, 3)
        R = q.shape[0]
        rm = np.broadcast_to(np.asarray(rmax, F), (R,)).astype(F)
        valid = TD.query_valid(q, rm)
        lo, hi = WT.bounds(q)
        hits, inst, flags = TD.miss_records(R), np.full(R, -1, np.int32), np.zeros(R, bool)
        entered, tested = [[] for _ in range(R)], [[] for _ in range(R)]
        if not self.box_insts:
            return (flags if within else (hits, inst)), entered, tested
        pairs = [pair_records(i, q) for i in self.box_insts] if pairs is None else pairs
        sel = np.nonzero(valid)[0]
        lbs = []
        for i_ in self.box_insts:                               # (the prune of a valid query alone: an invalid one never walks)
            lb, cand = leaf_lb2(i_, lo[sel], hi[sel])
            full = np.zeros((R, cand.size), F)
            full[sel] = lb
            lbs.append(full)
        for i in sel:
            st = {"best": TD.rmax_bound(rm[i]), "inst": -1, "tri": -1, "found": False, "w": None}

            def settled():
                return (not within) and st["found"] and st["best"] == 0

            def keep(clo, chi):
                k = top_gap2(clo, chi, lo[i], hi[i])
                return bool(not k > slackened(st["best"])), k

            def visit(j):
                if settled() and j > st["inst"]:
                    return False
                entered[i].append(j)
                d2, u, v, s, t, cand = pairs[j]
                lb = lbs[j][i]
                order = np.argsort(lb, kind="stable")           # the nearer leaf first
                order = order[lb[order] <= slackened(st["best"])]
                for c in order:
                    tri = int(cand[c])
                    if not lb[c] <= slackened(st["best"]):
                        continue
                    if settled() and not (j < st["inst"] or (j == st["inst"] and tri < st["tri"])):
                        continue
                    tested[i].append((j, tri))
                    x = d2[i, c]
                    with np.errstate(invalid="ignore"):
                        wins = x < st["best"] or (x == st["best"] and (st["inst"] < 0 or j < st["inst"] or (j == st["inst"] and tri < st["tri"])))
                        counts = bool(np.sqrt(x) <= rm[i]) and bool(wins)
                    if counts:
                        st["found"] = True
                        if within:
                            return True
                        st.update(best=x, inst=j, tri=tri, w=(u[i, c], v[i, c], s[i, c], t[i, c]))
                return False
            self.tree.walk(keep, visit)
            if within:
                flags[i] = st["found"]
            elif st["found"]:
                hits[i, 0], hits[i, 1], hits[i, 4], hits[i, 5] = st["w"]
                hits[i, 2] = np.sqrt(st["best"])
                hits.view(np.int32)[i, 3] = st["tri"]
                inst[i] = st["inst"]
        return (flags if within else (hits, inst)), entered, tested


# ---- the prune's margin, read in float64 ---------------------------------------------------------------------------

def ancestors_top(tree, j):
    """the child boxes (lo, hi) of the top-level tree that contain instance j: its own box and every ancestor's below the root"""
    out = []

    def down(link):
        if link < 0:
            return ~link == j
        loL, hiL, lL, loR, hiR, lR = tree.nodes[link]
        if down(lL):
            out.append((loL, hiL))
            return True
        if down(lR):
            out.append((loR, hiR))
            return True
        return False
    if tree.n > 1:
        down(0)
    return out


def ancestors_inside(tree, tri):
    """the boxes (mn, mx) of tri_dist_query_model.build_tree's tree on the way from the root's children to the leaf of `tri`: a
    real tree, fp16 boxes padded as the build pads them, inner boxes the unions"""
    nodes, root = tree
    out = []

    def down(k):
        mn, mx, left, right = nodes[k]
        if right is None:
            return ~left == tri
        for c in (left, right):
            if down(c):
                out.append((nodes[c][0], nodes[c][1]))
                return True
        return False
    if root is not None:
        down(root)
    return out


def margin_figures(world, q, hits, inst, trees):
    """For every query with a winner at d2 > 0: the largest LB^2 / d2 over the top-level boxes above the winning instance, and
    over the boxes above the winning leaf inside it -- LB^2 the kernel's float32 lower bound (top_gap2; lb2 on prune_interval),
    d2 the winner's float32 forward-posed squared distance, the quotient in float64. For a winner at d2 == 0 every LB^2 must
    be 0; the count of those that are not is returned as well. trees[j]: build_tree of instance j.
    Returns (top [n], inside [n], nonzero_at_zero)"""
    q = np.asarray(q, F).reshape(-1, 3, 3)
    lo, hi = WT.bounds(q)
    top, inside, bad = [], [], 0
    for i in np.nonzero(inst >= 0)[0]:
        j, tri = int(inst[i]), int(hits.view(np.int32)[i, 3])
        tris, cand, pose, M = world.box_insts[j]
        pr = pair_records((tris, [tri], pose), q[i:i + 1])
        d2 = D(pr[0][0, 0])
        gl, gh, _ = WB.prune_interval(M, pose, lo[i], hi[i])
        bound = TD.point_bound(M)
        t = [D(top_gap2(a, b, lo[i], hi[i])) for a, b in ancestors_top(world.tree, j)]
        n = [D(TD.lb2(bound, gl, gh, a, b)) for a, b in ancestors_inside(trees[j], tri)]
        if d2 == 0:
            bad += sum(x != 0 for x in t + n)
            continue
        top.append(max(t) / d2 if t else 0.0)
        inside.append(max(n) / d2 if n else 0.0)
    return np.array(top), np.array(inside), bad
