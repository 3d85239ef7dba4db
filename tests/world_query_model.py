"""The instance-world queries (psm_world_*_dev, include/psm_hip.h "instance worlds") in numpy, in two parts.

(a) The flat answer: instance_query_model over all N instances. Its combination in list order IS the general rule -- the
    smallest value, on an equal value the lexicographically lowest (inst, tri); OR; sum; parity over all instances. A world must
    answer exactly this, whatever its tree looks like.
(b) A float32 restatement of what world.hip adds: the object-space box of a hierarchy, the padded world box of an instance, the
    Morton keys and the tree over them, the inner boxes as exact min / max unions, and the two-level walk with its padded, slackened
    box tests, nearer child first, pruned against the best so far. What happens INSIDE an instance is not restated: entering an
    instance takes that instance's own answer from the per-instance yardsticks (query_model, point_query_model,
    inside_query_model on the moved query), which within one instance is order-independent. (b) returns the answer and the
    list of instances each query entered; (b) == (a) bit for bit says the culling never shows, the entered counts say it culls.

An instance is (tris [T, 3, 3], cand, pose) as in instance_query_model."""
import numpy as np

import inside_query_model as IQ
import instance_query_model as NQ
import point_query_model as PQ
import query_model as Q
import scene_query_model as SQ

F = np.float32
U = np.uint32
# world.hip's constants (DESIGN.md 4.11 derives them)
WORLD_PAD = F(2.0 ** -11)
WORLD_FLOOR = F(2.0 ** -100)
WORLD_QSLACK = F(2.0 ** -11)
WORLD_TSLACK = F(2.0 ** -12)
WORLD_PSLACK = F(2.0 ** -11)
QSTACK_MAX = 96


# ---- (a) the flat answer ----------------------------------------------------------------------------------------------------------

def per_instance_rays(insts, o, d, tmin, tmax):
    """each instance's own answers to the moved rays: [(hits [R, 4], any [R], count [R])]"""
    out = []
    for t, c, m in insts:
        mo, md = NQ.move(m, o), NQ.rotate(m, d)
        h, a = Q.query(t, c, mo, md, tmin, tmax)
        out.append((h, a, IQ.count(t, c, mo, md, tmin, tmax)))
    return out


def per_instance_points(insts, p, rmax):
    """each instance's own answers to the moved points: [(hits [R, 4], within [R], d2 [R])]"""
    out = []
    for t, c, m in insts:
        mp = NQ.move(m, p)
        h, w = PQ.query(t, c, mp, rmax)
        out.append((h, w, SQ.d2_of(t, mp, h)))
    return out


def per_instance_parities(insts, p, samples):
    """[instance][k]: the crossings of world ray k of every point, moved into the instance: uint32 [R]"""
    p = np.asarray(p, F).reshape(-1, 3)
    return [[IQ.count(t, c, NQ.move(m, p), NQ.rotate(m, np.broadcast_to(IQ.INSIDE_DIRECTIONS[k], p.shape)), F(0), F(np.inf))
             for k in range(samples)] for t, c, m in insts]


def flat_rays(per):
    """(a) of the ray queries from per_instance_rays: hits, inst, any, count"""
    hits, inst = SQ.combine_closest([r[0] for r in per])
    return hits, inst, np.logical_or.reduce([r[1] for r in per]), np.sum([r[2] for r in per], axis=0, dtype=U)


def flat_points(per):
    """(a) of the point queries from per_instance_points: hits, inst, within"""
    hits, inst = SQ.combine_closest([r[0] for r in per], [r[2] for r in per])
    return hits, inst, np.logical_or.reduce([r[1] for r in per])


def flat_parities(par):
    """(a): [samples, R] bool from per_instance_parities"""
    return (np.sum(np.asarray(par, np.uint64), axis=0) & 1) == 1


def signed(hits, inst, ins):
    out = hits.copy()
    out.view(U)[(inst >= 0) & ins, 2] |= U(0x80000000)
    return out


# ---- (b) boxes and tree -----------------------------------------------------------------------------------------------------------

def object_box(tris):
    """world_obj_boxes: min / max over v0, v0 + e1, v0 + e2 of every triangle, as the candidate tests hold them (float32)"""
    t = np.asarray(tris, F).reshape(-1, 3, 3)
    v0, e1, e2 = t[:, 0], (t[:, 1] - t[:, 0]).astype(F), (t[:, 2] - t[:, 0]).astype(F)
    pts = np.concatenate([v0, (v0 + e1).astype(F), (v0 + e2).astype(F)])
    return np.fmin.reduce(pts, axis=0).astype(F), np.fmax.reduce(pts, axis=0).astype(F)


def world_box(lo, hi, pose):
    """world_inst_boxes: centre R c + T, half extent |R| e, grown by WORLD_PAD * S + WORLD_FLOOR (one float32 operation order)"""
    m = np.asarray(pose, F).reshape(3, 4)
    h = F(0.5)
    c = (h * lo + h * hi).astype(F)
    e = (h * hi - h * lo).astype(F)
    S = max(F(np.abs(lo).max()), F(np.abs(hi).max()), F(np.abs(m[:, 3]).max()))
    cw, ew = np.zeros(3, F), np.zeros(3, F)
    for k in range(3):
        cw[k] = F(F(F(m[k, 0] * c[0]) + F(m[k, 1] * c[1])) + F(m[k, 2] * c[2])) + m[k, 3]
        ew[k] = F(F(abs(m[k, 0]) * e[0]) + F(abs(m[k, 1]) * e[1])) + F(abs(m[k, 2]) * e[2])
        S = max(S, F(abs(cw[k]) + ew[k]))
    pad = F(F(WORLD_PAD * S) + WORLD_FLOOR)
    return ((cw - ew).astype(F) - pad).astype(F), ((cw + ew).astype(F) + pad).astype(F)


def _part1by2(a):
    x = 0
    for b in range(21):
        x |= ((a >> b) & 1) << (3 * b)
    return x


def morton_keys(blo, bhi):
    """world_morton: (48-bit Morton code of the box centre over the centres' bounds) << 16 | index, python ints"""
    h = F(0.5)
    c = (h * blo + h * bhi).astype(F)
    lo, hi = c.min(axis=0), c.max(axis=0)
    keys = []
    for i in range(c.shape[0]):
        q = []
        for j in range(3):
            ext = F(hi[j] - lo[j])
            f = F(F(c[i, j] - lo[j]) / ext) if ext > 0 else F(0)
            f = min(max(f, F(0)), F(1))
            q.append(min(int(F(f * F(65536.0))), 65535))
        keys.append(((_part1by2(q[0]) | (_part1by2(q[1]) << 1) | (_part1by2(q[2]) << 2)) << 16) | i)
    return keys


class Tree:
    """the tree over the instances' boxes: nodes[k] = (loL, hiL, linkL, loR, hiR, linkR); link >= 0: a node, < 0: ~instance.
    The radix tree over the sorted distinct keys: a range splits where its highest differing key bit changes (world_emit)."""

    def __init__(self, blo, bhi):
        self.n = blo.shape[0]
        self.nodes, self.depth = [], 0
        if self.n < 2:
            return
        keys = morton_keys(blo, bhi)
        order = sorted(range(self.n), key=lambda i: keys[i])
        sk = [keys[i] for i in order]

        def make(a, b):   # -> link, lo, hi, height
            if a == b:
                i = order[a]
                return ~i, blo[i], bhi[i], 0
            bit = (sk[a] ^ sk[b]).bit_length() - 1
            s = a
            while (sk[s + 1] >> bit) & 1 == 0:   # the last key of the range with that bit clear
                s += 1
            me = len(self.nodes)
            self.nodes.append(None)
            lL, loL, hiL, hL = make(a, s)
            lR, loR, hiR, hR = make(s + 1, b)
            self.nodes[me] = (loL, hiL, lL, loR, hiR, lR)
            return me, np.fmin(loL, loR), np.fmax(hiL, hiR), max(hL, hR) + 1

        _, _, _, self.depth = make(0, self.n - 1)

    def walk(self, keep, visit):
        """world_walk's top level: keep(lo, hi) -> (ok, key); visit(inst) -> True when the query retires. Returns the instances
        entered, in order."""
        entered = []
        stack = [0 if self.n > 1 else ~0]
        while stack:
            cur = stack.pop()
            if cur < 0:
                entered.append(~cur)
                if visit(~cur):
                    break
                continue
            loL, hiL, lL, loR, hiR, lR = self.nodes[cur]
            okL, kL = keep(loL, hiL)
            okR, kR = keep(loR, hiR)
            left_first = okL and (not okR or kL <= kR)
            first, second = (lL, lR) if left_first else (lR, lL)
            if okL and okR:
                stack.append(second)
            if okL or okR:
                stack.append(first)
        return entered


class World:
    """(b): boxes, tree and walk of a list of instances"""

    def __init__(self, insts):
        self.insts = insts
        boxes = {}
        lo, hi = [], []
        for t, _, m in insts:
            if id(t) not in boxes:
                boxes[id(t)] = object_box(t)
            a, b = world_box(*boxes[id(t)], m)
            lo.append(a)
            hi.append(b)
        self.lo, self.hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
        self.tree = Tree(self.lo, self.hi)

    # -- the top level's tests, one query at a time (numpy float32 scalars; fmin / fmax are minNum / maxNum) --

    @staticmethod
    def _ray_keep(o, d, tmin, lim):
        """lim: a callable giving the bound to prune against (tmax, or the best t so far)"""
        with np.errstate(all="ignore"):
            dn = (d * (F(1) / np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))).astype(F)
            nocull = not (np.isfinite(dn).all() and F(F(dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2]) > F(0.5))
            iv = (F(1) / dn).astype(F)
            qpad = F(WORLD_QSLACK * np.abs(o).max())
            lo_t = F(tmin - F(WORLD_TSLACK * abs(tmin)))

        def keep(lo, hi):
            with np.errstate(all="ignore"):
                a = (((lo - qpad).astype(F) - o).astype(F) * iv).astype(F)
                b = (((hi + qpad).astype(F) - o).astype(F) * iv).astype(F)
                near, far = np.fmax.reduce(np.fmin(a, b)), np.fmin.reduce(np.fmax(a, b))
                x = lim()
                hi_t = F(x + F(WORLD_TSLACK * abs(x)))
                return bool(nocull or (not near > far and not near > hi_t and not far < lo_t)), near
        return keep

    @staticmethod
    def _point_keep(p, best):
        with np.errstate(all="ignore"):
            qpad = F(WORLD_QSLACK * np.abs(p).max())

        def keep(lo, hi):
            with np.errstate(all="ignore"):
                g = np.fmax(np.fmax((lo - qpad).astype(F) - p, p - (hi + qpad).astype(F)).astype(F), F(0))
                k = F(F(g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
                b = best()
                return bool(not k > F(b + F(WORLD_PSLACK * b))), k
        return keep

    # -- the queries: (answers ..., entered) with entered[i] the instances query i entered --

    def rays(self, o, d, tmin, tmax, per=None):
        """closest hit, any hit and hit count: ((hits, inst), any, count, (entered_closest, entered_any, entered_count))"""
        o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
        n = o.shape[0]
        lo, hi = np.broadcast_to(np.asarray(tmin, F), (n,)), np.broadcast_to(np.asarray(tmax, F), (n,))
        per = per_instance_rays(self.insts, o, d, lo, hi) if per is None else per
        hits, inst = SQ._miss(n), np.full(n, -1, np.int32)
        anyh, cnt = np.zeros(n, bool), np.zeros(n, U)
        ent = ([], [], [])
        for i in range(n):
            valid = bool(lo[i] <= hi[i])
            # closest
            st = {"best": hi[i], "inst": -1}

            def visit_closest(k):
                h = per[k][0][i]
                tri = int(h.view(np.int32)[3])
                if tri >= 0 and (h[2] < st["best"] or (h[2] == st["best"] and (st["inst"] < 0 or k < st["inst"]))):
                    st["best"], st["inst"] = h[2], k
                    hits[i], inst[i] = h, k
                return False
            ent[0].append(self.tree.walk(self._ray_keep(o[i], d[i], lo[i], lambda: st["best"]), visit_closest) if valid else [])

            def visit_any(k):
                anyh[i] |= bool(per[k][1][i])
                return bool(anyh[i])
            ent[1].append(self.tree.walk(self._ray_keep(o[i], d[i], lo[i], lambda: hi[i]), visit_any) if valid else [])

            def visit_count(k):
                cnt[i] += per[k][2][i]
                return False
            ent[2].append(self.tree.walk(self._ray_keep(o[i], d[i], lo[i], lambda: hi[i]), visit_count) if valid else [])
        return (hits, inst), anyh, cnt, ent

    def points(self, p, rmax, per=None):
        """closest point and within: ((hits, inst), within, (entered_closest, entered_within))"""
        p = np.asarray(p, F).reshape(-1, 3)
        n = p.shape[0]
        rm = np.broadcast_to(np.asarray(rmax, F), (n,))
        per = per_instance_points(self.insts, p, rm) if per is None else per
        hits, inst = SQ._miss(n), np.full(n, -1, np.int32)
        wi = np.zeros(n, bool)
        ent = ([], [])
        for i in range(n):
            with np.errstate(all="ignore"):
                valid = bool(np.isfinite(p[i]).all() and rm[i] >= 0)
                bound = F(F(F(rm[i] * rm[i]) * F(1.00000095367431640625)) + F(2.0 ** -126))
            st = {"best": bound, "inst": -1}

            def visit_closest(k):
                h, d2 = per[k][0][i], per[k][2][i]
                if int(h.view(np.int32)[3]) >= 0 and (d2 < st["best"] or (d2 == st["best"] and (st["inst"] < 0 or k < st["inst"]))):
                    st["best"], st["inst"] = d2, k
                    hits[i], inst[i] = h, k
                return False
            ent[0].append(self.tree.walk(self._point_keep(p[i], lambda: st["best"]), visit_closest) if valid else [])

            def visit_within(k):
                wi[i] |= bool(per[k][1][i])
                return bool(wi[i])
            ent[1].append(self.tree.walk(self._point_keep(p[i], lambda: bound), visit_within) if valid else [])
        return (hits, inst), wi, ent

    def parities(self, p, samples, par=None):
        """[samples, R] bool: ray k's crossings over the instances its walk entered are odd; and entered[k][i]"""
        p = np.asarray(p, F).reshape(-1, 3)
        n = p.shape[0]
        par = per_instance_parities(self.insts, p, samples) if par is None else par
        out = np.zeros((samples, n), bool)
        ent = [[] for _ in range(samples)]
        for k in range(samples):
            for i in range(n):
                if not np.isfinite(p[i]).all():
                    ent[k].append([])
                    continue
                tot = [0]

                def visit(j):
                    tot[0] += int(par[j][k][i])
                    return False
                ent[k].append(self.tree.walk(self._ray_keep(p[i], IQ.INSIDE_DIRECTIONS[k].astype(F), F(0), lambda: F(np.inf)), visit))
                out[k, i] = tot[0] & 1
        return out, ent


def average_entered(entered):
    return float(np.mean([len(e) for e in entered])) if entered else 0.0


# ---- the derived bound, evaluated in float64 --------------------------------------------------------------------

EPS = 2.0 ** -24


def move_bound(pose, x, objmag):
    """the bound on the WORLD-space displacement between a world point x and what the candidate test sees of it: the move's
    rounding (one subtraction, three products, two sums per coordinate: 4 eps sqrt 3 (|x| + |T|), mapped back by a matrix of norm
    <= 1 + 1.5e-5) plus the non-rigidity the pose check admits, |R^-T - R| <= 3e-5 sqrt 3 per unit of object coordinate"""
    m = np.asarray(pose, np.float64).reshape(3, 4)
    mag = np.abs(np.asarray(x, np.float64)).max() + np.abs(m[:, 3]).max()
    return 4 * EPS * np.sqrt(3.0) * mag * 1.0001 + 3e-5 * np.sqrt(3.0) * objmag


def move_discrepancy(pose, x):
    """observed: the float32 move of x mapped back to world space with the exact inverse of the float matrix, against x (float64)"""
    m = np.asarray(pose, np.float64).reshape(3, 4)
    x32 = NQ.move(pose, np.asarray(x, F).reshape(1, 3))[0].astype(np.float64)
    back = np.linalg.solve(m[:, :3].T, x32) + m[:, 3]   # R^-T x' + T: the world point whose exact move is x'
    return float(np.abs(back - np.asarray(x, F).astype(np.float64)).max()), float(np.abs(x32).max())


def forward_discrepancy(pose, x_obj):
    """observed, the other way round and with no inverse in what is measured: the distance (float64, the largest coordinate)
    between the forward image R x' + T of an object point -- what world_inst_boxes bounds -- and the float32 world point x whose
    float32 move gives x'. x is the float nearest to the exact preimage T + R^-T x_obj, and x' is the move's own result for it
    (x_obj up to the float32 grid), so the move's rounding and R against R^-T are both in the figure and the grid is not.
    Returns (observed, the largest |coordinate| of x', x)."""
    m = np.asarray(pose, F).reshape(3, 4).astype(np.float64)
    xo = np.asarray(x_obj, np.float64).reshape(3)
    x = (np.linalg.solve(m[:, :3].T, xo) + m[:, 3]).astype(F)
    seen = NQ.move(pose, x.reshape(1, 3))[0].astype(np.float64)
    fwd = m[:, :3] @ seen + m[:, 3]
    return float(np.abs(fwd - x.astype(np.float64)).max()), float(np.abs(seen).max()), x
