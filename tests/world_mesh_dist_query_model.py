"""Mesh clearance over an instance world (psm_world_mesh_closest_dev / psm_world_mesh_within_dev / psm_world_mesh_clearance_dev,
include/psm_hip.h "mesh clearance over a world"; world_mesh_dist.hip) in numpy, in two parts.

(a) The flat answer, a composition with no arithmetic of its own: the query triangle of (pose m, triangle t of `other`) is
    mesh_query_model.posed's; its record and instance are world_tri_dist_query_model.flat's for that triangle under the call's one
    rmax over the ordered instance list -- with skip = i, instance i's candidates are dropped and the indices kept; a triangle
    of other that is no leaf reads the miss record and -1. The clearance record of a pose is mesh_dist_query_model.reduce's:
    the smallest stored dist, then the lowest t, with t* in slot 6, and that cell's instance. The flag is tri >= 0 of that record.
(b) A restatement of what world_mesh_dist.hip's lanes do: world_tri_dist_query_model's two tests against best (1 + WORLD_PSLACK)
    on world_query_model's tree, skip decided where an instance is entered, and mesh_dist.hip's shared word -- read in begin(),
    re-read before every leaf, published at every improvement and at the end (the four FLAGS variants) -- with the lanes of a
    pose interleaved at leaf granularity under a schedule, a read returning any value the word has held so far. Then the pick:
    the closest walk of posed triangle t* with Dmin for rmax. (b) == (a) under every schedule is what the kernels rely on.

An instance is (tris [T, 3, 3], cand, pose [3, 4], M [3, 4]) as in world_box_query_model."""
import numpy as np

import mesh_dist_query_model as MD
import mesh_query_model as MQ
import tri_dist_query_model as TD
import world_tri_dist_query_model as WD
import world_tri_query_model as WT

F = np.float32
I = np.int32
NONE = MD.NONE
BOUND, REREAD, EARLY = 2, 4, 8                      # world_mesh_dist.hip's WMD_FLAG_*
VARIANTS = (0, BOUND, BOUND | REREAD, BOUND | REREAD | EARLY)   # PSM_MESH_BOUND = 0, 2, 3, 1


# ---- (a) the flat answer ------------------------------------------------------------------------------------------------------------

def without(insts, skip):
    """the ordered list with instance `skip` emptied: its candidates dropped, every index kept"""
    if skip is None or skip < 0:
        return list(insts)
    return [(i[0], np.zeros(0, np.int64)) + tuple(i[2:]) if j == skip else i for j, i in enumerate(insts)]


def miss_clearance(p):
    out = TD.miss_records(p)
    out.view(I)[:, 6] = -1
    return out


def reduce(hits, geom):
    """(clearance records [p, 8], their instances [p]) of the closest records [p, T, 8] and instances [p, T]"""
    rec = MD.reduce(hits)
    t = rec.view(I)[:, 6]
    inst = np.where(t >= 0, geom[np.arange(hits.shape[0]), t.clip(0)] if hits.shape[1] else -1, -1).astype(I)
    return rec, inst


def flat(insts, other_tris, other_leaves, poses, rmax=np.inf, skip=None, near=False):
    """(closest [p, T, 8], its instances [p, T], clearance [p, 8], its instances [p], within [p] bool). near: by
    world_tri_dist_query_model.flat_near, the brute force's shortcut for thousands of queries (the same answer)"""
    q = MQ.posed(other_tris, poses)
    p, t = q.shape[:2]
    hits, geom = TD.miss_records(p * t).reshape(p, t, 8), np.full((p, t), -1, I)
    keep = np.sort(np.asarray(other_leaves, np.int64).reshape(-1))
    if p and keep.size:
        h, g, _ = (WD.flat_near if near else WD.flat)(without(insts, skip), q[:, keep].reshape(-1, 3, 3), F(rmax))
        hits[:, keep], geom[:, keep] = h.reshape(p, keep.size, 8), g.reshape(p, keep.size)
    rec, inst = reduce(hits, geom)
    return hits, geom, rec, inst, rec.view(I)[:, 3] >= 0


# ---- (b) the lanes, the word, the pick ------------------------------------------------------------------------------------------------

class Word:
    """a pose's shared word and every value it has held; read() is stale by the policy: "fresh" the current value, "random" any
    value held so far, "oldest" always the first ("none": every read arrives too late to help)"""

    def __init__(self, rng=None, policy="fresh"):
        self.value, self.history, self.rng, self.policy = NONE, [NONE], rng, policy

    def read(self):
        if self.policy == "fresh":
            return self.value
        if self.policy == "oldest":
            return self.history[0]
        return self.history[self.rng.randint(len(self.history))]

    def atomic_min(self, key):
        old = self.value
        self.value = min(old, key)
        self.history.append(self.value)
        return old


def _key_dist(key):
    return np.asarray(key >> 32, np.uint32).view(F)


class MeshDistWorld(WD.TriDistWorld):
    """(b): world_query_model's boxes and tree, world_mesh_dist.hip's body"""

    def prepare(self, q):
        """per-query tables for the posed triangles q [R, 3, 3]: every pair's tri_dist and every leaf's lb2, per instance"""
        q = np.asarray(q, F).reshape(-1, 3, 3)
        lo, hi = WT.bounds(q)
        pairs = [WD.pair_records(i, q) for i in self.box_insts]
        finite = np.isfinite(q).all(axis=(1, 2))
        lbs = []
        for i_ in self.box_insts:
            lb, cand = WD.leaf_lb2(i_, lo[finite], hi[finite])
            full = np.zeros((q.shape[0], cand.size), F)
            full[finite] = lb
            lbs.append(full)
        return {"q": q, "lo": lo, "hi": hi, "pairs": pairs, "lbs": lbs, "finite": finite}

    def lane(self, tab, i, t, rmax, skip, mode, flags=0, word=None, log=None):
        """One lane as a generator: query i of the tables, triangle t of other. mode: "closest" (returns the record through
        log["record"]), "within" (log["found"]) or "clear" (publishes to `word`). Yields before every leaf: the scheduler's turn."""
        rm = F(rmax)
        st = {"rmax": rm, "best": TD.rmax_bound(rm), "found": False, "over": False, "seen": NONE, "inst": -1, "tri": -1, "w": None}
        log = {} if log is None else log
        log.update(entered=[], tested=[], record=None, found=False)
        lo, hi = tab["lo"][i], tab["hi"][i]
        with np.errstate(invalid="ignore"):
            valid = bool(tab["finite"][i]) and bool(rm >= 0)
        record = mode == "closest"

        def take(key):
            with np.errstate(all="ignore"):
                d = _key_dist(key)
                if d < st["rmax"]:
                    st["rmax"] = d
                nb = TD.rmax_bound(st["rmax"])
                if nb < st["best"]:
                    st["best"], st["found"] = nb, False
            if (key >> 32) == 0 and (key & 0xffffffff) < t:
                st["over"] = True

        def publish(go_on):
            with np.errstate(invalid="ignore"):
                own = MD.key_of(np.sqrt(st["best"]), t)
            if not own < st["seen"]:
                return
            old = word.atomic_min(own)
            st["seen"] = min(old, own)
            if go_on:
                take(st["seen"])

        def settled():
            return record and st["found"] and st["best"] == 0

        def lower(j, tri):
            return st["inst"] < 0 or j < st["inst"] or (j == st["inst"] and tri < st["tri"])

        def done():
            if mode == "within":
                return st["found"] or st["over"]
            return mode == "clear" and (st["over"] or (st["found"] and st["best"] == 0))

        if valid and mode == "clear" and flags & BOUND:
            st["seen"] = word.read()
            take(st["seen"])
            valid = not st["over"]
        if valid and self.box_insts:
            stack = [0 if self.tree.n > 1 else ~0]
            while stack and not done():
                cur = stack.pop()
                if cur >= 0:
                    loL, hiL, lL, loR, hiR, lR = self.tree.nodes[cur]
                    lim = WD.slackened(st["best"])
                    kL, kR = WD.top_gap2(loL, hiL, lo, hi), WD.top_gap2(loR, hiR, lo, hi)
                    okL, okR = bool(not kL > lim), bool(not kR > lim)
                    left_first = okL and (not okR or kL <= kR)
                    first, second = (lL, lR) if left_first else (lR, lL)
                    if okL and okR:
                        stack.append(second)
                    if okL or okR:
                        stack.append(first)
                    continue
                j = ~cur
                if j == skip or (mode != "closest" and st["over"]) or (settled() and j > st["inst"]):
                    continue
                log["entered"].append(j)
                d2, u, v, s, tt, cand = tab["pairs"][j]
                lb = tab["lbs"][j][i]
                for c in np.argsort(lb, kind="stable"):             # the nearer leaf first
                    if not lb[c] <= WD.slackened(st["best"]):
                        continue
                    tri = int(cand[c])
                    if settled() and not lower(j, tri):
                        continue
                    yield
                    if mode == "clear":
                        if flags & REREAD:
                            key = word.read()
                            st["seen"] = min(st["seen"], key)
                            take(key)
                        if st["over"] or (st["found"] and st["best"] == 0):
                            break
                    log["tested"].append((j, tri))
                    x = d2[i, c]
                    with np.errstate(invalid="ignore"):
                        near = bool(np.sqrt(x) <= st["rmax"])
                    if record:
                        if near and (x < st["best"] or (x == st["best"] and lower(j, tri))):
                            st.update(found=True, best=x, inst=j, tri=tri, w=(u[i, c], v[i, c], s[i, c], tt[i, c]))
                    elif mode == "within":
                        if near and x <= st["best"]:
                            st["found"] = True
                            break
                    elif near and (not st["found"] or x < st["best"]):
                        st["found"], st["best"] = True, x
                        if flags & EARLY:
                            publish(True)
                            if done():
                                break
        if mode == "clear" and st["found"]:
            publish(False)
        log["found"] = st["found"]
        if record:
            rec = TD.miss_records(1)[0]
            if st["found"]:
                rec[0], rec[1], rec[4], rec[5] = st["w"]
                rec[2] = np.sqrt(st["best"])
                rec.view(I)[3] = st["tri"]
            log["record"] = (rec, st["inst"] if st["found"] else -1)

    def run(self, gen):
        for _ in gen:
            pass

    def closest(self, tab, rmax, skip):
        """the closest kernel over the tables' queries: (records [R, 8], instances [R], entered [R] lists)"""
        n = tab["q"].shape[0]
        hits, geom, entered = TD.miss_records(n), np.full(n, -1, I), []
        for i in range(n):
            log = {}
            self.run(self.lane(tab, i, 0, rmax, skip, "closest", log=log))
            hits[i], geom[i] = log["record"]
            entered.append(log["entered"])
        return hits, geom, entered

    def within(self, tab, rmax, skip):
        """the within kernel, lane by lane: the OR over the tables' queries"""
        flag = False
        for i in range(tab["q"].shape[0]):
            log = {}
            self.run(self.lane(tab, i, 0, rmax, skip, "within", log=log))
            flag = flag or log["found"]
        return flag

    def clearance(self, tab, ts, rmax, skip, flags, rng=None, policy="fresh", order=None):
        """One pose's clearance launch and pick: the tables hold the pose's posed leaves, ts their triangle ids. The lanes run
        interleaved at leaf granularity: a random lane's turn each step (rng), or `order`, a list of lane positions to step
        (a lane that has ended is passed over; what is left then runs in turn). Returns (word, record [8], instance)."""
        word = Word(rng, policy)
        live = {k: self.lane(tab, k, int(ts[k]), rmax, skip, "clear", flags, word) for k in range(len(ts))}
        steps = list(order) if order is not None else None
        while live:
            if steps:
                k = steps.pop(0)
                if k not in live:
                    continue
            elif rng is not None and order is None:
                k = list(live)[rng.randint(len(live))]
            else:
                k = next(iter(live))
            try:
                next(live[k])
            except StopIteration:
                del live[k]
        rec, inst = miss_clearance(1)[0], -1
        if word.value != NONE:
            t_star = word.value & 0xffffffff
            k = list(ts).index(t_star)
            log = {}
            self.run(self.lane(tab, k, t_star, _key_dist(word.value), skip, "closest", log=log))
            rec[:] = log["record"][0]
            inst = log["record"][1]
            rec.view(I)[6] = t_star if inst >= 0 else -1
        return word.value, rec, inst
