"""The sphere sweeps of an instance world (psm_world_sweep_sphere_dev / psm_world_sweep_occluded_dev, include/psm_hip.h "sweep
queries over a world"; world_sweep.hip) in numpy, in two parts.

(a) The flat answer: sweep_query_model.query on the sweep moved into every instance of the ordered list (instance_query_model's
    move and rotate: a world ray's move), combined as scene_query_model combines closest hits: the smallest t, on a bit-equal t
    the lowest (inst, tri). A world must answer exactly this.
(b) A float32 restatement of what world_sweep.hip adds to that: the top-level slab test against the padded world boxes of
    world_query_model's tree, each grown by G = WORLD_QSLACK |origin|_inf + radius (1 + 2^-11), slackened by WORLD_TSLACK; the
    prune inside an instance, sweep_axis on the moved sweep against each leaf's own image box under the instance's fit
    transform with NO padding (a leaf the model keeps with the limit at its own t is kept by the kernel, whose leaf boxes are
    that image padded, whose inner boxes are unions and whose limit is never below the winner's t); and the walk. (b) == (a)
    says that neither level ever cuts the candidate that wins. (b) also returns the instances each sweep entered.

An instance is (tris [T, 3, 3], cand, pose [3, 4]) for (a) and (tris, cand, pose, M) for (b): M the float32 fit transform of the
instance's hierarchy. The kernel order of every float32 operation is kept (the library builds with -ffp-contract=off)."""
import numpy as np

import instance_query_model as NQ
import point_query_model as PQ
import scene_query_model as SQ
import sweep_query_model as SW
import world_box_query_model as WB
import world_query_model as WQ
from query_model import normalize3

F = np.float32
D = np.float64
WORLD_PAD = WQ.WORLD_PAD
WORLD_FLOOR = WQ.WORLD_FLOOR
WORLD_QSLACK = WQ.WORLD_QSLACK
WORLD_TSLACK = WQ.WORLD_TSLACK
RADIUS_GROW = F(1.00048828125)     # world_sweep.hip: 1 + 2^-11 on the radius


def _batch(origins, directs, radius, tmax):
    o = np.asarray(origins, F).reshape(-1, 3)
    d = np.asarray(directs, F).reshape(-1, 3)
    r = np.broadcast_to(np.asarray(radius, F), (o.shape[0],)).astype(F)
    tm = np.broadcast_to(np.asarray(tmax, F), (o.shape[0],)).astype(F)
    return o, d, r, tm


def world_valid(o, d, r, tm):
    """SweepBody::begin's rule on the WORLD sweep: finite origin, finite normalize3(direct), 0 <= radius < inf, tmax >= 0"""
    return SW.sweep_valid(o, normalize3(d), r, tm)


# ---- (a) the flat answer ------------------------------------------------------------------------------------------------------------

def flat(insts, origins, directs, radius, tmax=np.inf):
    """(a): (hits [R, 4] float32 as the kernel writes psm_hit -- the winning instance's object-space u, v, t, tri bits --, inst
    [R] int32 (-1: a miss), occluded [R] bool). An instance in which the moved sweep is not finite is skipped: that is
    sweep_query_model.query's own validity on the moved sweep"""
    o, d, r, tm = _batch(origins, directs, radius, tmax)
    hits, inst = SQ._miss(o.shape[0]), np.full(o.shape[0], -1, np.int32)
    if len(insts):
        per = [SW.query(i[0], i[1], NQ.move(i[2], o), NQ.rotate(i[2], d), r, tm)[0] for i in insts]
        hits, inst = SQ.combine_closest(per)
    bad = ~world_valid(o, d, r, tm)
    hits[bad], inst[bad] = SQ._miss(int(bad.sum())), -1
    return hits, inst, inst >= 0


def pair_contacts(inst, o, d, r, tm):
    """sweep_tri on every (sweep, candidate) pair of one instance, the sweep moved: t, u, v [R, C] (t = +inf: the pair does not
    count -- no contact within tmax, or the world sweep or the moved sweep is invalid), and the sorted candidate ids"""
    cand = np.sort(np.asarray(inst[1], np.int64).reshape(-1))
    mo, md = NQ.move(inst[2], o), normalize3(NQ.rotate(inst[2], d))
    ok = world_valid(o, d, r, tm) & SW.sweep_valid(mo, md, r, tm)
    t, u, v = (np.zeros((o.shape[0], cand.size), F) for _ in range(3))
    t[:] = np.inf
    if cand.size:
        v0, e1, e2 = PQ._split(np.asarray(inst[0], F).reshape(-1, 3, 3)[cand])
        for a in range(0, o.shape[0], max(1, (1 << 18) // cand.size)):
            b = min(o.shape[0], a + max(1, (1 << 18) // cand.size))
            t[a:b], u[a:b], v[a:b] = SW.sweep_tri(v0[None], e1[None], e2[None], mo[a:b, None, :], md[a:b, None, :], r[a:b, None], tm[a:b, None])
        t[~ok] = np.inf
    return t, u, v, cand


def lowest(contacts):
    """the answer by definition from pair_contacts of every instance in list order: the smallest t, on a bit-equal t the
    lexicographically lowest (inst, tri) -- the columns are in that order, so the first of the smallest"""
    R = contacts[0][0].shape[0]
    hits, inst = SQ._miss(R), np.full(R, -1, np.int32)
    t = np.concatenate([c[0] for c in contacts], axis=1)
    if t.shape[1] == 0:
        return hits, inst, inst >= 0
    u, v = np.concatenate([c[1] for c in contacts], axis=1), np.concatenate([c[2] for c in contacts], axis=1)
    tri = np.concatenate([c[3] for c in contacts])
    ins = np.concatenate([np.full(c[3].size, j, np.int64) for j, c in enumerate(contacts)])
    k = np.argmin(t, axis=1)
    i = np.arange(R)
    hit = np.isfinite(t[i, k])
    hits[hit, 0], hits[hit, 1], hits[hit, 2] = u[i, k][hit], v[i, k][hit], t[i, k][hit]
    hits.view(np.int32)[hit, 3] = tri[k][hit]
    inst[hit] = ins[k][hit]
    return hits, inst, hit


# ---- (b) the two tests and the walk ---------------------------------------------------------------------------------------------------

def growth(o, r):
    """G of WorldSweepBody::begin, float32: the query's pad and the sphere; o [..., 3], r [...]"""
    with np.errstate(all="ignore"):
        return ((WORLD_QSLACK * np.abs(o).max(axis=-1)).astype(F) + (r * RADIUS_GROW).astype(F)).astype(F)


def top_setup(o, d, r):
    """WorldRay::world_ray and the growth for sweeps (o, d [..., 3], r [...]): the reciprocal unit direction, nocull and G"""
    o, d, r = np.asarray(o, F), np.asarray(d, F), np.asarray(r, F)
    with np.errstate(all="ignore"):
        dn = normalize3(d)
        nocull = ~(np.isfinite(dn).all(axis=-1) & (((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]).astype(F) + dn[..., 2] * dn[..., 2]).astype(F) > F(0.5)))
        return (F(1) / dn).astype(F), nocull, growth(o, r)


def top_slab(o, d, r, blo, bhi, setup=None):
    """WorldRay::slab with qpad = G for sweeps (o, d [..., 3], r [...]) against boxes (blo, bhi [..., 3]), broadcast: tNear, tFar
    and nocull, float32 in the kernel's order (fmin / fmax are minNum / maxNum)"""
    o = np.asarray(o, F)
    iv, nocull, G = top_setup(o, d, r) if setup is None else setup
    with np.errstate(all="ignore"):
        G = np.asarray(G, F)[..., None]
        a = (((blo - G).astype(F) - o).astype(F) * iv).astype(F)
        b = (((bhi + G).astype(F) - o).astype(F) * iv).astype(F)
        near, far = np.fmax.reduce(np.fmin(a, b), axis=-1), np.fmin.reduce(np.fmax(a, b), axis=-1)
    return near, far, nocull


def top_kept(near, far, nocull, lim):
    """WorldRay::top_boxes against [0, lim], slackened, as negations: a NaN keeps the box"""
    with np.errstate(all="ignore"):
        lim = np.asarray(lim, F)
        hi_t = (lim + (WORLD_TSLACK * np.abs(lim)).astype(F)).astype(F)
        return nocull | (~(near > far) & ~(near > hi_t) & ~(far < F(0)))


def _fmaf(a, b, c):
    with np.errstate(all="ignore"):
        return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)   # (the product is exact in float64; one rounding of the sum)


def prune_near(inst, o, d, r):
    """SweepBody::children for every (sweep, candidate) of one instance on the leaf's exact, UNPADDED image box: sweep_axis on the
    moved sweep, then psm_query_dev.h's slab: tNear, tFar [R, C] float32"""
    tris, cand, pose, M = inst
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    mo, md = NQ.move(pose, o), normalize3(NQ.rotate(pose, d))
    inv, nlo, nhi = SW.sweep_axis(np.asarray(M, F).reshape(-1, 4)[:3], mo, md, r)
    bmin, bmax = WB.leaf_images(np.asarray(tris, F).reshape(-1, 3, 3)[cand], M)
    lo32, hi32 = np.nextafter(bmin.astype(F), F(np.inf)), np.nextafter(bmax.astype(F), F(-np.inf))   # inside the exact box
    lo32, hi32 = np.minimum(lo32, hi32), np.maximum(lo32, hi32)
    a, b = _fmaf(lo32[None], inv[:, None, :], nlo[:, None, :]), _fmaf(hi32[None], inv[:, None, :], nhi[:, None, :])
    return np.fmax.reduce(np.fmin(a, b), axis=-1), np.fmin.reduce(np.fmax(a, b), axis=-1)


def seen_contacts(inst, contact, o, d, r):
    """pair_contacts with the pairs the prune would cut at a limit of their own t set to +inf"""
    t, u, v, cand = contact
    if cand.size == 0:
        return contact
    near, far = prune_near(inst, o, d, r)
    with np.errstate(invalid="ignore"):
        kept = ~(near > far) & ~(near > t) & ~(far < F(0))
    return np.where(kept, t, F(np.inf)), u, v, cand


class SweepWorld(WQ.World):
    """(b): world_query_model's boxes and tree, world_sweep.hip's tests and walk"""

    def __init__(self, insts):
        super().__init__([(t, c, m) for t, c, m, _ in insts])
        self.sweep_insts = insts

    def sweeps(self, origins, directs, radius, tmax=np.inf, contacts=None):
        """((hits, inst), occluded, (entered by the first-contact walk, entered by the occluded walk))"""
        o, d, r, tm = _batch(origins, directs, radius, tmax)
        R = o.shape[0]
        contacts = [pair_contacts(i, o, d, r, tm) for i in self.sweep_insts] if contacts is None else contacts
        seen = [seen_contacts(i, c, o, d, r) for i, c in zip(self.sweep_insts, contacts)]
        own = [lowest([s]) for s in seen]                     # each instance's own answer among what its prune keeps
        valid = world_valid(o, d, r, tm)
        hits, inst, occ = SQ._miss(R), np.full(R, -1, np.int32), np.zeros(R, bool)
        ent = ([], [])
        iv, nocull, G = top_setup(o, d, r)
        for i in range(R):
            if not valid[i] or not self.sweep_insts:
                ent[0].append([])
                ent[1].append([])
                continue
            st = {"best": tm[i], "inst": -1}

            def keep(lo, hi, lim):
                near, far, nc = top_slab(o[i], d[i], r[i], lo, hi, (iv[i], nocull[i], G[i]))
                return bool(top_kept(near, far, nc, lim())), near

            def visit_first(j):
                h = own[j][0][i]
                if own[j][2][i] and (h[2] < st["best"] or (h[2] == st["best"] and (st["inst"] < 0 or j < st["inst"]))):
                    st["best"], st["inst"] = h[2], j
                    hits[i], inst[i] = h, j
                return False

            def visit_any(j):
                occ[i] |= bool(own[j][2][i])
                return bool(occ[i])
            ent[0].append(self.tree.walk(lambda lo, hi: keep(lo, hi, lambda: st["best"]), visit_first))
            ent[1].append(self.tree.walk(lambda lo, hi: keep(lo, hi, lambda: tm[i]), visit_any))
        return (hits, inst), occ, ent


# ---- the top level's margin chain, evaluated in float64 -----------------------------------------------------------

def top_figures(world, j, contact, o, d, r):
    """For instance j of a SweepWorld and pair_contacts `contact` of it, for every pair that counts [R, C]:
      outside:  how far the world centre origin + t dn (float64; dn the float64 unit direction) lies outside the instance's world
                box along its worst axis, beyond the radius -- against the PADDED box and against the box without its padding
      granted:  what is granted beyond the radius: by G alone (WORLD_QSLACK |origin|_inf + 2^-11 radius), and by G and the padding
      kept:     [R] whether the float32 top-level slab keeps the box with the limit at the smallest counting t of the sweep"""
    t, _, _, cand = contact
    counts = np.isfinite(t)
    od, rd = o.astype(D), r.astype(D)
    dn = d.astype(D) / np.linalg.norm(d.astype(D), axis=1, keepdims=True)
    c = od[:, None, :] + np.where(counts, t, 0).astype(D)[:, :, None] * dn[:, None, :]
    lo, hi = world.lo[j].astype(D), world.hi[j].astype(D)
    tris, _, pose = world.insts[j]
    olo, ohi = (x.astype(D) for x in WQ.object_box(tris))
    m = np.asarray(pose, F).reshape(3, 4).astype(D)
    cw, ew = m[:, :3] @ ((olo + ohi) / 2) + m[:, 3], np.abs(m[:, :3]) @ ((ohi - olo) / 2)      # the box without padding, exact
    pad = max(0.0, min(((cw - ew) - lo).min(), (hi - (cw + ew)).min()))                      # what world_inst_boxes put on, at least
    lo, hi = world.lo[j].astype(D), world.hi[j].astype(D)
    out_padded = np.maximum(lo - c, c - hi).max(axis=-1) - rd[:, None]
    out_bare = np.maximum((cw - ew) - c, c - (cw + ew)).max(axis=-1) - rd[:, None]
    g_alone = (float(WORLD_QSLACK) * np.abs(od).max(axis=1) + 2.0 ** -11 * rd)[:, None] + np.zeros_like(out_bare)
    near, far, nocull = top_slab(o, d, r, world.lo[j], world.hi[j])
    with np.errstate(invalid="ignore"):
        kept = top_kept(near, far, nocull, np.where(counts.any(axis=1), t.min(axis=1) if t.shape[1] else F(0), F(0)))
    return counts, out_padded, out_bare, g_alone, g_alone + pad, kept
