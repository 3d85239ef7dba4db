"""When a ray hit is well-posed, and what the ray queries owe a ray whose hits are not all so (psm_bvh_intersect_dev /
psm_bvh_occluded_dev / psm_bvh_count_hits_dev / psm_bvh_first_hits_dev, include/psm_hip.h).

The unclamped triangle test (query_model.tri_test, clamp=False) divides by det. For a ray lying almost in a triangle's plane det
is mostly rounding noise: (u, v) can pass while t is off by a large part of the scene, and the point o + t d is then nowhere near
the triangle. The walk keeps a box only if the ray's slab interval admits t (ray_axis / slab, psm_query_dev.h), so such a hit is
dropped at its own leaf box while a brute force over the leaves reports it. Neither is wrong about the geometry: the hit is not
geometry. The rule here says which hits the walk must never lose:

    a hit (ray, triangle, t) is WELL-POSED iff its point, mapped into the build's normalised space, lies no farther than
    HEADROOM outside the triangle's exact normalised bounding box, on every axis.

HEADROOM = PZERO / 2 = 2.5e-4 is the project's own: a leaf box is the triangle's normalised box padded by PZERO = 5e-4 and then
rounded to fp16, whose half-ulp on [0.5, 1) is 2^-12 = 2.44e-4, so at least 2.5e-4 of the padding survives the rounding there.
A padded corner in [1, 1 + PZERO) -- a leaf at the top of the scene -- meets a half-ulp of 2^-11 and can keep as little as 1.2e-5;
ray_axis's margin makes up for it with the constant 2^-12 on top of h on the boxes' upper planes (psm_query_dev.h). A well-posed hit's point therefore lies
in its leaf's box grown by that constant, and h has to cover only the float32 rounding of the slab arithmetic -- which
tests/test_ray_prune_cpu.py checks with leaf_interval() below.

Per ray: A = every candidate the model accepts (tri_test's own acceptance, a valid ray, tmin <= t <= tmax), W = the well-posed
ones of A; the ray is FULLY WELL-POSED iff W = A. RaySets holds both in sparse form, and the check_* functions are the contract:
bit for bit on fully well-posed rays, sound two-sided bounds on the others (an ill-posed hit may be reported or not, but is never
invented, and a well-posed hit is never missed)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import query_model as Q

F = np.float32
D = np.float64
HEADROOM = float(Q.PZERO) / 2.0   # 2.5e-4 normalised units: PZERO of padding less fp16's half-ulp 2^-12 on [0.5, 1)


def _affine(M):
    M = np.asarray(M, D).reshape(4, 4)
    return M[:3, :3], M[:3, 3]


def excess(tris, M, o, dn, t, tri):
    """How far (normalised units, the largest of the three axes, float64) the hit point o + t dn lies outside the exact normalised
    bounding box of triangle `tri`: P = M3 (o + t dn) + m against the per-axis min / max of M3 v + m over the three vertices.
    M: the hierarchy's info().transform, row-major; dn: the direction as query_model.normalize3 gives it. +inf for a non-finite P."""
    M3, m = _affine(M)
    tris = np.asarray(tris, D).reshape(-1, 3, 3)
    o, dn, t = np.asarray(o, D), np.asarray(dn, D), np.asarray(t, D)
    with np.errstate(all="ignore"):
        P = (o + t[..., None] * dn) @ M3.T + m
        V = tris[np.asarray(tri, np.int64)] @ M3.T + m
        lo, hi = V.min(axis=-2), V.max(axis=-2)
        e = np.maximum(np.maximum(lo - P, P - hi), 0.0).max(axis=-1)
    return np.where(np.isfinite(P).all(axis=-1), e, np.inf)


def well_posed(tris, M, o, dn, t, tri):
    """bool[...]: the hit (o, dn, t) of triangle `tri` is well-posed (the module's docstring): excess() <= HEADROOM"""
    return excess(tris, M, o, dn, t, tri) <= HEADROOM


# ---- the prune, restated ------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)


def leaf_boxes(leafs):
    """(triangle ids [n], boxes [n, 6] float32: min x y z, max x y z) of the oracle's leaf records (build_scene()["leafs"]): the
    fp16 corners as the walk reads them"""
    h = np.ascontiguousarray(leafs["box"]).view(np.float16).reshape(-1, 8)
    return leafs["pdata"][:, 3].astype(np.int64), h[:, [0, 1, 2, 4, 5, 6]].astype(F)


def leaf_interval(M, leaf_box, o, dn, grow=2.0 ** -12):
    """(near, far) float32[...] of the ray (o, dn) against one leaf's fp16 box [..., 6] (min x y z, max x y z): affine_row / ray_axis /
    slab of psm_query_dev.h in float32, one numpy operation per float operation and in their order. grow: the constant
    ray_axis adds to the margin of a box's upper planes (2^-12; 0 gives the margin as it was before that term). The two fmaf of every axis are
    emulated through float64 (the product is exact there, the sum is rounded to double and then to float): a double rounding
    can differ from the hardware's single one in the last bit, so this is a model of the prune, not a bit-exact copy."""
    M = np.asarray(M, F).reshape(4, 4)
    box = np.asarray(leaf_box, F)
    o, dn = np.asarray(o, F), np.asarray(dn, F)
    lows, highs = [], []
    with np.errstate(all="ignore"):
        for k in range(3):
            m0, m1, m2, m3 = M[k]
            P = ((m0 * o[..., 0] + m1 * o[..., 1]) + m2 * o[..., 2]) + m3
            S = ((np.abs(m0 * o[..., 0]) + np.abs(m1 * o[..., 1])) + np.abs(m2 * o[..., 2])) + np.abs(m3)
            h = (F(2.0) + S) * F(2.0 ** -16)
            Dk = (m0 * dn[..., 0] + m1 * dn[..., 1]) + m2 * dn[..., 2]
            Dk = np.where(np.abs(Dk) >= F(1e-20), Dk, np.copysign(F(1e-20), Dk)).astype(F)
            inv = F(1.0) / Dk
            nlo = -(P + h) * inv
            nhi = ((h + F(grow)) - P) * inv
            a, b = _fma(box[..., k], inv, nlo), _fma(box[..., 3 + k], inv, nhi)
            lows.append(np.fmin(a, b))
            highs.append(np.fmax(a, b))
        near = np.fmax(np.fmax(lows[0], lows[1]), lows[2])
        far = np.fmin(np.fmin(highs[0], highs[1]), highs[2])
    return near, far


# ---- rays ---------------------------------------------------------------------------------------------------------------------

def grazing_rays(rng, tris, n, tilt):
    """n rays lying in the plane of a random triangle each, tilted out of it by `tilt`: a point of the triangle by Dirichlet
    weights, a random unit direction in the plane plus (+-tilt) x the unit normal, the origin 0.5 .. 3 units back along it.
    Triangles without an area are not picked (they have no plane). Returns origins, directions float32 [n, 3]."""
    t = np.asarray(tris, D).reshape(-1, 3, 3)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    nrm = np.cross(e1, e2)
    with np.errstate(all="ignore"):
        area = np.linalg.norm(nrm, axis=1)
        ok = np.nonzero((area > 0) & (np.linalg.norm(e1, axis=1) > 0))[0]
    if ok.size == 0:
        ok = np.arange(t.shape[0])
    pick = ok[rng.randint(0, ok.size, n)]
    w = rng.dirichlet([1, 1, 1], n)
    p = np.einsum("ij,ijk->ik", w, t[pick])
    with np.errstate(all="ignore"):
        nn = nrm[pick] / area[pick, None]
        a = e1[pick] / np.linalg.norm(e1[pick], axis=1, keepdims=True)
    b = np.cross(nn, a)
    phi = rng.uniform(0, 2 * np.pi, n)[:, None]
    sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)[:, None]
    d = np.cos(phi) * a + np.sin(phi) * b + sign * tilt * nn
    d = np.nan_to_num(d / np.linalg.norm(d, axis=1, keepdims=True))
    o = p - rng.uniform(0.5, 3.0, n)[:, None] * d
    return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)


TILTS = (("tilt1e-3", 1e-3), ("tilt1e-5", 1e-5), ("tilt1e-7", 1e-7), ("tilt0", 0.0))
# The share of rays that may be left to the two-sided bounds, per class: conditions of the contract, not measurements (DESIGN.md
# 4.5 has the measured shares). The two flattest classes are capped, and must hold at least one such ray, on sponza_like(3001).
SHARE_CAP = {"random": 0.01, "outside": 0.01, "own": 0.01, "tilt1e-3": 0.01, "tilt1e-5": 0.01}
FLAT_CAP = {"tilt1e-7": 0.25, "tilt0": 0.25}
# (hierarchy, class) pairs left out of the share assertion by name, never out of the checks themselves. A grazing ray starts
# 0.5 .. 3 units from its triangle whatever the scene's scale, so where many triangles are far smaller than that distance times
# the tilt the rounding of t alone carries the hit point off the triangle, and the class is degenerate as a whole:
#   deep   a third of its triangles are below 1e-3 units (clusters down to 2^-20): 5 - 6 % of the rays at tilt 1e-5
#   fuzz1  (median edge 1.6e-3 units) 4 %, fuzz2 (5 triangles) 9 - 12 % at tilt 1e-5
#   fuzz5  (extent 1e-3, median edge 5e-6) 3 - 11 % at tilt 1e-3 and 1e-5
#   fuzz6  (extent 2e-7) over 95 % in every grazing class
# and fuzz7 is flat in z: the fit transform stretches its zero extent to the unit box, a hit point's rounding along z with it,
# and 15 % of the rays that come from outside (most of them along z) are left out under the identity.
NO_SHARE = ({(h, "tilt1e-5") for h in ("deep", "fuzz1", "fuzz2", "fuzz5", "fuzz6")}
            | {("fuzz5", "tilt1e-3"), ("fuzz6", "tilt1e-3"), ("fuzz7", "outside")})


def box_rays(rng, tris, n, outside=False):
    """random rays that start in the triangles' box or (outside) on a shell around it, pointing at a point inside it"""
    p = np.asarray(tris, F).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    if not outside:
        return rng.uniform(lo, hi, (n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    u = rng.normal(size=(n, 3)).astype(F)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = ((lo + hi) * F(0.5) + u * (hi - lo).max() * F(1.5)).astype(F)
    return o, (rng.uniform(lo, hi, (n, 3)) - o).astype(F)


def ray_classes(rng, tris, own_o, own_d, n):
    """The ray classes of the prune's tests, name -> (origins, directions): random in the box, from outside toward the box, the
    hierarchy's own rays (a scene's camera rays, a soup's or fixture's rays; the first n, or all when n is None) and grazing rays at
    each tilt"""
    own_o, own_d = np.asarray(own_o, F).reshape(-1, 3), np.asarray(own_d, F).reshape(-1, 3)
    out = {"random": box_rays(rng, tris, n), "outside": box_rays(rng, tris, n, outside=True),
           "own": (np.ascontiguousarray(own_o[:n]), np.ascontiguousarray(own_d[:n]))}
    for name, tilt in TILTS:
        out[name] = grazing_rays(rng, tris, n, tilt)
    return out


# ---- the per-ray sets ---------------------------------------------------------------------------------------------------------

def accepted_pairs(tris, origins, directs):
    """Every (ray, triangle) pair of tris [T, 3, 3] that the unclamped test accepts on a ray with a finite origin and normalised
    direction, whatever the window (a NaN t is in no window and is left out): a dict of arrays r, tri, t, u, v in (r, t, tri)
    order -- t compared as a float, so -0 == +0 and the id decides. It depends on neither the build nor the window: RaySets
    cuts it down to a hierarchy's leaves and a window."""
    o = np.asarray(origins, F).reshape(-1, 3)
    dn = Q.normalize3(np.asarray(directs, F).reshape(-1, 3))
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    R = o.shape[0]
    ok_ray = np.isfinite(o).all(axis=1) & np.isfinite(dn).all(axis=1)
    parts = []

    def chunk(ab):
        a, b = ab
        t, u, v, ok = Q.tri_test(tris, o[a:b], dn[a:b], clamp=False)
        ok &= ok_ray[a:b, None] & ~np.isnan(t)
        r, k = np.nonzero(ok)
        return (r + a).astype(np.int64), k.astype(np.int64), t[r, k], u[r, k], v[r, k]

    if R and tris.shape[0]:
        with ThreadPoolExecutor(max_workers=8) as pool:   # (numpy releases the GIL: ray chunks on a few threads)
            parts = list(pool.map(chunk, Q._chunks(R, tris.shape[0], 1 << 20)))
    cat = [np.concatenate([p[i] for p in parts]) if parts else np.zeros(0, (np.int64, np.int64, F, F, F)[i]) for i in range(5)]
    order = np.lexsort((cat[1], cat[2], cat[0]))
    r, tri, t, u, v = (x[order] for x in cat)
    return {"r": r, "tri": tri, "t": t, "u": u, "v": v, "o": o, "dn": dn, "T": tris.shape[0], "tris": tris}


def _miss_rows(shape):
    rows = np.zeros(shape + (4,), F)
    rows[..., 2] = np.inf
    rows.view(np.int32)[..., 3] = -1
    return rows


class RaySets:
    """A(ray) and W(ray) of a batch of rays against a built hierarchy: tris [T, 3, 3], cand = the hierarchy's leaves
    (PSM_BVH_LEAF_TRI), M = info().transform, per-ray windows. pairs: accepted_pairs() of the same triangles and rays, when the
    caller has it already. The pairs of A are held in (ray, t, tri) order: r, tri, t, u, v, wp (well-posed), start [R + 1]."""

    def __init__(self, tris, cand, M, origins, directs, tmin=0.0, tmax=np.inf, pairs=None):
        p = pairs if pairs is not None else accepted_pairs(tris, origins, directs)
        self.R = R = p["o"].shape[0]
        self.T = p["T"]
        lo, hi = Q._window(R, tmin), Q._window(R, tmax)
        leaf = np.zeros(max(self.T, 1), bool)
        leaf[np.asarray(cand, np.int64).reshape(-1)] = True
        r = p["r"]
        with np.errstate(invalid="ignore"):
            keep = leaf[p["tri"]] & (lo <= hi)[r] & (p["t"] >= lo[r]) & (p["t"] <= hi[r])
        self.r, self.tri, self.t, self.u, self.v = (p[k][keep] for k in ("r", "tri", "t", "u", "v"))
        self.excess = excess(p["tris"], M, p["o"][self.r], p["dn"][self.r], self.t, self.tri)
        self.wp = self.excess <= HEADROOM
        self.start = np.searchsorted(self.r, np.arange(R + 1))
        self.nA = np.diff(self.start)
        self.nW = np.bincount(self.r[self.wp], minlength=R)[:R] if R else np.zeros(0, np.int64)
        self.full = self.nA == self.nW
        w = np.nonzero(self.wp)[0]
        rw, first = np.unique(self.r[w], return_index=True)
        self.firstW = np.full(R, -1, np.int64)          # the pair that is the lexicographic best of W, -1: W is empty
        self.firstW[rw] = w[first]
        key = self.r * max(self.T, 1) + self.tri
        self._sorter = np.argsort(key, kind="stable")
        self._key = key[self._sorter]

    def share_not_full(self):
        return float((~self.full).mean()) if self.R else 0.0

    def records(self, idx):
        """psm_hit records [n, 4] of the pairs idx (u, v, t, tri bits)"""
        out = np.zeros((idx.size, 4), F)
        out[:, 0], out[:, 1], out[:, 2] = self.u[idx], self.v[idx], self.t[idx]
        out.view(np.int32)[:, 3] = self.tri[idx]
        return out

    def closest(self):
        """query_model.query's hits [R, 4]: the lexicographic best of A, the miss record where A is empty"""
        out = _miss_rows((self.R,))
        has = self.nA > 0
        out[has] = self.records(self.start[:-1][has])
        return out

    def first_hits(self, k):
        """kbest_query_model.first_hits' rows [R, k, 4] and count [R]"""
        rows = _miss_rows((self.R, k))
        for s in range(k):
            has = self.nA > s
            rows[has, s] = self.records(self.start[:-1][has] + s)
        return rows, np.minimum(self.nA, k).astype(np.uint32)

    def find(self, rays, tri):
        """the pair index of (ray, tri) in A, -1 where A has no such pair"""
        key = np.asarray(rays, np.int64) * max(self.T, 1) + np.asarray(tri, np.int64)
        pos = np.minimum(np.searchsorted(self._key, key), max(self._key.size - 1, 0))
        hit = (self._key[pos] == key) if self._key.size else np.zeros(key.shape, bool)
        return np.where(hit & (np.asarray(tri) >= 0), self._sorter[pos] if self._key.size else -1, -1)


def fully_well_posed(members, origins, directs):
    """bool [R]: the rays that are fully well-posed in EVERY member of a scene, an instanced scene or a world, whatever window a
    query then gives them (judged over -inf .. +inf): on these the combined queries owe the brute force's answers bit for bit.
    members: (tris, leaves, M, pose) each -- M the member hierarchy's info().transform; pose None, or the rigid pose through which
    instance_query_model moves a world ray into the member's object space, where its hierarchy is walked."""
    import instance_query_model as NQ
    o = np.asarray(origins, F).reshape(-1, 3)
    d = np.asarray(directs, F).reshape(-1, 3)
    out = np.ones(o.shape[0], bool)
    for tris, leaves, M, pose in members:
        mo, md = (o, d) if pose is None else (NQ.move(pose, o), NQ.rotate(pose, d))
        out &= RaySets(tris, leaves, M, mo, md, -np.inf, np.inf).full
    return out


def vote_rays_well_posed(members, points, directions):
    """bool [R]: the points all of whose vote rays (the inside queries': point, each row of `directions`) are fully well-posed"""
    p = np.asarray(points, F).reshape(-1, 3)
    return np.all([fully_well_posed(members, p, np.broadcast_to(k, p.shape)) for k in np.asarray(directions, F)], axis=0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _miss_record(buf):
    b = _bits(buf)
    return (b[..., 0] == 0) & (b[..., 1] == 0) & (b[..., 2] == 0x7F800000) & (b[..., 3] == 0xFFFFFFFF)


def _closest_rule(S, rays, buf):
    """the intersect rule on rays that need not be fully well-posed: None, or a message about the first offender"""
    buf = np.ascontiguousarray(buf, F)
    tri = buf.view(np.int32)[:, 3]
    miss = tri < 0
    bad = miss & ((S.nW[rays] > 0) | ~_miss_record(buf))
    if bad.any():
        return "a miss where W is not empty (or a malformed miss record)", np.nonzero(bad)[0]
    idx = S.find(rays, tri)
    bad = ~miss & (idx < 0)
    if bad.any():
        return "a hit that names a triangle outside A: invented", np.nonzero(bad)[0]
    h = np.nonzero(~miss)[0]
    bad = (_bits(buf[h]) != _bits(S.records(idx[h]))).any(axis=1)
    if bad.any():
        return "a hit whose (u, v, t) is not the model's for that (ray, triangle)", h[bad]
    fw = S.firstW[rays[h]]
    hw = fw >= 0
    tw, kw = S.t[np.maximum(fw, 0)], S.tri[np.maximum(fw, 0)]
    tg, kg = S.t[idx[h]], S.tri[idx[h]]
    bad = hw & ~((tg < tw) | ((tg == tw) & (kg <= kw)))
    if bad.any():
        return "a hit behind the best well-posed hit", h[bad]
    return None


def check_intersect(S, buf):
    """closest hit [R, 4] against the contract: bit-equal to the model on fully well-posed rays; on the others a miss only if W is
    empty, else a triangle of A with the model's record, no later in (t, tri) than the best of W"""
    buf = np.ascontiguousarray(buf, F).reshape(-1, 4)
    assert buf.shape[0] == S.R
    exp = S.closest()
    bad = np.nonzero(S.full & (_bits(buf) != _bits(exp)).any(axis=1))[0]
    assert bad.size == 0, ("intersect differs on fully well-posed rays", bad.size, bad[:4], buf[bad[:4]], exp[bad[:4]])
    rest = np.nonzero(~S.full)[0]
    err = _closest_rule(S, rest, buf[rest])
    assert err is None, ("intersect: " + err[0], rest[err[1]][:4], buf[rest[err[1]][:4]])


def check_occluded(S, occ):
    """any hit [R]: 1 where W is not empty, 0 where A is empty (exact on fully well-posed rays)"""
    occ = np.asarray(occ).astype(bool).reshape(-1)
    assert occ.shape[0] == S.R
    bad = np.nonzero((~occ & (S.nW > 0)) | (occ & (S.nA == 0)))[0]
    assert bad.size == 0, ("occluded outside its bounds", bad.size, bad[:8], S.nW[bad[:8]], S.nA[bad[:8]])


def check_count(S, count):
    """hit count [R]: |W| <= count <= |A| (exact on fully well-posed rays, where the two coincide)"""
    c = np.asarray(count).astype(np.int64).reshape(-1)
    assert c.shape[0] == S.R
    bad = np.nonzero((c < S.nW) | (c > S.nA))[0]
    assert bad.size == 0, ("countHits outside its bounds", bad.size, bad[:8], c[bad[:8]], S.nW[bad[:8]], S.nA[bad[:8]])


def check_first_hits(S, k, rows, count):
    """first k hits (rows [R, k, 4], count [R]): bit-equal to the model on fully well-posed rays; on the others every listed slot is
    a pair of A with the model's record, the slots ascend in (t, tri), the slots past count are misses, the count is at least
    min(k, |W|) and slot 0 obeys the intersect rule"""
    rows = np.ascontiguousarray(rows, F).reshape(S.R, k, 4)
    count = np.asarray(count).astype(np.int64).reshape(-1)
    exp, ecount = S.first_hits(k)
    bad = np.nonzero(S.full & ((_bits(rows) != _bits(exp)).any(axis=(1, 2)) | (count != ecount)))[0]
    assert bad.size == 0, ("firstHits differs on fully well-posed rays", k, bad.size, bad[:4], rows[bad[:4]], exp[bad[:4]])
    rest = np.nonzero(~S.full)[0]
    c = count[rest]
    bad = (c > np.minimum(S.nA[rest], k)) | (c < np.minimum(S.nW[rest], k))
    assert not bad.any(), ("firstHits: count outside its bounds", k, rest[bad][:8], c[bad][:8], S.nW[rest[bad]][:8], S.nA[rest[bad]][:8])
    prev = None
    for s in range(k):
        live = s < c
        slot = rows[rest, s]
        assert _miss_record(slot[~live]).all(), ("firstHits: a slot past count is not a miss", k, s, rest[~live][:4])
        idx = S.find(rest, np.where(live, slot.view(np.int32)[:, 3], -1))
        assert (idx[live] >= 0).all(), ("firstHits: a slot outside A: invented", k, s, rest[live & (idx < 0)][:4])
        same = (_bits(slot[live]) == _bits(S.records(idx[live]))).all(axis=1)
        assert same.all(), ("firstHits: a slot's record is not the model's", k, s, rest[live][~same][:4])
        if prev is not None:   # pairs of A are held in (t, tri) order: ascending slots have ascending pair indices
            assert (idx[live] > prev[live]).all(), ("firstHits: slots out of order", k, s, rest[live][idx[live] <= prev[live]][:4])
        prev = idx
    err = _closest_rule(S, rest, rows[rest, 0])
    assert err is None, ("firstHits slot 0: " + err[0], k, rest[err[1]][:4])


def check_shares(S, cap, what, at_least=0):
    """the rule cannot hide failures: at most `cap` of the rays are left to the two-sided bounds (and at least `at_least` rays)"""
    n = int((~S.full).sum())
    assert n <= cap * S.R and n >= at_least, ("%s: %d of %d rays are not fully well-posed (cap %g, at least %d)" % (what, n, S.R, cap, at_least))
