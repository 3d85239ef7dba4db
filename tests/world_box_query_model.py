"""The box queries of an instance world (psm_world_box_overlaps_dev / psm_world_box_count_dev / psm_world_box_triangles_dev,
include/psm_hip.h "box queries over a world"; world_box.hip) in numpy, in two parts.

(a) The flat answer: box_query_model's float32 box_tri over the forward-posed leaves of every instance of the ordered list:
    a flag, the count summed over the instances, and the min(k, c) lowest (inst, tri) ascending. A world must answer exactly this.
(b) A float32 restatement of what world_box.hip adds to that: the top-level test against the padded world boxes of
    world_query_model's tree, the prune inside an instance, and the walk. The hierarchy of an instance is the builder's and is
    not restated: the prune is applied to each leaf's own image box under the instance's fit transform, with NO padding -- a
    leaf the model keeps is kept by the kernel (whose leaf boxes are that image padded, and whose inner boxes are unions), so
    (b) == (a) says that neither level ever cuts a candidate that counts. (b) also returns the instances each query entered.

An instance here is (tris [T, 3, 3], cand, pose [3, 4], M [3, 4]): M the float32 fit transform of the instance's hierarchy (the
vertices' image is the unit cube). The kernel order of every float32 operation is kept (the library builds with
-ffp-contract=off)."""
import numpy as np

import box_query_model as BQ
import world_query_model as WQ
from point_query_model import _split

F = np.float32
D = np.float64
U = np.uint32
K_MAX = BQ.K_MAX
WORLD_QSLACK = WQ.WORLD_QSLACK
WORLD_BOX_PAD = F(2.0 ** -11)     # world_box.hip
WORLD_BOX_QREL = F(2.0 ** -8)
EPS = 2.0 ** -24


# ---- the forward pose -------------------------------------------------------------------------------------------------------------

def fwd_vec(pose, d):
    """fwd_vec(m, d)_k = (m[4k] d.x + m[4k+1] d.y) + m[4k+2] d.z, float32, one rounding per operation"""
    m, d = np.asarray(pose, F).reshape(3, 4), np.asarray(d, F)
    return np.stack([((m[k, 0] * d[..., 0] + m[k, 1] * d[..., 1]).astype(F) + m[k, 2] * d[..., 2]).astype(F) for k in range(3)], axis=-1)


def fwd_point(pose, x):
    """fwd_point(m, x)_k = fwd_vec(m, x)_k + m[4k+3]"""
    m = np.asarray(pose, F).reshape(3, 4)
    return (fwd_vec(m, x) + m[:, 3]).astype(F)


def posed_leaves(tris, pose):
    """(v0', e1', e2') of every triangle: the stored (v0, e1, e2) posed forward; the edges are R e1 and R e2"""
    v0, e1, e2 = _split(tris)
    return fwd_point(pose, v0), fwd_vec(pose, e1), fwd_vec(pose, e2)


# ---- (a) the flat answer ------------------------------------------------------------------------------------------------------------

def counts_matrix(inst, lo, hi, staged=True):
    """[boxes, candidates] bool for one instance, and its sorted candidate ids. staged: box_tri's three unit axes (no product:
    the triangle's extent against fl(lo - v0'), fl(hi - v0')) are evaluated for every pair first, in box_tri's own float32
    operations, and all 13 axes only for the pairs that pass them -- the same answer as box_tri on every pair
    (test_world_box_cpu holds the two against each other), much sooner for boxes that are small against the world"""
    tris, cand, pose = inst[0], inst[1], inst[2]
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    valid = BQ.box_valid(lo, hi)
    ok = np.zeros((lo.shape[0], cand.size), bool)
    if cand.size:
        v0, e1, e2 = posed_leaves(np.asarray(tris, F).reshape(-1, 3, 3)[cand], pose)
        zero = F(0)
        pmx = np.where(e2 > np.where(e1 > zero, e1, zero), e2, np.where(e1 > zero, e1, zero))
        pmn = np.where(e2 < np.where(e1 < zero, e1, zero), e2, np.where(e1 < zero, e1, zero))
        step = max(1, (1 << 20) // cand.size)
        for a in range(0, lo.shape[0], step):
            b = min(lo.shape[0], a + step)
            if not staged:
                ok[a:b] = BQ.box_tri(v0[None], e1[None], e2[None], lo[a:b, None, :], hi[a:b, None, :]) & valid[a:b, None]
                continue
            with np.errstate(all="ignore"):
                first = valid[a:b, None].copy()
                for k in range(3):
                    first = first & (pmx[None, :, k] >= (lo[a:b, None, k] - v0[None, :, k])) & (pmn[None, :, k] <= (hi[a:b, None, k] - v0[None, :, k]))
            r, c = np.nonzero(first)
            ok[a + r, c] = BQ.box_tri(v0[c], e1[c], e2[c], lo[a + r], hi[a + r])
    return ok, cand


def rows_of(oks, cands, k):
    """the three answers from per-instance [R, cand] matrices in list order: flag, count, tri rows, inst rows, rows' count"""
    R = oks[0].shape[0] if oks else 0
    ok = np.concatenate(oks, axis=1) if oks else np.zeros((R, 0), bool)
    tri = np.concatenate(cands) if cands else np.zeros(0, np.int64)
    ins = np.concatenate([np.full(c.size, i, np.int64) for i, c in enumerate(cands)]) if cands else np.zeros(0, np.int64)
    count = ok.sum(axis=1).astype(U)
    trows, irows = np.full((R, k), -1, np.int32), np.full((R, k), -1, np.int32)
    rank = np.cumsum(ok, axis=1) - 1     # the columns are in (inst, tri) order
    r, c = np.nonzero(ok & (rank < k))
    trows[r, rank[r, c]] = tri[c]
    irows[r, rank[r, c]] = ins[c]
    return count > 0, count, trows, irows, np.minimum(count, U(k)).astype(U)


def may_meet(inst, lo, hi):
    """[boxes] bool: the boxes that can pass box_tri's unit axes for SOME leaf of the instance. A pair passes unit axis k only if
    max P_k >= fl(lo_k - v0'_k) and min P_k <= fl(hi_k - v0'_k); the rounding is monotone and relative (eps = 2^-24), so a box that
    misses the float64 bounds of all posed leaves by more than 2^-18 of the largest magnitude involved on some axis passes for
    none. Only a shortcut of the brute force: (test_world_box_cpu holds flat() against box_tri on every pair)"""
    tris, cand, pose = inst[0], inst[1], inst[2]
    cand = np.asarray(cand, np.int64).reshape(-1)
    if cand.size == 0:
        return np.zeros(np.asarray(lo).reshape(-1, 3).shape[0], bool)
    v0, e1, e2 = (x.astype(D) for x in posed_leaves(np.asarray(tris, F).reshape(-1, 3, 3)[cand], pose))
    pts = np.concatenate([v0, v0 + e1, v0 + e2])
    blo, bhi = pts.min(0), pts.max(0)
    lo, hi = np.asarray(lo, F).reshape(-1, 3).astype(D), np.asarray(hi, F).reshape(-1, 3).astype(D)
    with np.errstate(invalid="ignore"):
        slack = 2.0 ** -18 * (np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True) + np.abs(pts).max() + np.abs(e1).max() + np.abs(e2).max())
        return ~((lo > bhi + slack) | (hi < blo - slack)).any(axis=1)


def flat(insts, lo, hi, k=K_MAX):
    """(a): (overlaps [R] bool, count [R] uint32, tri [R, k] int32, inst [R, k] int32, rows' count [R] uint32)"""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    R = lo.shape[0]
    valid = BQ.box_valid(lo, hi)
    rs, js, ts = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for j, inst in enumerate(insts):
        sel = np.nonzero(valid & may_meet(inst, lo, hi))[0]
        if sel.size == 0:
            continue
        ok, cand = counts_matrix(inst, lo[sel], hi[sel])
        r, c = np.nonzero(ok)
        rs.append(sel[r])
        js.append(np.full(r.size, j, np.int64))
        ts.append(cand[c])
    r, j, t = np.concatenate(rs), np.concatenate(js), np.concatenate(ts)
    order = np.lexsort((t, j, r))                      # by box, then (inst, tri)
    r, j, t = r[order], j[order], t[order]
    count = np.bincount(r, minlength=R).astype(np.int64)
    rank = np.arange(r.size) - (np.cumsum(count) - count)[r]
    trows, irows = np.full((R, k), -1, np.int32), np.full((R, k), -1, np.int32)
    keep = rank < k
    trows[r[keep], rank[keep]] = t[keep]
    irows[r[keep], rank[keep]] = j[keep]
    count = count.astype(U)
    return count > 0, count, trows, irows, np.minimum(count, U(k)).astype(U)


# ---- (b) the two tests and the walk ---------------------------------------------------------------------------------------------------

def plain_fit(tris):
    """the plain fit transform of a mesh as float32 [3, 4]: each axis' bounds to [0, 1] (an axis without extent: scale 1)"""
    v = np.asarray(tris, F).reshape(-1, 3).astype(D)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    ext = np.where(ext > 0, ext, 1.0)
    M = np.zeros((3, 4))
    M[:, :3] = np.diag(1.0 / ext)
    M[:, 3] = -lo / ext
    return M.astype(F)


def top_keep(clo, chi, lo, hi):
    """WorldBoxBody::keep_top: the child box [clo, chi] grown by WORLD_QSLACK * |q|_inf against the closed world box, negations"""
    with np.errstate(all="ignore"):
        pad = F(WORLD_QSLACK * max(F(np.abs(lo).max()), F(np.abs(hi).max())))
        out = ((chi + pad).astype(F) < lo) | ((clo - pad).astype(F) > hi)
    return not bool(out.any())


def box_row(N, lo, hi):
    """box_row (psm_box_dev.h) for rows N [..., 4] and boxes lo / hi [..., 3], broadcast: the grown interval (glo, ghi)"""
    a, b = (N[..., :3] * lo).astype(F), (N[..., :3] * hi).astype(F)
    mn, mx, ab = np.fmin(a, b), np.fmax(a, b), np.fmax(np.abs(a), np.abs(b))
    ilo = (((mn[..., 0] + mn[..., 1]).astype(F) + mn[..., 2]).astype(F) + N[..., 3]).astype(F)
    ihi = (((mx[..., 0] + mx[..., 1]).astype(F) + mx[..., 2]).astype(F) + N[..., 3]).astype(F)
    S = (((ab[..., 0] + ab[..., 1]).astype(F) + ab[..., 2]).astype(F) + np.abs(N[..., 3])).astype(F)
    h = ((F(2) + S).astype(F) * F(2.0 ** -16)).astype(F)
    return (ilo - h).astype(F), (ihi + h).astype(F)


def compose(M, pose):
    """N [3, 4] float32: N_kj = (M_k0 R_j0 + M_k1 R_j1) + M_k2 R_j2 (row k of M3 R^T), N_k3 = M_k3"""
    M, m = np.asarray(M, F).reshape(-1, 4)[:3], np.asarray(pose, F).reshape(3, 4)
    N = np.zeros((3, 4), F)
    for k in range(3):
        for j in range(3):
            N[k, j] = F(F(F(M[k, 0] * m[j, 0]) + F(M[k, 1] * m[j, 1])) + F(M[k, 2] * m[j, 2]))
        N[k, 3] = M[k, 3]
    return N


def prune_interval(M, pose, lo, hi):
    """WorldBoxBody::enter for boxes lo / hi [..., 3]: the grown interval per normalised axis, (glo, ghi) [..., 3] float32, and
    the margin g [..., 3] granted beside box_row's own h"""
    m = np.asarray(pose, F).reshape(3, 4)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    with np.errstate(all="ignore"):
        N = compose(M, m)
        sl, sh = (lo - m[:, 3]).astype(F), (hi - m[:, 3]).astype(F)
        qmax = np.fmax(np.abs(lo).max(axis=-1), np.abs(hi).max(axis=-1)).astype(F)
        reach = (np.fmax(np.abs(sl).max(axis=-1), np.abs(sh).max(axis=-1)) + (WORLD_BOX_QREL * qmax).astype(F)).astype(F)
        glo, ghi = box_row(N, sl[..., None, :], sh[..., None, :])
        W = ((np.abs(N[:, 0]) + np.abs(N[:, 1])).astype(F) + np.abs(N[:, 2])).astype(F)
        g = ((F(2) + ((W * reach[..., None]).astype(F) + np.abs(N[:, 3])).astype(F)).astype(F) * WORLD_BOX_PAD).astype(F)
        return (glo - g).astype(F), (ghi + g).astype(F), g


def leaf_images(tris, M):
    """the exact (float64) image box of every stored triangle (v0, v0 + e1, v0 + e2) under the fit transform: no padding"""
    v0, e1, e2 = (x.astype(D) for x in _split(tris))
    Md = np.asarray(M, F).reshape(-1, 4)[:3].astype(D)
    V = np.stack([v0, v0 + e1, v0 + e2], axis=-2)
    img = V @ Md[:, :3].T + Md[:, 3]
    return img.min(axis=-2), img.max(axis=-2)


def prune_keeps(inst, lo, hi):
    """[boxes, candidates] bool: the leaves of one instance whose unpadded image box meets the grown interval of each box"""
    tris, cand, pose, M = inst
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    if cand.size == 0:
        return np.zeros((lo.shape[0], 0), bool)
    tmin, tmax = leaf_images(np.asarray(tris, F).reshape(-1, 3, 3)[cand], M)
    glo, ghi, _ = prune_interval(M, pose, lo, hi)
    with np.errstate(invalid="ignore"):
        return (~(tmax[None] < glo[:, None, :].astype(D)) & ~(tmin[None] > ghi[:, None, :].astype(D))).all(axis=-1)


class BoxWorld(WQ.World):
    """(b): world_query_model's boxes and tree, world_box.hip's tests and walk"""

    def __init__(self, insts):
        super().__init__([(t, c, m) for t, c, m, _ in insts])
        self.box_insts = insts

    def boxes(self, lo, hi, k=K_MAX):
        """((overlaps, count, tri, inst, rows' count), (entered by the count / triangles walk, entered by the overlaps walk))"""
        lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
        R = lo.shape[0]
        valid = BQ.box_valid(lo, hi)
        pairs = [counts_matrix(inst, lo, hi) for inst in self.box_insts]
        keeps = [prune_keeps(inst, lo, hi) for inst in self.box_insts]
        seen = [np.zeros_like(p[0]) for p in pairs]           # what the full walk reaches and counts
        flag = np.zeros(R, bool)
        ent = ([], [])
        for i in range(R):
            if not valid[i] or not self.box_insts:
                ent[0].append([])
                ent[1].append([])
                continue

            def keep(clo, chi):
                return top_keep(clo, chi, lo[i], hi[i]), F(0)

            def visit_all(j):
                seen[j][i] = pairs[j][0][i] & keeps[j][i]
                return False

            def visit_any(j):
                flag[i] |= bool((pairs[j][0][i] & keeps[j][i]).any())
                return bool(flag[i])
            ent[0].append(self.tree.walk(keep, visit_all))
            ent[1].append(self.tree.walk(keep, visit_any))
        if not self.box_insts:
            return flat([], lo, hi, k), ent
        f, count, trows, irows, nrows = rows_of(seen, [p[1] for p in pairs], k)
        return (flag, count, trows, irows, nrows), ent

    def reachable(self, lo, hi):
        """brute force: per box the set of instances whose padded world box meets the slack-grown world box"""
        lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
        valid = BQ.box_valid(lo, hi)
        return [sorted(j for j in range(len(self.box_insts)) if top_keep(self.lo[j], self.hi[j], lo[i], hi[i])) if valid[i] else []
                for i in range(lo.shape[0])]


# ---- the prune's chain, evaluated in float64 ---------------------------------------------------------------------

def prune_figures(inst, lo, hi):
    """For one instance and boxes lo / hi [B, 3] against ALL its candidates: which pairs count (float32, [B, C]); whether the
    float32 interval keeps the leaf's exact unpadded image; and per normalised axis [B, C, 3]
      observed: the distance between the exact image of the stored triangle and the exact interval of the shifted box under the
                float32 N (both in float64),
      bound:    the chain's claim for it -- E: 3e-5 sqrt 3 |N_k|_1 D; the rounding of N: 5.4e-7 |N_k|_1 D; the forward posing:
                eps (16 D + Q) |N_k|_1; box_tri: 16 eps |e'|_inf |N_k|_1,
      granted:  the margin g_k (box_row's own h is left to its own rounding)."""
    tris, cand, pose, M = inst
    ok, cand = counts_matrix(inst, lo, hi)
    kept = prune_keeps(inst, lo, hi)
    t = np.asarray(tris, F).reshape(-1, 3, 3)[cand]
    tmin, tmax = leaf_images(t, M)
    m = np.asarray(pose, F).reshape(3, 4)
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    N = compose(M, m).astype(D)
    sl, sh = lo.astype(D) - m[:, 3].astype(D), hi.astype(D) - m[:, 3].astype(D)
    pa, pb = sl[:, None, :] * N[:, :3], sh[:, None, :] * N[:, :3]                      # [B, axis, j]
    elo, ehi = np.minimum(pa, pb).sum(-1) + N[:, 3], np.maximum(pa, pb).sum(-1) + N[:, 3]
    observed = np.maximum(0, np.maximum(tmin[None] - ehi[:, None, :], elo[:, None, :] - tmax[None]))
    W = np.abs(N[:, :3]).sum(axis=1)                                                   # [axis]
    Dm = np.maximum(np.abs(sl), np.abs(sh)).max(axis=1)                                # [B]
    Q = np.maximum(np.abs(lo), np.abs(hi)).max(axis=1).astype(D)
    _, e1, e2 = posed_leaves(t, m)
    size = np.abs(np.concatenate([e1, e2], axis=-1).astype(D)).max(axis=-1)            # [C]
    world = (3e-5 * np.sqrt(3.0) * 1.0001 + 5.4e-7 + 16 * EPS) * Dm[:, None] + EPS * Q[:, None] + 16 * EPS * size[None]
    bound = world[:, :, None] * W
    g = prune_interval(M, m, lo, hi)[2].astype(D)
    return ok, kept, observed, bound, np.broadcast_to(g[:, None, :], observed.shape)
