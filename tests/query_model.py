"""A numpy float32 restatement of the ray queries (psm_bvh_intersect_dev / psm_bvh_occluded_dev, include/psm_hip.h) and of the
clamped triangle test they leave behind (tri_test, trace.hip; intersectTriangle, vertex.glsl:140-189; psmo_brute_force).

Every operation is one float32 numpy operation in the order psm_math.h writes it: the library is compiled with -ffp-contract=off,
so each of its float32 operations rounds once, as numpy's do (no fused multiply-add on either side; division and sqrt are
correctly rounded on both). The brute forces here are the yardsticks of tests/test_query_cpu.py and tests/test_gpu_query.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F = np.float32
PZERO = F(0.0005)        # constants.glsl:72
INF = F(10000.0)         # constants.glsl:82
TOL = F(0.00001)
ONE_TOL = F(1.00001)


def dot3(a, b):
    """psm_math.h dot3: (a.x b.x + a.y b.y) + a.z b.z"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    """psm_math.h cross3"""
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2],
                     a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def normalize3(a):
    """psm_math.h normalize3: a * (1 / sqrt(dot3(a, a)))"""
    a = np.asarray(a, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F(1.0) / np.sqrt(dot3(a, a))
        return a * inv[..., None]


def tri_test(tris, orig, dirn, clamp):
    """The triangle test of every ray against every triangle: tris [T, 3, 3] (world space), orig / dirn [R, 3] (dirn already
    normalised). Returns t, u, v, ok [R, T]; ok is the test's own acceptance (det, u, v, u + v) -- the t rule is the caller's.
    clamp=True: intersectTriangle's invDev = 1 / (max(|det|, 1e-6) sign(det)); False: the queries' 1 / det."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    v0 = tris[None, :, 0, :]
    e1 = (tris[:, 1, :] - tris[:, 0, :])[None]   # bvh_prepare_tris: v1 - v0, v2 - v0
    e2 = (tris[:, 2, :] - tris[:, 0, :])[None]
    o = np.asarray(orig, F)[:, None, :]
    d = np.asarray(dirn, F)[:, None, :]
    with np.errstate(all="ignore"):
        pvec = cross3(d, e2)
        det = dot3(e1, pvec)
        ok = ~(np.abs(det) <= F(0.0))
        if clamp:
            ad = np.abs(det)
            m = np.where(ad < F(0.000001), F(0.000001), ad)          # pmax(|det|, 1e-6): x < y ? y : x
            sg = np.where(det > 0, F(1.0), np.where(det < 0, F(-1.0), F(0.0)))
            invDev = F(1.0) / (m * sg)
        else:
            invDev = F(1.0) / det
        tvec = o - v0
        u = dot3(tvec, pvec) * invDev
        ok &= ~((u < -TOL) | (u > ONE_TOL))
        qvec = cross3(tvec, e1)
        v = dot3(d, qvec) * invDev
        ok &= ~((v < -TOL) | ((u + v) > ONE_TOL))
        t = dot3(e2, qvec) * invDev
    return t, u, v, ok


def _chunks(n_rays, n_tris, budget=1 << 22):
    step = max(1, budget // max(n_tris, 1))
    for a in range(0, n_rays, step):
        yield a, min(n_rays, a + step)


def brute_force_clamped(tris, origins, directs):
    """psmo_brute_force for many rays: the clamped test, a hit is t >= -PZERO (greaterEqualF(t, 0)) and t < INF - PZERO, the first
    triangle of the smallest t wins. Returns found [R] bool and hits [R] with fields u, v, t, tri (a miss: t = INF, tri = -1)."""
    origins = np.asarray(origins, F).reshape(-1, 3)
    d = normalize3(np.asarray(directs, F).reshape(-1, 3))
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    R = origins.shape[0]
    out = np.zeros(R, [("u", F), ("v", F), ("t", F), ("tri", np.int32)])
    out["t"], out["tri"] = INF, -1
    for a, b in _chunks(R, tris.shape[0]):
        t, u, v, ok = tri_test(tris, origins[a:b], d[a:b], clamp=True)
        with np.errstate(invalid="ignore"):
            hit = ok & ((t - F(0.0)) > -PZERO) & (t < INF - PZERO)
        tt = np.where(hit, t, INF)
        k = np.argmin(tt, axis=1)              # the first of the smallest: strict `T < best` in index order
        r = np.arange(b - a)
        best = tt[r, k]
        found = best < INF
        out["t"][a:b] = np.where(found, best, INF)
        out["tri"][a:b] = np.where(found, k, -1)
        out["u"][a:b] = np.where(found, u[r, k], F(0))
        out["v"][a:b] = np.where(found, v[r, k], F(0))
    return out["tri"] >= 0, out


def _window(n, x):
    return np.broadcast_to(np.asarray(x, F), (n,)).astype(F)


def ray_valid(origins, dirn, tmin, tmax):
    """The queries' rays that can hit at all: finite origin and normalised direction (NaN, inf and zero directions are not),
    tmin <= tmax (false with a NaN)."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(origins).all(axis=1) & np.isfinite(dirn).all(axis=1) & (tmin <= tmax)


def query(tris, cand, origins, directs, tmin=0.0, tmax=np.inf):
    """psm_bvh_intersect_dev and psm_bvh_occluded_dev over the candidate triangle ids `cand` (the hierarchy's leaves,
    PSM_BVH_LEAF_TRI): the unclamped test, a hit counts iff tmin <= t <= tmax, closest = smallest t and on bit-equal t the lowest
    id. Returns (hits [R, 4] float32 as the kernel writes psm_hit -- u, v, t, tri bits; a miss is 0, 0, +inf, -1 -- , any [R] bool)."""
    origins = np.asarray(origins, F).reshape(-1, 3)
    d = normalize3(np.asarray(directs, F).reshape(-1, 3))
    R = origins.shape[0]
    lo, hi = _window(R, tmin), _window(R, tmax)
    cand = np.sort(np.asarray(cand, np.int64).reshape(-1))
    tris = np.asarray(tris, F).reshape(-1, 3, 3)[cand]
    hits = np.zeros((R, 4), F)
    hits[:, 2] = np.inf
    hits.view(np.int32)[:, 3] = -1
    anyhit = np.zeros(R, bool)
    valid = ray_valid(origins, d, lo, hi)
    if cand.size == 0:
        return hits, anyhit

    def chunk(ab):
        a, b = ab
        t, u, v, ok = tri_test(tris, origins[a:b], d[a:b], clamp=False)
        with np.errstate(invalid="ignore"):
            hit = ok & valid[a:b, None] & (t >= lo[a:b, None]) & (t <= hi[a:b, None])
        found = hit.any(axis=1)
        tt = np.where(hit, t, np.inf).astype(F)
        best = tt.min(axis=1)
        # the lowest id among the hits whose t compares equal to the smallest (-0 == +0; candidates are sorted by id)
        k = np.argmax(hit & (t == best[:, None]), axis=1)
        r = np.arange(b - a)
        sel = found
        hits[a:b, 0] = np.where(sel, u[r, k], F(0))
        hits[a:b, 1] = np.where(sel, v[r, k], F(0))
        hits[a:b, 2] = np.where(sel, t[r, k], F(np.inf))
        hits.view(np.int32)[a:b, 3] = np.where(sel, cand[k], -1)
        anyhit[a:b] = found

    # (numpy's array operations release the GIL: ray chunks on a few threads)
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(chunk, _chunks(R, cand.size, 1 << 20)))
    return hits, anyhit


def deep_fixture(seed=0, clusters=21, per=64, rays=256):
    """A hierarchy deeper than the pipeline's 16-entry stack: `clusters` clusters of `per` small triangles at x = 2^-k (k = 0 ..
    clusters-1) -- every Morton level splits one cluster from the rest, both internal, so a ray along the row pushes a subtree per
    level -- and `rays` rays from near the origin along +x through all of them. Returns tris [n, 3, 3], origins, directions."""
    rng = np.random.RandomState(5150 + seed)
    out = []
    for k in range(clusters):
        c = F(2.0) ** F(-k)
        s = c * F(0.25)
        centre = np.array([c, 0.0, 0.0], F) + rng.uniform(-1, 1, (per, 1, 3)).astype(F) * np.array([s, s, s], F)
        out.append(centre + rng.uniform(-1, 1, (per, 3, 3)).astype(F) * s * F(0.5))
    tris = np.concatenate(out).astype(F)
    o = np.zeros((rays, 3), F)
    o[:, 0] = F(-0.5)
    d = np.zeros((rays, 3), F)
    d[:, 0] = F(1.0)
    o[:, 1:] = rng.uniform(-1e-3, 1e-3, (rays, 2)).astype(F)
    d[:, 1:] = rng.uniform(-1e-4, 1e-4, (rays, 2)).astype(F)
    return tris, o, d
