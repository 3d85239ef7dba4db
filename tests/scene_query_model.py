"""The scene queries (psm_scene_*_dev, include/psm_hip.h "scene queries") in numpy: the combination rules across geometries, on top
of the per-candidate yardsticks -- query_model (rays), point_query_model (points), inside_query_model (counts and votes), which
are used as they are.

A scene is a list of geometries (tris [T, 3, 3], cand): the triangles of one hierarchy and the ids of its leaves. A candidate of
the scene is (geom, tri). The rules:
  closest hit / closest point   the smallest t / d2; on a bit-equal value the lexicographically lowest (geom, tri)
  any hit / within              the OR over the geometries
  hit count                     the sum over the geometries
  inside                        ray k votes iff its crossings summed over ALL geometries are odd; then the majority
  signed distance               the scene's closest point with the scene's inside sign; a miss casts no rays
combine_closest / combine_points are the rules alone, over per-geometry results: the GPU tests also feed them the
single-hierarchy queries' own outputs."""
import numpy as np

import inside_query_model as IQ
import point_query_model as PQ
import query_model as Q

F = np.float32


def _miss(n):
    hits = np.zeros((n, 4), F)
    hits[:, 2] = np.inf
    hits.view(np.int32)[:, 3] = -1
    return hits


def combine_closest(per_geom, keys=None):
    """per_geom: one psm_hit array [R, 4] per geometry, in scene order, each what that geometry alone answers (within one geometry
    the lowest tri of the smallest value has already won). keys: the values compared, default the records' t. The smallest key
    wins; a later geometry replaces an earlier one only with a strictly smaller key (-0 == +0: the earlier one stays), which is
    "the lowest (geom, tri) on a bit-equal value". Returns hits [R, 4] and geom [R] int32 (-1: a miss)."""
    n = per_geom[0].shape[0]
    hits, geom = _miss(n), np.full(n, -1, np.int32)
    best = np.full(n, np.inf, F)
    for g, h in enumerate(per_geom):
        k = h[:, 2] if keys is None else keys[g]
        found = h.view(np.int32)[:, 3] >= 0
        with np.errstate(invalid="ignore"):
            take = found & ((geom < 0) | (k < best))
        hits[take] = h[take]
        geom[take] = g
        best[take] = k[take]
    return hits, geom


def d2_of(tris, points, hits):
    """the squared distance a closest-point record was chosen by: closest_on_tri of its own triangle, recomputed (the record holds
    sqrt(d2), and two different d2 can round to one distance). +inf on a miss."""
    p = np.asarray(points, F).reshape(-1, 3)
    tri = hits.view(np.int32)[:, 3]
    found = np.nonzero(tri >= 0)[0]
    out = np.full(p.shape[0], np.inf, F)
    if found.size:
        v0, e1, e2 = PQ._split(np.asarray(tris, F).reshape(-1, 3, 3)[tri[found]])
        out[found] = PQ.closest_on_tris(v0, e1, e2, p[found])[2]
    return out


def combine_points(geoms, points, per_geom):
    """combine_closest for closest-point records: the value compared is d2 (d2_of), not the distance in the record"""
    return combine_closest(per_geom, [d2_of(g[0], points, h) for g, h in zip(geoms, per_geom)])


def intersect(geoms, origins, directs, tmin=0.0, tmax=np.inf):
    """psm_scene_intersect_dev and psm_scene_occluded_dev: (hits [R, 4], geom [R] int32, any [R] bool)"""
    res = [Q.query(t, c, origins, directs, tmin, tmax) for t, c in geoms]
    hits, geom = combine_closest([r[0] for r in res])
    return hits, geom, np.logical_or.reduce([r[1] for r in res])


def count(geoms, origins, directs, tmin=0.0, tmax=np.inf):
    """psm_scene_count_hits_dev: uint32 [R]"""
    return np.sum([IQ.count(t, c, origins, directs, tmin, tmax) for t, c in geoms], axis=0, dtype=np.uint32)


def closest_point(geoms, points, rmax=np.inf):
    """psm_scene_closest_point_dev and psm_scene_within_dev: (hits [R, 4], geom [R] int32, within [R] bool)"""
    res = [PQ.query(t, c, points, rmax) for t, c in geoms]
    hits, geom = combine_points(geoms, points, [r[0] for r in res])
    return hits, geom, np.logical_or.reduce([r[1] for r in res])


def parities(geoms, points, samples=5):
    """[samples, R] bool: row k = "the crossings of ray k summed over all geometries are odd" -- the XOR of the geometries' own"""
    return np.logical_xor.reduce([IQ.parities(t, c, points, samples) for t, c in geoms])


def inside(geoms, points, samples=3):
    """psm_scene_inside_dev: bool [R]"""
    assert samples in (1, 3, 5)
    return IQ.vote(parities(geoms, points, samples), samples)


def signed_distance(geoms, points, rmax=np.inf, samples=3):
    """psm_scene_signed_distance_dev: (hits [R, 4], geom [R] int32)"""
    p = np.asarray(points, F).reshape(-1, 3)
    hits, geom, _ = closest_point(geoms, p, rmax)
    found = np.nonzero(geom >= 0)[0]
    ins = inside(geoms, p[found], samples)
    hits.view(np.uint32)[found[ins], 2] |= np.uint32(0x80000000)
    return hits, geom


def split(tris, sizes):
    """tris cut into consecutive parts of the given sizes (the last takes the rest): a list of [Tg, 3, 3] and their offsets"""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    offs = offs[offs < tris.shape[0]]
    ends = np.concatenate([offs[1:], [tris.shape[0]]])
    return [tris[a:b] for a, b in zip(offs, ends)], offs


def merged_ids(hits, geom, offs):
    """the records of a scene over consecutive parts with tri as the id in the concatenation: tri + the part's offset"""
    out = hits.copy()
    found = geom >= 0
    out.view(np.int32)[found, 3] += np.asarray(offs, np.int32)[geom[found]]
    return out
