"""The k-best queries of an instance world (psm_world_first_hits_dev / psm_world_nearest_dev, include/psm_hip.h; world.hip;
DESIGN.md 4.14) in numpy. No float arithmetic is restated here: per instance the query is moved by instance_query_model.move /
rotate and answered by kbest_query_model.first_hits / nearest as it is (the per-instance rows, sorted by (value, tri)); the d2 a
closest-point slot was chosen by comes from scene_query_model.d2_of. What this adds is the merge: the per-instance rows, in list
order, sorted by a stable sort on the value as a float (-0 == +0) -- which leaves equal values in (inst, tri) order -- and cut at
k. A member of the world's k smallest is among its own instance's k smallest, so merging rows of k slots is a complete model.

An instance is (tris [T, 3, 3], cand, pose) as in instance_query_model."""
import numpy as np

import instance_query_model as NQ
import kbest_query_model as KQ
import scene_query_model as SQ

F = np.float32


def _merge(rows_per, val_per, count_per, k):
    """rows [R, k, 4], inst [R, k] int32 (-1 in a miss slot) and count [R] uint32 from per-instance rows [R, k, 4], the values
    they were sorted by [R, k] and their counts [R], all in list order"""
    R = rows_per[0].shape[0]
    rows = np.concatenate(rows_per, axis=1)                                              # [R, N k, 4]: inst-major, slots ascending
    val = np.concatenate(val_per, axis=1)
    live = np.concatenate([np.arange(k)[None] < c[:, None] for c in count_per], axis=1)
    inst = np.repeat(np.arange(len(rows_per), dtype=np.int32), k)
    key = np.where(live, val, F(np.inf)).astype(F)                                       # (a counting value is never a NaN)
    order = np.argsort(key, axis=1, kind="stable")                                       # by value as floats; equal: (inst, tri)
    # the live slots first (one may sit at +inf, where the misses were put): stable again, so the order among them stays
    order = np.take_along_axis(order, np.argsort(~np.take_along_axis(live, order, axis=1), axis=1, kind="stable"), axis=1)[:, :k]
    count = np.minimum(live.sum(axis=1), k).astype(np.uint32)
    out = np.zeros((R, k, 4), F)
    out[:, :, 2] = np.inf
    out.view(np.int32)[:, :, 3] = -1
    oinst = np.full((R, k), -1, np.int32)
    r = np.arange(R)
    for s in range(order.shape[1]):
        filled = s < count
        out[filled, s] = rows[r, order[:, s]][filled]
        oinst[filled, s] = inst[order[:, s]][filled]
    return out, oinst, count


def first_hits(insts, origins, directs, k, tmin=0.0, tmax=np.inf):
    """psm_world_first_hits_dev over the ordered list `insts`: rows [R, k, 4], inst [R, k], count [R]; the key is (t, inst, tri)"""
    per = [KQ.first_hits(t, c, NQ.move(m, origins), NQ.rotate(m, directs), k, tmin, tmax) for t, c, m in insts]
    return _merge([r for r, _ in per], [r[:, :, 2] for r, _ in per], [c for _, c in per], k)


def nearest(insts, points, k, rmax=np.inf):
    """psm_world_nearest_dev: rows [R, k, 4] (u, v, dist, tri), inst [R, k], count [R]; the key is (d2, inst, tri), d2 the
    instance's own value for its own moved point"""
    rows_per, val_per, count_per = [], [], []
    for t, c, m in insts:
        mp = NQ.move(m, points)
        rows, count = KQ.nearest(t, c, mp, k, rmax)
        rows_per.append(rows)
        val_per.append(np.stack([SQ.d2_of(t, mp, np.ascontiguousarray(rows[:, s])) for s in range(k)], axis=1))
        count_per.append(count)
    return _merge(rows_per, val_per, count_per, k)
