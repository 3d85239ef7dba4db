"""A numpy restatement of mesh clearance (psm_bvh_mesh_closest_dev / psm_bvh_mesh_within_dev / psm_bvh_mesh_clearance_dev,
include/psm_hip.h "mesh clearance"; mesh_dist.hip): a composition, with no arithmetic of its own.

The query triangle of (pose m, triangle t of `other`) is mesh_query_model.posed's; its record is tri_dist_query_model.query's
for that triangle under the call's one rmax; a triangle of other that is no leaf reads the miss record. The clearance record of
a pose is the record of t*, the lowest t among the triangles whose record has the smallest float32 dist, with t* in slot 6; a
pose where no pair counts reads {0, 0, +inf, -1, 0, 0, -1, 0}. The flag is tri >= 0 of that record.

It also restates the word the lanes of a pose share in the launch, key = (bits(dist) << 32) | t, and simulates the protocol
around it under arbitrary schedules. The yardstick of tests/test_mesh_dist_cpu.py and tests/test_gpu_mesh_dist.py."""
import numpy as np

import mesh_query_model as MQ
import tri_dist_query_model as TD

F = np.float32
NONE = (1 << 64) - 1   # the word before anything is published


def closest(tris, leaves, other_tris, other_leaves, poses, rmax=np.inf):
    """psm_bvh_mesh_closest_dev by brute force: [p, T, 8] float32 records (tri_dist_query_model.query's layout)"""
    q = MQ.posed(other_tris, poses)
    p, t = q.shape[:2]
    hits = TD.miss_records(p * t).reshape(p, t, 8)
    keep = np.sort(np.asarray(other_leaves, np.int64).reshape(-1))
    if p and keep.size:
        n = p * keep.size
        rec, _ = TD.query(tris, leaves, q[:, keep].reshape(n, 3, 3), np.full(n, rmax, F))
        hits[:, keep] = rec.reshape(p, keep.size, 8)
    return hits


def key_of(dist, t):
    """(bits(dist) << 32) | t as a Python int"""
    return (int(np.asarray(dist, F).view(np.uint32)) << 32) | int(t)


def reduce(hits):
    """the clearance records [p, 8] of closest()'s records [p, T, 8]: per pose the lowest (dist, t) over the triangles that
    found one, compared on the float32 dist as stored, that triangle's record with t in slot 6; else the miss record with -1"""
    p, t = hits.shape[:2]
    out = TD.miss_records(p)
    out.view(np.int32)[:, 6] = -1
    found = hits.view(np.int32)[:, :, 3] >= 0
    for q in range(p):
        ids = np.nonzero(found[q])[0]
        if ids.size:
            d = hits[q, ids, 2]
            best = ids[d == d.min()].min()
            out[q] = hits[q, best]
            out.view(np.int32)[q, 6] = best
    return out


def query(tris, leaves, other_tris, other_leaves, poses, rmax=np.inf):
    """the three queries: (closest [p, T, 8], clearance [p, 8], within [p] bool)"""
    hits = closest(tris, leaves, other_tris, other_leaves, poses, rmax)
    rec = reduce(hits)
    return hits, rec, rec.view(np.int32)[:, 3] >= 0


def simulate(dists, rng, early=True):
    """One pose's launch under a random schedule, the per-lane work done by the caller's records. dists: {t: [d, ...]} -- for
    lane t (a triangle of other) the float32 dists of its candidates that count, in the order its walk meets them (empty: it
    finds none). Lanes run interleaved in a shuffled order; each step of a lane first reads a snapshot of the word that is
    randomly stale -- any value the word has held so far, or "none" --, keeps the lowest key it has seen, drops candidates
    beyond its D (acceptance dist <= D, closed) and retires on (0, t') with t' < t; it publishes early (when its best improves)
    or only at its end, and only below the last key it saw. Returns the final word."""
    history = [NONE]
    word = [NONE]

    def lane(t, cand):
        seen, best = NONE, None
        for d in cand:
            stale = history[rng.randint(len(history))]
            seen = min(seen, stale)
            if seen != NONE:
                if (seen >> 32) == 0 and (seen & 0xffffffff) < t:
                    return
                D = np.asarray(seen >> 32, np.uint32).view(F)
                if best is not None and best > D:
                    best = None
                if not d <= D:
                    yield
                    continue
            if best is None or d < best:
                best = d
                if early and rng.randint(2):
                    seen = publish(t, best, seen)
            yield
        if best is not None:
            publish(t, best, seen)

    def publish(t, d, seen):
        own = key_of(d, t)
        if own < seen:
            old = word[0]
            word[0] = min(old, own)
            history.append(word[0])
            return min(old, own)
        return seen

    live = [lane(t, c) for t, c in dists.items()]
    while live:
        k = rng.randint(len(live))
        try:
            next(live[k])
        except StopIteration:
            live.pop(k)
    return word[0]
