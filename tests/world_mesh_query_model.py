"""The mesh queries of an instance world (psm_world_mesh_overlaps_dev / psm_world_mesh_count_dev / psm_world_mesh_triangles_dev,
include/psm_hip.h "mesh queries over a world"; world_mesh.hip) in numpy: a composition, with no arithmetic of its
own. mesh_query_model.posed makes the query triangles of every (pose, triangle of `other`) as psm_mesh_dev.h makes them, and
world_tri_query_model.flat answers them over the ordered instance list. A triangle of `other` that is no leaf answers 0 / -1;
skip removes an instance from the list and keeps the indices of the others. The yardstick of tests/test_world_mesh_cpu.py and
tests/test_gpu_world_mesh.py.

An instance is (tris [T, 3, 3], cand, pose [3, 4], ...) as in world_tri_query_model (flat reads the first three)."""
import numpy as np

import mesh_query_model as MQ
import world_tri_query_model as WT

K_MAX = WT.K_MAX


def query(insts, other_tris, other_leaves, poses, k=K_MAX, skip=None):
    """(flag [p] bool, count [p, T] uint32 -- the full count --, tri [p, T, k] int32, inst [p, T, k] int32, the rows' count
    [p, T] uint32 = min(k, count))"""
    q = MQ.posed(other_tris, poses)
    p, t = q.shape[:2]
    count = np.zeros((p, t), np.uint32)
    tri = np.full((p, t, k), -1, np.int32)
    inst = np.full((p, t, k), -1, np.int32)
    rcount = np.zeros((p, t), np.uint32)
    keep = np.sort(np.asarray(other_leaves, np.int64).reshape(-1))
    insts = list(insts)
    if skip is not None:
        if not 0 <= skip < len(insts):
            raise ValueError("skip must be an index of the instance list")
        kept = [j for j in range(len(insts)) if j != skip]   # the list without it ...
    else:
        kept = list(range(len(insts)))
    if p and keep.size and kept:
        _, c, tr, ir, rc = WT.flat([insts[j] for j in kept], q[:, keep].reshape(-1, 3, 3), k)
        ir = np.where(ir >= 0, np.asarray(kept, np.int32)[np.maximum(ir, 0)], -1).astype(np.int32)   # ... and the indices kept
        count[:, keep], rcount[:, keep] = c.reshape(p, -1), rc.reshape(p, -1)
        tri[:, keep], inst[:, keep] = tr.reshape(p, -1, k), ir.reshape(p, -1, k)
    return (count > 0).any(axis=1), count, tri, inst, rcount
