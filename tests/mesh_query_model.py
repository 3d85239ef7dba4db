"""A numpy restatement of the mesh queries (psm_bvh_mesh_overlaps_dev / psm_bvh_mesh_count_dev / psm_bvh_mesh_triangles_dev,
include/psm_hip.h "mesh queries"; mesh.hip, psm_mesh_dev.h mesh_query_tri).

The query triangle of (pose m, leaf t of `other`) is made from other's STORED record (v0, e1 = v1 - v0, e2 = v2 - v0) in float32,
every operation one numpy float32 operation in the order psm_mesh_dev.h and psm_world_box_dev.h write them (the library builds
with -ffp-contract=off): a = fwd_point(m, v0), b = a + fwd_vec(m, e1), c = a + fwd_vec(m, e2). The answers are then
tri_query_model.query's for those triangles, one by one; a triangle of other that is no leaf answers 0 / -1. The yardstick of
tests/test_mesh_query_cpu.py and tests/test_gpu_mesh_query.py."""
import numpy as np

import tri_query_model as TQ
from point_query_model import _split

F = np.float32
K_MAX = TQ.K_MAX
ORTHONORMAL_TOL = 1e-5   # psm_hip.h: the largest entry of R^T R - 1 a pose may have


def poses12(poses):
    """poses as the C ABI takes them: float32 [p, 12], the rows of [R | T], from one matrix or [p, 3, 4] / [p, 4, 4]; a pose
    that is not finite or not rigid is refused (ValueError), as pose_fault refuses it"""
    m = np.asarray(poses)
    if m.ndim == 2:
        m = m[None]
    m = m[:, :3, :].astype(F)
    if not np.isfinite(m).all():
        raise ValueError("a pose has a non-finite entry")
    r = m[:, :, :3].astype(np.float64)
    if m.shape[0] and np.abs(np.einsum("pia,pib->pab", r, r) - np.eye(3)).max() > ORTHONORMAL_TOL:
        raise ValueError("a pose is not rigid")
    return np.ascontiguousarray(m.reshape(-1, 12))


def fwd_vec(m, d):
    """fwd_vec (psm_world_box_dev.h): m [..., 12], d [..., 3] float32, broadcast"""
    return np.stack([(m[..., 4 * k] * d[..., 0] + m[..., 4 * k + 1] * d[..., 1]) + m[..., 4 * k + 2] * d[..., 2] for k in range(3)], axis=-1)


def fwd_point(m, x):
    """fwd_point (psm_world_box_dev.h)"""
    return np.stack([((m[..., 4 * k] * x[..., 0] + m[..., 4 * k + 1] * x[..., 1]) + m[..., 4 * k + 2] * x[..., 2]) + m[..., 4 * k + 3]
                     for k in range(3)], axis=-1)


def pose_records(m, v0, e1, e2):
    """mesh_query_tri (psm_mesh_dev.h) record by record: m [n, 12], v0 / e1 / e2 [n, 3], float32; returns [n, 3, 3] = a, b, c"""
    m, v0, e1, e2 = (np.asarray(x, F) for x in (m, v0, e1, e2))
    with np.errstate(all="ignore"):
        a = fwd_point(m, v0)
        b = a + fwd_vec(m, e1)
        c = a + fwd_vec(m, e2)
    return np.stack([a, b, c], axis=1).astype(F)


def posed(other_tris, poses):
    """the query triangles [p, T, 3, 3] of every triangle of `other` (loaded as other_tris) at every pose"""
    m = poses12(poses)
    v0, e1, e2 = _split(other_tris)
    p, t = m.shape[0], v0.shape[0]
    rep = np.repeat(m, t, axis=0)
    return pose_records(rep, np.tile(v0, (p, 1)), np.tile(e1, (p, 1)), np.tile(e2, (p, 1))).reshape(p, t, 3, 3)


def query(tris, leaves, other_tris, other_leaves, poses, k=K_MAX):
    """The three mesh queries by brute force. tris / leaves: the queried hierarchy's loaded triangles and its leaves' ids
    (PSM_BVH_LEAF_TRI); other_tris / other_leaves: the other hierarchy's. Returns (flag [p] bool, count [p, T] uint32 -- the full
    count --, rows [p, T, k] int32, the rows' count [p, T] uint32 = min(k, count))"""
    q = posed(other_tris, poses)
    p, t = q.shape[:2]
    count = np.zeros((p, t), np.uint32)
    rows = np.full((p, t, k), -1, np.int32)
    rcount = np.zeros((p, t), np.uint32)
    keep = np.sort(np.asarray(other_leaves, np.int64).reshape(-1))
    if p and keep.size:
        _, c, r, rc = TQ.query(tris, leaves, q[:, keep].reshape(-1, 3, 3), k)
        count[:, keep], rows[:, keep], rcount[:, keep] = c.reshape(p, -1), r.reshape(p, -1, k), rc.reshape(p, -1)
    return (count > 0).any(axis=1), count, rows, rcount
