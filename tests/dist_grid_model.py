"""A numpy restatement of the distance-field grids (psm_grid_distance_dev / psm_grid_signed_distance_dev, include/psm_hip.h "voxel
grids: distance fields"; grid_dist.hip): every voxel is what the point queries' models (point_query_model.query,
inside_query_model.signed_distance) give for the voxel's centre. The yardstick of tests/test_dist_grid_cpu.py and, for small
grids, of tests/test_gpu_dist_grid.py; and what the cases of the GPU test are worth (ties, zeros, misses, the signed kinds)."""
import numpy as np

import grid_query_model as GQ
import inside_query_model as IQ
import point_query_model as PQ

F = np.float32


def _shape(grid):
    nx, ny, nz = grid[2]
    return nz, ny, nx


def field(tris, leaves, grid, rmax=np.inf):
    """(dist float32 [nz, ny, nx], tri int32 [nz, ny, nx]): psm_bvh_closest_point_dev's t and tri of every centre"""
    hits, _ = PQ.query(tris, leaves, GQ.voxel_centres(*grid), rmax)
    return hits[:, 2].copy().reshape(_shape(grid)), hits.view(np.int32)[:, 3].copy().reshape(_shape(grid))


def signed_field(tris, leaves, grid, rmax=np.inf, samples=3):
    """the same with psm_bvh_signed_distance_dev's t"""
    hits = IQ.signed_distance(tris, leaves, GQ.voxel_centres(*grid), rmax, samples)
    return hits[:, 2].copy().reshape(_shape(grid)), hits.view(np.int32)[:, 3].copy().reshape(_shape(grid))


def ties_zeros_misses(tris, leaves, grid, rmax):
    """what a grid tests: the voxels with two or more triangles at the bit-equal smallest d2 (the lowest id must win there), the
    voxels at distance exactly 0, and the voxels with no triangle within rmax"""
    cand = np.sort(np.asarray(leaves, np.int64).reshape(-1))
    v0, e1, e2 = PQ._split(np.asarray(tris, F).reshape(-1, 3, 3)[cand])
    p = GQ.voxel_centres(*grid)
    _, _, d2 = PQ.closest_on_tris(v0[None], e1[None], e2[None], p[:, None, :])
    best = d2.min(axis=1)
    ties = int(((d2 == best[:, None]).sum(axis=1) >= 2).sum())
    zeros = int((best == 0).sum())
    misses = int((~(np.sqrt(d2) <= F(rmax)).any(axis=1)).sum())
    return ties, zeros, misses


def signed_kinds(tris, leaves, grid, rmax, samples=3):
    """(hit and inside, hit and outside, miss and inside) voxel counts of a signed field: the negative values, the finite positive
    ones, and the voxels deep inside that stay +inf"""
    dist, tri = signed_field(tris, leaves, grid, rmax, samples)
    ins = IQ.inside(tris, leaves, GQ.voxel_centres(*grid), samples).reshape(dist.shape)
    hit = tri >= 0
    assert np.array_equal(np.signbit(dist), hit & ins)
    return int((hit & ins).sum()), int((hit & ~ins).sum()), int((~hit & ins).sum())
