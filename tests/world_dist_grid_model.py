"""A numpy restatement of the distance-field grids over an instance world (psm_grid_world_distance_dev /
psm_grid_world_signed_distance_dev, include/psm_hip.h "voxel grids over a world: distance fields"; world_grid_dist.hip; DESIGN.md
4.31): every voxel is what the flat answer of the world's point queries (world_query_model (a): the smallest d2 over all
instances, on a bit-equal d2 the lexicographically lowest (inst, tri); the parity over all instances) gives for the voxel's
centre. The yardstick of tests/test_world_dist_grid_cpu.py and, for small grids, of tests/test_gpu_world_dist_grid.py; and what
the cases of the GPU test are worth (ties between instances, zeros, misses, the signed kinds).

An instance is world_query_model's: (tris [T, 3, 3], cand, pose [3, 4]). grid = (origin, cell, dims)."""
import numpy as np

import grid_query_model as GQ
import inside_query_model as IQ
import world_query_model as WQ

F = np.float32
U = np.uint32


def _shape(grid):
    nx, ny, nz = (int(x) for x in grid[2])
    return nz, ny, nx


def records(insts, grid, rmax=np.inf):
    """(hits [V, 4] float32, inst [V] int32, per-instance answers): psm_world_closest_point_dev's records of every centre"""
    per = WQ.per_instance_points(insts, GQ.voxel_centres(*grid), rmax)
    hits, inst, _ = WQ.flat_points(per)
    return hits, inst.astype(np.int32), per


def _split(hits, inst, grid):
    s = _shape(grid)
    return hits[:, 2].copy().reshape(s), hits.view(np.int32)[:, 3].copy().reshape(s), np.asarray(inst, np.int32).copy().reshape(s)


def field(insts, grid, rmax=np.inf):
    """(dist float32, tri int32, inst int32), each [nz, ny, nx]: t, tri and the instance of every centre's record"""
    hits, inst, _ = records(insts, grid, rmax)
    return _split(hits, inst, grid)


def inside(insts, grid, samples=3):
    """psm_world_inside_dev of every centre: bool [V], the vote over `samples` rays of the parity summed over all instances"""
    par = WQ.flat_parities(WQ.per_instance_parities(insts, GQ.voxel_centres(*grid), samples))
    return IQ.vote(par, samples)


def signed_field(insts, grid, rmax=np.inf, samples=3):
    """the same with psm_world_signed_distance_dev's t: the sign bit set where there is a record and the centre is inside"""
    hits, inst, _ = records(insts, grid, rmax)
    return _split(WQ.signed(hits, inst, inside(insts, grid, samples)), inst, grid)


def worth(insts, grid, rmax, coincident=()):
    """what a grid tests: (ties, apart, zeros, misses) -- the voxels where two or more INSTANCES hold the bit-equal smallest d2
    (the lowest instance must win there), those of them where two of the tied instances are not a coincident pair (`coincident`:
    pairs (i, j) of instances at one pose over one mesh), the voxels at distance exactly 0, and the voxels with no triangle
    within rmax"""
    per = WQ.per_instance_points(insts, GQ.voxel_centres(*grid), np.inf)
    d2 = np.stack([np.where(h.view(np.int32)[:, 3] >= 0, x, F(np.inf)) for h, _, x in per])   # [instance, V]
    best = d2.min(axis=0)
    tied = (d2 == best[None]) & np.isfinite(best)[None]
    ties = tied.sum(axis=0) >= 2
    merged = tied.copy()
    for i, j in coincident:   # a coincident pair counts as one body
        merged[max(i, j)] &= ~tied[min(i, j)]
    apart = merged.sum(axis=0) >= 2
    hits, _, _ = records(insts, grid, rmax)
    misses = hits.view(np.int32)[:, 3] < 0
    return int(ties.sum()), int(apart.sum()), int((best == 0).sum()), int(misses.sum())


def signed_kinds(insts, grid, rmax, samples=3):
    """(hit and inside, hit and outside, miss and inside) voxel counts of a signed field: the negative values, the finite positive
    ones, and the voxels deep inside a body that stay +inf with the sign bit clear"""
    dist, tri, inst = signed_field(insts, grid, rmax, samples)
    ins = inside(insts, grid, samples).reshape(dist.shape)
    hit = tri >= 0
    assert np.array_equal(hit, inst >= 0) and np.array_equal(np.signbit(dist), hit & ins)
    return int((hit & ins).sum()), int((hit & ~ins).sum()), int((~hit & ins).sum())
