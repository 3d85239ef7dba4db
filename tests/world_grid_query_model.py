"""The voxel grids over an instance world (psm_grid_world_surface_dev / _counts_dev / _instances_dev / _solid_dev, include/psm_hip.h
"voxel grids over a world"; world_grid.hip) in numpy. The answers are defined voxel by voxel by the world's box
queries, so the model is world_box_query_model.flat() -- box_tri in float32 over the forward-posed leaves of every instance -- over
grid_query_model.voxel_boxes(), packed with grid_query_model.pack_bricks(); the owner is slot 0 of flat()'s k = 1 instance row.

An instance is world_box_query_model's: (tris [T, 3, 3], cand, pose [3, 4]). grid = (origin, cell, dims).

lattice_world() and exact_counts(): a world where every number lies on the 1/8 lattice -- the triangles of
grid_query_model.lattice_soup(), poses that are signed axis permutations with translations on the lattice, the grids
grid_query_model.LATTICE_GRIDS -- so that every float32 operation of the posing and of box_tri is exact, and a recount in
integers (the 13 separating axes on coordinates scaled by 8, closed) must give the same counts."""
import itertools

import numpy as np

import grid_query_model as GQ
import world_box_query_model as WB

F = np.float32
U = np.uint32


def _shape(dims):
    nx, ny, nz = (int(x) for x in dims)
    return nz, ny, nx


def answers(insts, grid):
    """(dense flags bool, counts uint32, owner int32), each [nz, ny, nx]: flat()'s flag, count and slot 0 of its k = 1 instance row
    for every voxel's box"""
    lo, hi = GQ.voxel_boxes(*grid)
    flag, count, _, irows, _ = WB.flat(insts, lo, hi, 1)
    s = _shape(grid[2])
    return flag.reshape(s), count.astype(U).reshape(s), irows[:, 0].astype(np.int32).reshape(s)


def surface(insts, grid):
    """psm_grid_world_surface_dev: the brick words"""
    return GQ.pack_bricks(answers(insts, grid)[0])


def signed_permutations():
    """the 48 signed axis permutations as float32 3 x 3 matrices: rotations and reflections, all entries 0 or +-1"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            r = np.zeros((3, 3), F)
            for k in range(3):
                r[k, perm[k]] = signs[k]
            out.append(r)
    return out


def lattice_poses(seed, count):
    """`count` poses [3, 4] float32: a signed axis permutation (every second one a reflection) and a translation on the 1/8
    lattice within half a unit; the first is the identity, the last repeats the second (coincident bodies)"""
    rng = np.random.RandomState(seed)
    perms = signed_permutations()
    turns = [[r for r in perms if np.linalg.det(r.astype(np.float64)) > 0], [r for r in perms if np.linalg.det(r.astype(np.float64)) < 0]]
    poses = [np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)]
    while len(poses) < count - 1:
        r = turns[len(poses) & 1][rng.randint(24)]
        t = rng.randint(-4, 5, 3) / 8.0
        poses.append(np.concatenate([r, t.reshape(3, 1)], axis=1).astype(F))
    poses.append(poses[1].copy())
    return poses[:count]


def lattice_world(seed=31, counts=(60, 40), instances=5):
    """(soups, entries): two lattice soups and `instances` entries (soup index, lattice pose), the soups taken in turn; the last
    entry is the second once more, soup and pose: two coincident bodies"""
    soups = [GQ.lattice_soup(seed + k, n) for k, n in enumerate(counts)]
    poses = lattice_poses(seed, instances)
    entries = [(k % len(soups), p) for k, p in enumerate(poses)]
    entries[-1] = (entries[1][0], entries[-1][1])
    return soups, entries


def _int8(x):
    y = np.asarray(x, np.float64) * 8.0
    assert np.array_equal(y, np.round(y)), "not on the 1/8 lattice"
    return y.astype(np.int64)


def _separated(axis, pts, lo, hi):
    """axis [T, 3], pts [T, 3, 3] (the triangle's vertices), lo / hi [V, 3], all int64: [V, T] bool, whether the axis separates
    (strictly: the test is closed)"""
    p = np.einsum("tk,tvk->tv", axis, pts)
    pmin, pmax = p.min(axis=1), p.max(axis=1)
    a, b = axis[None] * lo[:, None], axis[None] * hi[:, None]          # [V, T, 3]
    bmin, bmax = np.minimum(a, b).sum(axis=2), np.maximum(a, b).sum(axis=2)
    return (pmax[None] < bmin) | (pmin[None] > bmax)


def exact_counts(insts, grid):
    """the counts of a lattice world on a lattice grid in integers: uint32 [nz, ny, nx]"""
    lo, hi = GQ.voxel_boxes(*grid)
    lo, hi = _int8(lo), _int8(hi)
    total = np.zeros(lo.shape[0], np.int64)
    for tris, cand, pose in (i[:3] for i in insts):
        t = _int8(np.asarray(tris, F).reshape(-1, 3, 3)[np.sort(np.asarray(cand, np.int64))])
        m = np.asarray(pose, np.float64).reshape(3, 4)
        r, tr = np.round(m[:, :3]).astype(np.int64), _int8(m[:, 3])
        assert np.array_equal(r.astype(np.float64), m[:, :3])
        pts = np.einsum("ij,tvj->tvi", r, t) + tr
        e = [pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 1], pts[:, 0] - pts[:, 2]]
        axes = [np.broadcast_to(np.eye(3, dtype=np.int64)[k], (t.shape[0], 3)) for k in range(3)]
        axes.append(np.cross(e[0], e[1]))
        axes += [np.cross(np.eye(3, dtype=np.int64)[k][None], f) for k in range(3) for f in e]
        sep = np.zeros((lo.shape[0], t.shape[0]), bool)
        for a in axes:
            sep |= _separated(a, pts, lo, hi)
        total += (~sep).sum(axis=1)
    return total.astype(U).reshape(_shape(grid[2]))
