"""A numpy restatement of "dense -> sparse" (include/psm_hip.h "voxel grids: sparse"; grid_sparse.hip): the
sparse grids are defined by the dense calls, so the model takes a dense answer -- VoxelGrid's words, or DistanceGrid's dist and
tri -- and states the list and the slots it implies. Also the geometry of the coarse pass, without the tree: every triangle a
leaf, its box the triangle's own bounds. The yardstick of tests/test_sparse_grid_cpu.py and tests/test_gpu_sparse_grid.py."""
import numpy as np

import grid_query_model as GQ

F = np.float32
U = np.uint32
INF_BITS = 0x7F800000


def brick_shape(dims):
    """(nbz, nby, nbx) of dims = (nx, ny, nz)"""
    nx, ny, nz = (int(x) for x in dims)
    return (nz + 3) // 4, (ny + 3) // 4, (nx + 3) // 4


def bricked(dense, fill):
    """a dense [nz, ny, nx] array as [bricks, 4, 4, 4] in brick order (bz * nby + by) * nbx + bx, axes (z, y, x) within the
    brick -- lane (z & 3) * 16 + (y & 3) * 4 + (x & 3) when flattened --, `fill` in the voxels outside the grid. Written
    voxel by voxel on purpose."""
    dense = np.asarray(dense)
    nz, ny, nx = dense.shape
    nbz, nby, nbx = (nz + 3) // 4, (ny + 3) // 4, (nx + 3) // 4
    out = np.full((nbz * nby * nbx, 4, 4, 4), fill, dense.dtype)
    for z in range(nz):
        for y in range(ny):
            b = ((z // 4) * nby + y // 4) * nbx
            for x in range(nx):
                out[b + x // 4, z & 3, y & 3, x & 3] = dense[z, y, x]
    return out


def bricked_fast(dense, fill):
    """bricked() by reshaping, for the grids of the GPU tests (tests/test_sparse_grid_cpu.py holds the two equal)"""
    dense = np.asarray(dense)
    nz, ny, nx = dense.shape
    nbz, nby, nbx = (nz + 3) // 4, (ny + 3) // 4, (nx + 3) // 4
    pad = np.full((4 * nbz, 4 * nby, 4 * nbx), fill, dense.dtype)
    pad[:nz, :ny, :nx] = dense
    return np.ascontiguousarray(pad.reshape(nbz, 4, nby, 4, nbx, 4).transpose(0, 2, 4, 1, 3, 5)).reshape(-1, 4, 4, 4)


def surface_list(words):
    """(ids uint32 ascending, words uint64) of a dense surface's words [nbz, nby, nbx]: the bricks whose word is non-zero"""
    flat = np.asarray(words, np.uint64).reshape(-1)
    ids = np.nonzero(flat)[0].astype(U)
    return ids, flat[ids]


def distance_list(dist, tri, fast=True):
    """(ids uint32 ascending, dist float32 [n, 4, 4, 4], tri int32 [n, 4, 4, 4]) of a dense field: the bricks with a record, a
    voxel with tri >= 0; the voxels outside the grid hold +inf / -1"""
    make = bricked_fast if fast else bricked
    d, t = make(np.asarray(dist, F), F(np.inf)), make(np.asarray(tri, np.int32), np.int32(-1))
    ids = np.nonzero((t >= 0).any(axis=(1, 2, 3)))[0].astype(U)
    return ids, d[ids], t[ids]


def slots(ids, per_brick, empty):
    """the answers of a caller's list: slot i is per_brick[ids[i]], or `empty` (a scalar) for an id at or above the brick
    count"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    per_brick = np.asarray(per_brick)
    out = np.full((ids.size,) + per_brick.shape[1:], empty, per_brick.dtype)
    ok = ids < per_brick.shape[0]
    out[ok] = per_brick[ids[ok]]
    return out


def _planes(grid):
    """per axis the float32 planes origin + float32(i) * cell, i = 0 .. dims: voxel_boxes' lo and hi"""
    o, c, d = GQ._axes(*grid)
    return [(o[k] + (np.arange(d[k] + 1).astype(F) * c[k]).astype(F)).astype(F) for k in range(3)], o, c, d


def brick_boxes(grid):
    """(lo, hi) float32 [bricks, 3] in brick order: lo of voxel 4 b, hi of the brick's last voxel inside the grid"""
    planes, _, _, d = _planes(grid)
    nbz, nby, nbx = brick_shape(grid[2])
    bz, by, bx = np.meshgrid(np.arange(nbz), np.arange(nby), np.arange(nbx), indexing="ij")
    b = [bx.reshape(-1), by.reshape(-1), bz.reshape(-1)]
    lo = np.stack([planes[k][4 * b[k]] for k in range(3)], axis=1)
    hi = np.stack([planes[k][np.minimum(4 * b[k] + 4, d[k])] for k in range(3)], axis=1)
    return lo, hi


def brick_centres(grid):
    """float32 [bricks, 3]: origin + (float32(4 b) + 2) * cell, the corner of voxel 4 b + 2 with a centre's operations"""
    _, o, c, _ = _planes(grid)
    nbz, nby, nbx = brick_shape(grid[2])
    bz, by, bx = np.meshgrid(np.arange(nbz), np.arange(nby), np.arange(nbx), indexing="ij")
    b = [bx.reshape(-1), by.reshape(-1), bz.reshape(-1)]
    return np.stack([(o[k] + (((4 * b[k]).astype(F) + F(2)).astype(F) * c[k]).astype(F)).astype(F) for k in range(3)], axis=1)


def coarse_radius(grid, rmax):
    """the coarse pass's radius in float32, operation for operation grid_sparse.hip's coarse_bound: R = ((rmax + 1.5 |cell|) +
    2^-18 E) (1 + 2^-10), E the largest of |origin_k| + (dims_k + 4) cell_k"""
    _, o, c, d = _planes(grid)
    with np.errstate(over="ignore", invalid="ignore"):
        off = F(1.5) * np.sqrt(F(F(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), dtype=F)
        E = max(F(abs(o[k]) + F(F(F(d[k]) + F(4)) * c[k])) for k in range(3))
        return F(F(F(F(rmax) + off) + F(E * F(2.0 ** -18))) * F(1 + 2.0 ** -10))


def coarse_surface(tris, grid):
    """bool [bricks]: the brick's box meets the bounds of some triangle (closed) -- what the coarse pass asks with every
    triangle a leaf and no padding: the tree's boxes are only larger"""
    v = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    tlo, thi = v.min(1), v.max(1)
    lo, hi = (x.astype(np.float64) for x in brick_boxes(grid))
    return ((lo[:, None, :] <= thi[None]) & (hi[:, None, :] >= tlo[None])).all(2).any(1)


def coarse_distance(tris, grid, rmax):
    """bool [bricks]: the brick's centre lies within coarse_radius() of the bounds of some triangle"""
    v = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    tlo, thi = v.min(1), v.max(1)
    q = brick_centres(grid).astype(np.float64)
    gap = np.maximum(np.maximum(tlo[None] - q[:, None, :], q[:, None, :] - thi[None]), 0.0)
    R = float(coarse_radius(grid, rmax))
    return (np.sqrt((gap * gap).sum(2)) <= R).any(1)
