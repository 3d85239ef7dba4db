"""A numpy restatement of the voxel grids (psm_grid_surface_dev / psm_grid_counts_dev / psm_grid_solid_dev, include/psm_hip.h
"voxel grids"; grid.hip): the voxel boxes and centres in float32, the brick words, and the three answers as the box and inside
models give them for every voxel. The yardstick of tests/test_grid_query_cpu.py and tests/test_gpu_grid_query.py."""
import numpy as np

import box_query_model as BQ
import inside_query_model as IQ

F = np.float32


def _axes(origin, cell, dims):
    o = np.asarray(origin, F).reshape(3)
    c = np.broadcast_to(np.asarray(cell, F).reshape(-1), (3,)).astype(F)
    d = [int(x) for x in np.asarray(dims).reshape(3)]
    return o, c, d


def _index(d):
    """ix, iy, iz of every voxel in the dense order (iz * ny + iy) * nx + ix"""
    iz, iy, ix = np.meshgrid(np.arange(d[2]), np.arange(d[1]), np.arange(d[0]), indexing="ij")
    return ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)


def voxel_boxes(origin, cell, dims):
    """(lo, hi) float32 [nz * ny * nx, 3]: lo_k = origin_k + float32(i_k) * cell_k, hi_k = origin_k + float32(i_k + 1) * cell_k,
    each a float32 product and then a float32 sum"""
    o, c, d = _axes(origin, cell, dims)
    idx = _index(d)
    lo, hi = np.empty((idx[0].size, 3), F), np.empty((idx[0].size, 3), F)
    for k in range(3):
        i = idx[k].astype(F)
        prod_lo = (i * c[k]).astype(F)
        prod_hi = ((i + F(1)) * c[k]).astype(F)
        lo[:, k] = (o[k] + prod_lo).astype(F)
        hi[:, k] = (o[k] + prod_hi).astype(F)
    return lo, hi


def voxel_centres(origin, cell, dims):
    """float32 [nz * ny * nx, 3]: c_k = origin_k + (float32(i_k) + 0.5) * cell_k"""
    o, c, d = _axes(origin, cell, dims)
    idx = _index(d)
    out = np.empty((idx[0].size, 3), F)
    for k in range(3):
        half = (idx[k].astype(F) + F(0.5)).astype(F)
        out[:, k] = (o[k] + (half * c[k]).astype(F)).astype(F)
    return out


def pack_bricks(dense):
    """bool [nz, ny, nx] -> uint64 [nbz, nby, nbx]: bit (z & 3) * 16 + (y & 3) * 4 + (x & 3) of brick (x // 4, y // 4, z // 4) is
    voxel (x, y, z); the bits of voxels outside the grid are 0. Written voxel by voxel on purpose."""
    dense = np.asarray(dense, bool)
    nz, ny, nx = dense.shape
    out = np.zeros(((nz + 3) // 4, (ny + 3) // 4, (nx + 3) // 4), np.uint64)
    for z, y, x in zip(*np.nonzero(dense)):
        out[z // 4, y // 4, x // 4] |= np.uint64(1) << np.uint64((z & 3) * 16 + (y & 3) * 4 + (x & 3))
    return out


def unpack_bricks(bricks, dims):
    """uint64 [nbz, nby, nbx] and dims = (nx, ny, nz) -> bool [nz, ny, nx] (the padding bits are not looked at)"""
    nx, ny, nz = (int(x) for x in dims)
    bricks = np.asarray(bricks, np.uint64)
    out = np.zeros((nz, ny, nx), bool)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                j = (z & 3) * 16 + (y & 3) * 4 + (x & 3)
                out[z, y, x] = (int(bricks[z // 4, y // 4, x // 4]) >> j) & 1
    return out


def _shape(dims):
    nx, ny, nz = (int(x) for x in dims)
    return nz, ny, nx


def counts(tris, leaves, grid):
    """psm_grid_counts_dev: uint32 [nz, ny, nx], box_query_model.query's count of every voxel's box. grid = (origin, cell, dims)"""
    lo, hi = voxel_boxes(*grid)
    return BQ.query(tris, leaves, lo, hi, 1)[1].reshape(_shape(grid[2]))


def surface_dense(tris, leaves, grid):
    lo, hi = voxel_boxes(*grid)
    return BQ.query(tris, leaves, lo, hi, 1)[0].reshape(_shape(grid[2]))


def surface(tris, leaves, grid):
    """psm_grid_surface_dev: the brick words of box_query_model.query's flag of every voxel's box"""
    return pack_bricks(surface_dense(tris, leaves, grid))


def shared_face_counts(tris, leaves, grid):
    """How often the closed rule shows: the number of (triangle, pair of voxels sharing a face) where the triangle lies in the
    plane of that face -- its three vertices have the plane's coordinate bit for bit -- and is counted by both voxels."""
    o, c, d = _axes(*grid)
    lo, hi = voxel_boxes(*grid)
    ok, cand = BQ.counts_matrix(tris, leaves, lo, hi)
    ok = ok.reshape(d[2], d[1], d[0], cand.size)
    v = np.asarray(tris, F).reshape(-1, 3, 3)[cand]
    found = 0
    for k in range(3):
        flat = (v[:, 0, k] == v[:, 1, k]) & (v[:, 0, k] == v[:, 2, k])
        for p in range(1, d[k]):
            plane = F(o[k] + F(F(p) * c[k]))
            t = np.nonzero(flat & (v[:, 0, k] == plane))[0]
            if t.size == 0:
                continue
            a = np.take(ok, p - 1, axis=2 - k)[..., t]     # (ok's axes are z, y, x: axis k of the grid is axis 2 - k)
            b = np.take(ok, p, axis=2 - k)[..., t]
            found += int((a & b).sum())
    return found


def lattice_soup(seed, count):
    """test_gpu_box_query.lattice_soup: triangles with vertices on the 1/8 lattice of [-1, 1]^3, each vertex within a step of one
    lattice point; half of them crowd one octant"""
    rng = np.random.RandomState(seed)
    a = rng.randint(-8, 9, (count, 1, 3))
    a[count // 2:] = rng.randint(0, 5, (count - count // 2, 1, 3))
    return (np.clip(a + rng.randint(-1, 2, (count, 3, 3)), -8, 8) / 8.0).astype(F)


# the lattice case's grids: the 8^3 grid of [-1, 1]^3 and the same grid moved by half a cell along one, two and three axes
LATTICE_GRIDS = [((-1.0 + 0.125 * s[0], -1.0 + 0.125 * s[1], -1.0 + 0.125 * s[2]), 0.25, (8, 8, 8))
                 for s in ((0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1))]


def solid_dense(tris, leaves, grid, samples=3):
    ins = IQ.inside(tris, leaves, voxel_centres(*grid), samples).reshape(_shape(grid[2]))
    return surface_dense(tris, leaves, grid) | ins


def solid(tris, leaves, grid, samples=3):
    """psm_grid_solid_dev: surface | inside_query_model.inside(the voxels' centres, samples)"""
    return pack_bricks(solid_dense(tris, leaves, grid, samples))
