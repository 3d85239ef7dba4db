"""The sparse grids without a GPU (psm_grid_sparse_*_dev, include/psm_hip.h "voxel grids: sparse"; grid_sparse.hip; DESIGN.md
4.33): the five entry points and their names, what is refused before any device is touched, the numpy statement of "dense ->
sparse" (tests/sparse_grid_model.py), the closed-at-rmax case of tests/test_gpu_sparse_grid.py by the models, what hipcc makes of
grid_sparse.hip, and that the coarse pass's geometry drops no brick of the dense answer's list."""
import ctypes
import os
import re

import numpy as np
import pytest

import dist_grid_model as DG
import grid_query_model as GQ
import sparse_grid_model as SG
from util import ROOT

F = np.float32
U = np.uint32
HEADER = os.path.join(ROOT, "include", "psm_hip.h")
CSRC = os.path.join(ROOT, "prismarine-core_amd", "csrc")
NAMES = ("psm_grid_sparse_surface_bricks_dev", "psm_grid_sparse_distance_bricks_dev", "psm_grid_sparse_surface_dev",
         "psm_grid_sparse_distance_dev", "psm_grid_sparse_signed_distance_dev")
INVALID = [((0, 0, 0), 1.0, (0, 4, 4)), ((0, 0, 0), 0.0, (4, 4, 4)), ((0, np.nan, 0), 1.0, (4, 4, 4)), ((0, 0, 0), 1.0, (1 << 20, 1 << 20, 8))]
# the cases of tests/test_gpu_sparse_grid.py
SOUP_GRID = ((-3.0, -3.0, -3.0), 0.2, (30, 30, 30))
PLANE_GRID = ((0.0, 0.0, 0.0), 1.0, (4, 4, 12))


def soup():
    rng = np.random.RandomState(41)
    c = rng.uniform(-1, 1, (300, 1, 3))
    return (c + rng.uniform(-0.15, 0.15, (300, 3, 3))).astype(F)


def plane(z):
    return np.array([[[-8, -8, z], [24, -8, z], [-8, 24, z]]], F)


def test_the_header_declares_the_sparse_grids_under_the_grid_prefix(psm):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, code), name
        assert name in psm.EXPORTS and hasattr(psm.lib(), name)
    assert re.search(r"#define PSM_GRID_SPARSE_BRICKS_MAX \(1u << 27\)", code)
    # none is a query of the lifecycle matrix: its count stays what tests/test_query_lifecycle_cpu.py pins
    assert len(re.findall(r"\bint (psm_(?:bvh|scene|instances|world)_\w+_dev)\(", text)) == 64
    section = text[text.index("voxel grids: sparse (new"):text.index("#define PSM_GRID_SPARSE_BRICKS_MAX")]
    for word in ("ascending", "not an atomic append", "padding", "Duplicates are allowed", "PSM_SPARSE_COARSE", "671 613 696", "captured into a"):
        assert word in section, word
    # the two hierarchy sections no longer list the sparse output or the coarse level as missing; the worlds' still do
    hier = text[text.index("voxel grids over a built hierarchy"):text.index("voxel grids: sparse (new")]
    world = text[text.index("voxel grids over a world (new"):]
    assert "a sparse output" not in hier and "a coarse level that culls" not in hier
    assert "a sparse output" in world and "a coarse level that culls" in world
    assert callable(psm.TriangleHierarchy.sparseVoxelize) and callable(psm.TriangleHierarchy.sparseDistanceField)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.hpp")).read()
    for method in ("int sparseVoxelize(", "int sparseDistanceField(", "int sparseSignedDistanceField("):
        assert method in hpp, method


def test_invalid_grids_rmax_and_null_handles_are_refused_without_a_device(psm):
    lib = psm.lib()
    for origin, cell, dims in INVALID:
        with pytest.raises(ValueError):      # (refused before the hierarchy is looked at)
            psm.TriangleHierarchy.sparseVoxelize(None, origin, cell, dims)
        for signed in (False, True):
            with pytest.raises(ValueError):
                psm.TriangleHierarchy.sparseDistanceField(None, origin, cell, dims, 1.0, signed=signed)
    for rmax in (np.nan, -1.0, -np.inf, -1e-30):
        with pytest.raises(ValueError, match="rmax must be >= 0"):
            psm.TriangleHierarchy.sparseDistanceField(None, (0, 0, 0), 1.0, (4, 4, 4), rmax)
    # NULL handles are refused, never dereferenced
    g = psm.Grid()
    g.origin[:], g.cell[:], g.dims[:] = [0, 0, 0], [1, 1, 1], [4, 4, 4]
    r, n, s = ctypes.c_float(1.0), ctypes.c_uint32(1), ctypes.c_uint32(3)
    assert lib.psm_grid_sparse_surface_bricks_dev(None, ctypes.byref(g), n, None, None) == -1
    assert lib.psm_grid_sparse_distance_bricks_dev(None, ctypes.byref(g), r, n, None, None) == -1
    assert lib.psm_grid_sparse_surface_dev(None, ctypes.byref(g), None, n, None) == -1
    assert lib.psm_grid_sparse_distance_dev(None, ctypes.byref(g), r, None, n, None, None) == -1
    assert lib.psm_grid_sparse_signed_distance_dev(None, ctypes.byref(g), r, s, None, n, None, None) == -1


def test_the_model_of_dense_to_sparse():
    """bricked() by its definition against the reshaping form, the lists, the slots of a caller's list, and the Python classes'
    dense() as the inverse"""
    rng = np.random.RandomState(5)
    for dims in ((5, 7, 9), (1, 1, 1), (4, 4, 4), (3, 1, 13)):
        nx, ny, nz = dims
        dense = rng.uniform(-1, 1, (nz, ny, nx)).astype(F)
        slow, fast = SG.bricked(dense, F(np.inf)), SG.bricked_fast(dense, F(np.inf))
        assert slow.shape == (int(np.prod(SG.brick_shape(dims))), 4, 4, 4) and np.array_equal(slow.view(U), fast.view(U))
        nbz, nby, nbx = SG.brick_shape(dims)
        for z, y, x in ((0, 0, 0), (nz - 1, ny - 1, nx - 1), (nz // 2, ny // 2, nx // 2)):
            b = ((z // 4) * nby + y // 4) * nbx + x // 4
            assert slow[b].reshape(64)[(z & 3) * 16 + (y & 3) * 4 + (x & 3)] == dense[z, y, x]
        assert int(np.isposinf(slow).sum()) == 64 * slow.shape[0] - nx * ny * nz
    # a field with three bricks in the band
    dist = np.full((9, 7, 5), np.inf, F)
    tri = np.full((9, 7, 5), -1, np.int32)
    for z, y, x, t in ((0, 0, 0, 4), (8, 6, 4, 9), (4, 3, 1, 2)):
        dist[z, y, x], tri[z, y, x] = 0.5 + t, t
    ids, d, t = SG.distance_list(dist, tri)
    slow_ids, sd, st = SG.distance_list(dist, tri, fast=False)
    assert ids.dtype == U and ids.tolist() == slow_ids.tolist() == [0, 4, 11] and np.array_equal(d.view(U), sd.view(U)) and np.array_equal(t, st)
    assert d.shape == t.shape == (3, 4, 4, 4) and (t >= 0).sum() == 3 and t[0, 0, 0, 0] == 4 and t[2, 0, 2, 0] == 9 and t[1, 0, 3, 1] == 2
    words = np.zeros((3, 2, 2), np.uint64)
    words[0, 1, 0], words[2, 1, 1] = 5, 1 << 63
    wids, w = SG.surface_list(words)
    assert wids.tolist() == [2, 11] and w.tolist() == [5, 1 << 63]
    # a caller's list: any order, duplicates, an id past the grid is an empty brick
    got = SG.slots([11, 0, 0, 12, 2 ** 32 - 1], SG.bricked_fast(tri, np.int32(-1)), -1)
    assert got.shape == (5, 4, 4, 4) and got[0, 0, 2, 0] == 9 and got[1, 0, 0, 0] == got[2, 0, 0, 0] == 4 and (got[3:] == -1).all()
    assert SG.slots([2, 99], words.reshape(-1), 0).tolist() == [5, 0]


def test_the_python_results_go_back_to_dense(psm):
    dims = (5, 7, 9)
    dist = np.full((9, 7, 5), np.inf, F)
    tri = np.full((9, 7, 5), -1, np.int32)
    for z, y, x, t in ((0, 0, 0, 4), (8, 6, 4, 9), (4, 3, 1, 2)):
        dist[z, y, x], tri[z, y, x] = -0.5 - t, t
    ids, d, t = SG.distance_list(dist, tri)
    sparse = psm.SparseDistanceGrid(ids, d, t, dims, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    back = sparse.dense()
    assert isinstance(back, psm.DistanceGrid) and back.dims == dims
    assert np.array_equal(back.dist.view(U), dist.view(U)) and np.array_equal(back.tri, tri) and len(sparse) == 3
    assert sparse.coords().tolist() == [[0, 0, 0], [0, 0, 1], [1, 1, 2]]
    assert psm.SparseDistanceGrid(ids, d, None, dims, (0.0,) * 3, (1.0,) * 3).dense().tri is None
    # an id past the grid and a duplicate change nothing
    more = psm.SparseDistanceGrid(np.concatenate([ids, ids[:1], [U(12)]]).astype(U), np.concatenate([d, d[:1], d[:1]]),
                                  np.concatenate([t, t[:1], t[:1]]), dims, (0.0,) * 3, (1.0,) * 3).dense()
    assert np.array_equal(more.dist.view(U), dist.view(U)) and np.array_equal(more.tri, tri)
    words = np.zeros((3, 2, 2), np.uint64)
    words[0, 1, 0], words[2, 1, 1] = 5, 1 << 63
    wids, w = SG.surface_list(words)
    grid = psm.SparseVoxelGrid(wids, w, dims, (0.0,) * 3, (1.0,) * 3).dense()
    assert isinstance(grid, psm.VoxelGrid) and grid.bricks.dtype == np.uint64 and np.array_equal(grid.bricks, words)


def test_the_closed_at_rmax_case_has_the_shape_the_gpu_test_expects():
    """one large triangle in the plane z = 0 under a 4 x 4 x 12 grid of unit cells: every centre lies over the triangle, at its own
    z. rmax = 4.5 reaches the centres at z = 4.5 exactly -- the lowest layer of brick 1, its 16 voxels of lanes 0 .. 15 -- and
    the float below 4.5 does not. The same triangle in the plane z = 4 lies in the face bricks 0 and 1 share: both list it"""
    leaves = np.arange(1)
    dist, tri = DG.field(plane(0), leaves, PLANE_GRID, 4.5)
    assert np.array_equal(dist[:5, 0, 0], np.array([0.5, 1.5, 2.5, 3.5, 4.5], F))
    ids, d, t = SG.distance_list(dist, tri, fast=False)
    assert ids.tolist() == [0, 1] and (t[0] == 0).all() and np.isfinite(d[0]).all()
    lanes = d[1].reshape(64)
    assert (lanes[:16] == 4.5).all() and np.isposinf(lanes[16:]).all() and (t[1].reshape(64)[:16] == 0).all() and (t[1].reshape(64)[16:] == -1).all()
    below = np.nextafter(F(4.5), F(0))
    assert below < 4.5 and SG.distance_list(*DG.field(plane(0), leaves, PLANE_GRID, below))[0].tolist() == [0]
    wids, words = SG.surface_list(GQ.surface(plane(4), leaves, PLANE_GRID))
    assert wids.tolist() == [0, 1] and words.tolist() == [0xFFFF << 48, 0xFFFF]
    assert SG.surface_list(GQ.surface(plane(0), leaves, PLANE_GRID))[0].tolist() == [0]


def test_the_sparse_kernels_fit_their_launch_bounds_and_fetch_the_tree_as_scalars():
    """what hipcc makes of grid_sparse.hip with the Makefile's flags, as tests/test_dist_grid_cpu.py holds
    grid_dist.hip: nothing spilled, no private segment, no scratch; the wave's stack of QSTACK_MAX links as a walk's only LDS;
    the records, the triangles and the list's ids come through scalar loads, no vector load is left in a walk; plain C++;
    nothing contracted -- every fused instruction belongs to the expansion of a division or a square root"""
    from util import csrc_asm, kernel_asm, kernel_meta
    asm = csrc_asm("grid_sparse.hip")
    walks = {"sparse_coarse_surface": 0, "sparse_coarse_distance": 1, "sparse_any_surface": 0, "sparse_any_distance": 1,
             "sparse_fill_surface": 0, "sparse_fill_distance": 1, "sparse_fill_records": 1}
    others = {"sparse_centres": 0, "sparse_unpack": 0, "sparse_count": 16, "sparse_scan": 33 * 4, "sparse_scatter": 64}
    found = re.findall(r"\.name:\s+_ZN3psm\d+(sparse_[a-z_]+?)E", asm)
    assert sorted(found) == sorted(list(walks) + list(others))
    for kernel in found:
        mangled = re.search(r"\.name:\s+(_ZN3psm\d+%sE\w+)" % kernel, asm).group(1)
        blk, body = kernel_asm(asm, mangled)
        walk = kernel in walks
        assert kernel_meta(blk, "vgpr_count") <= 64, kernel                           # eight waves a SIMD
        assert kernel_meta(blk, "vgpr_spill_count") == 0 and kernel_meta(blk, "sgpr_spill_count") == 0, kernel
        assert kernel_meta(blk, "private_segment_fixed_size") == 0 and "scratch_" not in body, kernel
        assert kernel_meta(blk, "group_segment_fixed_size") == (96 * 4 if walk else others[kernel]), kernel

        def count(op):
            return len(re.findall(r"\b%s\b" % op, body))

        div, root = count("v_div_fmas_f32"), count(r"v_sqrt_f32\w*")
        assert count("v_fma_f32") == 3 * div + 2 * root and count(r"v_fmac_f32\w*") == 2 * div, kernel
        assert (div > 0 and root > 0) if walks.get(kernel) else (div == 0 and root == 0), kernel
        if walk:
            assert "s_load_dwordx8" in body and "global_load" not in body and "flat_load" not in body, kernel
            assert "v_readfirstlane_b32" in body and "ds_write_b32" in body and "ds_read_b32" in body, kernel
        assert "global_store" in body, kernel                                          # ordinary vector stores
    for name in ("grid_sparse.hip", "psm_grid_walk.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert "asm(" not in src and "asm volatile" not in src and "atomic" not in src.replace("No atomics", ""), name
    assert "constexpr int QSTACK_MAX = 96;" in open(os.path.join(CSRC, "psm_query_dev.h")).read()
    # the walks exist once, in the header, and the new file goes through the shared host pieces
    text = open(os.path.join(CSRC, "grid_sparse.hip")).read()
    for piece in ("grid_front(", "grid_built(", "grid_args(", "grid_slabs(", "slabs_for(", "sign_launch(", "grid_for("):
        assert piece in text, piece
    walk_h = open(os.path.join(CSRC, "psm_grid_walk.h")).read()
    assert walk_h.count("PSM_D void grid_walk(") == 1 and walk_h.count("PSM_D void dist_walk(") == 1
    for f in ("grid.hip", "grid_dist.hip", "grid_sparse.hip"):
        t = open(os.path.join(CSRC, f)).read()
        assert "void grid_walk(" not in t and "void dist_walk(" not in t and '#include "psm_grid_walk.h"' in t, f


@pytest.fixture(scope="module")
def dense_cases():
    """(name, triangles, grid, rmax, the dense field's list, the dense surface's list) of the GPU tests' cases, by the models with
    every triangle a leaf -- computed once"""
    cases = []
    lattice = GQ.lattice_soup(31, 500)
    for name, tris, grid, rmax in [("soup", soup(), SOUP_GRID, 0.25), ("plane", plane(0), PLANE_GRID, 4.5), ("plane at 4", plane(4), PLANE_GRID, 0.0)] + \
            [("lattice %d" % k, lattice, g, 0.25) for k, g in enumerate(GQ.LATTICE_GRIDS[:2])]:
        leaves = np.arange(tris.shape[0])
        band = SG.distance_list(*DG.field(tris, leaves, grid, rmax))[0]
        surface = SG.surface_list(GQ.surface(tris, leaves, grid))[0] if name != "soup" else None   # (27 000 boxes by the voxel-by-voxel model: left to the GPU test)
        cases.append((name, tris, grid, rmax, band, surface))
    return cases


def test_the_soup_case_leaves_most_bricks_empty(dense_cases):
    """brick 0 holds centres <= -2.3 and the soup lies >= -1.15: with rmax = 0.25 the outer bricks are empty by arithmetic"""
    name, tris, grid, rmax, band, _ = dense_cases[0]
    assert name == "soup" and tris.min() >= -1.15 and tris.max() <= 1.15
    assert 0 < band.size < 512 and 0 not in band and 511 not in band
    assert SG.brick_shape(grid[2]) == (8, 8, 8)


def test_the_coarse_pass_drops_no_brick_of_the_dense_list(dense_cases):
    """the coarse predicate's geometry in numpy (tests/sparse_grid_model.py: every triangle a leaf, its box its own bounds -- the
    tree's boxes are only larger): every brick the dense answer lists passes it, and it is worth having: it drops bricks"""
    dropped = 0
    for name, tris, grid, rmax, band, surface in dense_cases:
        near = SG.coarse_distance(tris, grid, rmax)
        assert near[band].all(), name
        dropped += int((~near).sum())
        if surface is not None:
            meets = SG.coarse_surface(tris, grid)
            assert meets[surface].all(), name
            dropped += int((~meets).sum())
        # the radius covers rmax and the farthest centre of a brick, 1.5 cells an axis, with room
        cell = np.broadcast_to(np.asarray(grid[1], np.float64).reshape(-1), (3,))
        exact = float(rmax) + 1.5 * float(np.sqrt((cell * cell).sum()))
        R = float(SG.coarse_radius(grid, rmax))
        assert exact < R < exact * 1.002 + 1e-4, (name, exact, R)
    assert dropped > 300
    # the soup's surface through the bounds alone: the bricks whose box meets no triangle's bounds hold no voxel that does
    tris, grid = dense_cases[0][1], dense_cases[0][2]
    meets = SG.coarse_surface(tris, grid)
    lo, hi = SG.brick_boxes(grid)
    assert 0 < meets.sum() < 512 and not meets[0] and (lo[0] == F(-3.0)).all() and np.allclose(hi[0], -2.2) and np.allclose(hi[-1], 3.0)
    assert np.allclose(SG.brick_centres(grid)[0], -2.6)
