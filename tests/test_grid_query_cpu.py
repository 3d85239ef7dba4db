"""The voxel grids without a GPU (psm_grid_surface_dev / psm_grid_counts_dev / psm_grid_solid_dev, include/psm_hip.h "voxel
grids"): the brick layout and the voxel box as tests/grid_query_model.py states them, the package's statement of
the same box, the four entry points and their names, the grids refused before any device is touched, and that the cases of
tests/test_gpu_grid_query.py test what they say they test, by the model."""
import ctypes
import os
import re

import numpy as np
import pytest

import grid_query_model as GQ
import inside_query_model as IQ
from util import ROOT

F = np.float32
HEADER = os.path.join(ROOT, "include", "psm_hip.h")
NAMES = ("psm_grid_surface_dev", "psm_grid_counts_dev", "psm_grid_solid_dev", "psm_grid_brick_count")
LATTICE = ((-1.0, -1.0, -1.0), 0.25, (8, 8, 8))
AWKWARD = ((0.1, -3.3, 1e3), (0.07, 0.013, 0.3), (5, 7, 9))
INVALID = [((0, 0, 0), 1.0, (0, 4, 4)), ((0, 0, 0), 1.0, (4, 4, (1 << 20) + 1)), ((0, 0, 0), 0.0, (4, 4, 4)),
           ((0, 0, 0), (1.0, -1.0, 1.0), (4, 4, 4)), ((0, 0, 0), np.nan, (4, 4, 4)), ((0, 0, 0), np.inf, (4, 4, 4)),
           ((np.inf, 0, 0), 1.0, (4, 4, 4)), ((0, np.nan, 0), 1.0, (4, 4, 4)), ((0, 0, 3e38), 1e35, (4, 4, 1000)),
           ((0, 0, 0), 1.0, (1 << 20, 1 << 20, 8))]


def test_pack_and_unpack_pin_the_bit_and_the_brick_order():
    """every voxel of a 5 x 7 x 9 grid set alone: one bit of one word, where the header says; the round trip gives it back"""
    nx, ny, nz = dims = (5, 7, 9)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                dense = np.zeros((nz, ny, nx), bool)
                dense[z, y, x] = True
                words = GQ.pack_bricks(dense)
                assert words.shape == (3, 2, 2) and words.dtype == np.uint64
                flat = words.reshape(-1)
                brick = ((z // 4) * 2 + y // 4) * 2 + x // 4
                assert int(flat[brick]) == 1 << ((z & 3) * 16 + (y & 3) * 4 + (x & 3))
                assert np.count_nonzero(flat) == 1
                assert np.array_equal(GQ.unpack_bricks(words, dims), dense)
    full = GQ.pack_bricks(np.ones((nz, ny, nx), bool))
    assert sum(bin(int(w)).count("1") for w in full.reshape(-1)) == nx * ny * nz      # the padding bits are 0
    assert int(full[2, 1, 1]) == 0x111                                               # z = 8, y = 4 .. 6, x = 4: bits 0, 4, 8
    rng = np.random.RandomState(1)
    dense = rng.randint(0, 2, (nz, ny, nx)).astype(bool)
    assert np.array_equal(GQ.unpack_bricks(GQ.pack_bricks(dense), dims), dense)


@pytest.mark.parametrize("grid", [LATTICE, AWKWARD], ids=["lattice", "awkward"])
def test_the_package_states_the_model_s_voxel_box(psm, grid):
    lo, hi = psm.voxel_boxes(*grid)
    mlo, mhi = GQ.voxel_boxes(*grid)
    nx, ny, nz = grid[2]
    assert lo.dtype == hi.dtype == F and lo.shape == hi.shape == (nx * ny * nz, 3)
    assert np.array_equal(lo.view(np.uint32), mlo.view(np.uint32)) and np.array_equal(hi.view(np.uint32), mhi.view(np.uint32))
    assert np.array_equal(psm.voxel_centres(*grid).view(np.uint32), GQ.voxel_centres(*grid).view(np.uint32))
    # the order is (iz * ny + iy) * nx + ix, and hi of voxel i is lo of voxel i + 1 bit for bit on every axis
    lo3, hi3 = lo.reshape(nz, ny, nx, 3).view(np.uint32), hi.reshape(nz, ny, nx, 3).view(np.uint32)
    assert np.array_equal(hi3[:, :, :-1, 0], lo3[:, :, 1:, 0])
    assert np.array_equal(hi3[:, :-1, :, 1], lo3[:, 1:, :, 1])
    assert np.array_equal(hi3[:-1, :, :, 2], lo3[1:, :, :, 2])
    assert (lo < hi).all()
    o = np.asarray(grid[0], F)
    assert np.array_equal(lo[0], o + F(0) * np.broadcast_to(np.asarray(grid[1], F), 3))
    if grid is LATTICE:   # exact arithmetic: the planes are the lattice's
        assert np.array_equal(np.unique(lo[:, 0]), np.arange(8, dtype=F) / 4 - 1) and hi.max() == 1.0


def test_the_header_declares_the_grid_calls_under_their_own_prefix(psm):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, code), name
        assert name in psm.EXPORTS
        assert hasattr(psm.lib(), name)
    # none of them is a query of the lifecycle matrix: its count stays what tests/test_query_lifecycle_cpu.py pins
    assert len(re.findall(r"\bint (psm_(?:bvh|scene|instances|world)_\w+_dev)\(", text)) == 64
    assert re.search(r"typedef struct \{\s*float origin\[3\];.*?float cell\[3\];.*?uint32_t dims\[3\];.*?\} psm_grid;", code, re.S)
    assert ctypes.sizeof(psm.Grid) == 36
    for cls, method in ((psm.TriangleHierarchy, "voxelize"), (psm.TriangleHierarchy, "voxelCounts"), (psm.VoxelGrid, "dense"),
                        (psm.VoxelGrid, "occupied")):
        assert callable(getattr(cls, method))
    for word in ("voxel grids", "not covered", "PSM_GRID_DIM_MAX", "grid query before build", "context-owned scratch"):
        assert word in text, word


def test_invalid_grids_are_refused_without_a_device(psm):
    lib = psm.lib()
    for origin, cell, dims in INVALID:
        with pytest.raises(ValueError):
            psm.voxel_boxes(origin, cell, dims)
        for method in (psm.TriangleHierarchy.voxelize, psm.TriangleHierarchy.voxelCounts):
            with pytest.raises(ValueError):      # (refused before the hierarchy is looked at)
                method(None, origin, cell, dims)
        g = psm.Grid()
        with np.errstate(over="ignore"):
            g.origin[:] = [float(F(x)) for x in origin]
            g.cell[:] = [float(F(x)) for x in np.broadcast_to(np.asarray(cell, np.float64).reshape(-1), 3)]
        g.dims[:] = list(dims)
        assert lib.psm_grid_brick_count(ctypes.byref(g)) == 0, (origin, cell, dims)
    with pytest.raises(ValueError):
        psm.voxel_boxes((0, 0), 1.0, (4, 4, 4))
    with pytest.raises(ValueError):
        psm.voxel_boxes((0, 0, 0), 1.0, (4, 4.5, 4))
    assert lib.psm_grid_brick_count(None) == 0
    for dims, bricks in (((5, 7, 9), 12), ((1, 1, 1), 1), ((4, 4, 4), 1), ((3, 1, 130), 33), ((84, 84, 84), 9261),
                         ((1 << 20, 1 << 14, 4), 1 << 30), ((1 << 20, 1 << 14, 5), 1 << 31)):   # (2^31 bricks: refused)
        g = psm.Grid()
        g.origin[:], g.cell[:], g.dims[:] = [0, 0, 0], [1e-3, 1e-3, 1e-3], list(dims)
        expect = 0 if bricks >= 1 << 31 else bricks
        assert lib.psm_grid_brick_count(ctypes.byref(g)) == expect, dims
    # NULL handles are refused, never dereferenced
    g = psm.Grid()
    g.origin[:], g.cell[:], g.dims[:] = [0, 0, 0], [1, 1, 1], [4, 4, 4]
    assert lib.psm_grid_surface_dev(None, ctypes.byref(g), None) == -1
    assert lib.psm_grid_counts_dev(None, ctypes.byref(g), None) == -1
    assert lib.psm_grid_solid_dev(None, ctypes.byref(g), ctypes.c_uint32(3), None) == -1


def test_voxel_grid_reads_its_bricks_as_the_model_packs_them(psm):
    rng = np.random.RandomState(2)
    for dims in ((5, 7, 9), (1, 1, 1), (4, 4, 4), (3, 1, 130)):
        nx, ny, nz = dims
        dense = rng.randint(0, 2, (nz, ny, nx)).astype(bool)
        vg = psm.VoxelGrid(GQ.pack_bricks(dense), dims, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        assert np.array_equal(vg.dense(), dense) and vg.dense().dtype == np.bool_ and vg.occupied() == int(dense.sum())
    top = np.zeros((4, 4, 4), bool)
    top[3, 3, 3] = True                     # bit 63
    vg = psm.VoxelGrid(GQ.pack_bricks(top), (4, 4, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert int(vg.bricks[0, 0, 0]) == 1 << 63 and np.array_equal(vg.dense(), top) and vg.occupied() == 1


def test_the_grid_kernels_fit_their_launch_bounds_and_fetch_the_tree_as_scalars():
    """what hipcc makes of grid.hip with the Makefile's flags: the two walks within 64 VGPRs, nothing spilled, no
    scratch, the wave's stack of QSTACK_MAX links as their only LDS; the record and the triangle come through scalar loads (the
    link is wave-uniform), no vector load is left in the walk; nothing contracted; plain C++"""
    from util import csrc_asm, kernel_asm, kernel_meta
    asm = csrc_asm("grid.hip")
    names = {k: re.search(r"\.name:\s+(_ZN3psm\d+%s\w+)" % k, asm).group(1) for k in ("grid_surface", "grid_counts", "grid_centres", "grid_fill")}
    for kernel, mangled in names.items():
        blk, body = kernel_asm(asm, mangled)
        assert kernel_meta(blk, "vgpr_count") <= 64, kernel
        assert kernel_meta(blk, "vgpr_spill_count") == 0 and kernel_meta(blk, "sgpr_spill_count") == 0, kernel
        assert kernel_meta(blk, "private_segment_fixed_size") == 0 and "scratch_" not in body, kernel
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body, kernel            # one rounding per operation
        walk = kernel in ("grid_surface", "grid_counts")
        assert kernel_meta(blk, "group_segment_fixed_size") == (96 * 4 if walk else 0), kernel
        if walk:
            assert "s_load_dwordx8" in body and "global_load" not in body and "flat_load" not in body, kernel
            assert "v_readfirstlane_b32" in body and "ds_write_b32" in body and "ds_read_b32" in body, kernel
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "grid.hip")).read()
    assert "asm(" not in src and "asm volatile" not in src
    assert "constexpr int QSTACK_MAX = 96;" in open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "psm_query_dev.h")).read()


def test_the_lattice_case_tests_the_closed_rule():
    """what tests/test_gpu_grid_query.py's lattice case asserts on the GPU, by the model: with this seed a triangle lying in a
    shared voxel face is counted by both voxels, on the unshifted grid (every triangle taken as a leaf)"""
    tris = GQ.lattice_soup(31, 500)
    ids = np.arange(tris.shape[0])
    assert GQ.shared_face_counts(tris, ids, GQ.LATTICE_GRIDS[0]) >= 1
    # and the model's three answers agree with one another on a shifted grid
    grid = GQ.LATTICE_GRIDS[3]
    cnt = GQ.counts(tris, ids, grid)
    assert cnt.shape == (8, 8, 8) and cnt.dtype == np.uint32
    assert np.array_equal(GQ.unpack_bricks(GQ.surface(tris, ids, grid), grid[2]), cnt > 0) and 0 < (cnt > 0).sum() < 512


def test_the_solid_case_fills_a_closed_mesh():
    """the solid case's mesh and grid, by the model: the filled count lies strictly between the surface count and the voxel
    count, and the filled voxels are the surface's and those whose centre is inside the sphere"""
    tris = IQ.icosphere(2)
    ids = np.arange(tris.shape[0])
    grid = ((-1.2, -1.2, -1.2), 0.2, (12, 12, 12))
    surf = GQ.surface_dense(tris, ids, grid)
    filled = GQ.solid_dense(tris, ids, grid, 3)
    assert surf.sum() < filled.sum() < 12 ** 3 and (filled >= surf).all()
    c = GQ.voxel_centres(*grid).astype(np.float64).reshape(12, 12, 12, 3)
    r = np.linalg.norm(c, axis=-1)
    assert filled[r < 0.9].all() and not filled[(r > 1.0 + 0.2 * 3 ** 0.5)].any()
    assert np.array_equal(GQ.unpack_bricks(GQ.solid(tris, ids, grid, 3), grid[2]), filled)
