"""The distance-field grids without a GPU (psm_grid_distance_dev / psm_grid_signed_distance_dev, include/psm_hip.h "voxel
grids: distance fields"): the two entry points and their names, the grids and the rmax refused before any device
is touched, what hipcc makes of grid_dist.hip, and that the cases of tests/test_gpu_dist_grid.py test what they say they test,
by the model (tests/dist_grid_model.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dist_grid_model as DG
import grid_query_model as GQ
import inside_query_model as IQ
from util import ROOT

F = np.float32
HEADER = os.path.join(ROOT, "include", "psm_hip.h")
NAMES = ("psm_grid_distance_dev", "psm_grid_signed_distance_dev")
INVALID = [((0, 0, 0), 1.0, (0, 4, 4)), ((0, 0, 0), 1.0, (4, 4, (1 << 20) + 1)), ((0, 0, 0), 0.0, (4, 4, 4)),
           ((0, 0, 0), (1.0, -1.0, 1.0), (4, 4, 4)), ((0, 0, 0), np.nan, (4, 4, 4)), ((0, 0, 0), np.inf, (4, 4, 4)),
           ((np.inf, 0, 0), 1.0, (4, 4, 4)), ((0, np.nan, 0), 1.0, (4, 4, 4)), ((0, 0, 3e38), 1e35, (4, 4, 1000)),
           ((0, 0, 0), 1.0, (1 << 20, 1 << 20, 8))]
SPHERE_GRID = ((-1.2, -1.2, -1.2), 0.2, (12, 12, 12))
PARTIAL_GRID = ((-1.2, -1.1, -1.3), (0.5, 0.33, 0.29), (5, 7, 9))


def test_the_header_declares_the_distance_grids_under_the_grid_prefix(psm):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, code), name
        assert name in psm.EXPORTS
        assert hasattr(psm.lib(), name)
    # neither is a query of the lifecycle matrix: its count stays what tests/test_query_lifecycle_cpu.py pins
    assert len(re.findall(r"\bint (psm_(?:bvh|scene|instances|world)_\w+_dev)\(", text)) == 64
    assert callable(psm.TriangleHierarchy.distanceField)
    grid = psm.DistanceGrid("d", "t", (1, 2, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert (grid.dist, grid.tri, grid.dims, grid.origin, grid.cell) == ("d", "t", (1, 2, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for word in ("voxel grids: distance fields", "rmax must be >= 0", "sweeping-based", "graph capture of the signed call"):
        assert word in text, word
    # the hierarchy's grids no longer list the distance field as missing; the world's still do
    hier = text[text.index("voxel grids over a built hierarchy"):text.index("typedef struct {\n    float origin[3];")]
    world = text[text.index("voxel grids over a world"):]
    assert "signed-distance grid" not in hier and "signed-distance grid" in world


def test_invalid_grids_and_rmax_are_refused_without_a_device(psm):
    lib = psm.lib()
    for origin, cell, dims in INVALID:
        for signed in (False, True):
            with pytest.raises(ValueError):      # (refused before the hierarchy is looked at)
                psm.TriangleHierarchy.distanceField(None, origin, cell, dims, signed=signed)
    for rmax in (np.nan, -1.0, -np.inf, -1e-30):
        for signed in (False, True):
            with pytest.raises(ValueError, match="rmax must be >= 0"):
                psm.TriangleHierarchy.distanceField(None, (0, 0, 0), 1.0, (4, 4, 4), rmax=rmax, signed=signed)
    # NULL handles are refused, never dereferenced
    g = psm.Grid()
    g.origin[:], g.cell[:], g.dims[:] = [0, 0, 0], [1, 1, 1], [4, 4, 4]
    assert lib.psm_grid_distance_dev(None, ctypes.byref(g), ctypes.c_float(1.0), None, None) == -1
    assert lib.psm_grid_signed_distance_dev(None, ctypes.byref(g), ctypes.c_float(1.0), ctypes.c_uint32(3), None, None) == -1


def test_the_distance_kernels_fit_their_launch_bounds_and_fetch_the_tree_as_scalars():
    """what hipcc makes of grid_dist.hip with the Makefile's flags: nothing spilled, no private segment, no
    scratch; the wave's stack of QSTACK_MAX links as the walks' only LDS; the record and the triangle come through scalar loads
    (the link is wave-uniform), no vector load is left in the walk; plain C++. Nothing contracted: closest_on_tri divides and
    the walk takes square roots, and hipcc expands a correctly rounded float32 division into three v_fma_f32 and two
    v_fmac_f32 around one v_div_fmas_f32, and a square root into two v_fma_f32 after one v_sqrt_f32 -- every fused
    instruction of a kernel belongs to one of those expansions, none to a product and a sum of the source"""
    from util import csrc_asm, kernel_asm, kernel_meta
    asm = csrc_asm("grid_dist.hip")
    names = {k: re.search(r"\.name:\s+(_ZN3psm\d+%s\w+)" % k, asm).group(1) for k in ("grid_dist_dense", "grid_dist_records", "grid_dist_scatter")}
    for kernel, mangled in names.items():
        blk, body = kernel_asm(asm, mangled)
        walk = kernel != "grid_dist_scatter"
        assert kernel_meta(blk, "vgpr_count") <= 64, kernel                           # eight waves a SIMD
        assert kernel_meta(blk, "vgpr_spill_count") == 0 and kernel_meta(blk, "sgpr_spill_count") == 0, kernel
        assert kernel_meta(blk, "private_segment_fixed_size") == 0 and "scratch_" not in body, kernel
        assert kernel_meta(blk, "group_segment_fixed_size") == (96 * 4 if walk else 0), kernel

        def count(op):
            return len(re.findall(r"\b%s\b" % op, body))

        div, root = count("v_div_fmas_f32"), count(r"v_sqrt_f32\w*")
        assert count("v_fma_f32") == 3 * div + 2 * root and count(r"v_fmac_f32\w*") == 2 * div, kernel
        assert (div > 0 and root > 0) if walk else (div == 0 and root == 0), kernel
        if walk:
            assert "s_load_dwordx8" in body and "global_load" not in body and "flat_load" not in body, kernel
            assert "v_readfirstlane_b32" in body and "ds_write_b32" in body and "ds_read_b32" in body, kernel
            assert "global_store" in body, kernel                                      # ordinary vector stores
    csrc = os.path.join(ROOT, "prismarine-core_amd", "csrc")
    src = open(os.path.join(csrc, "grid_dist.hip")).read()
    assert "asm(" not in src and "asm volatile" not in src
    assert "constexpr int QSTACK_MAX = 96;" in open(os.path.join(csrc, "psm_query_dev.h")).read()


def test_the_lattice_case_has_ties_zeros_and_misses():
    """what tests/test_gpu_dist_grid.py's lattice case asserts on the GPU, by the model (every triangle taken as a leaf): per
    grid 90 to 100 voxels with two or more triangles at the bit-equal smallest d2, 95 to 119 at distance exactly 0, and 12 to 20
    with no triangle within 0.25"""
    tris = GQ.lattice_soup(31, 500)
    ids = np.arange(tris.shape[0])
    for grid in GQ.LATTICE_GRIDS:
        ties, zeros, misses = DG.ties_zeros_misses(tris, ids, grid, 0.25)
        assert 90 <= ties <= 100 and 95 <= zeros <= 119 and 12 <= misses <= 20, (grid, ties, zeros, misses)
    # and in a tie voxel the model's field names the lowest id
    dist, tri = DG.field(tris, ids, GQ.LATTICE_GRIDS[0])
    assert dist.shape == tri.shape == (8, 8, 8) and dist.dtype == F and tri.dtype == np.int32 and (tri >= 0).all()
    near, near_tri = DG.field(tris, ids, GQ.LATTICE_GRIDS[0], 0.25)
    hit = near_tri >= 0
    assert np.array_equal(near[hit].view(np.uint32), dist[hit].view(np.uint32)) and np.isposinf(near[~hit]).all()


def test_the_signed_case_has_all_three_kinds_of_voxel():
    """the signed case's mesh and grids at rmax = 0.3, by the model: (hit and inside, hit and outside, miss and inside) -- the
    negative values, the finite positive ones and the voxels deep inside the sphere that stay +inf with the sign bit clear"""
    tris = IQ.icosphere(2)
    ids = np.arange(tris.shape[0])
    assert DG.signed_kinds(tris, ids, SPHERE_GRID, 0.3, 3) == (320, 608, 160)
    assert DG.signed_kinds(tris, ids, PARTIAL_GRID, 0.3, 3) == (49, 108, 32)
    dist, tri = DG.signed_field(tris, ids, SPHERE_GRID, 0.3, 3)
    deep = (tri < 0) & (np.linalg.norm(GQ.voxel_centres(*SPHERE_GRID).astype(np.float64), axis=1).reshape(dist.shape) < 0.6)
    assert deep.sum() > 100 and (dist[deep].view(np.uint32) == 0x7F800000).all()
