"""The distance-field grids over an instance world without a GPU (psm_grid_world_distance_dev /
psm_grid_world_signed_distance_dev, include/psm_hip.h "voxel grids over a world: distance fields"): the two entry
points and their names, the grids and the rmax refused before any device is touched, what hipcc makes of world_grid_dist.hip, and
that the cases of tests/test_gpu_world_dist_grid.py test what they say they test, by the model (tests/world_dist_grid_model.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import grid_query_model as GQ
import inside_query_model as IQ
import world_dist_grid_model as WD
import world_grid_query_model as WG
from util import ROOT

F = np.float32
HEADER = os.path.join(ROOT, "include", "psm_hip.h")
NAMES = ("psm_grid_world_distance_dev", "psm_grid_world_signed_distance_dev")
INVALID = [((0, 0, 0), 1.0, (0, 4, 4)), ((0, 0, 0), 1.0, (4, 4, (1 << 20) + 1)), ((0, 0, 0), 0.0, (4, 4, 4)),
           ((0, 0, 0), (1.0, -1.0, 1.0), (4, 4, 4)), ((0, 0, 0), np.nan, (4, 4, 4)), ((0, 0, 0), np.inf, (4, 4, 4)),
           ((np.inf, 0, 0), 1.0, (4, 4, 4)), ((0, np.nan, 0), 1.0, (4, 4, 4)), ((0, 0, 3e38), 1e35, (4, 4, 1000)),
           ((0, 0, 0), 1.0, (1 << 20, 1 << 20, 8))]

# the lattice case: what tests/test_gpu_world_dist_grid.py asserts per grid of GQ.LATTICE_GRIDS (zeros, misses at LATTICE_RMAX)
LATTICE_RMAX = 0.25
LATTICE_WORTH = [(127, 42, 60, 139), (125, 34, 50, 139), (110, 39, 61, 151), (118, 35, 52, 153)]

# the signed case: three posed icospheres of radius 0.7, the first two overlapping (centres 0.97 apart), the second a reflection
SIGNED_MESH_LEVEL, SIGNED_RADIUS, SIGNED_RMAX = 1, 0.7, 0.3
SIGNED_POSES = [np.array([[1, 0, 0, -0.5], [0, 1, 0, 0.1], [0, 0, 1, 0.0]], F),
                np.array([[0, -1, 0, 0.4], [-1, 0, 0, -0.2], [0, 0, 1, 0.3]], F),
                np.array([[0, 0, 1, 0.1], [1, 0, 0, 0.2], [0, 1, 0, -1.6]], F)]
SIGNED_GRIDS = [((-1.4, -1.2, -2.4), 0.2, (13, 12, 18)), ((-1.4, -1.1, -2.5), (0.55, 0.33, 0.29), (5, 7, 13))]
SIGNED_KINDS = {1: [(374, 843, 61), (50, 142, 11)], 3: [(374, 843, 61), (50, 142, 11)], 5: [(375, 842, 61), (50, 142, 11)]}


def signed_world():
    """(meshes, entries) of the signed case"""
    return [IQ.icosphere(SIGNED_MESH_LEVEL, SIGNED_RADIUS)], [(0, m) for m in SIGNED_POSES]


def _insts(meshes, entries):
    """world_query_model's instances of a world whose every triangle is a leaf"""
    return [(meshes[k], np.arange(meshes[k].shape[0], dtype=np.int32), m) for k, m in entries]


def test_the_header_declares_the_world_distance_grids_under_the_grid_prefix(psm):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\(psm_world\*" % name, code), name
        assert name in psm.EXPORTS
        assert hasattr(psm.lib(), name)
    # neither is a query of the lifecycle matrix: its count stays what tests/test_query_lifecycle_cpu.py pins
    assert len(re.findall(r"\bint (psm_(?:bvh|scene|instances|world)_\w+_dev)\(", text)) == 64
    assert callable(psm.InstanceWorld.distanceField)
    grid = psm.DistanceGrid("d", "t", (1, 2, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert grid.inst is None and (grid.dist, grid.tri, grid.dims) == ("d", "t", (1, 2, 3))
    assert psm.DistanceGrid("d", "t", (1, 2, 3), (0.0,) * 3, (1.0,) * 3, inst="i").inst == "i"
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for method in ("InstanceWorld::distanceField(", "InstanceWorld::signedDistanceField("):
        assert method in inl, method
    # the sections: the new one after "voxel grids over a world", with its own list of what is missing
    section = text[text.index("voxel grids over a world: distance fields"):]
    assert text.index("voxel grids over a world (new") < text.index("voxel grids over a world: distance fields")
    for word in ("signed-distance grid", "rmax must be >= 0", "the skip of one instance", "a per-voxel rmax", "graph capture of the signed call",
                 "a flat scene or an instanced list"):
        assert word in section[:section.index("int psm_grid_world_distance_dev(")], word
    # the hierarchy's distance fields no longer list a world as missing, nor do the world's grids list the signed-distance grid
    hier = text[text.index("voxel grids: distance fields"):text.index("int psm_grid_distance_dev(")]
    world = text[text.index("voxel grids over a world (new"):text.index("int psm_grid_world_surface_dev(")]
    assert "distance grids over a world" not in hier and "a signed-distance grid;" not in world


def test_invalid_grids_and_rmax_are_refused_without_a_device(psm):
    lib = psm.lib()
    for origin, cell, dims in INVALID:
        for signed in (False, True):
            with pytest.raises(ValueError):      # (refused before the world is looked at)
                psm.InstanceWorld.distanceField(None, origin, cell, dims, signed=signed)
    for rmax in (np.nan, -1.0, -np.inf, -1e-30):
        for signed in (False, True):
            with pytest.raises(ValueError, match="rmax must be >= 0"):
                psm.InstanceWorld.distanceField(None, (0, 0, 0), 1.0, (4, 4, 4), rmax=rmax, signed=signed)
    # NULL handles are refused, never dereferenced
    g = psm.Grid()
    g.origin[:], g.cell[:], g.dims[:] = [0, 0, 0], [1, 1, 1], [4, 4, 4]
    assert lib.psm_grid_world_distance_dev(None, ctypes.byref(g), ctypes.c_float(1.0), None, None, None) == -1
    assert lib.psm_grid_world_signed_distance_dev(None, ctypes.byref(g), ctypes.c_float(1.0), ctypes.c_uint32(3), None, None, None) == -1


def test_the_world_distance_kernels_fit_their_launch_bounds_and_fetch_both_levels_as_scalars():
    """what hipcc makes of world_grid_dist.hip with the Makefile's flags: every kernel of the file is a
    world_grid_dist_*; within the launch bound's VGPRs (64 lanes x 4 waves per SIMD: 128); nothing spilled, no private segment,
    no scratch; the wave's one stack of QSTACK_MAX links as the only LDS; the top-level node, the row, the hierarchy's
    constants, the record and the triangle come through scalar loads (the link is wave-uniform), no vector load is left in the
    walks; plain C++. Nothing contracted: 4.30's rule -- every fused instruction belongs to the expansion of a correctly rounded
    division (three v_fma_f32 and two v_fmac_f32 around one v_div_fmas_f32) or square root (two v_fma_f32 after one v_sqrt_f32),
    none to a product and a sum of the source"""
    from util import csrc_asm, kernel_asm, kernel_meta
    asm = csrc_asm("world_grid_dist.hip")
    csrc = os.path.join(ROOT, "prismarine-core_amd", "csrc")
    src = open(os.path.join(csrc, "world_grid_dist.hip")).read()
    bounds = re.findall(r"__launch_bounds__\(QUERY_BLOCK, (\d+)\) void (world_grid_dist_\w+)\(", src)
    assert sorted(k for _, k in bounds) == ["world_grid_dist_dense", "world_grid_dist_records"]
    found = re.findall(r"\.name:\s+(_ZN3psm\d+(\w+?)ENS_\w+)", asm)
    assert sorted(k for _, k in found) == sorted(k for _, k in bounds)       # every kernel of the file is a world_grid_dist_*
    for waves, kernel in bounds:
        assert int(waves) == 4, kernel
        mangled = [m for m, k in found if k == kernel][0]
        blk, body = kernel_asm(asm, mangled)
        assert kernel_meta(blk, "vgpr_count") <= 128, kernel
        assert kernel_meta(blk, "vgpr_spill_count") == 0 and kernel_meta(blk, "sgpr_spill_count") == 0, kernel
        assert kernel_meta(blk, "private_segment_fixed_size") == 0 and "scratch_" not in body, kernel
        assert kernel_meta(blk, "group_segment_fixed_size") == 96 * 4, kernel

        def count(op):
            return len(re.findall(r"\b%s\b" % op, body))

        div, root = count("v_div_fmas_f32"), count(r"v_sqrt_f32\w*")
        assert div > 0 and root > 0, kernel
        assert count("v_fma_f32") == 3 * div + 2 * root and count(r"v_fmac_f32\w*") == 2 * div, kernel
        assert "s_load_dwordx8" in body and "s_load_dwordx16" in body, kernel       # a record's words, a top-level node
        assert "global_load" not in body and "flat_load" not in body, kernel
        assert "v_readfirstlane_b32" in body and "ds_write_b32" in body and "ds_read_b32" in body, kernel
        assert "global_store" in body, kernel                                        # ordinary vector stores
    assert "asm(" not in src and "asm volatile" not in src
    assert "constexpr int QSTACK_MAX = 96;" in open(os.path.join(csrc, "psm_query_dev.h")).read()
    # the pieces world_grid.hip and this file share are in a header of their own, once
    assert "PSM_D uint32_t uni(" not in src and "PSM_D uint32_t uni(" in open(os.path.join(csrc, "psm_world_uni_dev.h")).read()


def test_the_lattice_case_has_ties_between_instances_zeros_and_misses():
    """what tests/test_gpu_world_dist_grid.py's lattice case asserts on the GPU, by the model (every triangle taken as a leaf): per
    grid at least 100 voxels where two or more instances hold the bit-equal smallest d2, at least 30 of them between bodies that
    are not coincident, at least 50 at distance exactly 0, and at least 100 with no triangle within 0.25; and instance 4, which
    is coincident with instance 1, never wins"""
    soups, entries = WG.lattice_world()
    insts = _insts(soups, entries)
    assert entries[4][0] == entries[1][0] and np.array_equal(entries[4][1], entries[1][1])
    for grid, pinned in zip(GQ.LATTICE_GRIDS, LATTICE_WORTH):
        ties, apart, zeros, misses = worth = WD.worth(insts, grid, LATTICE_RMAX, coincident=[(1, 4)])
        assert ties >= 100 and apart >= 30 and zeros >= 50 and misses >= 100, (grid, worth)
        assert worth == pinned, (grid, worth)
        dist, tri, inst = WD.field(insts, grid)
        assert dist.shape == tri.shape == inst.shape == (8, 8, 8) and dist.dtype == F and tri.dtype == inst.dtype == np.int32
        assert (tri >= 0).all() and (inst >= 0).all() and not (inst == 4).any() and (inst == 1).any()
        assert int((dist == 0).sum()) == zeros
        near, near_tri, near_inst = WD.field(insts, grid, LATTICE_RMAX)
        hit = near_tri >= 0
        assert int((~hit).sum()) == misses and np.array_equal(hit, near_inst >= 0) and np.isposinf(near[~hit]).all()
        assert np.array_equal(near[hit].view(np.uint32), dist[hit].view(np.uint32)) and np.array_equal(near_inst[hit], inst[hit])


def test_the_signed_case_has_all_three_kinds_of_voxel():
    """the signed case's world and grids at rmax = 0.3, by the model: (hit and inside, hit and outside, miss and inside) -- the
    negative values, the finite positive ones and the voxels deep inside a sphere that stay +inf with the sign bit clear; the
    parity is summed over all instances, so the lens two spheres share is outside"""
    insts = _insts(*signed_world())
    assert np.linalg.det(SIGNED_POSES[1][:, :3].astype(np.float64)) < 0
    assert np.linalg.norm((SIGNED_POSES[0][:, 3] - SIGNED_POSES[1][:, 3]).astype(np.float64)) < 2 * SIGNED_RADIUS
    for samples, pinned in SIGNED_KINDS.items():
        for grid, kinds in zip(SIGNED_GRIDS, pinned):
            got = WD.signed_kinds(insts, grid, SIGNED_RMAX, samples)
            if grid is SIGNED_GRIDS[0]:
                assert min(got) >= 30, (samples, got)
            assert got == kinds, (samples, grid, got)
    dist, tri, inst = WD.signed_field(insts, SIGNED_GRIDS[0], SIGNED_RMAX, 3)
    deep = (tri < 0) & WD.inside(insts, SIGNED_GRIDS[0], 3).reshape(dist.shape)
    assert deep.sum() >= 30 and (dist[deep].view(np.uint32) == 0x7F800000).all() and (inst[deep] == -1).all()
    # the lens: inside both of the overlapping spheres, outside by the parity -- a positive distance
    c = GQ.voxel_centres(*SIGNED_GRIDS[0]).astype(np.float64)
    lens = np.logical_and.reduce([np.linalg.norm(c - m[:, 3].astype(np.float64), axis=1) < 0.62 for m in SIGNED_POSES[:2]]).reshape(dist.shape)
    assert lens.sum() >= 5 and not np.signbit(dist[lens]).any()
