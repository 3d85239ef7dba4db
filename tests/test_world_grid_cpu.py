"""The voxel grids over an instance world without a GPU (psm_grid_world_surface_dev / _counts_dev / _instances_dev / _solid_dev,
include/psm_hip.h "voxel grids over a world"): the model of tests/world_grid_query_model.py against an exact
recount on a lattice world, the four entry points and their names, the grids refused before a world is looked at, and what hipcc
makes of world_grid.hip."""
import ctypes
import os
import re

import numpy as np
import pytest

import grid_query_model as GQ
import world_grid_query_model as WG
from test_grid_query_cpu import INVALID
from util import ROOT

F = np.float32
HEADER = os.path.join(ROOT, "include", "psm_hip.h")
NAMES = ("psm_grid_world_surface_dev", "psm_grid_world_counts_dev", "psm_grid_world_instances_dev", "psm_grid_world_solid_dev")


def _insts():
    soups, entries = WG.lattice_world()
    return [(soups[k], np.arange(soups[k].shape[0]), pose) for k, pose in entries]


def test_the_lattice_world_is_on_the_lattice_and_poses_are_rigid():
    soups, entries = WG.lattice_world()
    assert len(soups) == 2 and len(entries) == 5 and [k for k, _ in entries] == [0, 1, 0, 1, 1]
    for _, pose in entries:
        r = pose[:, :3].astype(np.float64)
        assert np.array_equal(r @ r.T, np.eye(3)) and set(np.abs(r).reshape(-1)) == {0.0, 1.0}
        assert np.array_equal(pose[:, 3] * 8, np.round(pose[:, 3] * 8))
    assert np.array_equal(entries[0][1][:, :3], np.eye(3)) and np.array_equal(entries[4][1], entries[1][1])
    assert any(np.linalg.det(p[:, :3].astype(np.float64)) < 0 for _, p in entries)        # a reflection is among them


@pytest.mark.parametrize("grid", GQ.LATTICE_GRIDS, ids=["unshifted", "x", "yz", "xyz"])
def test_the_model_equals_an_exact_recount_on_the_lattice_world(grid):
    """every float32 operation of the posing and of box_tri is exact here, so the counts are the integers' -- and the three
    answers agree with one another; a triangle posed into a shared voxel face counts on both sides"""
    insts = _insts()
    dense, count, owner = WG.answers(insts, grid)
    assert count.shape == (8, 8, 8) and count.dtype == np.uint32 and owner.dtype == np.int32 and dense.dtype == np.bool_
    assert np.array_equal(count, WG.exact_counts(insts, grid))
    assert np.array_equal(dense, count > 0) and np.array_equal(dense, owner >= 0)
    assert 0 < dense.sum() < 512 and len(np.unique(owner)) > 2 and owner.max() <= 3        # (instance 4 lies on instance 1)
    assert np.array_equal(GQ.unpack_bricks(WG.surface(insts, grid), grid[2]), dense)
    # the owner is the lowest instance that counts alone
    for i in range(len(insts)):
        alone = WG.answers([insts[i]], grid)[1] > 0
        assert not (alone & (owner > i)).any() and (alone | (owner != i)).all()
    # coincident instances: the counts of the pair are twice those of one
    assert np.array_equal(WG.answers([insts[1], insts[4]], grid)[1], 2 * WG.answers([insts[1]], grid)[1])


def test_a_triangle_posed_into_a_shared_face_counts_on_both_sides():
    face = np.array([[[0, 0.05, 0.05], [0, 0.2, 0.05], [0, 0.05, 0.2]]], F)                     # in the plane x = 0 of its own space
    pose = np.array([[0, 1, 0, 0.5], [1, 0, 0, 0.0], [0, 0, -1, 0.25]], F)                  # ... posed into the plane y = 0
    grid = GQ.LATTICE_GRIDS[0]
    _, count, owner = WG.answers([(face, np.arange(1), pose)], grid)
    assert count.sum() == 2 and count[4, 3, 6] == 1 and count[4, 4, 6] == 1 and (owner[count > 0] == 0).all()


def test_the_header_declares_the_world_grid_calls_under_psm_grid_world(psm):
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\(psm_world\*" % name, code), name
        assert name in psm.EXPORTS
        assert hasattr(psm.lib(), name)
    # none of them is a query of the lifecycle matrix: its count stays what tests/test_query_lifecycle_cpu.py pins
    assert len(re.findall(r"\bint (psm_(?:bvh|scene|instances|world)_\w+_dev)\(", text)) == 64
    for method in ("voxelize", "voxelCounts", "voxelInstances"):
        assert callable(getattr(psm.InstanceWorld, method)), method
    for word in ("voxel grids over a world", "psm_world_box_triangles_dev(k = 1)", "graph capture of solid", "the skip of one instance"):
        assert word in text, word
    assert "InstanceWorld have no grids" not in psm.TriangleHierarchy.voxelize.__doc__
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for method in ("voxelize", "voxelizeSolid", "voxelCounts", "voxelInstances"):
        assert "InstanceWorld::%s(" % method in inl, method


def test_invalid_grids_are_refused_before_the_world_is_looked_at(psm):
    lib = psm.lib()
    for origin, cell, dims in INVALID:
        for method in (psm.InstanceWorld.voxelize, psm.InstanceWorld.voxelCounts, psm.InstanceWorld.voxelInstances):
            with pytest.raises(ValueError):
                method(None, origin, cell, dims)
        with pytest.raises(ValueError):
            psm.InstanceWorld.voxelize(None, origin, cell, dims, solid=True)
    # a NULL world is refused, never dereferenced
    g = psm.Grid()
    g.origin[:], g.cell[:], g.dims[:] = [0, 0, 0], [1, 1, 1], [4, 4, 4]
    assert lib.psm_grid_world_surface_dev(None, ctypes.byref(g), None) == -1
    assert lib.psm_grid_world_counts_dev(None, ctypes.byref(g), None) == -1
    assert lib.psm_grid_world_instances_dev(None, ctypes.byref(g), None) == -1
    assert lib.psm_grid_world_solid_dev(None, ctypes.byref(g), ctypes.c_uint32(3), None) == -1


def test_the_world_grid_kernels_fit_their_launch_bounds():
    """what hipcc makes of world_grid.hip with the Makefile's flags: each walk within its launch bound's VGPRs
    (64 lanes x 4 waves per SIMD: 128), nothing spilled, no scratch, the wave's one stack of QSTACK_MAX links as the only LDS,
    nothing contracted, the link made wave-uniform; plain C++"""
    from util import csrc_asm, kernel_asm, kernel_meta
    asm = csrc_asm("world_grid.hip")
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "world_grid.hip")).read()
    bounds = re.findall(r"__launch_bounds__\(QUERY_BLOCK, (\d+)\) void (world_grid_\w+)\(", src)
    assert sorted(k for _, k in bounds) == ["world_grid_counts", "world_grid_instances", "world_grid_surface"]
    found = re.findall(r"\.name:\s+(_ZN3psm\d+(\w+?)ENS_\w+)", asm)
    assert sorted(k for _, k in found) == sorted(k for _, k in bounds)                    # every kernel of the file is a world_grid_*
    for waves, kernel in bounds:
        assert 4 <= int(waves) <= 8, kernel                                            # at most the other world kernels' budget
        mangled = [m for m, k in found if k == kernel][0]
        blk, body = kernel_asm(asm, mangled)
        assert kernel_meta(blk, "vgpr_count") <= 512 // int(waves), kernel
        assert kernel_meta(blk, "vgpr_spill_count") == 0 and kernel_meta(blk, "sgpr_spill_count") == 0, kernel
        assert kernel_meta(blk, "private_segment_fixed_size") == 0, kernel
        assert kernel_meta(blk, "group_segment_fixed_size") == 96 * 4, kernel
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body, kernel             # one rounding per operation
        assert "v_readfirstlane_b32" in body, kernel
    assert "asm(" not in src
