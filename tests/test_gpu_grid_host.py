"""What the host pieces the eleven grid entry points share (grid.hip's grid_front / grid_built / slabs_for / grid_slabs; DESIGN.md
4.32) newly have in common on the GPU: the one scratch of a context that solid (17 bytes a voxel) and signed (32 bytes a voxel)
both grow, of a hierarchy and of a world of it. The four grid suites (test_gpu_grid_query.py, test_gpu_dist_grid.py,
test_gpu_world_grid.py, test_gpu_world_dist_grid.py) hold every call's answers, refusals and slab paths each on its own; here one
fresh context takes all eleven in turn, and every answer is compared bit for bit with the point-wise and box-wise queries by
those suites' own helpers."""
import ctypes

import numpy as np
import pytest

import inside_query_model as IQ
import test_gpu_dist_grid as HD
import test_gpu_grid_query as HG
import test_gpu_world_dist_grid as WD
import test_gpu_world_grid as WG
from test_gpu_world_box import _World

pytestmark = pytest.mark.gpu

U = np.uint32
SMALL = ((-1.6, -1.6, -1.6), 0.8, (4, 4, 4))                    # 1 brick
BIG = ((-1.6, -1.6, -1.6), (0.16, 0.16, 3.2 / 36), (20, 20, 36))   # 5 x 5 x 9 = 225 bricks
RMAX = 0.3
# name, rmax?, samples?, outputs
HIERARCHY = {"surface": ("psm_grid_surface_dev", False, False, 1), "counts": ("psm_grid_counts_dev", False, False, 1),
             "solid": ("psm_grid_solid_dev", False, True, 1), "distance": ("psm_grid_distance_dev", True, False, 2),
             "signed": ("psm_grid_signed_distance_dev", True, True, 2)}
WORLD = {"surface": ("psm_grid_world_surface_dev", False, False, 1), "counts": ("psm_grid_world_counts_dev", False, False, 1),
         "instances": ("psm_grid_world_instances_dev", False, False, 1), "solid": ("psm_grid_world_solid_dev", False, True, 1),
         "distance": ("psm_grid_world_distance_dev", True, False, 3), "signed": ("psm_grid_world_signed_distance_dev", True, True, 3)}


class _Refusals:
    """one refusal per call through the C ABI, of a kind that changes from call to call, into a guard buffer that must keep its
    fill: room for the three outputs of the larger grid, so that a call that wrongly ran would stay inside it"""

    def __init__(self, psm, ctx):
        self.psm, self.ctx, self.lib = psm, ctx, psm.lib()
        self.cells = 20 * 20 * 36
        self.h = ctx.buf_alloc(3 * 4 * self.cells + 16)
        ctx.buf_upload(self.h, np.full(3 * self.cells + 4, 0x4D4D4D4D, U))
        self.at = ctx.buf_ptr(self.h)[0]
        self.made = 0

    def refuse(self, handle, entry, grid):
        name, has_rmax, has_samples, outs = entry
        kinds = ["null", "grid", "aligned"] + (["rmax"] if has_rmax else []) + (["samples"] if has_samples else [])
        kind = kinds[self.made % len(kinds)]
        self.made += 1
        g = self.psm._grid(*grid)
        if kind == "grid":
            g.cell[1] = 0.0
        ptrs = [self.at + 4 * self.cells * k for k in range(outs)]
        if kind == "aligned":
            ptrs[-1] += 2
        args = [handle, None if kind == "null" else ctypes.byref(g)]
        if has_rmax:
            args.append(ctypes.c_float(np.nan if kind == "rmax" else RMAX))
        if has_samples:
            args.append(ctypes.c_uint32(2 if kind == "samples" else 3))
        rc = getattr(self.lib, name)(*args, *[ctypes.c_void_p(p) for p in ptrs])
        said = self.lib.psm_last_error(self.ctx._h)
        text = {"null": b": NULL pointer", "grid": b": invalid grid: cell must be finite and > 0", "aligned": b"-byte aligned",
                "rmax": b": rmax must be >= 0", "samples": b": samples must be 1, 3 or 5"}[kind]
        assert rc == -1 and said.startswith(name.encode()) and text in said, (name, kind, rc, said)
        self.ctx.sync()
        assert (self.ctx.buf_download(self.h, U, 3 * self.cells + 4) == 0x4D4D4D4D).all(), (name, kind)

    def close(self):
        self.ctx.buf_free(self.h)


def test_the_eleven_grid_calls_share_one_context_scratch(psm):
    """A context of its own, so that the scratch starts from nothing; an icosphere and a world of two posed copies of it. On a grid
    of 1 brick, then one of 225 bricks, then the first again, every entry point is called in turn, signed before solid: on the
    first grid the scratch is allocated at its smallest (64 bricks' worth), on the second the signed call asks for 2 x 225 = 450
    bricks' worth and the area is freed and grown to 512 while solid's request of 225 then fits, on the third everything runs in
    the grown area. Every answer is, bit for bit, what the box and point queries answer for the voxels' boxes and centres; after
    every step one refused call of each entry point just used leaves a guard buffer untouched."""
    tris = IQ.icosphere(2)
    own = psm.Context(0)
    try:
        with _World(psm, own, [tris], [(0, m) for m in WG.SPHERE_POSES]) as sc:
            th, w = sc.ths[0], sc.world
            guard = _Refusals(psm, own)
            try:
                for grid in (SMALL, BIG, SMALL):
                    dense, _ = HG.check_grid(psm, th, tris, grid, model=False)
                    guard.refuse(th._h, HIERARCHY["surface"], grid)
                    guard.refuse(th._h, HIERARCHY["counts"], grid)
                    HD.check_field(psm, th, tris, grid, rmax=RMAX, model=False)
                    guard.refuse(th._h, HIERARCHY["distance"], grid)
                    dist, _ = HD.check_field(psm, th, tris, grid, rmax=RMAX, signed=True, samples=3, model=False)
                    guard.refuse(th._h, HIERARCHY["signed"], grid)
                    solid = th.voxelize(*grid, solid=True, samples=3).dense()
                    HG._same(solid, HG._solid_expected(psm, th, grid, 3), "solid against surface | inside")
                    guard.refuse(th._h, HIERARCHY["solid"], grid)
                    # (the coarse grid's eight middle voxels all meet the surface; the finer one has an inside to fill)
                    assert grid is SMALL or (dense.sum() < solid.sum() and np.signbit(dist).any() and np.isposinf(dist).any())

                    wdense, _, owner = WG.check_grid(psm, sc, grid, model=False)
                    for call in ("surface", "counts", "instances"):
                        guard.refuse(w._w, WORLD[call], grid)
                    WD.check_field(psm, sc, grid, rmax=RMAX, model=False)
                    guard.refuse(w._w, WORLD["distance"], grid)
                    wdist, _, _ = WD.check_field(psm, sc, grid, rmax=RMAX, signed=True, samples=3, model=False)
                    guard.refuse(w._w, WORLD["signed"], grid)
                    wsolid = w.voxelize(*grid, solid=True, samples=3).dense()
                    WG._same(wsolid, WG._solid_expected(psm, w, grid, 3), "the world's solid against surface | inside")
                    guard.refuse(w._w, WORLD["solid"], grid)
                    assert grid is SMALL or (wdense.sum() < wsolid.sum() and np.signbit(wdist).any() and set(np.unique(owner)) == {-1, 0, 1})
                assert guard.made == 3 * 11
            finally:
                guard.close()
    finally:
        own.close()
