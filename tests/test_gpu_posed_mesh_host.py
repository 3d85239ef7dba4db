"""The host path the twelve posed-mesh entry points share, on the GPU (mesh.hip's mesh_upload() and the pieces beside it;
DESIGN.md 4.28). What each entry point answers is held by its own family's tests; here all twelve run alternately on one
context while the pose area and the key area grow under them: 2 poses, then 600, then the 2 again. 600 poses regrow both areas
(each starts at 4 096 B: 85 poses of 48 B, 512 words of 8 B). Every comparison is byte for byte."""
import numpy as np
import pytest

from test_gpu_world_box import _World, _hier
from test_world_box_cpu import _pose, cube, signed_permutations

pytestmark = pytest.mark.gpu

F = np.float32
K = 4
RMAX = 0.5
POSE_AREA, KEY_AREA = 4096, 4096


def lattice_mesh():
    """36 right triangles on the 1/4 lattice of [0, 1.25]^3, legs of 1/4 along two axes that change with the triangle: none is
    degenerate, so the build keeps all"""
    tris = []
    for n, (x, y, z) in enumerate((x, y, z) for x in range(3) for y in range(3) for z in range(4)):
        a = np.array([x, y, z], F) / 2
        e = np.eye(3, dtype=F) / 4
        tris.append([a, a + e[n % 3], a + e[(n + 1) % 3]])
    return np.array(tris, F)


def poses_of(p):
    """p signed permutations with translations on the 1/4 lattice, some through the cubes, some within RMAX, some beyond"""
    perms = signed_permutations()
    return [_pose(perms[i % 48], [((7 * i) % 13 - 4) / 4, ((5 * i) % 11 - 3) / 4, ((3 * i) % 7 - 2) / 4]) for i in range(p)]


def every_entry_point(th, world, other, poses):
    """the twelve calls, a hierarchy's and the world's in turn (a clearance call follows a call of the other family that used
    no key words); {name: [every output as a numpy array]}"""
    out = {}

    def rows(r):
        return [r.tri, r.count] + ([] if r.geom is None else [r.geom])

    def recs(r):
        return [r.buffer] + ([] if r.geom is None else [r.geom])

    out["meshOverlaps"] = [th.meshOverlaps(other, poses)]
    out["clearanceToMesh"] = recs(world.clearanceToMesh(other, poses, RMAX, skip=1))
    out["meshCount"] = [th.meshCount(other, poses)]
    out["closestToMesh"] = recs(world.closestToMesh(other, poses, RMAX, skip=1))
    out["meshClearance"] = recs(th.meshClearance(other, poses, RMAX))
    out["overlapsMesh"] = [world.overlapsMesh(other, poses, skip=1)]
    out["meshTriangles"] = rows(th.meshTriangles(other, poses, K))
    out["withinOfMesh"] = [world.withinOfMesh(other, poses, RMAX, skip=1)]
    out["meshClosest"] = recs(th.meshClosest(other, poses, RMAX))
    out["countOnMesh"] = [world.countOnMesh(other, poses, skip=1)]
    out["meshWithin"] = [th.meshWithin(other, poses, RMAX)]
    out["trianglesOnMesh"] = rows(world.trianglesOnMesh(other, poses, K, skip=1))
    assert len(out) == 12
    return out


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


def test_all_twelve_entry_points_share_the_upload_while_its_areas_grow(psm, ctx):
    otris = lattice_mesh()
    poses = poses_of(600)
    assert 2 * 48 <= POSE_AREA < 600 * 48 and 2 * 8 <= KEY_AREA < 600 * 8   # the small call fits both areas, the large one neither
    with _World(psm, ctx, [cube()], [(0, _pose(np.eye(3), [0, 0, 0])), (0, _pose(np.eye(3), [2, 0, 0]))]) as sc:
        th, world = sc.ths[0], sc.world
        other = _hier(psm, ctx, otris)
        try:
            assert other.info().leaf_count == otris.shape[0] == 36 and th.info().leaf_count == 12
            small, large, again = (every_entry_point(th, world, other, poses[:n]) for n in (2, 600, 2))
        finally:
            other.close()
    for name in small:
        assert len(small[name]) == len(large[name]) == len(again[name]), name
        for first, big, second in zip(small[name], large[name], again[name]):
            assert first.shape[0] == 2 and big.shape[0] == 600 and first.dtype == big.dtype == second.dtype, name
            assert np.array_equal(_bytes(second), _bytes(first)), name
            assert np.array_equal(_bytes(big[:2]), _bytes(first)), name
    assert np.array_equal(large["meshOverlaps"][0], large["meshCount"][0].any(axis=1))
    assert np.array_equal(large["overlapsMesh"][0], large["countOnMesh"][0].any(axis=1))
    # the inputs do what they are there for: poses that meet, poses within RMAX alone, pairs beyond it; instance 1 is left out
    for flags, within, closest in ((large["meshOverlaps"][0], large["meshWithin"][0], large["meshClosest"][0]),
                                   (large["overlapsMesh"][0], large["withinOfMesh"][0], large["closestToMesh"][0])):
        tri = closest.view(np.int32)[..., 3]
        assert flags.any() and (within & ~flags).any() and (~within).any() and (tri >= 0).any() and (tri < 0).any()
    assert (large["closestToMesh"][1] == 0).any() and not (large["closestToMesh"][1] == 1).any()
    assert (large["overlapsMesh"][0] != large["meshOverlaps"][0]).sum() == 0   # (the world without instance 1 is the cube)
