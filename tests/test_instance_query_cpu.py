"""CPU tests (no GPU) of the instanced scene queries (psm_instances_*_dev, query.hip; InstancedScene): the canonical move and the
combination in numpy (tests/instance_query_model.py) against the scene model and the single-mesh models, the tie cases across
instances, the library's new exports and host-side refusals, the kernels' code generation and the header layer."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import point_query_model as PQ
import query_model as Q
import scene_query_model as SQ
from util import QUERY_VGPRS, check_query_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32
# (a package without the instanced queries has no such name, and this module does not import)
Instance = importlib.import_module("prismarine-core_amd").Instance
INSTANCE_EXPORTS = ("psm_instances_intersect_dev", "psm_instances_occluded_dev", "psm_instances_count_hits_dev",
                    "psm_instances_closest_point_dev", "psm_instances_within_dev", "psm_instances_inside_dev",
                    "psm_instances_signed_distance_dev")


def _soup(seed, n):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + rng.uniform(-0.25, 0.25, (n, 3, 3))).astype(F)


def _insts(parts, poses):
    return [(t, np.arange(t.shape[0]), m) for t, m in zip(parts, poses)]


def _queries(seed, n):
    rng = np.random.RandomState(seed)
    o, d = rng.uniform(-1.2, 1.2, (n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    o[0], d[1], d[2] = [np.nan, 0, 0], 0, [np.inf, 0, 0]
    tmin = rng.uniform(-1, 0.5, n).astype(F)
    tmax = (tmin + rng.uniform(0, 2, n)).astype(F)
    tmin[3], tmax[4] = 2, np.nan
    p = rng.uniform(-1.3, 1.3, (n, 3)).astype(F)
    p[0] = [0, np.inf, 0]
    r = rng.uniform(0, 0.4, n).astype(F)
    r[1:5] = [np.nan, -1, 0, np.inf]
    return o, d, tmin, tmax, p, r


def test_the_move_is_the_stated_operation_order():
    """x'_j = (R[0][j] d.x + R[1][j] d.y) + R[2][j] d.z with d = x - T, in float32, written out once more by hand; the identity
    moves nothing (not even -0 or a denormal), NaN and infinity reach every component"""
    rng = np.random.RandomState(1)
    m = NQ.random_pose(rng, reflect=True)
    x = rng.uniform(-3, 3, (50, 3)).astype(F)
    got = NQ.move(m, x)
    for i in (0, 7, 49):
        d = [F(x[i, k] - m[k, 3]) for k in range(3)]
        for j in range(3):
            assert got[i, j] == F(F(F(m[0, j] * d[0]) + F(m[1, j] * d[1])) + F(m[2, j] * d[2]))
    odd = np.array([[-0.0, 1e-42, 3], [1, -2, 1e30]], F)
    assert np.array_equal(NQ.move(NQ.IDENTITY, odd), odd) and np.array_equal(NQ.rotate(NQ.IDENTITY, odd), odd)
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
        assert not np.isfinite(NQ.move(m, F([bad]))).any()
    # a rigid pose keeps lengths to float32 rounding, and to_world undoes the move
    assert np.allclose(np.linalg.norm(NQ.rotate(m, x), axis=1), np.linalg.norm(x, axis=1), rtol=1e-6)
    assert np.allclose(NQ.to_world(m, NQ.move(m, x)), x, atol=1e-5)


def test_identity_instances_are_the_scene_model():
    tris = np.concatenate([IQ.icosphere(1), _soup(3, 120)])
    parts, _ = SQ.split(tris, (50, 1, 70))
    geoms = [(t, np.arange(t.shape[0])) for t in parts]
    insts = _insts(parts, [NQ.IDENTITY] * len(parts))
    o, d, tmin, tmax, p, r = _queries(11, 900)
    for lo, hi in ((F(0), F(np.inf)), (tmin, tmax)):
        got, exp = NQ.intersect(insts, o, d, lo, hi), SQ.intersect(geoms, o, d, lo, hi)
        for a, b in zip(got, exp):
            assert np.array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b)
        assert np.array_equal(NQ.count(insts, o, d, lo, hi), SQ.count(geoms, o, d, lo, hi))
    for rm in (F(np.inf), r):
        got, exp = NQ.closest_point(insts, p, rm), SQ.closest_point(geoms, p, rm)
        for a, b in zip(got, exp):
            assert np.array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b)
        sd, sdi = NQ.signed_distance(insts, p, rm, 3)
        esd, esdi = SQ.signed_distance(geoms, p, rm, 3)
        assert np.array_equal(sd.view(U), esd.view(U)) and np.array_equal(sdi, esdi)
    assert np.array_equal(NQ.parities(insts, p, 5), SQ.parities(geoms, p, 5))


@pytest.mark.parametrize("sizes,reflect", [((100,), False), ((1, 70), True), ((50, 1, 7, 90, 3, 3, 20), False)], ids=["2", "3", "8"])
def test_a_cut_mesh_under_one_pose_answers_as_the_uncut_mesh_under_it(sizes, reflect):
    """every part gets the SAME seeded rigid pose: each query is moved by the same arithmetic whichever part it meets, so the
    instanced answers are the uncut mesh's for the moved query -- floats by their bits, (inst, tri) by the part's offset, counts
    and votes exactly; the mesh holds duplicated triangles in different parts, so the tie rule is exercised too"""
    tris = np.concatenate([IQ.icosphere(1), _soup(3, 160)])
    tris[150:170] = tris[5:25]
    parts, offs = SQ.split(tris, sizes)
    pose = NQ.random_pose(np.random.RandomState(len(sizes)), reflect)
    insts, all_ids = _insts(parts, [pose] * len(parts)), np.arange(tris.shape[0])
    o, d, tmin, tmax, p, r = _queries(12, 1200)
    mo, md, mp = NQ.move(pose, o), NQ.rotate(pose, d), NQ.move(pose, p)
    for lo, hi in ((F(0), F(np.inf)), (tmin, tmax), (F(-np.inf), F(np.inf))):
        hits, inst, anyh = NQ.intersect(insts, o, d, lo, hi)
        exp, exp_any = Q.query(tris, all_ids, mo, md, lo, hi)
        assert np.array_equal(SQ.merged_ids(hits, inst, offs).view(U), exp.view(U))
        assert np.array_equal(anyh, exp_any) and np.array_equal(inst >= 0, anyh)
        assert np.array_equal(NQ.count(insts, o, d, lo, hi), IQ.count(tris, all_ids, mo, md, lo, hi))
    assert (inst[:3] == -1).all() and (inst >= 0).sum() > 200
    for rm in (F(np.inf), r):
        hits, inst, wi = NQ.closest_point(insts, p, rm)
        exp, exp_wi = PQ.query(tris, all_ids, mp, rm)
        assert np.array_equal(SQ.merged_ids(hits, inst, offs).view(U), exp.view(U)) and np.array_equal(wi, exp_wi)
    # inside: the world rays, each moved -- the uncut mesh counted along the rotated directions
    par = np.array([(IQ.count(tris, all_ids, mp, NQ.rotate(pose, np.broadcast_to(IQ.INSIDE_DIRECTIONS[k], p.shape)), F(0), F(np.inf)) & 1) == 1
                    for k in range(5)])
    assert np.array_equal(NQ.parities(insts, p, 5), par)
    for s in (1, 3, 5):
        assert np.array_equal(NQ.inside(insts, p, s), IQ.vote(par, s))
        sd, sinst = NQ.signed_distance(insts, p, r, s)
        assert np.array_equal(sinst, inst)
        assert np.array_equal(np.signbit(sd[:, 2]), (inst >= 0) & IQ.vote(par, s))


def test_one_hierarchy_at_two_poses_behaves_as_two_bodies():
    """a unit sphere at x = -2 and at x = +2 (the second turned and mirrored): a point inside either is inside, one between them
    is outside and nearest to the nearer body, and a ray along x crosses four surfaces"""
    ball = IQ.icosphere(3)
    turned = NQ.random_pose(np.random.RandomState(4), reflect=True)
    turned[:, 3] = [2, 0, 0]
    left = NQ.IDENTITY.copy()
    left[:, 3] = [-2, 0, 0]
    insts = _insts([ball, ball], [left, turned])
    p = np.array([[-2, 0.1, 0], [2, -0.2, 0.3], [0.3, 0, 0], [-0.4, 0, 0], [5, 5, 5]], F)
    assert list(NQ.inside(insts, p, 3)) == [True, True, False, False, False]
    hits, inst, _ = NQ.closest_point(insts, p)
    assert list(inst) == [0, 1, 1, 0, 1]
    assert abs(hits[2, 2] - 0.7) < 0.01 and abs(hits[3, 2] - 0.6) < 0.01
    sd, _ = NQ.signed_distance(insts, p, np.inf, 3)
    assert list(np.signbit(sd[:, 2])) == [True, True, False, False, False]
    o, d = np.array([[-5, 0.01, 0.02]], F), np.array([[1, 0, 0]], F)
    assert NQ.count(insts, o, d)[0] == 4
    h, i, _ = NQ.intersect(insts, o, d)
    assert i[0] == 0 and abs(h[0, 2] - 2.0) < 0.01
    h, i, _ = NQ.intersect(insts, o, d, F(4.5), F(np.inf))      # the window holds over the whole scene
    assert i[0] == 1 and abs(h[0, 2] - 6.0) < 0.01
    # the object-space record maps to the world point through the winning instance's matrix
    tri = h.view(np.int32)[0, 3]
    world = NQ.to_world(turned, PQ.point_of(ball, np.array([tri]), h[:1, 0], h[:1, 1]))
    assert np.allclose(world, [[1, 0.01, 0.02]], atol=0.02)


def test_ties_across_instances_lowest_inst_then_lowest_tri():
    """the same triangle seen through the same pose by two instances gives bit-equal t and d2: instance 0 wins whatever the ids;
    two poses that differ only by a translation that is exact in float32 tie as well"""
    t = np.array([[[-1, -1, 1], [1, -1, 1], [0, 1, 1]]], F)
    far = _soup(8, 7) + F([0, 0, 5])
    a, b = np.concatenate([far, t]), np.concatenate([t, far[:1], t])
    pose = NQ.random_pose(np.random.RandomState(9))
    o = NQ.to_world(pose, np.array([[0, 0, 0], [0.1, -0.2, 0]])).astype(F)
    d = NQ.to_world(pose, np.array([[0, 0, 1]])).astype(F) - pose[:, 3]
    d = np.repeat(d, 2, 0)
    for parts, tri in (((a, b), 7), ((b, a), 0)):
        insts = _insts(parts, [pose, pose])
        hits, inst, _ = NQ.intersect(insts, o, d)
        assert (inst == 0).all() and (hits.view(np.int32)[:, 3] == tri).all()
        ph, pinst, _ = NQ.closest_point(insts, o)
        assert (pinst == 0).all() and (ph.view(np.int32)[:, 3] == tri).all()
        assert (NQ.count(insts, o, d) >= 3).all()               # the triangle three times (and whatever lies behind)
    # the same hierarchy at the same pose twice: the lower index, counted twice, an even parity
    insts = _insts([a, a], [pose, pose])
    hits, inst, _ = NQ.intersect(insts, o, d)
    one, _ = Q.query(a, np.arange(8), NQ.move(pose, o), NQ.rotate(pose, d))
    assert np.array_equal(hits.view(U), one.view(U)) and (inst == 0).all()
    assert not NQ.inside(_insts([IQ.icosphere(1)] * 2, [pose, pose]), pose[None, :, 3], 3).any()
    # a strictly nearer triangle in a later instance wins
    near = NQ.IDENTITY.copy()
    near[:, 3] = [0, 0, -0.5]
    z = np.zeros((1, 3), F)
    hits, inst, _ = NQ.intersect(_insts([t, t], [NQ.IDENTITY, near]), z, F([[0, 0, 1]]))
    assert inst[0] == 1 and hits[0, 2] == 0.5
    hits, inst, _ = NQ.closest_point(_insts([t, t], [NQ.IDENTITY, near]), z)
    assert inst[0] == 1 and hits[0, 2] == 0.5


def test_library_exports_the_instanced_queries(psm):
    lib = psm.lib()
    for s in INSTANCE_EXPORTS:
        assert hasattr(lib, s) and s in psm.EXPORTS
    for m in ("intersect", "occluded", "countHits", "closestPoint", "within", "inside", "signedDistance", "setTransform", "transforms"):
        assert callable(getattr(psm.InstancedScene, m))
    assert ctypes.sizeof(psm.Instance) == 8 + 48 and psm.Instance is Instance
    hdr = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    assert "float world_from_object[12];" in hdr and "} psm_instance;" in hdr
    for s in INSTANCE_EXPORTS:
        assert re.search(r"^int %s\(const psm_instance\* insts, uint32_t count," % s, hdr, re.M), s


def test_instanced_scene_refuses_bad_lists_and_poses(psm):
    eye = np.eye(4, dtype=F)
    for n in (0, psm.SCENE_MAX_GEOMETRIES + 1):
        with pytest.raises(ValueError, match="1 .. 32"):
            psm.InstancedScene(None, [(None, eye)] * n)
    scaled, sheared, nan, row = eye.copy(), eye.copy(), eye.copy(), eye.copy()
    scaled[:3, :3] *= F(1.001)
    sheared[0, 1] = 1e-3
    nan[1, 3] = np.nan
    row[3, 0] = 0.5
    for bad in (scaled, sheared, nan, row, scaled[:3], np.eye(3), np.zeros(12), np.full((3, 4), np.inf), 1.0):
        with pytest.raises(ValueError, match="transform"):
            psm.InstancedScene(None, [(None, eye), (None, bad)])
    mirror = np.diag([1, -1, 1, 1]).astype(F)
    turn = np.concatenate([NQ.random_pose(np.random.RandomState(0)), [[0, 0, 0, 1]]]).astype(np.float64)
    sc = psm.InstancedScene(None, [(None, eye), (None, mirror[:3]), (None, turn)])
    assert sc.transforms().shape == (3, 3, 4) and sc.transforms().dtype == F
    assert np.array_equal(sc.transforms()[2], turn[:3].astype(F))
    sc.setTransform(0, turn[:3])
    sc.setTransform(-1, eye)
    assert np.array_equal(sc.transforms()[0], turn[:3].astype(F)) and np.array_equal(sc.transforms()[2], eye[:3])
    for bad in (scaled, nan):
        with pytest.raises(ValueError):
            sc.setTransform(1, bad)
    with pytest.raises(IndexError):
        sc.setTransform(3, eye)
    assert np.array_equal(sc.transforms()[1], mirror[:3])
    got = sc.transforms()
    got[:] = 0                                  # a copy: the scene's poses are its own
    assert sc.transforms().any()


def test_instanced_queries_refuse_bad_lists_without_a_device(psm):
    """what is refused before any context or device is looked at: a NULL list, a count of 0 or 33, a list whose hierarchies are
    all NULL -- whatever the matrices (rigid, scaled, sheared, with a NaN), n and the data pointers are"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    scaled, sheared, nan = list(eye), list(eye), list(eye)
    scaled[0] = 2.0
    sheared[1] = 0.5
    nan[7] = float("nan")
    u32, three = ctypes.c_uint32, ctypes.c_uint32(3)
    for mat in (eye, scaled, sheared, nan):
        lists = (psm.Instance * 33)()
        for k in range(33):
            lists[k].bvh = None
            lists[k].world_from_object[:] = mat
        for n in (ctypes.c_size_t(1), ctypes.c_size_t(0)):
            for lst, count in ((None, 1), (lists, 0), (lists, 33), (lists, 1), (lists, 2), (lists, 32)):
                for d_in, d_out in ((p, p), (None, None)):
                    assert lib.psm_instances_intersect_dev(lst, u32(count), d_in, n, d_out, d_out) == -1
                    assert lib.psm_instances_closest_point_dev(lst, u32(count), d_in, n, d_out, d_out) == -1
                    assert lib.psm_instances_signed_distance_dev(lst, u32(count), d_in, n, three, d_out, d_out) == -1
                    assert lib.psm_instances_inside_dev(lst, u32(count), d_in, n, three, d_out) == -1
                    for fn in (lib.psm_instances_occluded_dev, lib.psm_instances_within_dev, lib.psm_instances_count_hits_dev):
                        assert fn(lst, u32(count), d_in, n, d_out) == -1


def test_instanced_query_kernels_codegen():
    """the seven instanced kernels, and the fourteen existing kernels still at their ceilings: sharing the walk with the
    instanced kernels must not move the scene kernels"""
    assert len(QUERY_VGPRS) == 21
    check_query_kernels(QUERY_VGPRS)


def test_instanced_query_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "instance_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "instance_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    # its main() holds the glm::mat4 -> row-major 3 x 4 copy and the last-row check to known matrices (no device is touched)
    assert subprocess.call([exe]) == 0


BAKED_CASES = [(0, 2), (1, 3), (2, 8)]   # (seed, parts) of the instanced-against-baked comparison (tests/test_gpu_instance_query.py)


@pytest.mark.parametrize("seed,parts", BAKED_CASES)
def test_baked_comparison_seeds_leave_out_at_most_one_percent(seed, parts):
    """the seeds of the GPU suite's instanced-against-baked comparison, judged by the CPU models alone: the threshold is 8 x the
    largest float32 / float64 deviation of the model on these very inputs (two independent float32 roundings meet), and at most
    1 % of the rays and of the points have a decision margin at or below it; enough queries hit for the comparison to mean
    something"""
    pieces, poses, rays, pts = NQ.baked_case(seed, parts)
    assert len(pieces) == parts
    insts = _insts(pieces, poses)
    margin, dev = NQ.ray_margin_and_deviation(insts, *rays)
    print("rays: deviation %.3g, threshold %.3g, left out %.4f" % (dev, 8 * dev, (margin <= 8 * dev).mean()))
    assert 0 < dev < 1e-4 and (margin <= 8 * dev).mean() <= 0.01
    assert (NQ.intersect(insts, *rays)[1] >= 0).mean() > 0.1
    margin, dev = NQ.point_margin_and_deviation(insts, *pts)
    print("points: deviation %.3g, threshold %.3g, left out %.4f" % (dev, 8 * dev, (margin <= 8 * dev).mean()))
    assert 0 < dev < 1e-4 and (margin <= 8 * dev).mean() <= 0.01
    within = NQ.closest_point(insts, *pts)[2].mean()
    assert 0.2 < within < 0.8
