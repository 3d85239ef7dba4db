"""Every query on hierarchies that were rebuilt, shrunk and refitted ("Queries over a hierarchy's life"). The other
query test files ask a handle in its first state: allocated to its triangle count, built once by plain launches, no larger
earlier tree behind it. Here one handle, allocated once for 3 001 triangles, lives through the states of STATES in that order
(tests/query_lifecycle.py has the query matrix: all 64 exported queries) and at every state must be indistinguishable from its
fresh twin -- a handle allocated to the count and built once from the same triangles and matrix, the configuration the other
files hold to the models: the same info() (leaf count, root, transform bit for bit), the same leaf list, the same node records
over the 2 (leaves - 1) uint4 in use -- the build has one writer per word and the sort is stable, so node numbering does not
depend on history and the records are compared as they are, without util.canonical_nodes --, the same lone-leaf word, and the
same bytes in every output buffer of every query. Every comparison is exact.

Four walks, each over its own handle: the 25 queries of one hierarchy; the six mesh queries with the lived handle as `other`; the
lists and the world that hold it (a world must refuse between a rebuild and psm_world_set_instances, and leave the outputs alone);
and a handle under which the context's sort falls back from the hybrid to the eight passes and stays there. In the un-built
window after every reload -- an earlier, often larger, tree still complete in memory -- and after psm_bvh_stage_bounds alone every
entry point must return PSM_ERR_STATE and write nothing.

Against the models as well as the twin, from `deep` on (two handles that are wrong alike would pass the twin): the ray queries
(test_gpu_query._check: intersect, occluded; test_gpu_inside_query._check_count: countHits), the point queries
(test_gpu_point_query._check: closestPoint, within; test_gpu_inside_query._check_points: inside, signedDistance), the k-best
queries (test_gpu_kbest_query.check_rays / check_points), the box, sweep, triangle and clearance queries (check_boxes,
check_sweeps, check_tris, check_clearance) and the mesh queries and mesh clearance (test_gpu_mesh_query.check_mesh,
test_gpu_mesh_dist.check: against the numpy models up to 64 triangles, against triCount / triTriangles / triClosest of the posed
triangles -- themselves held to their models here -- above). By the twin alone: the scene, instanced and world forms (their
checkers take the containers of their own files, not a list or a world made here); the world over the twin is the one their
files hold to the flat models."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

try:   # (imported before the library loads its HIP runtime, as tests/test_gpu_query.py)
    import torch
except ImportError:
    torch = None

import inside_query_model as IQ
import instance_query_model as NQ
import query_lifecycle as QL
import query_model as Q
from test_gpu_box_query import check_boxes
from test_gpu_inside_query import _check_count as check_count
from test_gpu_inside_query import _check_points as check_inside
from test_gpu_kbest_query import check_points as check_nearest
from test_gpu_kbest_query import check_rays as check_first_hits
from test_gpu_mesh_dist import check as check_mesh_dist
from test_gpu_mesh_query import check_mesh
from test_gpu_point_query import ROT_SCALE, SHEAR, _hier
from test_gpu_point_query import _check as check_points
from test_gpu_query import _check as check_rays
from test_gpu_sweep_query import check_sweeps
from test_gpu_tri_dist_query import check_clearance
from test_gpu_tri_query import check_tris
from test_gpu_world_box import _soup
from util import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
KS = (4, 16)
TRI = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)   # the tiny fixtures of test_point_query_tiny_hierarchies
POINT = np.repeat(TRI[:, :1], 3, axis=1)                    # three equal vertices: the build keeps no leaf
STATES = ["fresh", "replayed", "matrix_by_replay_shear", "matrix_by_replay", "deep", "two_leaves", "lone_leaf", "no_leaves",
          "regrown_plain", "regrown_replayed", "refit", "rebuilt_after_refit"]
LEAVES = {"two_leaves": 2, "lone_leaf": 1, "no_leaves": 0, "regrown_plain": 32, "regrown_replayed": 32, "refit": 32,
          "rebuilt_after_refit": 32}
MODELLED = STATES[STATES.index("deep"):]

# a state of the life: its triangles and build matrix; refit_of: the triangles the tree was built from when the state is a refit
State = namedtuple("State", "name tris opt refit_of")


def _moved_cornell(cornell):
    """Cornell with 8 triangles shrunk about their centres and one collapsed to a segment (two equal vertices: it keeps its leaf)"""
    moved = cornell.copy()
    k = np.random.RandomState(9).choice(cornell.shape[0], 9, replace=False)
    c = moved[k[:8]].mean(axis=1, keepdims=True)
    moved[k[:8]] = (c + (moved[k[:8]] - c) * F(0.5)).astype(F)
    moved[k[8], 1] = moved[k[8], 0]
    return moved


def walk(scenes, th, window=lambda what: None):
    """Takes th through STATES, yielding a State at each. window(what) is called wherever th is not built: after every clear and
    reload, and once more after psm_bvh_stage_bounds has run alone (not before the refit, which that stage would forbid)."""
    def reload(tris, stage=True):
        th.clearTribuffer()
        th.loadTriangles(tris.reshape(-1, 9))
        window("reloaded")
        if stage:
            th.stage("bounds")
            window("bounds staged")

    def rebuild(times, opt=None):
        for _ in range(times):
            th.markDirty()
            th.build(opt)

    sponza = np.ascontiguousarray(scenes.sponza_like(3001)["tris"], F).reshape(-1, 3, 3)
    cornell = np.ascontiguousarray(scenes.cornell()["tris"], F).reshape(-1, 3, 3)
    assert sponza.shape[0] == 3001 and cornell.shape[0] == 32
    th.allocate(3001)                      # once: every later state lives in this allocation
    th.loadTriangles(sponza.reshape(-1, 9))
    th.build()                             # the first build of a count: plain launches
    yield State("fresh", sponza, None, None)
    rebuild(3)                             # capture, replay, replay
    yield State("replayed", sponza, None, None)
    rebuild(1, SHEAR)                      # replays: only the matrix moves
    yield State("matrix_by_replay_shear", sponza, SHEAR, None)
    rebuild(1, ROT_SCALE)
    yield State("matrix_by_replay", sponza, ROT_SCALE, None)
    deep = Q.deep_fixture()[0]
    reload(deep)
    rebuild(3)
    yield State("deep", deep, None, None)
    two = np.concatenate([TRI, POINT, TRI + F([0.5, 0, 0])])
    reload(two)
    rebuild(2)
    yield State("two_leaves", two, None, None)
    lone = np.concatenate([POINT, TRI, POINT])
    reload(lone)
    rebuild(2)                             # SM_ROOT back to -1, sorted_tri[0] rewritten, straight after the deep fixture's tree
    yield State("lone_leaf", lone, None, None)
    none = np.concatenate([POINT] * 4)
    reload(none)
    rebuild(1)
    yield State("no_leaves", none, None, None)
    th.setBuildGraph(False)
    reload(cornell)
    rebuild(1)
    th.setBuildGraph(True)
    yield State("regrown_plain", cornell, None, None)
    rebuild(3)                             # a new graph, for a count the handle has never replayed
    yield State("regrown_replayed", cornell, None, None)
    moved = _moved_cornell(cornell)
    reload(moved, stage=False)
    th.refit()
    yield State("refit", moved, None, cornell)
    rebuild(1)                             # a replay over the refitted boxes
    yield State("rebuilt_after_refit", moved, None, None)


def twin_of(psm, ctx, st):
    """the fresh twin of a state: allocated to the count, built once (a refit: built once from the original, refitted the same way)"""
    if st.refit_of is None:
        return _hier(psm, ctx, st.tris, st.opt)
    tw = _hier(psm, ctx, st.refit_of)
    tw.clearTribuffer()
    tw.loadTriangles(st.tris.reshape(-1, 9))
    tw.refit()
    return tw


def same_tree(psm, life, twin, name):
    """info(), the leaf list, the node records in use and the leaf-order triangle words of the two handles are equal; returns info()"""
    a, b = life.info(), twin.info()
    assert (a.triangle_count, a.leaf_count, a.root) == (b.triangle_count, b.leaf_count, b.root), name
    assert bytes(a.transform) == bytes(b.transform), (name, list(a.transform), list(b.transform))
    assert bytes(a.bounds_min) == bytes(b.bounds_min) and bytes(a.bounds_max) == bytes(b.bounds_max), name
    n = a.leaf_count
    if name in LEAVES:
        assert n == LEAVES[name], (name, n)
    if n < 2:
        assert a.root == -1, (name, a.root)
    assert np.array_equal(life.download(psm.BVH_LEAF_TRI, np.int32, n), twin.download(psm.BVH_LEAF_TRI, np.int32, n)), name
    words = 8 * max(n - 1, 0)              # 2 (leaves - 1) uint4: one 32-byte record per internal node
    assert np.array_equal(life.download(psm.BVH_NODE32, np.uint32, words), twin.download(psm.BVH_NODE32, np.uint32, words)), name
    assert np.array_equal(life.download(psm.BVH_SORTED_TRI, np.int32, n), twin.download(psm.BVH_SORTED_TRI, np.int32, n)), name
    return a


def same_answers(got, want, names, what):
    assert len(got) == names and set(got) == set(want), (what, len(got), sorted(set(got) ^ set(want)))
    assert QL.differing(got, want) == [], what


def refused_unbuilt(psm, ctx, rows, first, other, what):
    """every row's entry point returns PSM_ERR_STATE with a `before build` message and leaves its outputs as they were"""
    for row in rows:
        rc, msg, untouched = QL.raw_call(psm, ctx, row, first, other)
        assert rc == QL.ERR_STATE and "before build" in msg, (what, row.export, rc, msg)
        assert untouched, (what, row.export, "wrote to its outputs")


def held_to_the_models(psm, th, tris, seed, aux, aux_tris):
    """the families' own checkers on th over the batches answers() ran (the same seed)"""
    r, p, b, s = QL.gen_rays(tris, seed), QL.gen_points(tris, seed), QL.gen_boxes(tris, seed), QL.gen_sweeps(tris, seed)
    q, qd, m = QL.gen_tris(tris, seed), QL.gen_tri_dist(tris, seed), QL.gen_mesh(tris, seed)
    check_rays(psm, th, tris, r["o"], r["d"], r["tmin"], r["tmax"])
    check_count(psm, th, tris, r["o"], r["d"], r["tmin"], r["tmax"])
    check_first_hits(psm, th, tris, r["o"], r["d"], KS, r["tmin"], r["tmax"])
    check_points(psm, th, tris, p["p"], p["r"])
    check_inside(psm, th, tris, p["p"], p["r"], samples=(3,))
    check_nearest(psm, th, tris, p["p"], KS, p["r"])
    check_boxes(psm, th, tris, b["lo"], b["hi"], KS)
    check_sweeps(psm, th, tris, s["o"], s["d"], s["r"], s["tmax"])
    check_tris(psm, th, tris, q["q"], KS)
    check_clearance(psm, th, tris, qd["q"], qd["r"])
    small = tris.shape[0] <= 64
    check_mesh(psm, th, tris, aux, aux_tris, list(m["poses"]), KS, model=small)
    for rmax in (np.inf, m["r"]):
        check_mesh_dist(psm, th, tris, aux, aux_tris, list(m["poses"]), rmax, model=small)


def test_single_hierarchy_queries_over_a_life(psm, ctx, scenes, oracle):
    aux_tris = IQ.icosphere(1, 1.0)        # the mesh queries' other hierarchy: fixed
    aux = _hier(psm, ctx, aux_tris)
    life = psm.TriangleHierarchy(ctx)
    rows = QL.rows_of("TriangleHierarchy")
    names = sum(len(r.variants) for r in rows)
    reached, windows, transforms = [], [], []
    try:
        def window(what):
            refused_unbuilt(psm, ctx, rows, [life._h], aux, (reached[-1], what))
            windows.append(what)

        for seed, st in enumerate(walk(scenes, life, window)):
            twin = twin_of(psm, ctx, st)
            try:
                info = same_tree(psm, life, twin, st.name)
                if st.name not in LEAVES:      # (the build drops what is smaller than 1e-5 of the fitted bounds: 992 of deep's 1 344)
                    assert info.leaf_count == oracle.build_scene(st.tris, st.opt)["count"], st.name
                got = QL.run(life, st.tris, 100 + seed, other=aux)
                same_answers(QL.bytes_of(got), QL.answers(twin, st.tris, 100 + seed, other=aux), names, st.name)
                if st.name == "no_leaves":
                    for name, (row, res) in got.items():
                        assert QL.is_miss(row, res), name
                else:
                    assert not all(QL.is_miss(row, res) for row, res in got.values()), st.name
                if st.name in MODELLED:
                    held_to_the_models(psm, life, st.tris, 100 + seed, aux, aux_tris)
                reached.append(st.name)
                transforms.append(bytes(info.transform))
                print("state %s: %d triangles, %d leaves, root %d, transform row 0 %s" % (st.name, info.triangle_count, info.leaf_count,
                                                                                        info.root, list(info.transform)[:4]))
            finally:
                twin.close()
        assert reached == STATES
        assert len({transforms[k] for k in (1, 2, 3)}) == 3      # replayed, shear, rotate-scale: the matrix moved each time
        assert windows == ["reloaded", "bounds staged"] * 5 + ["reloaded"]
    finally:
        life.close()
        aux.close()


def test_mesh_queries_with_a_lived_other(psm, ctx, scenes):
    """the lane mapping goes by other's leaf list, which must not keep rows of a larger earlier build"""
    ico_tris = IQ.icosphere(1, 1.0)        # the queried hierarchy: fixed
    ico = _hier(psm, ctx, ico_tris)
    life = psm.TriangleHierarchy(ctx)
    rows = [r for r in QL.rows_of("TriangleHierarchy") if r.gen == "mesh"]
    names = sum(len(r.variants) for r in rows)
    reached = []
    try:
        def window(what):
            refused_unbuilt(psm, ctx, rows, [ico._h], life, (reached[-1], what))

        for seed, st in enumerate(walk(scenes, life, window)):
            twin = twin_of(psm, ctx, st)
            try:
                same_tree(psm, life, twin, st.name)
                kw = dict(only=("mesh",), into_origin=True)
                got = QL.run(ico, st.tris, 200 + seed, other=life, **kw)
                assert len(rows) == 6 and len(got) == names
                same_answers(QL.bytes_of(got), QL.answers(ico, st.tris, 200 + seed, other=twin, **kw), names, st.name)
                if st.name == "no_leaves":
                    for name, (row, res) in got.items():
                        assert QL.is_miss(row, res), name
                else:
                    assert (got["psm_bvh_mesh_closest_dev rmax=inf"][1].tri >= 0).sum() == 4 * life.info().leaf_count
                if st.name in MODELLED:
                    m = QL.gen_mesh(st.tris, 200 + seed, into_origin=True)
                    small = st.tris.shape[0] <= 64
                    check_mesh(psm, ico, ico_tris, life, st.tris, list(m["poses"]), KS, model=small)
                    for rmax in (np.inf, m["r"]):
                        check_mesh_dist(psm, ico, ico_tris, life, st.tris, list(m["poses"]), rmax, model=small)
                reached.append(st.name)
            finally:
                twin.close()
        assert reached == STATES
    finally:
        life.close()
        ico.close()


def _refuses(psm, obj, rows, batches, other, match):
    """every row's Python method raises PsmError with the message"""
    for row in rows:
        with pytest.raises(psm.PsmError, match=match):
            QL.call(obj, row, dict(batches[row.gen], other=other), row.variants[0])


def test_lists_and_worlds_that_hold_a_lived_hierarchy(psm, ctx, scenes):
    aux_tris = IQ.icosphere(1, 1.0)
    aux = _hier(psm, ctx, aux_tris)
    life = psm.TriangleHierarchy(ctx)
    rng = np.random.RandomState(31)
    poses = [NQ.random_pose(rng, reflect=False, shift=0.5), NQ.random_pose(rng, reflect=True, shift=0.5),
             NQ.random_pose(rng, reflect=False, shift=0.5)]
    members = lambda th: [(th, poses[0]), (aux, poses[1]), (th, poses[2])]
    scene = psm.QueryScene(ctx, [life, aux])                        # the lists read their handles at every call
    insts = psm.InstancedScene(ctx, [(life, poses[0]), (aux, poses[1])])
    world_rows, list_rows = QL.rows_of("InstanceWorld"), QL.rows_of("QueryScene")
    world_names, list_names = sum(len(r.variants) for r in world_rows), sum(len(r.variants) for r in list_rows)
    assert (len(world_rows), len(list_rows), len(QL.rows_of("InstancedScene"))) == (25, 7, 7)
    small = {g: (QL.gen_mesh(aux_tris, 7) if g == "mesh" else QL.GENERATORS[g](aux_tris, 7)) for g in QL.GENERATORS}
    world, reached = None, []

    def world_refuses(what):
        """all 25 entry points and setTransform: PSM_ERR_STATE naming the first stale instance, the outputs untouched"""
        for row in world_rows:
            rc, msg, untouched = QL.raw_call(psm, ctx, row, [world._w], aux, world=True)
            assert rc == QL.ERR_STATE and (row.export + ": instance 0's hierarchy was rebuilt") in msg, (what, row.export, rc, msg)
            assert untouched, (what, row.export, "wrote to its outputs")
        _refuses(psm, world, world_rows, small, aux, "instance 0's hierarchy was rebuilt")
        with pytest.raises(psm.PsmError, match="instance 0's hierarchy was rebuilt"):
            world.setTransform(1, poses[1])

    def window(what):
        _refuses(psm, scene, list_rows, small, None, "geometry 0 is not built")
        _refuses(psm, insts, QL.rows_of("InstancedScene"), small, None, "instance 0 is not built")
        world_refuses((reached[-1], what))

    try:
        for seed, st in enumerate(walk(scenes, life, window)):
            twin = twin_of(psm, ctx, st)
            twin_world = None
            try:
                if world is None:
                    world = psm.InstanceWorld(ctx, members(life))
                elif st.refit_of is not None:
                    world.refresh()                                  # a refit is no rebuild: the documented refresh() suffices
                else:
                    world_refuses(st.name)                           # a rebuild: stale until the instances are set again
                    world.setInstances(members(life))
                twin_world = psm.InstanceWorld(ctx, members(twin))
                assert len(world) == len(twin_world) == 3
                posed = np.concatenate([NQ.posed(st.tris, poses[0]), NQ.posed(aux_tris, poses[1]), NQ.posed(st.tris, poses[2])])
                same_answers(QL.answers(world, posed, 300 + seed, other=aux), QL.answers(twin_world, posed, 300 + seed, other=aux),
                             world_names, ("world", st.name))
                same_answers(QL.answers(scene, posed, 400 + seed), QL.answers(psm.QueryScene(ctx, [twin, aux]), posed, 400 + seed),
                             list_names, ("scene", st.name))
                same_answers(QL.answers(insts, posed, 500 + seed),
                             QL.answers(psm.InstancedScene(ctx, [(twin, poses[0]), (aux, poses[1])]), posed, 500 + seed),
                             list_names, ("instances", st.name))
                if st.name == "no_leaves":                           # a member without leaves contributes nothing: aux alone answers
                    alone = psm.InstanceWorld(ctx, [(aux, poses[1])])
                    try:
                        a, b = QL.run(world, posed, 300 + seed, other=aux), QL.run(alone, posed, 300 + seed, other=aux)
                        for name in ("psm_world_count_hits_dev", "psm_world_box_count_dev", "psm_world_tri_count_dev", "psm_world_mesh_count_dev",
                                     "psm_world_within_dev", "psm_world_occluded_dev"):
                            assert np.array_equal(a[name][1], b[name][1]), name
                        hit = a["psm_world_intersect_dev"][1]
                        assert np.isin(hit.geom, (-1, 1)).all() and (hit.geom == 1).any()
                    finally:
                        alone.close()
                reached.append(st.name)
            finally:
                if twin_world is not None:
                    twin_world.close()
                twin.close()
        assert reached == STATES
    finally:
        if world is not None:
            world.close()
        life.close()
        aux.close()


def _largest_chunk():
    """the largest chunk (keys in LDS) radix_local is instantiated for: the PSM_LOCAL list of sort_hybrid, sort.hip"""
    text = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "sort.hip")).read()
    caps = [int(c) for c in re.findall(r"PSM_LOCAL\((\d+), \d+\)", text)]
    assert caps and max(caps) == 6144
    return max(caps)


def test_queries_when_the_sort_falls_back_under_a_handle(psm, ctx, oracle):
    """One handle of capacity 8 192 holds 7 000 triangles three times over: a well-spread soup (hybrid sort, a graph exists), the
    same soup shrunk into a corner of bounds that two far triangles keep wide (one sixteen-bit bin holds more keys than the
    largest chunk: the sort goes through global memory once, then the context falls back to the eight passes and another graph
    is captured), the spread soup again (still the eight passes). At each stage the handle equals its twin, and intersect,
    closestPoint and triClosest equal their models."""
    rs = psm.RadixSort(ctx)
    spread = _soup(81, 7000, 1.0, 0.05)
    lo, hi = spread.reshape(-1, 3).min(0), spread.reshape(-1, 3).max(0)
    clustered = ((spread - lo) * F(0.001) + lo).astype(F)                    # the soup, shrunk into a corner of its own bounds
    clustered[-2:] = spread[:2] + (hi - lo) * F(0.9)                         # two triangles far out keep the bounds wide
    built = oracle.build_scene(clustered)
    top = (built["keys"] >> np.uint64(47)).astype(np.int64)                  # the sixteen bits the global passes sort by
    longest = int(np.bincount(top - top.min()).max())
    assert longest > _largest_chunk(), longest                               # no instantiated chunk holds this bin: 7 000 suffice
    top = (oracle.build_scene(spread)["keys"] >> np.uint64(47)).astype(np.int64)
    assert np.bincount(top - top.min()).max() < 1024 and top.size == 7000    # ... and the spread soup overflows nothing
    rows = QL.rows_of("TriangleHierarchy")
    names = sum(len(r.variants) for r in rows if r.gen != "mesh")
    life = psm.TriangleHierarchy(ctx)
    life.allocate(8192)
    assert rs.getAlgorithm() == (2, 2)
    try:
        # (the build drops the few clustered triangles smaller than 1e-5 of the fitted bounds: the oracle's count)
        for stage, (tris, algorithm, leaves) in enumerate(((spread, (2, 2), 7000), (clustered, (2, 0), built["count"]), (spread, (2, 0), 7000))):
            life.clearTribuffer()
            life.loadTriangles(tris.reshape(-1, 9))
            for _ in range(3):
                life.markDirty()
                life.build()
            assert life.info().leaf_count == leaves
            assert rs.getAlgorithm() == algorithm, (stage, rs.getAlgorithm())
            print("fall-back stage %d: getAlgorithm() = %s, longest bin %d" % (stage, rs.getAlgorithm(), longest if stage == 1 else 0))
            twin = _hier(psm, ctx, tris)
            try:
                same_tree(psm, life, twin, "fall-back stage %d" % stage)
                same_answers(QL.answers(life, tris, 600 + stage), QL.answers(twin, tris, 600 + stage), names, stage)
                r, p, qd = QL.gen_rays(tris, 600 + stage), QL.gen_points(tris, 600 + stage), QL.gen_tri_dist(tris, 600 + stage)
                check_rays(psm, life, tris, r["o"], r["d"], r["tmin"], r["tmax"])
                check_points(psm, life, tris, p["p"], p["r"])
                check_clearance(psm, life, tris, qd["q"], qd["r"])
            finally:
                twin.close()
    finally:
        rs.setAlgorithm(2)
        life.close()
