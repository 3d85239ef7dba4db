"""CPU tests (no GPU) of mesh clearance over an instance world (psm_world_mesh_closest_dev / psm_world_mesh_within_dev /
psm_world_mesh_clearance_dev, world_mesh_dist.hip; InstanceWorld.closestToMesh / withinOfMesh / clearanceToMesh):
the restated walk with the shared word (world_mesh_dist_query_model part (b)) answers bit for bit what the flat list answers
(part (a)) on a general world and on the lattice world, with and without skip, at several rmax; the protocol under a few hundred
schedules and all four FLAGS variants, stale reads included; ties; the edge cases; the populations the GPU test asserts, shown by
the flat model alone; the exports, the header text, the Python surface and the refusals that need no device; what
world_mesh_dist.hip compiles to; a posed pair on the host under sanitizers; the header layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_dist_query_model as MD
import mesh_query_model as MQ
import test_gpu_world_mesh_dist as GT
import test_world_box_cpu as WBT
import test_world_tri_cpu as WTT
import tri_dist_query_model as TD
import world_box_query_model as WB
import world_mesh_dist_query_model as WM
import world_mesh_query_model as WMQ
import world_tri_dist_query_model as WD
from point_query_model import _split
from test_gpu_world_mesh import general_poses
from test_mesh_dist_cpu import live
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
I = np.int32
POINT = np.repeat(F([[[0.25, 0.25, 0.25]]]), 3, axis=1)   # three equal vertices: the build keeps no leaf
EYE = WBT._pose(np.eye(3), np.zeros(3))


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ua, ub = (x.view(np.uint32) if x.dtype == F else x for x in (a, b))
    assert np.array_equal(ua, ub), "%s: %s against %s" % (what, a[np.nonzero(ua != ub)[0][:1]], b[np.nonzero(ua != ub)[0][:1]])


def _key(rec):
    """the word a clearance record stands for"""
    return WM.NONE if rec.view(I)[3] < 0 else MD.key_of(rec[2], rec.view(I)[6])


def _walk_is_flat(insts, otris, poses, rmax, skip, what, variants=WM.VARIANTS, rng=None):
    """(b) == (a) for the three queries at every pose, the clearance under each FLAGS variant; returns (a) and, per pose, the
    instances the closest lanes entered"""
    oleaves = live(otris)
    hits, geom, rec, inst, within = WM.flat(insts, otris, oleaves, poses, rmax, skip)
    assert np.array_equal(within, (hits.view(I)[:, :, 3] >= 0).any(axis=1)) and np.array_equal(inst >= 0, within)
    q = MQ.posed(otris, poses)
    world = WM.MeshDistWorld(insts)
    entered = []
    for m in range(q.shape[0]):
        tab = world.prepare(q[m, oleaves])
        h, g, ent = world.closest(tab, rmax, skip)
        _bits(h, hits[m, oleaves], "%s, pose %d: closest records" % (what, m))
        _bits(g, geom[m, oleaves], "%s, pose %d: closest instances" % (what, m))
        assert world.within(tab, rmax, skip) == within[m], (what, m)
        for flags in variants:
            word, r, i = world.clearance(tab, oleaves, rmax, skip, flags, rng, "fresh" if rng is None else "random")
            assert word == _key(rec[m]), (what, m, flags)
            _bits(r, rec[m], "%s, pose %d, flags %d: clearance record" % (what, m, flags))
            assert i == inst[m], (what, m, flags)
        entered.append(ent)
    return (hits, geom, rec, inst, within), entered


# ---- the walk against the flat answer ----------------------------------------------------------------------------------------------

def _lattice_case():
    """the lattice world of DESIGN.md 4.25 and a half-size cube with a dropped triangle, at signed permutations and whole / half
    translations: cutting the block, touching it, and off it by exact distances that many pairs share"""
    insts = WBT.lattice_world()
    otris = np.concatenate([WBT.cube() * F(0.5), POINT])
    perms = WBT.signed_permutations()
    poses = [WBT._pose(perms[j], t) for j, t in zip((0, 11, 30, 45), ([0.75, 0.75, 0.75], [5.5, 0, 0], [0, -4, 1.5], [3, 3, 4.5]))]
    return insts, otris, poses


def test_lattice_world_walk_is_the_flat_answer():
    insts, otris, poses = _lattice_case()
    for rmax, skip in ((np.inf, None), (1.5, None), (0.0, None), (np.inf, 0), (2.5, 7)):
        (hits, geom, rec, inst, within), _ = _walk_is_flat(insts, otris, poses, rmax, skip, "lattice rmax %s skip %s" % (rmax, skip))
        assert (hits.view(I)[:, 12, 3] == -1).all() and (geom[:, 12] == -1).all()      # the dropped triangle
        if np.isinf(rmax):
            assert within.all() and rec[0, 2] == 0 and (rec[1:, 2] > 0).all()
            assert not np.isin(geom, (48, 49, 50) if skip is None else ()).any()       # coincident instances: the lower one
        if skip is not None:
            assert not (geom == skip).any()
    base = WM.flat(insts, otris, live(otris), poses, np.inf, None)                     # the winner of pose 1 skipped: another one
    s = int(base[3][1])
    left = WM.flat(insts, otris, live(otris), poses, np.inf, s)
    assert left[3][1] >= 0 and left[3][1] != s and left[2][1, 2] >= base[2][1, 2]


def test_general_world_walk_is_the_flat_answer():
    rng = np.random.RandomState(61)
    insts = WBT.general_world()
    otris = np.concatenate([WBT._soup(rng, 9, 0.5), POINT, WBT._soup(rng, 8, 0.5)])
    poses = general_poses(rng, 3, -1.0, 0.7)
    first = None
    for rmax, skip in ((np.inf, None), (0.3, None), (0.02, None), (np.inf, 3), (0.3, 0)):
        (hits, geom, rec, inst, within), ent = _walk_is_flat(insts, otris, poses, rmax, skip, "general rmax %s skip %s" % (rmax, skip),
                                                             rng=np.random.RandomState(7))
        assert (geom[:, 9] == -1).all()
        if first is None:
            first = (hits, geom, rec, inst, ent)
            assert within.all()
            mean = np.mean([len(e) for pose in ent for e in pose])
            print("general: %d instances, a closest lane entered %.1f on average" % (len(insts), mean))
            assert mean < len(insts) - 2                   # and it culls: the far members are not entered once a near pair is held
        if skip is not None:
            assert not (geom == skip).any() and not (inst == skip).any()
    assert (first[3] == 3).any() or (first[1] == 3).any()                               # (skip = 3 took something away)
    m = WM.flat(insts, otris, live(otris), poses, 0.02, None)
    assert (m[0].view(I)[:, :, 3] < 0).any()                                            # misses by rmax


# ---- the protocol under schedules ---------------------------------------------------------------------------------------------------

def _protocol_cases():
    rng = np.random.RandomState(62)
    insts, otris, poses = _lattice_case()
    small = [insts[j] for j in (0, 1, 2, 5, 9, 20, 33, 48, 49, 50)]
    gen = WBT.general_world(seed=23, members=5)
    gtris = WBT._soup(rng, 8, 0.6)
    gposes = general_poses(rng, 2, -1.0, 0.3)
    return [("lattice", small, otris, poses[:3], np.inf, None), ("lattice skip", small, otris, poses[1:3], 6.0, 0),
            ("general", gen, gtris, gposes, np.inf, None), ("general rmax", gen, gtris, gposes, 0.4, 2)]


def test_protocol_reaches_the_reduction_under_every_schedule():
    """the lanes of a pose interleaved at random at leaf granularity, every read any value the word has held so far: the final
    word is (Dmin, t*) and the pick record the flat one, under all four FLAGS variants"""
    schedules = 0
    for name, insts, otris, poses, rmax, skip in _protocol_cases():
        oleaves = live(otris)
        _, _, rec, inst, _ = WM.flat(insts, otris, oleaves, poses, rmax, skip)
        q = MQ.posed(otris, poses)
        world = WM.MeshDistWorld(insts)
        for m in range(q.shape[0]):
            tab = world.prepare(q[m, oleaves])
            for flags in WM.VARIANTS:
                for seed in range(10):
                    rng = np.random.RandomState(1000 * seed + 10 * m + flags)
                    word, r, i = world.clearance(tab, oleaves, rmax, skip, flags, rng, "random")
                    assert word == _key(rec[m]) and i == inst[m], (name, m, flags, seed)
                    _bits(r, rec[m], "%s pose %d flags %d seed %d" % (name, m, flags, seed))
                    schedules += 1
    print("%d schedules" % schedules)
    assert schedules >= 300


def test_a_stale_read_that_arrives_late_changes_nothing():
    """the winner's lane runs to its end and publishes; every other lane then reads "none" at each of its reads, long after the
    word was set (the oldest value it has held): more work, the same word. And the reverse: the winner runs last."""
    for name, insts, otris, poses, rmax, skip in _protocol_cases():
        oleaves = live(otris)
        _, _, rec, inst, _ = WM.flat(insts, otris, oleaves, poses, rmax, skip)
        q = MQ.posed(otris, poses)
        world = WM.MeshDistWorld(insts)
        for m in range(q.shape[0]):
            tab = world.prepare(q[m, oleaves])
            win = int(np.nonzero(oleaves == rec.view(I)[m, 6])[0][0]) if rec.view(I)[m, 6] >= 0 else 0
            last = [k for k in range(oleaves.size) if k != win]
            for flags in WM.VARIANTS:
                for order, policy in (([win] * 4000, "oldest"), ([k for k in last for _ in range(4000)], "oldest"), ([win] * 4000, "fresh")):
                    word, r, i = world.clearance(tab, oleaves, rmax, skip, flags, None, policy, order)
                    assert word == _key(rec[m]) and i == inst[m], (name, m, flags, policy)
                    _bits(r, rec[m], "%s pose %d flags %d %s" % (name, m, flags, policy))


# ---- ties ------------------------------------------------------------------------------------------------------------------------------

def test_ties():
    c = WBT.cube()
    M = WB.plain_fit(c)
    near = F([[[0.25, 0.25, 1.5], [0.75, 0.25, 1.5], [0.25, 0.75, 1.75]]])                  # 0.5 above the top face
    far = F([[[0.25, 0.25, 9], [0.75, 0.25, 9], [0.25, 0.75, 9]]])
    # two triangles of other at a bit-equal dist: the lower t; the record is the same
    otris = np.concatenate([far, near, far, near])
    three = [(c, np.arange(12), EYE, M), (c, np.arange(12), WBT._pose(np.eye(3), [5, 0, 0]), M), (c, np.arange(12), EYE, M)]
    (hits, geom, rec, inst, _), _ = _walk_is_flat(three, otris, [EYE], np.inf, None, "other twice")
    assert rec.view(I)[0, 6] == 1 and rec[0, 2] == 0.5 and hits[0, 1, 2] == hits[0, 3, 2]
    _bits(hits[0, 1], hits[0, 3], "the same record twice")
    # coincident instances: the lower instance; with it skipped, its twin, the same record
    assert inst[0] == 0 and (geom[0] == [0, 0, 0, 0]).all()
    (hits2, geom2, rec2, inst2, _), _ = _walk_is_flat(three, otris, [EYE], np.inf, 0, "skip on the winner")
    assert inst2[0] == 2 and (geom2[0] == 2).all()
    _bits(rec2, rec, "the twin's record")
    (_, _, rec3, inst3, _), _ = _walk_is_flat(three, otris, [EYE], np.inf, 1, "skip on a non-winner")
    _bits(rec3, rec, "a non-winner skipped")
    assert inst3[0] == 0
    (_, _, rec4, inst4, _), _ = _walk_is_flat(three[:1], otris, [EYE], np.inf, 0, "a world of one, skipped")
    assert inst4[0] == -1 and rec4.view(I)[0, 3] == -1 and rec4.view(I)[0, 6] == -1
    # a pose that cuts several instances: dist 0, and the pair is overlapsMesh's first
    insts, cube_tris, poses = _lattice_case()
    for skip in (None, 0):
        (hits, geom, rec, inst, _), _ = _walk_is_flat(insts, cube_tris, poses[:1], np.inf, skip, "cutting", variants=(14,))
        _, count, trows, irows, _ = WMQ.query(insts, cube_tris, live(cube_tris), poses[:1], 1, skip)
        assert (count[0] > 3).sum() > 3 and np.array_equal(hits[0, :, 2] == 0, count[0] > 0)
        t_star = int(np.nonzero(count[0] > 0)[0][0])
        assert rec[0, 2] == 0 and rec.view(I)[0, 6] == t_star
        assert rec.view(I)[0, 3] == trows[0, t_star, 0] and inst[0] == irows[0, t_star, 0]
        meets = count[0] > 0
        assert np.array_equal(hits.view(I)[0, meets, 3], trows[0, meets, 0]) and np.array_equal(geom[0, meets], irows[0, meets, 0])


# ---- edge cases ----------------------------------------------------------------------------------------------------------------------

def test_rmax_edges_tiny_meshes_and_the_empty_world():
    c = WBT.cube()
    one = F([[[0, 0, 3], [1, 0, 3], [0, 1, 3]]])                                             # a one-leaf member: enter()'s lone leaf
    insts = [(c, np.arange(12), EYE, WB.plain_fit(c)), (one, np.arange(1), EYE, WB.plain_fit(one))]
    base = F([[[0.25, 0.25, 2.0], [0.75, 0.25, 2.0], [0.25, 0.75, 2.0]]])                    # 1 above the cube, 1 below the triangle
    otris = np.concatenate([POINT, base])
    for rmax, found in ((np.inf, True), (1.0, True), (np.nextafter(F(1), F(0)), False), (0.0, False), (-0.0, False), (1e-30, False),
                        (np.nan, False), (-1.0, False), (-np.inf, False)):
        (hits, geom, rec, inst, within), _ = _walk_is_flat(insts, otris, [EYE], rmax, None, "rmax %s" % rmax)
        assert within[0] == found and (inst[0] == 0) == found and (rec[0, 2] == 1) == found
        assert geom[0, 0] == -1 and hits.view(I)[0, 0, 3] == -1
    (_, _, rec, inst, _), _ = _walk_is_flat(insts, otris, [EYE], 1.0, 0, "the lone leaf wins")
    assert inst[0] == 1 and rec.view(I)[0, 3] == 0 and rec[0, 2] == 1
    (_, _, rec, inst, _), _ = _walk_is_flat(insts, otris, [EYE], 1.0, 1, "the lone leaf skipped")
    assert inst[0] == 0
    on = np.concatenate([c[3:4], POINT])                                                     # on the mesh: rmax = 0, -0 and tiny find it
    for rmax in (0.0, -0.0, 1e-30):
        (_, _, rec, inst, within), _ = _walk_is_flat(insts, on, [EYE], rmax, None, "on the mesh")
        assert within[0] and rec[0, 2] == 0 and inst[0] == 0 and rec.view(I)[0, 6] == 0
    # other with 0 and 1 leaves; the empty world
    for o, leaves in ((np.concatenate([POINT] * 3), 0), (base, 1)):
        (hits, geom, rec, inst, within), _ = _walk_is_flat(insts, o, [EYE, WBT._pose(np.eye(3), [0, 0, 0.5])], np.inf, None, "%d leaves" % leaves)
        assert live(o).size == leaves and within.all() == bool(leaves) and (inst >= 0).all() == bool(leaves)
    (hits, geom, rec, inst, within), _ = _walk_is_flat([], otris, [EYE], np.inf, None, "the empty world")
    _bits(hits[0], TD.miss_records(2), "empty world: closest")
    _bits(rec, WM.miss_clearance(1), "empty world: clearance")
    assert (geom == -1).all() and inst[0] == -1 and not within[0]
    assert [float(x) for x in rec[0, [0, 1, 2, 4, 5, 7]]] == [0, 0, np.inf, 0, 0, 0] and list(rec.view(I)[0, [3, 6]]) == [-1, -1]


def test_identity_world_of_one_is_mesh_clearance():
    rng = np.random.RandomState(63)
    tris = WBT._soup(rng, 50)
    cand = np.sort(rng.permutation(50)[:44])
    otris = np.concatenate([WBT._soup(rng, 6, 0.8), POINT, WBT._soup(rng, 5, 0.8)])
    poses = general_poses(rng, 3, -2.0, 0.4)
    for rmax in (np.inf, 0.2):
        want_hits, want_rec, want_within = MD.query(tris, cand, otris, live(otris), poses, rmax)
        (hits, geom, rec, inst, within), _ = _walk_is_flat([(tris, cand, EYE, WB.plain_fit(tris))], otris, poses, rmax, None, "identity")
        _bits(hits, want_hits, "closest")
        _bits(rec, want_rec, "clearance")
        assert np.array_equal(within, want_within) and np.array_equal(geom, np.where(hits.view(I)[:, :, 3] >= 0, 0, -1))
    assert within.any() and not within.all()


# ---- the populations the GPU test asserts, by the flat model alone ---------------------------------------------------------------------

def test_the_gpu_populations_case_shows_every_population():
    """tests/test_gpu_world_mesh_dist.py's populations case with the members' leaves as a build keeps them: every population the
    GPU test asserts is non-empty in the flat model, and the walk (b) enters a winner's instance after another"""
    meshes, entries, otris, poses, rmax = GT.populations_case()
    insts = [(meshes[k], live(meshes[k]), m, WB.plain_fit(meshes[k])) for k, m in entries]
    counts = GT.populations(insts, otris, live(otris), poses, rmax)
    print(counts)
    for name in GT.POPULATIONS:
        assert counts[name] > 0, name


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

ENTRIES = ("psm_world_mesh_closest_dev", "psm_world_mesh_within_dev", "psm_world_mesh_clearance_dev")
METHODS = ("closestToMesh", "withinOfMesh", "clearanceToMesh")


def test_library_exports_world_mesh_clearance(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS, s
        assert re.search(r"\b%s\(psm_world\* world, psm_bvh\* other, const float\* poses, size_t p, int32_t skip, float r(max)?,\s" % s, header), s
    section = header[header.index("/* mesh clearance over a world"):header.index("int psm_world_mesh_closest_dev(")]
    for text in ("DESIGN.md 4.26", "BIT FOR BIT", "psm_world_tri_closest_dev", "{0, 0, +inf, -1, 0, 0, -1, 0}", "{0, 0, +inf, -1, 0, 0, 0, 0}",
                 "the lowest t", "comparing the float32 dist", "(bits(dist) << 32) | t", "it needs no instance", "the other indices are KEPT",
                 "d_hits not 16-byte aligned", "d_inst not 4-byte aligned", "mesh query before build", "p == 0 returns PSM_OK",
                 "ONE synchronisation", "CANNOT be captured", "PSM_MESH_BOUND", "PSM_MESH_SKIP", "NaN or negative is not a refusal",
                 "when the world is empty"):
        assert text in section, text
    covered = section[section.index("not covered:"):]
    for text in ("QueryScene", "InstancedScene", "per-pose rmax", "more than one skipped instance", "k\n *     closest pairs", "dual-tree",
                 "penetration depth", "graph capture"):
        assert text in covered, text
    assert "since added: clearance over an InstanceWorld" in header
    for m in METHODS:
        assert callable(getattr(psm.InstanceWorld, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.TriangleHierarchy):
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for m, s in zip(METHODS, ENTRIES):
        assert re.search(r"int %s\(TriangleHierarchy \* other, const glm::mat4 \* poses, size_t p, int skip, float r" % m, hpp)
        assert "InstanceWorld::%s(" % m in inl and s + "(world," in inl
    csrc = os.path.join(ROOT, "prismarine-core_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^SRC := .*\bworld_mesh_dist\.hip\b", mk, re.M) and re.search(r"^world_mesh_dist\.o: psm_mesh_dist_key\.h", mk, re.M)
    assert "int world_mesh_dist_launch(" in open(os.path.join(csrc, "psm_world_dev.h")).read()
    src = open(os.path.join(csrc, "world_mesh_dist.hip")).read()
    for text in ("struct WorldMeshDistBody : WorldBoxPrune", "tri_dist_lb2(", "mesh_query_tri(", "mesh_split(", "if (in == m.skip) return -1;",
                 "__hip_atomic_load(word(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)", "atomicMin(word()"):
        assert text in src, text
    assert "asm(" not in src and "asm volatile" not in src                                 # plain HIP atomics throughout
    host = open(os.path.join(csrc, "world.hip")).read()
    # (the knob is read once for every clearance entry point, beside the other shared host pieces: DESIGN.md 4.28)
    assert 'getenv("PSM_MESH_BOUND")' in open(os.path.join(csrc, "mesh.hip")).read() and "mesh_bound()" in host
    assert "hipMemsetAsync(d_keys, 0xff" in host
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "clearanceToMesh" in open(os.path.join(ROOT, doc)).read(), doc


def test_result_views_and_witness_points(psm):
    hits = TD.miss_records(6).reshape(2, 3, 8)
    hits[1, 2] = [0.25, 0.5, 2.0, 0, 0.125, 0.75, 0, 0]
    hits.view(I)[1, 2, 3] = 7
    geom = np.full((2, 3), -1, I)
    geom[1, 2] = 4
    got = psm.QueryTriHits(hits, geom)                                                   # closestToMesh's: [p, T] views
    assert got.tri.shape == (2, 3) and got.tri[1, 2] == 7 and got.dist[1, 2] == 2 and got.geom[1, 2] == 4 and np.isinf(got.dist[0]).all()
    assert (got.u[1, 2], got.v[1, 2], got.s[1, 2], got.t[1, 2]) == (0.25, 0.5, 0.125, 0.75)
    assert psm.QueryMeshHits(TD.miss_records(2), True).geom is None                       # a hierarchy's: as before
    # clearanceToMesh's: the two witness points of a lattice pair are that far apart
    c = WBT.cube()
    insts = [(c, np.arange(12), WBT._pose(np.eye(3), [5, 0, 0]), None), (c, np.arange(12), EYE, None)]
    otris = F([[[0.25, 0.25, 1.5], [0.75, 0.25, 1.5], [0.25, 0.75, 1.75]]])
    poses = [EYE, WBT._pose(np.eye(3), [5, 0, 0.25])]
    _, _, rec, inst, _ = WM.flat(insts, otris, [0], poses)
    pair = psm.QueryMeshHits(rec, True, inst)
    assert list(pair.geom) == [1, 0] and list(pair.other) == [0, 0] and list(pair.dist) == [0.5, 0.75]
    posed = [WTT.posed_triangles(i).astype(F) for i in insts]
    on_world, on_other = pair.points_world(posed, otris, poses)
    assert np.allclose(np.linalg.norm(on_world - on_other, axis=1), [0.5, 0.75]) and np.allclose(on_world[:, 2], 1)
    miss = psm.QueryMeshHits(WM.miss_clearance(2), True, np.full(2, -1, I)).points_world(posed, otris, poses)
    assert np.isnan(miss[0]).all() and np.isnan(miss[1]).all()
    with pytest.raises(ValueError):
        psm.QueryMeshHits(rec, True).points_world(posed, otris, poses)


def test_world_mesh_clearance_refusals_that_need_no_device(psm):
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    other = lib.psm_world_mesh_overlaps_dev(None, None, p, ctypes.c_size_t(1), ctypes.c_int32(-1), p)
    assert other != 0
    for s in ENTRIES:                                                                   # no world: refused before anything is touched
        tail = (p,) if s.endswith("within_dev") else (p, p)
        none = (None,) if s.endswith("within_dev") else (None, None)
        assert getattr(lib, s)(None, None, p, ctypes.c_size_t(1), ctypes.c_int32(-1), ctypes.c_float(1.0), *tail) == other
        assert getattr(lib, s)(None, None, None, ctypes.c_size_t(0), ctypes.c_int32(-1), ctypes.c_float(1.0), *none) == other
    assert not any(buf)

    class NoCall(psm.InstanceWorld):   # the Python layer refuses the poses, other, rmax and skip before any call
        def __init__(self):
            self.ctx, self._w, self.hierarchies = None, None, [None, None]

        def _fresh(self, name):
            raise AssertionError("a call was about to be made")

    class Other(psm.TriangleHierarchy):
        def __init__(self):
            self.ctx, self._h, self.triangleCount = None, None, 5

    w, th = NoCall(), Other()
    eye = np.eye(3, 4)
    scaled = eye.copy()
    scaled[:, :3] *= 1.01
    nan = eye.copy()
    nan[0, 3] = np.nan
    calls = (lambda m, r=1.0, s=None: w.closestToMesh(th, m, r, s), lambda m, r=1.0, s=None: w.withinOfMesh(th, m, r, s),
             lambda m, r=1.0, s=None: w.clearanceToMesh(th, m, r, s))
    for call in calls:
        for bad in (scaled, nan, [eye, scaled], np.eye(3), np.zeros((2, 2, 3, 4))):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError, match="rmax must be one scalar"):
            call(eye, [1.0, 2.0])
        for skip in (2, -1, 0.5, True):
            with pytest.raises(psm.PsmError, match="skip must be None or an instance index"):
                call(eye, 1.0, skip)
        with pytest.raises(AssertionError, match="a call was about to be made"):
            call(eye, 1.0, 1)
    with pytest.raises(TypeError):
        w.clearanceToMesh(object(), eye)


# What each kernel reaches with the Makefile's flags, as ceilings: VGPRs, SGPRs, the waves per SIMD its
# __launch_bounds__ ask for (what the unforced figure gives: 512 / VGPRs rounded up to 8), no scratch, no spills, no lane writes,
# the LDS of the 16-entry stack. The clearance kernel's four instances: the shared bound off (0), read in begin() alone (2),
# re-read before every leaf (6), and published early too (14: the default).
WORLD_MESH_DIST_KERNELS = {"24world_query_mesh_closestE": (144, 104, 3, 0), "23world_query_mesh_withinE": (172, 106, 2, 0),
                           "21world_query_mesh_pickE": (143, 96, 3, 0), "26world_query_mesh_clearanceILj0EEEv": (173, 102, 2, 0),
                           "26world_query_mesh_clearanceILj2EEEv": (176, 104, 2, 0), "26world_query_mesh_clearanceILj6EEEv": (178, 106, 2, 2),
                           "26world_query_mesh_clearanceILj14EEEv": (176, 106, 2, 2)}
# (the last figure: SGPRs parked in lanes of a VGPR. The two instances that re-read the word before every leaf park one 64-bit
# kernel argument: written once before the grid-stride loop, read once per query in begin(), never inside the walk)


def test_world_mesh_dist_kernels_codegen():
    asm = csrc_asm("world_mesh_dist.hip")
    assert asm.count(".amdhsa_kernel ") == len(WORLD_MESH_DIST_KERNELS) + 1       # and the fill kernel
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "world_mesh_dist.hip")).read()
    bounds = re.search(r"WMD_CLOSEST_WAVES = (\d+), WMD_WITHIN_WAVES = (\d+), WMD_CLEAR_WAVES = (\d+), WMD_PICK_WAVES = (\d+)", src)
    assert [int(x) for x in bounds.groups()] == [3, 2, 2, 3]
    for name, (vgprs, sgprs, waves, parked) in WORLD_MESH_DIST_KERNELS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%sNS_17WorldMeshDistArgsE" % name)

        def meta(key):
            return kernel_meta(blk, key)
        print(name, meta("vgpr_count"), meta("sgpr_count"), meta("private_segment_fixed_size"))
        assert meta("vgpr_count") <= vgprs and meta("sgpr_count") <= sgprs, (name, meta("vgpr_count"), meta("sgpr_count"))
        assert 512 // ((vgprs + 7) // 8 * 8) == waves, name                    # the bound asks for what the registers give
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") <= parked, (name, meta("sgpr_spill_count"))
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name          # nothing in scratch
        assert body.count("v_writelane_b32") <= parked and body.count("v_readlane_b32") <= parked, name
        first_loop = body.index("Loop Header")
        assert "v_writelane_b32" not in body[first_loop:], name              # parked once, before the loops
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack
        assert "v_div_fixup_f32" in body and "v_sqrt_f32" in body and "v_pk_" not in body, name   # IEEE division and sqrtf, nothing paired
        clear = "clearance" in name
        assert ("global_atomic_umin_x2" in body) == clear, name               # the publication: one 64-bit atomic minimum
        loads = len(re.findall(r"global_load_dwordx2 [^\n]*sc1", body))       # agent-scope loads of the word
        assert (loads >= 1) == (clear and "Lj0E" not in name), (name, loads)


def _host_records(n_poses=24, per=200):
    """(other's pose[12], its v0, e1, e2, the instance's pose[12], its v0, e1, e2) float32 [n, 42]: pairs over five decades of
    size under exact poses and poses at the edge of the pose check, near, far, touching (a shared vertex) and coincident"""
    rng = np.random.RandomState(64)
    recs = []
    for k in range(n_poses):
        scale = 10.0 ** (k % 5 - 2)
        a, b = WBT._soup(rng, per, scale), WBT._soup(rng, per, scale)
        b[::7] = a[::7]                                                                 # coincident triangles
        po = WBT._edge_pose(rng, rng.normal(size=3) * scale) if k % 2 else WBT._pose(WBT._rotation(rng, k % 4 == 0), rng.normal(size=3) * scale)
        pi = WBT._edge_pose(rng, rng.normal(size=3) * scale) if k % 3 == 0 else WBT._pose(WBT._rotation(rng, k % 4 == 2), rng.normal(size=3) * scale)
        if k % 6 == 0:
            pi = po.copy()                                                              # the same pose: the coincident ones meet
        s0, s1, s2 = _split(a)
        c0, c1, c2 = _split(b)
        recs.append(np.concatenate([np.broadcast_to(po.reshape(1, 12), (per, 12)), s0, s1, s2,
                                    np.broadcast_to(pi.reshape(1, 12), (per, 12)), c0, c1, c2], axis=1))
    rec = np.concatenate(recs).astype(F)
    rec[::211, 12] = np.nan
    rec[5::211, 3] = np.float32(3e38)                                                   # a posed image that overflows
    return rec


def test_posed_pair_on_the_host_is_the_model(tmp_path):
    """mesh_query_tri of psm_mesh_dev.h, fwd_point / fwd_vec of psm_world_box_dev.h, tri_dist of psm_tri_dist_dev.h and mesh_key of
    psm_mesh_dist_key.h as world_mesh_dist.hip joins them, as a stand-alone host program with its own main, built with
    -ffp-contract=off and the address and undefined-behaviour sanitizers and run as a process of its own on the CPU: d2, the four
    weights and the key of every pair are the model's bit for bit"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout = (str(tmp_path / x) for x in ("world_mesh_dist_host", "records.bin", "out.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "world_mesh_dist_host.cpp"), "-o", exe])
    rec = _host_records()
    assert rec.shape[1] == 42 and rec.shape[0] >= 4000
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, np.uint32).reshape(-1, 8)
    assert got.shape[0] == rec.shape[0]
    with np.errstate(all="ignore"):
        q = MQ.pose_records(rec[:, :12], rec[:, 12:15], rec[:, 15:18], rec[:, 18:21])
        m = rec[:, 21:33]
        v0, e1, e2 = MQ.fwd_point(m, rec[:, 33:36]), MQ.fwd_vec(m, rec[:, 36:39]), MQ.fwd_vec(m, rec[:, 39:42])
        want = np.stack(TD.tri_dist(v0, e1, e2, q[:, 0], q[:, 1], q[:, 2]), axis=1).astype(F)
        dist = np.sqrt(want[:, 0])
    gf = got[:, :5].view(F)
    same = (got[:, :5] == want.view(np.uint32)) | (np.isnan(gf) & np.isnan(want))
    bad = np.nonzero(~same.all(axis=1))[0]
    assert bad.size == 0, "%d differ, first %d: got %s want %s" % (bad.size, bad[0], gf[bad[0]], want[bad[0]])
    ok = ~np.isnan(dist)
    keys = (got[:, 6].astype(np.uint64) << np.uint64(32)) | got[:, 5].astype(np.uint64)
    assert [int(k) for k in keys[ok]] == [MD.key_of(d, t) for d, t in zip(dist[ok], np.nonzero(ok)[0])]
    assert (got[:, 7] == 0).all()
    assert (want[:, 0] == 0).sum() > 50 and (want[:, 0] > 0).sum() > 3000 and np.isnan(want[:, 0]).any()


def test_world_mesh_clearance_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "world_mesh_dist_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_mesh_dist_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
