"""CPU tests (no GPU) of the triangle queries over an instance world (psm_world_tri_overlaps_dev / psm_world_tri_count_dev /
psm_world_tri_triangles_dev, world_tri.hip; InstanceWorld.overlapsTriangle / countOnTriangle / trianglesOnTriangle; DESIGN.md
4.20): the restatement of the top-level test, the prune and the walk (world_tri_query_model part (b)) answers bit for bit what the
flat list answers (part (a)) on a lattice world and on a general one; the prune's margin in float64; the culling is exactly the set
of reachable instances; an identity world of one is the bare hierarchy; rows and prefixes; invalid queries; the exports, the header
text, the Python surface and the refusals that need no device; what world_tri.hip compiles to and that world_box.hip's kernels did
not move; the header layer; the posed candidate test on the host under sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import instance_query_model as NQ
import tri_query_model as TQ
import world_box_query_model as WB
import world_tri_query_model as WT
from test_world_box_cpu import _edge_pose, _pose, _rotation, _soup, cube, fit_like, general_world, lattice_world
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
U = np.uint32


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = np.nonzero(np.atleast_1d((a != b).reshape(a.shape[0], -1).any(axis=1)))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def _same_answers(got, want, what):
    for g, w, name in zip(got, want, ("overlaps", "count", "tri", "inst", "rows' count")):
        _same(g, w, "%s: %s" % (what, name))


def posed_triangles(inst):
    """the posed leaves of an instance as float64 triangles [C, 3, 3]: v0', v0' + e1', v0' + e2'"""
    tris, cand, pose = inst[0], inst[1], inst[2]
    v0, e1, e2 = (x.astype(D) for x in WB.posed_leaves(np.asarray(tris, F).reshape(-1, 3, 3)[np.sort(cand)], pose))
    return np.stack([v0, v0 + e1, v0 + e2], axis=1)


def lattice_queries(insts):
    """lattice triangles (integer and half-integer vertices), copies of posed stored triangles, their coplanar neighbours (the
    copy moved along its own edges), and points and segments on vertices, edge midpoints and edges: all exact in float32"""
    rng = np.random.RandomState(31)
    q = [rng.randint(-4, 9, (500, 3, 3)) * 0.5]
    for inst in insts[::3]:
        t = posed_triangles(inst)
        q.append(t)                                                                 # the stored triangles themselves
        q.append(t + (t[:, 1] - t[:, 0])[:, None, :])                               # coplanar, sharing a vertex or an edge
        q.append(t + 0.5 * (t[:, 2] - t[:, 0])[:, None, :])                         # coplanar, overlapping
        q.append(np.repeat(t[:, :1], 3, axis=1))                                    # the point v0'
        q.append(np.repeat(0.5 * (t[:, 1:2] + t[:, 2:3]), 3, axis=1))               # the midpoint of the edge v1' v2'
        q.append(np.stack([t[:, 0], t[:, 1], t[:, 1]], axis=1))                     # the segment v0' v1'
        q.append(np.stack([t[:, 2], t[:, 2] + 2 * (t[:, 1] - t[:, 2]), t[:, 2]], axis=1))   # a segment along an edge, longer
    q = np.concatenate(q)
    assert np.array_equal(q.astype(F).astype(D), q)
    return q.astype(F)


def test_lattice_world_walk_is_the_flat_answer():
    insts = lattice_world()
    q = lattice_queries(insts)
    want = WT.flat(insts, q, 16)
    dense = WB.rows_of([WT.counts_matrix(i, q, staged=False)[0] for i in insts], [np.sort(i[1]) for i in insts], 16)
    _same_answers(want, dense, "lattice: flat() against tri_tri on every pair")
    got, ent = WT.TriWorld(insts).tris(q, 16)
    _same_answers(got, want, "lattice")
    count = want[1]
    assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count[:500] == 0).any()
    assert (count[500:] >= 1).all()                      # every copy, neighbour, point and segment is on its stored triangle
    # coincident instances: every shared triangle once per instance, the lowest instance first
    both = np.nonzero((want[3][:, :] == 0).any(axis=1) & (want[1] <= 16) & (want[3] == 48).any(axis=1))[0]
    assert both.size > 0
    for i in both[:20]:
        n = want[4][i]
        t0 = want[2][i, :n][want[3][i, :n] == 0]
        t48 = want[2][i, :n][want[3][i, :n] == 48]
        assert list(t0) == list(t48) and list(want[3][i, :n]) == sorted(want[3][i, :n])
    assert np.mean([len(e) for e in ent[0]]) < 0.6 * len(insts)          # and it culls


def triangles_around(rng, insts, per):
    """query triangles over three decades of size around points of the posed triangles, points on posed vertices, copies of posed
    stored triangles (as float32 rounds them), one triangle through everything, and invalid ones"""
    q = []
    for inst in insts:
        t = posed_triangles(inst)
        at = t[rng.randint(0, t.shape[0], per), 0]
        size = np.abs(t[:, 0] - t[:, 0].mean(0)).max() + 1e-3
        c = at + rng.normal(size=(per, 3)) * size * 0.1
        q.append(c[:, None, :] + rng.normal(size=(per, 3, 3)) * size * 10.0 ** rng.uniform(-3, 0, (per, 1, 1)))
        q.append(np.repeat(t[:2, :1], 3, axis=1))                  # point queries on posed vertices
        q.append(t[2:4])
    q = np.concatenate(q).astype(F)
    everything = np.array([[[-3e3, -3e3, -3e3], [3e3, 3e3, -3e3], [0, 0, 6e3]]], F)
    bad = np.zeros((4, 3, 3), F)
    bad[0, 0, 0], bad[1, 1, 1], bad[2, 2, 2], bad[3, 0, 1] = np.nan, np.inf, -np.inf, np.nan
    bad[3, 2, 0] = np.inf
    return np.concatenate([q, everything, bad])


def test_general_world_walk_is_the_flat_answer():
    rng = np.random.RandomState(32)
    insts = general_world()
    q = triangles_around(rng, insts, 24)
    want = WT.flat(insts, q, 16)
    got, ent = WT.TriWorld(insts).tris(q, 16)
    _same_answers(got, want, "general")
    count = want[1]
    assert (count[-4:] == 0).all() and all(e == [] for e in ent[0][-4:])                  # the invalid queries
    assert (count[:-5] > 0).mean() > 0.3 and (want[3][:, 0] == len(insts) - 1).any()     # the +1000 member is found
    assert len(ent[0][-5]) == len(insts) and count[-5] > 0                               # the huge triangle enters everything
    per = 24 + 4
    for j in range(len(insts)):                                                          # points on posed v0' count there
        assert (want[3][j * per + 24:j * per + 26] == j).any(axis=1).all(), j


def touching_queries(rng, inst, scale, per):
    """`per` world triangles per triangle of an instance that touch the posed triangle (float64) or miss it by a few ulps: a
    vertex of the query, or a point of one of its edges, on a vertex, a point of an edge or an interior point of the posed
    triangle, moved by -8 .. 8 ulps; in half of them the contact is also a corner of the query's bounding box, the tightest case
    of the prune"""
    t = np.repeat(posed_triangles(inst), per, axis=0)
    n = t.shape[0]
    w = rng.uniform(0, 1, (n, 3))
    kind = rng.randint(0, 3, n)
    w[kind == 0] = np.eye(3)[rng.randint(0, 3, (kind == 0).sum())]
    w[kind == 1, rng.randint(0, 3, (kind == 1).sum())] = 0
    w /= w.sum(axis=1, keepdims=True)
    p = (t * w[:, :, None]).sum(axis=1)
    p = p + rng.randint(-8, 9, (n, 1)) * np.spacing(np.abs(p).astype(F)).astype(D) * np.sign(rng.normal(size=(n, 3)))
    ext = 10.0 ** rng.uniform(-3, 0.5, (n, 1)) * scale
    u, v = rng.normal(size=(n, 3)) * ext, rng.normal(size=(n, 3)) * ext
    away = -np.sign(t.mean(axis=1) - p)
    away[away == 0] = 1
    corner = rng.randint(0, 2, n).astype(bool)[:, None]               # the query leaves the contact away from the triangle on every
    u, v = np.where(corner, away * np.abs(u), u), np.where(corner, away * np.abs(v), v)   # axis: the contact is its box's corner
    with_edge = rng.randint(0, 2, n).astype(bool)[:, None]            # the contact on the query's edge a b, else on its vertex a
    s = rng.uniform(0.1, 0.9, (n, 1))
    a = np.where(with_edge, p - u * s, p)
    b = np.where(with_edge, p + u * (1 - s), p + u)
    return np.stack([a, b, p + v], axis=1).astype(F)


def test_prune_margin_covers_every_candidate_that_counts():
    """DESIGN.md 4.20's chain in float64 (4.16's, with the query's bounding box for the box): over plain, rotating and
    rotate-and-scale fit transforms (condition numbers to 16), exact poses and poses at the edge of the pose check's E, six decades
    of object size with translations up to 1000 sizes away, random query triangles and triangles built to touch each posed
    triangle at a vertex, an edge point or an interior point with a vertex or an edge, moved by -8 .. 8 ulps. For every pair that
    counts in float32, on every normalised axis: observed <= bound <= granted / 4; the float32 interval keeps the leaf's exact
    image with no padding; the instance's padded world box, and its union with another box, pass the top-level test.
    Measured: 13 789 pairs that count, the largest observed / bound 0.154, the largest bound / granted 0.079."""
    rng = np.random.RandomState(33)
    worst_ob, worst_bg, total, conds = 0.0, 0.0, 0, []
    for mag in range(-3, 4):
        scale = 10.0 ** mag
        for kind in (0, 1, 2):
            for edge in (False, True):
                tris = _soup(rng, 60, scale)
                M = fit_like(rng, tris, kind)
                conds.append(np.linalg.cond(M[:, :3].astype(D)))
                t = rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 3)
                pose = _edge_pose(rng, t) if edge else _pose(_rotation(rng, kind == 1), t)
                inst = (tris, np.arange(60), pose, M)
                v0 = WB.posed_leaves(tris, pose)[0].astype(D)
                centre = v0.mean(0) + rng.uniform(-1.2, 1.2, (60, 1, 3)) * scale
                spread = 10.0 ** rng.uniform(-3, 0, (60, 1, 1)) * scale
                sets = [(centre + rng.normal(size=(60, 3, 3)) * spread).astype(F), touching_queries(rng, inst, scale, 6)]
                world = WT.TriWorld([inst])
                other = (rng.uniform(-5, 5, 3) * scale).astype(F)
                for q in sets:
                    ok, kept, observed, bound, granted = WT.prune_figures(inst, q)
                    lo, hi = WT.bounds(q)
                    assert ok.any() and kept[ok].all(), (mag, kind, edge)
                    assert (observed[ok] <= bound[ok]).all(), (mag, kind, edge, (observed[ok] / bound[ok]).max())
                    assert (bound <= granted / 4).all(), (mag, kind, edge, (bound / granted).max())
                    worst_ob = max(worst_ob, (observed[ok] / bound[ok]).max())
                    worst_bg = max(worst_bg, (bound / granted).max())
                    total += int(ok.sum())
                    for i in np.nonzero(ok.any(axis=1))[0]:
                        assert WB.top_keep(world.lo[0], world.hi[0], lo[i], hi[i]), (mag, kind, edge, i)
                        assert WB.top_keep(np.fmin(world.lo[0], other), np.fmax(world.hi[0], other), lo[i], hi[i])
    print("pairs that count: %d; the largest observed / bound %.3g, bound / granted %.3g; condition numbers up to %.1f"
          % (total, worst_ob, worst_bg, max(conds)))
    assert max(conds) > 12 and total > 10000


def test_culling_is_exactly_the_reachable_instances():
    """a 16 x 16 grid of cubes, two cube widths apart: the instances the count walk enters are exactly those whose padded world
    box meets the slack-grown bounding box of the query -- ancestors contain leaves, so nothing else is entered and nothing is
    skipped; the overlaps walk enters a prefix of that order"""
    c = cube()
    M = WB.plain_fit(c)
    insts = [(c, np.arange(12), _pose(np.eye(3), (2 * x, 2 * y, 0)), M) for x in range(16) for y in range(16)]
    world = WT.TriWorld(insts)
    rng = np.random.RandomState(34)
    c0 = rng.uniform(-1, 32, (120, 1, 3)) * (1, 1, 0.05)
    q = c0 + rng.normal(size=(120, 3, 3)) * 10.0 ** rng.uniform(-2, 0.9, (120, 1, 1))
    big = np.array([[[-0.5, -0.5, 0.5], [31, -0.5, 0.5], [-0.5, 31, 0.5]],          # a plane through the lower left half
                    [[-40, -40, 0.25], [200, -40, 0.25], [-40, 200, 0.25]],         # a plane through everything
                    [[-9, -9, -9], [-9, -9, -9], [-9, -9, -9]]], D)                 # a point outside
    q = np.concatenate([q, big]).astype(F)
    got, ent = world.tris(q, 16)
    _same_answers(got, WT.flat(insts, q, 16), "grid")
    assert got[1][-2] == 256 * 8 and got[1][-1] == 0                               # (the four side faces, two triangles each)
    reach = world.reachable(q)
    sizes = []
    for i in range(q.shape[0]):
        assert sorted(ent[0][i]) == reach[i] and len(set(ent[0][i])) == len(ent[0][i]), i
        assert ent[1][i] == ent[0][i][:len(ent[1][i])], i
        sizes.append(len(reach[i]))
    assert sizes[-1] == 0 and sizes[-2] == 256 and sizes[-3] == 256 and np.mean(sizes[:-3]) < 0.2 * len(insts)


def test_identity_world_of_one_is_the_bare_hierarchy():
    rng = np.random.RandomState(35)
    tris = _soup(rng, 150)
    cand = rng.permutation(150)[:140]
    inst = (tris, cand, NQ.IDENTITY, WB.plain_fit(tris))
    q = (rng.uniform(-1, 1, (300, 1, 3)) + rng.uniform(-0.4, 0.4, (300, 3, 3))).astype(F)
    q[0, 0, 0], q[1, 2, 2] = np.nan, -np.inf
    q[2:12] = tris[cand[:10]]
    q[12:15] = [[[-3, -3, z], [3, -3, z + 0.1], [0, 3, z - 0.1]] for z in (-0.5, 0.0, 0.5)]      # planes through the soup
    flag, count, rows, nrows = TQ.query(tris, cand, q, 16)
    assert (count[:2] == 0).all() and (count[2:12] >= 1).all() and (count > 16).any()
    for got in (WT.flat([inst], q, 16), WT.TriWorld([inst]).tris(q, 16)[0]):
        _same(got[0], flag, "flag")
        _same(got[1], count, "count")
        _same(got[2], rows, "rows")
        _same(got[4], nrows, "rows' count")
        assert np.array_equal(got[3], np.where(rows >= 0, 0, -1))


def test_rows_are_sorted_prefixes_and_counts_agree():
    rng = np.random.RandomState(36)
    insts = general_world(37, 8)
    q = triangles_around(rng, insts, 20)
    flag, count, big_t, big_i, nbig = WT.flat(insts, q, 16)
    brute = np.concatenate([WT.counts_matrix(i, q, staged=False)[0] for i in insts], axis=1)      # tri_tri on every pair
    assert np.array_equal(brute, np.concatenate([WT.counts_matrix(i, q)[0] for i in insts], axis=1))
    dense = WB.rows_of([WT.counts_matrix(i, q, staged=False)[0] for i in insts], [np.sort(i[1]) for i in insts], 16)
    _same_answers((flag, count, big_t, big_i, nbig), dense, "flat() against tri_tri on every pair")
    brute = brute.sum(axis=1)
    assert np.array_equal(count, brute) and np.array_equal(flag, count > 0)
    assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count == 0).any()
    world = WT.TriWorld(insts)
    for k in (1, 2, 3, 8, 16):
        for f, c_, tr, ir, n in (WT.flat(insts, q, k), world.tris(q, k)[0]):
            assert np.array_equal(tr, big_t[:, :k]) and np.array_equal(ir, big_i[:, :k]) and np.array_equal(c_, count)
            assert np.array_equal(n, np.minimum(count, k)) and np.array_equal(n > 0, f)
            assert np.array_equal(tr >= 0, np.arange(k)[None] < n[:, None]) and np.array_equal(tr >= 0, ir >= 0)
            key = ir.astype(np.int64) * (1 << 32) + tr
            assert ((key[:, :-1] < key[:, 1:]) | (tr[:, 1:] < 0)).all()


def test_invalid_queries_answer_nothing():
    """a NaN or an infinity in any of the nine numbers: flag 0, count 0, rows of -1, no instance entered -- beside a valid query on
    the same triangles that counts"""
    insts = lattice_world()[:6]
    good = posed_triangles(insts[0])[:1].astype(F)
    q = np.repeat(good, 28, axis=0)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for j in range(9):
            q[1 + 9 * k + j].reshape(9)[j] = bad
    for got, ent in ((WT.flat(insts, q, 4), None), WT.TriWorld(insts).tris(q, 4)):
        flag, count, tr, ir, n = got
        assert flag[0] and count[0] >= 1 and tr[0, 0] >= 0
        assert not flag[1:].any() and not count[1:].any() and not n[1:].any() and (tr[1:] == -1).all() and (ir[1:] == -1).all()
        assert ent is None or all(e == [] for e in ent[0][1:] + ent[1][1:])


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

WORLD_TRI_ENTRIES = ("psm_world_tri_overlaps_dev", "psm_world_tri_count_dev", "psm_world_tri_triangles_dev")
WORLD_TRI_METHODS = ("overlapsTriangle", "countOnTriangle", "trianglesOnTriangle")


def test_library_exports_the_world_triangle_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in WORLD_TRI_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert "triangle queries over a world" in header and "It is valid iff its nine numbers are finite" in header
    assert "tri_tri(fwd_point(m, v0), fwd_vec(m, e1), fwd_vec(m, e2), a, b, c)" in header
    assert "an identity world of one answers as psm_bvh_tri_overlaps_dev" in header
    for m in WORLD_TRI_METHODS:
        assert callable(getattr(psm.InstanceWorld, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.TriangleHierarchy):
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for m, s in zip(WORLD_TRI_METHODS, WORLD_TRI_ENTRIES):
        assert re.search(r"int %s\(const psm_tri_query \*" % m, hpp) and "InstanceWorld::%s(" % m in inl and s + "(world," in inl


def test_world_tri_refusals_that_need_no_device(psm):
    """no world: the code the other world queries give, before anything is looked at; the Python layer refuses k before any call
    and packs [n, 3, 3] and [n, 9] into psm_tri_query records"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    other = lib.psm_world_intersect_dev(None, None, ctypes.c_size_t(1), None, None)
    assert other != 0
    for fn in (lib.psm_world_tri_overlaps_dev, lib.psm_world_tri_count_dev):
        assert fn(None, p, ctypes.c_size_t(1), p) == other
        assert fn(None, None, ctypes.c_size_t(0), None) == other
    fn = lib.psm_world_tri_triangles_dev
    assert fn(None, p, ctypes.c_size_t(1), ctypes.c_uint32(1), p, p, p) == other
    assert fn(None, None, ctypes.c_size_t(0), ctypes.c_uint32(0), None, None, None) == other
    assert fn(None, p, ctypes.c_size_t(1), ctypes.c_uint32(17), p, p, p) == other
    assert not any(buf)

    class NoCall:   # a world that cannot make a call
        ctx = None
        _scene = True

        def _launch_np(self, packed, out, name, *extra):
            assert packed.shape == (2, 12) and packed.dtype == F and not packed[:, 3::4].any()
            assert np.array_equal(packed.reshape(2, 3, 4)[:, :, :3].reshape(2, 9), np.arange(18, dtype=F).reshape(2, 9))
            assert name == "psm_bvh_tri_triangles_dev" and out == "tris" and extra[0].value == 16   # (_call renames it to the world's)
            raise AssertionError("a launch was made")
        _tri_query = psm.InstanceWorld._tri_query
        trianglesOnTriangle = psm.InstanceWorld.trianglesOnTriangle
    q = np.arange(18, dtype=F)
    for k in (0, 17, 1 << 20):
        with pytest.raises(psm.PsmError, match="psm_world_tri_triangles_dev: k must be 1 .. 16"):
            NoCall().trianglesOnTriangle(q.reshape(2, 3, 3), k)
    with pytest.raises(ValueError):
        NoCall().trianglesOnTriangle(q.reshape(2, 3, 3), 2.5)
    for shape in ((2, 3, 3), (2, 9)):
        with pytest.raises(AssertionError, match="a launch was made"):
            NoCall().trianglesOnTriangle(q.reshape(shape), 16)


# The VGPRs each kernel reaches with the Makefile's flags, as ceilings under the 128 of __launch_bounds__(64, 4), and the LDS it
# declares (the 16-entry stack; the key list is dynamic, k x 512 B, and does not show here)
WORLD_TRI_VGPRS = {"world_query_tri_any": 120, "world_query_tri_count": 120, "world_query_tri_tris": 122}


def test_world_tri_kernels_codegen():
    asm = csrc_asm("world_tri.hip")
    assert asm.count(".amdhsa_kernel ") == 3
    for name, ceiling in WORLD_TRI_VGPRS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9WorldArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= 128, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name
        assert meta("group_segment_fixed_size") == 16 * 64 * 4 == 4096, name
        assert "v_rcp_f32" not in body and "v_sqrt_f32" not in body and "v_div_" not in body, name
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body, name
        assert ("ds_read_b64" in body and "ds_write_b64" in body) or name != "world_query_tri_tris", name
    assert 4096 + TQ.K_MAX * 64 * 8 == 12288                                  # the most LDS a launch asks for: stack + 16 keys


def test_the_shared_header_is_what_both_files_use():
    """the pieces live once, in psm_world_box_dev.h; neither kernel file restates them; the Makefile knows the dependency"""
    csrc = os.path.join(ROOT, "prismarine-core_amd", "csrc")
    shared = open(os.path.join(csrc, "psm_world_box_dev.h")).read()
    for piece in ("v3 fwd_vec(", "v3 fwd_point(", "float absmax3(", "WORLD_BOX_PAD = 0x1p-11f", "WORLD_BOX_QREL = 0x1p-8f", "bool keep_top(",
                  "static void axis(", "bool keep("):
        assert shared.count(piece) == 1, piece
        for f in ("world_box.hip", "world_tri.hip"):
            assert piece not in open(os.path.join(csrc, f)).read(), (f, piece)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^world_box\.o world_tri\.o: psm_world_box_dev\.h$", mk, re.M) and re.search(r"^SRC := .*\bworld_tri\.hip\b", mk, re.M)


def test_world_tri_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "world_tri_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_tri_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)


def _host_records():
    """(pose [n, 12], v0, e1, e2, a, b, c [n, 3]) float32: stored triangles and world triangles over six decades of size under
    exact poses and poses at the edge of the pose check: each touching query with the triangle it was built on and with a random
    other one, random queries with random triangles, and some records with NaN and inf in the query"""
    rng = np.random.RandomState(38)
    recs = []
    for mag in range(-3, 3):
        scale = 10.0 ** mag
        for edge in (False, True):
            tris = _soup(rng, 40, scale)
            t = rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 3)
            pose = _edge_pose(rng, t) if edge else _pose(_rotation(rng, mag % 2 == 0), t)
            inst = (tris, np.arange(40), pose, None)
            q = touching_queries(rng, inst, scale, 5)
            own = np.repeat(np.arange(40), 5)
            v0 = WB.posed_leaves(tris, pose)[0].astype(D)
            rq = (v0[rng.randint(0, 40, 200)][:, None, :] + rng.normal(size=(200, 3, 3)) * scale * 10.0 ** rng.uniform(-2, 0, (200, 1, 1))).astype(F)
            for qq, which in ((q, own), (q, rng.randint(0, 40, own.size)), (rq, rng.randint(0, 40, 200))):
                s0, s1, s2 = TQ._split(tris[which])
                recs.append(np.concatenate([np.broadcast_to(pose.reshape(1, 12), (qq.shape[0], 12)), s0, s1, s2, qq.reshape(-1, 9)], axis=1))
    rec = np.concatenate(recs).astype(F)
    rec[::97, 21] = np.nan
    rec[1::97, 26] = np.inf
    rec[2::97, 29] = -np.inf
    return rec


def test_posed_candidate_test_on_the_host_is_the_model(tmp_path):
    """fwd_point / fwd_vec of psm_world_box_dev.h and tri_tri of psm_tri_dev.h as a stand-alone host program with its own main,
    built with -ffp-contract=off and the address and undefined-behaviour sanitizers and run as a process of its own on the CPU:
    the posed leaf of every record is the model's bit for bit and its flag is the model's"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout, fposed = (str(tmp_path / x) for x in ("world_tri_pose_host", "records.bin", "flags.bin", "posed.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "world_tri_pose_host.cpp"), "-o", exe])
    rec = _host_records()
    assert rec.shape[1] == 30 and rec.shape[0] >= 5000
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout, fposed], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, np.uint8).astype(bool)
    posed = np.fromfile(fposed, F).reshape(-1, 9)
    # the model poses per record: fwd_point / fwd_vec take one pose, so the records are grouped by their pose
    want_posed = np.zeros((rec.shape[0], 9), F)
    _, first, inverse = np.unique(rec[:, :12], axis=0, return_index=True, return_inverse=True)
    for g, f in enumerate(first):
        rows = np.nonzero(inverse.reshape(-1) == g)[0]
        pose = rec[f, :12].reshape(3, 4)
        want_posed[rows, 0:3] = WB.fwd_point(pose, rec[rows, 12:15])
        want_posed[rows, 3:6] = WB.fwd_vec(pose, rec[rows, 15:18])
        want_posed[rows, 6:9] = WB.fwd_vec(pose, rec[rows, 18:21])
    assert posed.shape == want_posed.shape and np.array_equal(posed.view(U), want_posed.view(U))
    want = TQ.tri_tri(want_posed[:, 0:3], want_posed[:, 3:6], want_posed[:, 6:9], rec[:, 21:24], rec[:, 24:27], rec[:, 27:30])
    bad = np.nonzero(got != want)[0] if got.shape == want.shape else np.zeros(1, int)
    assert got.shape == want.shape and bad.size == 0, "%d differ, first %d: %s" % (bad.size, bad[0], rec[bad[0]])
    assert 0.1 < want.mean() < 0.8 and not want[::97].any() and not want[1::97].any() and not want[2::97].any()
