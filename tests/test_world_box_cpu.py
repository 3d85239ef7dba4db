"""CPU tests (no GPU) of the box queries over an instance world (psm_world_box_overlaps_dev / psm_world_box_count_dev /
psm_world_box_triangles_dev, world_box.hip; InstanceWorld.overlapsBox / countInBox / trianglesInBox): the
restatement of the top-level test, the prune and the walk (world_box_query_model part (b)) answers bit for bit what the flat list
answers (part (a)) on a lattice world and on a general one; the prune's margin in float64; the culling is exactly the set of
reachable instances; an identity world of one is the bare hierarchy; rows and prefixes; the exports, the header text, the Python
surface and the refusals that need no device; what world_box.hip compiles to; the header layer; the key list under sanitizers."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import box_query_model as BQ
import instance_query_model as NQ
import world_box_query_model as WB
from util import ROOT, csrc_asm, kernel_asm, kernel_meta
from world_pose_cases import touching_boxes as _touching_boxes

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


def cube():
    """the unit cube [0, 1]^3 as 12 triangles, two in each face"""
    c = np.array(list(itertools.product((0, 1), repeat=3)), F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[c[a], c[b], c[d]] for a, b, d, _ in quads] + [[c[a], c[d], c[e]] for a, _, d, e in quads], F)


def signed_permutations():
    """the 48 signed axis permutations as float32 3 x 3 matrices: rotations and reflections, all entries 0 or +-1"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            r = np.zeros((3, 3), F)
            for k in range(3):
                r[k, perm[k]] = signs[k]
            out.append(r)
    return out


def _pose(r, t):
    return np.concatenate([np.asarray(r, D), np.asarray(t, D).reshape(3, 1)], axis=1).astype(F)


def lattice_world():
    """cubes at the 48 signed permutations and integer translations in a 3^3 block: touching, overlapping and coincident (the
    first three poses come again at the end). Everything is exact in float32."""
    rng = np.random.RandomState(11)
    c = cube()
    M = WB.plain_fit(c)
    cand = np.arange(12)
    poses = [_pose(r, rng.randint(-1, 3, 3)) for r in signed_permutations()]
    poses += [p.copy() for p in poses[:3]]
    return [(c, cand, p, M) for p in poses]


def grid_cells(lo, hi, cells, shifts=((0, 0, 0),)):
    """the cells of a cells^3 grid of [lo, hi], and the same shifted by half a cell on the axes a shift marks"""
    step = (np.asarray(hi, D) - np.asarray(lo, D)) / cells
    idx = np.array(list(itertools.product(range(cells), repeat=3)), D)
    a, b = [], []
    for s in shifts:
        base = np.asarray(lo, D) + (idx + 0.5 * np.asarray(s, D)) * step
        a.append(base)
        b.append(base + step)
    return np.concatenate(a).astype(F), np.concatenate(b).astype(F)


def test_lattice_world_walk_is_the_flat_answer():
    insts = lattice_world()
    lo, hi = grid_cells((-2, -2, -2), (4, 4, 4), 6, ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)))
    pts = np.array(list(itertools.product((-1.0, 0.0, 0.5, 1.0, 2.0), repeat=3)), F)
    lo, hi = np.concatenate([lo, pts]), np.concatenate([hi, pts])
    want = WB.flat(insts, lo, hi, 16)
    dense = WB.rows_of([WB.counts_matrix(i, lo, hi, staged=False)[0] for i in insts], [np.sort(i[1]) for i in insts], 16)
    _same_answers(want, dense, "lattice: flat() against box_tri on every pair")
    world = WB.BoxWorld(insts)
    got, ent = world.boxes(lo, hi, 16)
    _same_answers(got, want, "lattice")
    count = want[1]
    assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count == 0).any()
    # coincident instances: every shared triangle once per instance, the lowest instance first
    both = np.nonzero((want[3][:, :] == 0).any(axis=1) & (want[1] <= 16) & (want[3] == 48).any(axis=1))[0]
    assert both.size > 0
    for i in both[:20]:
        n = want[4][i]
        t0 = want[2][i, :n][want[3][i, :n] == 0]
        t48 = want[2][i, :n][want[3][i, :n] == 48]
        assert list(t0) == list(t48) and list(want[3][i, :n]) == sorted(want[3][i, :n])
    assert np.mean([len(e) for e in ent[0]]) < 0.5 * len(insts)          # and it culls


def _rotation(rng, reflect=False):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if reflect:
        q[:, 0] = -q[:, 0]
    return q


def fit_like(rng, tris, kind):
    """a fit transform as the build makes them, float32 [3, 4]: kind 0 the plain fit, 1 a rotation, 2 rotate-and-scale with
    condition number up to 16 (uniformly scaled into the unit cube)"""
    if kind == 0:
        return WB.plain_fit(tris)
    v = np.asarray(tris, F).reshape(-1, 3).astype(D)
    s = np.ones(3) if kind == 1 else np.array([1.0, rng.uniform(1, 16), 16.0])[rng.permutation(3)]
    A = _rotation(rng) @ np.diag(s) @ _rotation(rng)
    y = v @ A.T
    lo, ext = y.min(0), (y.max(0) - y.min(0)).max()
    M = np.zeros((3, 4))
    M[:, :3] = A / ext
    M[:, 3] = -lo / ext
    return M.astype(F)


def _soup(rng, n, scale=1.0, offset=0.0):
    c = rng.uniform(-1, 1, (n, 1, 3))
    return ((c + rng.uniform(-0.3, 0.3, (n, 3, 3))) * scale + offset).astype(F)


def general_world(seed=21, members=14):
    """random rotations and reflections, translations over 1e-3 .. 1e3, the three kinds of fit transform, and a member whose
    object coordinates sit at +1000 and whose pose brings it back to the origin"""
    rng = np.random.RandomState(seed)
    insts = []
    for j in range(members):
        tris = _soup(rng, 40, 10.0 ** rng.uniform(-1, 0.5))
        t = rng.normal(size=3)
        t = t / np.linalg.norm(t) * 10.0 ** rng.uniform(-3, 3)
        if j % 3 == 0:
            t = rng.uniform(-2, 2, 3)                       # a cluster that overlaps around the origin
        insts.append((tris, rng.permutation(40)[:36], _pose(_rotation(rng, j % 2 == 1), t), fit_like(rng, tris, j % 3)))
    far = _soup(rng, 40, 1.0, 1000.0)
    r = _rotation(rng)
    insts.append((far, np.arange(40), _pose(r, -r @ np.full(3, 1000.0)), WB.plain_fit(far)))
    return insts


def boxes_around(rng, insts, per):
    """boxes over three decades of size around points of the posed triangles, one box around everything, and invalid ones"""
    lo, hi = [], []
    for tris, cand, pose, _ in insts:
        v0, e1, e2 = WB.posed_leaves(tris, pose)
        at = v0[rng.randint(0, v0.shape[0], per)].astype(D)
        size = np.abs(v0.astype(D) - v0.astype(D).mean(0)).max() + 1e-3
        c = at + rng.normal(size=(per, 3)) * size * 0.1
        half = size * 10.0 ** rng.uniform(-3, 0, (per, 3))
        lo.append(c - half)
        hi.append(c + half)
        lo.append(v0[:2].astype(D))                         # point boxes on posed vertices
        hi.append(v0[:2].astype(D))
    lo, hi = np.concatenate(lo).astype(F), np.concatenate(hi).astype(F)
    everything = np.array([[-3e3] * 3]), np.array([[3e3] * 3])
    bad_lo = np.array([[np.nan, 0, 0], [0, 0, 0], [-np.inf, 0, 0], [1, 0, 0]], F)
    bad_hi = np.array([[1, 1, 1], [1, np.inf, 1], [1, 1, 1], [0, 1, 1]], F)
    return np.concatenate([lo, everything[0].astype(F), bad_lo]), np.concatenate([hi, everything[1].astype(F), bad_hi])


def test_general_world_walk_is_the_flat_answer():
    rng = np.random.RandomState(22)
    insts = general_world()
    lo, hi = boxes_around(rng, insts, 24)
    want = WB.flat(insts, lo, hi, 16)
    got, ent = WB.BoxWorld(insts).boxes(lo, hi, 16)
    _same_answers(got, want, "general")
    count = want[1]
    assert count[-5] == sum(len(i[1]) for i in insts) and (count[-4:] == 0).all()        # everything; the invalid boxes
    assert list(zip(want[3][-5], want[2][-5])) == [(0, t) for t in sorted(insts[0][1])[:16]]
    assert (count[:-5] > 0).mean() > 0.3 and (want[3][:, 0] == len(insts) - 1).any()     # the +1000 member is found
    assert ent[0][-5] == sorted(ent[0][-5], key=ent[0][-5].index) and len(ent[0][-5]) == len(insts)
    assert all(e == [] for e in ent[0][-4:])


def _edge_pose(rng, t):
    """a pose at the edge of the pose check: R (1 + G) with R^T R - 1 = 2 G + G^2 up to 0.95e-5 in its largest entry"""
    g = rng.uniform(-1, 1, (3, 3))
    g = (g + g.T) / 2
    g *= 0.475e-5 / np.abs(g).max()
    p = _pose(_rotation(rng, rng.randint(2) == 1) @ (np.eye(3) + g), t)
    r = p[:, :3].astype(D)
    e = np.abs(r.T @ r - np.eye(3)).max()
    assert 0.8e-5 < e <= 1e-5, e
    return p


def test_prune_margin_covers_every_candidate_that_counts():
    """DESIGN.md 4.16's chain in float64: over plain, rotating and rotate-and-scale fit transforms (condition numbers to 16), exact
    poses and poses at the edge of the pose check's E, six decades of object size with translations up to 1000 sizes away, random
    boxes and boxes built to touch each posed triangle at a vertex, an edge and a face, moved by -8 .. 8 ulps. For every pair that
    counts in float32, on every normalised axis: observed <= bound <= granted / 4; the float32 interval keeps the leaf's exact
    image with no padding; the instance's padded world box, and its union with another box, pass the top-level test.
    Measured: 22 725 pairs that count, the largest observed / bound 0.146, the largest bound / granted 0.061."""
    rng = np.random.RandomState(23)
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
                centre = v0.mean(0) + rng.uniform(-1.2, 1.2, (60, 3)) * scale
                half = 10.0 ** rng.uniform(-3, 0, (60, 3)) * scale
                pairs = [((centre - half).astype(F), (centre + half).astype(F)), _touching_boxes(rng, inst, scale, 6)]
                world = WB.BoxWorld([inst])
                other = (rng.uniform(-5, 5, 3) * scale).astype(F)
                for lo, hi in pairs:
                    ok, kept, observed, bound, granted = WB.prune_figures(inst, lo, hi)
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
    assert max(conds) > 12 and total > 20000


def test_culling_is_exactly_the_reachable_instances():
    """a 16 x 16 grid of cubes, two cube widths apart: the instances the count walk enters are exactly those whose padded world
    box meets the slack-grown world box -- ancestors contain leaves, so nothing else is entered and nothing is skipped; the
    overlaps walk enters a prefix of that order"""
    c = cube()
    M = WB.plain_fit(c)
    insts = [(c, np.arange(12), _pose(np.eye(3), (2 * x, 2 * y, 0)), M) for x in range(16) for y in range(16)]
    world = WB.BoxWorld(insts)
    rng = np.random.RandomState(24)
    lo, hi = grid_cells((-1, -1, -1), (32, 32, 2), 5)
    c0 = rng.uniform(-1, 32, (40, 3)) * (1, 1, 0.05)
    h0 = 10.0 ** rng.uniform(-2, 1.1, (40, 3))
    big_lo, big_hi = np.array([[-0.5, -0.5, 0.25], [-5, -5, -5]], F), np.array([[15.5, 15.5, 0.5], [40, 40, 5]], F)   # a quarter; everything
    lo, hi = np.concatenate([lo, (c0 - h0).astype(F), big_lo]), np.concatenate([hi, (c0 + h0).astype(F), big_hi])
    got, ent = world.boxes(lo, hi, 16)
    _same_answers(got, WB.flat(insts, lo, hi, 16), "grid")
    assert got[1][-2] == 64 * 8 and got[1][-1] == 256 * 12
    reach = world.reachable(lo, hi)
    sizes = []
    for i in range(lo.shape[0]):
        assert sorted(ent[0][i]) == reach[i] and len(set(ent[0][i])) == len(ent[0][i]), i
        assert ent[1][i] == ent[0][i][:len(ent[1][i])], i
        sizes.append(len(reach[i]))
    assert 0 in sizes and sizes[-2] == 64 and sizes[-1] == 256 and np.mean(sizes) < 0.2 * len(insts)


def test_identity_world_of_one_is_the_bare_hierarchy():
    rng = np.random.RandomState(25)
    tris = _soup(rng, 150)
    cand = rng.permutation(150)[:140]
    inst = (tris, cand, NQ.IDENTITY, WB.plain_fit(tris))
    centre, half = rng.uniform(-1, 1, (300, 3)), rng.uniform(0, 0.5, (300, 3))
    lo, hi = (centre - half).astype(F), (centre + half).astype(F)
    lo[0, 0], hi[1, 2] = np.nan, -np.inf
    flag, count, rows, nrows = BQ.query(tris, cand, lo, hi, 16)
    for got in (WB.flat([inst], lo, hi, 16), WB.BoxWorld([inst]).boxes(lo, hi, 16)[0]):
        _same(got[0], flag, "flag")
        _same(got[1], count, "count")
        _same(got[2], rows, "rows")
        _same(got[4], nrows, "rows' count")
        assert np.array_equal(got[3], np.where(rows >= 0, 0, -1))


def test_rows_are_sorted_prefixes_and_counts_agree():
    rng = np.random.RandomState(26)
    insts = general_world(27, 8)
    lo, hi = boxes_around(rng, insts, 20)
    flag, count, big_t, big_i, nbig = WB.flat(insts, lo, hi, 16)
    brute = np.concatenate([WB.counts_matrix(i, lo, hi, staged=False)[0] for i in insts], axis=1)      # box_tri on every pair
    assert np.array_equal(brute, np.concatenate([WB.counts_matrix(i, lo, hi)[0] for i in insts], axis=1))
    dense = WB.rows_of([WB.counts_matrix(i, lo, hi, staged=False)[0] for i in insts], [np.sort(i[1]) for i in insts], 16)
    _same_answers((flag, count, big_t, big_i, nbig), dense, "flat() against box_tri on every pair")
    brute = brute.sum(axis=1)
    assert np.array_equal(count, brute) and np.array_equal(flag, count > 0)
    assert (count > 16).any() and ((count > 0) & (count < 16)).any() and (count == 0).any()
    world = WB.BoxWorld(insts)
    for k in (1, 2, 3, 8, 16):
        for f, c_, tr, ir, n in (WB.flat(insts, lo, hi, k), world.boxes(lo, hi, k)[0]):
            assert np.array_equal(tr, big_t[:, :k]) and np.array_equal(ir, big_i[:, :k]) and np.array_equal(c_, count)
            assert np.array_equal(n, np.minimum(count, k)) and np.array_equal(n > 0, f)
            assert np.array_equal(tr >= 0, np.arange(k)[None] < n[:, None]) and np.array_equal(tr >= 0, ir >= 0)
            key = ir.astype(np.int64) * (1 << 32) + tr
            assert ((key[:, :-1] < key[:, 1:]) | (tr[:, 1:] < 0)).all()


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

WORLD_BOX_ENTRIES = ("psm_world_box_overlaps_dev", "psm_world_box_count_dev", "psm_world_box_triangles_dev")
WORLD_BOX_METHODS = ("overlapsBox", "countInBox", "trianglesInBox")


def test_library_exports_the_world_box_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in WORLD_BOX_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert "box queries over a world" in header and "The edges are R e1 and R e2 -- not differences of posed vertices" in header
    assert "fwd_point(m, x)_k = ((m[4k] * x.x + m[4k+1] * x.y) + m[4k+2] * x.z) + m[4k+3]" in header
    assert "fwd_vec  (m, d)_k =  (m[4k] * d.x + m[4k+1] * d.y) + m[4k+2] * d.z" in header
    for m in WORLD_BOX_METHODS:
        assert callable(getattr(psm.InstanceWorld, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.TriangleHierarchy):
            assert not hasattr(other, m), (other, m)
    lists = psm.QueryTriLists(np.full((3, 4), -1, np.int32), np.zeros(3, U))
    assert lists.geom is None and lists.tri.shape == (3, 4) and len(lists) == 3
    lists = psm.QueryTriLists(np.full((3, 4), -1, np.int32), np.zeros(3, U), np.full((3, 4), -1, np.int32))
    assert lists.geom.shape == (3, 4)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for m, s in zip(WORLD_BOX_METHODS, WORLD_BOX_ENTRIES):
        assert re.search(r"int %s\(const psm_box_query \*" % m, hpp) and "InstanceWorld::%s(" % m in inl and s + "(world," in inl


def test_world_box_refusals_that_need_no_device(psm):
    """no world: the code the other world queries give, before anything is looked at; the Python layer refuses k before any call"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    other = lib.psm_world_intersect_dev(None, None, ctypes.c_size_t(1), None, None)
    assert other != 0
    for fn in (lib.psm_world_box_overlaps_dev, lib.psm_world_box_count_dev):
        assert fn(None, p, ctypes.c_size_t(1), p) == other
        assert fn(None, None, ctypes.c_size_t(0), None) == other
    fn = lib.psm_world_box_triangles_dev
    assert fn(None, p, ctypes.c_size_t(1), ctypes.c_uint32(1), p, p, p) == other
    assert fn(None, None, ctypes.c_size_t(0), ctypes.c_uint32(0), None, None, None) == other
    assert fn(None, p, ctypes.c_size_t(1), ctypes.c_uint32(17), p, p, p) == other
    assert not any(buf)

    class NoCall:   # a world that cannot make a call
        ctx = None
        _scene = True

        def _launch_np(self, *a):
            raise AssertionError("a launch was made")
        _box_query = psm.InstanceWorld._box_query
        trianglesInBox = psm.InstanceWorld.trianglesInBox
    lo = np.zeros((2, 3), F)
    for k in (0, 17, 1 << 20):
        with pytest.raises(psm.PsmError, match="psm_world_box_triangles_dev: k must be 1 .. 16"):
            NoCall().trianglesInBox(lo, lo, k)
    with pytest.raises(ValueError):
        NoCall().trianglesInBox(lo, lo, 2.5)
    with pytest.raises(AssertionError, match="a launch was made"):
        NoCall().trianglesInBox(lo, lo, 16)


# The VGPRs each kernel reaches with the Makefile's flags, as ceilings under the 128 of __launch_bounds__(64, 4), and the LDS it
# declares (the 16-entry stack; the key list is dynamic, k x 512 B, and does not show here)
WORLD_BOX_VGPRS = {"world_query_box_any": 118, "world_query_box_count": 118, "world_query_box_tris": 118}


def test_world_box_kernels_codegen():
    asm = csrc_asm("world_box.hip")
    assert asm.count(".amdhsa_kernel ") == 3
    for name, ceiling in WORLD_BOX_VGPRS.items():
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
        assert ("ds_read_b64" in body and "ds_write_b64" in body) or name != "world_query_box_tris", name
    # by LDS alone a CU's 160 KB hold 35 / 26 / 20 / 13 waves at k = 1 / 4 / 8 / 16 (the kernels ask for 16)
    assert [160 * 1024 // (4096 + k * 64 * 8) for k in (1, 4, 8, 16)] == [35, 26, 20, 13]


def test_world_box_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "world_box_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_box_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)


def test_the_key_list_against_std_sort_under_the_sanitizers(tmp_path):
    """the kernel's own list (psm_world_box_list.h) as a stand-alone host program with its own main, built with the address and
    undefined-behaviour sanitizers and run as a process of its own on the CPU: k = 1 .. 16, keys with the top bit set in either
    half, a list of exactly k slots"""
    exe = str(tmp_path / "world_box_list_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "world_box_list_host.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0 and b" 0 bad" in done.stdout, done.stdout.decode(errors="replace")
