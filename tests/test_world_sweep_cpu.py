"""CPU tests (no GPU) of the sphere sweeps over an instance world (psm_world_sweep_sphere_dev / psm_world_sweep_occluded_dev,
world_sweep.hip; InstanceWorld.sphereCast / sphereCastOccluded): the flat answer (world_sweep_query_model part
(a)) is the definition -- sweep_tri on every (sweep, instance, triangle) with the sweep moved, the smallest t, then the lowest
(instance, triangle); the restatement of the top-level test, the prune and the walk (part (b)) answers record for record what the
flat list answers, on random rigid worlds of 2, 33 and 257 poses and on a lattice world; the top level's margin in float64; the
exports, the header text, the Python surface and the refusals that need no device; what world_sweep.hip compiles to; the header
layer."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import instance_query_model as NQ
import sweep_query_model as SW
import world_box_query_model as WB
import world_sweep_query_model as WS
from test_sweep_query_cpu import _grazing_sweeps
from test_world_box_cpu import _pose, _rotation, fit_like, lattice_world, signed_permutations
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
U = np.uint32


def _same_records(got, want, what):
    """hits bit for bit (u, v, t, tri), the instance and the flag"""
    for g, w, name in zip(got, want, ("hits", "inst", "occluded")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        a, b = (g.view(U), w.view(U)) if g.dtype == F else (g, w)
        bad = np.nonzero(np.atleast_1d((a != b).reshape(a.shape[0], -1).any(axis=1)))[0]
        assert bad.size == 0, "%s: %s: %d differ, first %d: %s against %s" % (what, name, bad.size, bad[0], g[bad[0]], w[bad[0]])


def _soup(rng, n, spread=1.0, size=0.3):
    c = rng.uniform(-spread, spread, (n, 1, 3))
    return (c + rng.uniform(-size, size, (n, 3, 3))).astype(F)


def rigid_world(n, seed):
    """n random rigid poses, every second a reflection, of three small soups (the three kinds of fit transform), two of the
    poses coincident (the last is the first's again), and the spread of the translations"""
    rng = np.random.RandomState(seed)
    meshes = [_soup(rng, 12), _soup(rng, 18, 0.7, 0.4), _soup(rng, 9, 1.0, 0.6)]
    fits = [fit_like(rng, t, k) for k, t in enumerate(meshes)]
    cands = [np.arange(12), rng.permutation(18)[:16], np.arange(9)]
    spread = 1.5 * max(1.0, n ** (1.0 / 3.0))
    insts = []
    for k in range(n):
        w = k % 3
        insts.append((meshes[w], cands[w], NQ.random_pose(rng, reflect=bool(k & 1), shift=spread), fits[w]))
    if n > 2:
        insts[-1] = (insts[0][0], insts[0][1], insts[0][2].copy(), insts[0][3])
    return insts, spread


def world_sweeps(rng, insts, spread, count):
    """sweeps through the world (origins inside and around it, directions towards points of it), radii over 1e-3 .. half the
    world, finite and infinite tmax, and a row of invalid ones at the end"""
    o = rng.uniform(-spread - 2, spread + 2, (count, 3))
    d = rng.uniform(-spread - 1, spread + 1, (count, 3)) - o
    d *= 10.0 ** rng.uniform(-2, 2, (count, 1))                       # any length
    r = 10.0 ** rng.uniform(-3, np.log10(spread + 1.0), count)
    tm = np.where(rng.uniform(size=count) < 0.5, np.inf, rng.uniform(0, 2 * spread + 2, count))
    o, d, r, tm = o.astype(F), d.astype(F), r.astype(F), tm.astype(F)
    r[:8] = 0                                                         # a radius of 0 is valid
    tm[8:12] = 0                                                      # and so is tmax = 0: only a start that touches counts
    bad = count - 8
    o[bad, 0], d[bad + 1, 1], r[bad + 2], r[bad + 3], tm[bad + 4], tm[bad + 5] = np.nan, np.inf, -1, np.inf, -1, np.nan
    d[bad + 6], r[bad + 7] = 0, np.nan
    return o, d, r, tm


@functools.lru_cache(maxsize=None)
def _case(n):
    """a world, its sweeps, sweep_tri on every pair and the flat answer, once for the tests that share them"""
    insts, spread = rigid_world(n, 300 + n)
    o, d, r, tm = world_sweeps(np.random.RandomState(n), insts, spread, 3000 if n < 200 else 2000)
    contacts = [WS.pair_contacts(i, o, d, r, tm) for i in insts]
    for c in contacts:
        for x in c:
            x.setflags(write=False)
    return insts, (o, d, r, tm), contacts, WS.flat(insts, o, d, r, tm)


@pytest.mark.parametrize("n", [2, 33, 257])
def test_flat_is_the_definition(n):
    """flat() -- sweep_query_model.query per instance on the moved sweep, combined in list order -- is sweep_tri on every
    (sweep, instance, triangle) with the smallest t, then the lowest (instance, triangle), winning"""
    insts, (o, d, r, tm), contacts, want = _case(n)
    _same_records(WS.lowest(contacts), want, "%d poses" % n)
    hits, inst, occ = want
    assert (inst[-8:] == -1).all() and not occ[-8:].any() and np.isinf(hits[-8:, 2]).all()         # the invalid sweeps miss
    assert 0.1 < occ.mean() < 0.95 and (hits[occ, 2] == 0).any() and (hits[occ, 2] > 0).any()
    assert (occ[:8].any() or n == 2) and (hits[8:12, 2][occ[8:12]] == 0).all()      # radius 0 touches; tmax 0: only starts
    assert len(np.unique(inst[occ])) > min(n, 20) // 2
    if n > 2:   # the last instance is the first's pose again: it never wins, the tie goes to the lowest instance
        assert (inst == 0).any() and not (inst == n - 1).any()
        t_last = np.where(np.isfinite(contacts[-1][0]), contacts[-1][0], np.inf).min(axis=1)
        assert (t_last[inst == 0] == hits[inst == 0, 2]).all()


@pytest.mark.parametrize("n", [2, 33, 257])
def test_walk_is_the_flat_answer(n):
    insts, (o, d, r, tm), contacts, want = _case(n)
    (hits, inst), occ, ent = WS.SweepWorld(insts).sweeps(o, d, r, tm, contacts)
    _same_records((hits, inst, occ), want, "%d poses" % n)
    assert all(e == [] for e in ent[0][-8:])
    if n > 30:                                                        # and it culls (the radii reach up to the whole world)
        small = r < 0.1
        assert np.mean([len(e) for e, s in zip(ent[0], small) if s]) < 0.5 * n
        assert np.mean([len(e) for e in ent[1]]) <= np.mean([len(e) for e in ent[0]])


def test_lattice_world_walk_is_the_flat_answer():
    """cubes at the 48 signed axis permutations and integer translations, three of them twice: sweeps along the axes and the
    diagonals from lattice points with exact radii tie on t across touching and coincident cubes"""
    insts = lattice_world()
    rng = np.random.RandomState(31)
    at = np.array([(x, y, z) for x in (-2.5, -1.0, 0.5, 1.0, 2.5) for y in (-2.5, 0.0, 0.5, 2.0) for z in (-1.5, 0.5, 1.0, 3.5)], F)
    dirs = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 1, 0), (1, -1, 1), (0, 2, 0)], F)
    o = np.repeat(at, len(dirs), axis=0)
    d = np.tile(dirs, (len(at), 1))
    r = rng.choice(np.array([0, 0.125, 0.25, 0.5, 1.0], F), o.shape[0])
    tm = rng.choice(np.array([np.inf, 0.5, 1.0, 4.0], F), o.shape[0])
    want = WS.flat(insts, o, d, r, tm)
    contacts = [WS.pair_contacts(i, o, d, r, tm) for i in insts]
    _same_records(WS.lowest(contacts), want, "lattice: flat() against sweep_tri on every pair")
    (hits, inst), occ, ent = WS.SweepWorld(insts).sweeps(o, d, r, tm, contacts)
    _same_records((hits, inst, occ), want, "lattice")
    assert 0.3 < occ.mean() < 1 and (hits[occ, 2] == 0).any() and (hits[occ, 2] > 0).any()
    # coincident instances (48, 49, 50 are 0, 1, 2 again): every contact ties, the lowest instance has it
    assert np.isin(inst, (0, 1, 2)).any() and not np.isin(inst, (48, 49, 50)).any()
    tied = sum(int((np.concatenate([c[0][i] for c in contacts]) == hits[i, 2]).sum() > 1) for i in np.nonzero(occ)[0])
    assert tied > 50
    assert np.mean([len(e) for e in ent[0]]) < 0.8 * len(insts)


def test_an_instance_in_which_the_moved_sweep_is_not_finite_is_skipped():
    """origin - T overflows in the first instance and is 0 in the second: the answer is the second's alone (the flat answer only:
    the model's tree is not made for centres 4e38 apart; tests/test_gpu_world_sweep.py puts the case to the kernels)"""
    rng = np.random.RandomState(32)
    tris = _soup(rng, 20)
    M = WB.plain_fit(tris)
    big = F(2e38)
    insts = [(tris, np.arange(20), _pose(np.eye(3), (-big, 0, 0)), M), (tris, np.arange(20), _pose(np.eye(3), (big, 0, 0)), M)]
    n = 200
    o = np.tile(np.array([[big, 0, 0]], F), (n, 1))
    d = rng.normal(size=(n, 3)).astype(F)
    r = (10.0 ** rng.uniform(-2, 0, n)).astype(F)
    with np.errstate(all="ignore"):
        assert not np.isfinite(NQ.move(insts[0][2], o)).all(axis=1).any() and (NQ.move(insts[1][2], o) == 0).all()
        want = WS.flat(insts, o, d, r, np.inf)
        alone = SW.query(tris, np.arange(20), np.zeros((n, 3), F), d, r, np.inf)
        _same_records(want, (alone[0], np.where(alone[1], 1, -1).astype(np.int32), alone[1]), "the finite instance alone")
        assert 0.1 < want[2].mean()


# ---- the top level's margin chain ---------------------------------------------------------------------------------

def _extreme_sweeps(rng, inst, per):
    """sweeps along a world axis onto the posed vertex of the instance that is extreme on that axis, from outside: at contact the
    centre stands a radius outside the instance's world box, the case the growth G is for; small offsets across the axis"""
    tris, cand, pose, _ = inst
    v = NQ.to_world(pose, np.asarray(tris, F)[np.sort(cand)].reshape(-1, 3))
    size = np.abs(v - v.mean(0)).max()
    o, d, r = [], [], []
    for k in range(3):
        for sign in (1.0, -1.0):
            tip = v[np.argmax(sign * v[:, k])]
            rr = 10.0 ** rng.uniform(-3, 0.3, per) * size
            off = rng.normal(size=(per, 3)) * rr[:, None] * 10.0 ** rng.uniform(-4, -0.5, (per, 1))
            off[:, k] = 0
            start = tip + off
            start[:, k] += sign * (rr + size * 10.0 ** rng.uniform(-2, 1, per))
            dd = np.zeros((per, 3))
            dd[:, k] = -sign
            o.append(start)
            d.append(dd)
            r.append(rr)
    return np.concatenate(o).astype(F), np.concatenate(d).astype(F), np.concatenate(r).astype(F)


def test_top_level_margin_keeps_every_instance_that_holds_a_contact():
    """DESIGN.md 4.18's chain in float64. Worlds of a near cluster, members 1e-3 .. 1e3 away and a member whose object coordinates
    sit at +1000 and whose pose (translation ~1000) brings it back; random sweeps with radii from 1e-3 to half the world, sweeps
    that graze a vertex, an edge and a face of a posed triangle within -8 .. 8 ulps of the radius, and sweeps along an axis onto
    the vertex that is extreme on it. For every (sweep, instance, triangle) that counts: the float32 top-level slab keeps the
    instance's box with the limit at t; the world centre origin + t dn lies outside the box without its padding, beyond the
    radius, by at most 1/4 of what G and the padding grant beyond the radius; and outside the PADDED box, beyond the radius,
    by at most 1/4 of what G alone grants beyond it (it never lies outside at all: the padding alone covers the move).
    Measured: 168 940 triples that count; the largest observed / granted 1.82e-4 without the padding (the padding covers the
    move's rounding and the pose check's E as for rays, and 2^-11 of the radius the 1.5e-5 of |R^T d| and the leaf residual);
    against the padded box the centre never comes outside beyond the radius: the nearest, in units of G's grant, -0.0726."""
    rng = np.random.RandomState(33)
    worst_bare, worst_padded, total = -np.inf, -np.inf, 0
    for seed in range(3):
        insts = []
        for j in range(9):
            tris = _soup(rng, 30, 10.0 ** rng.uniform(-1, 0.5), 0.3)
            t = rng.normal(size=3)
            t = t / np.linalg.norm(t) * 10.0 ** rng.uniform(-3, 3) if j % 3 else rng.uniform(-2, 2, 3)
            # (every third pose a signed axis permutation: the world box is then tight on the posed vertices)
            rot = signed_permutations()[rng.randint(48)] if j % 3 == 2 else _rotation(rng, j % 2 == 1)
            insts.append((tris, rng.permutation(30)[:27], _pose(rot, t), fit_like(rng, tris, j % 3)))
        far = (_soup(rng, 30) + F(1000)).astype(F)
        rot = _rotation(rng)
        insts.append((far, np.arange(30), _pose(rot, -rot @ np.full(3, 1000.0)), WB.plain_fit(far)))
        world = WS.SweepWorld(insts)
        wlo, whi = world.lo[np.abs(world.lo).max(axis=1) < 50].min(0), world.hi[np.abs(world.hi).max(axis=1) < 50].max(0)
        half = float((whi - wlo).max()) / 2
        sets = []
        o = rng.uniform(wlo - 1, whi + 1, (1500, 3))
        d = rng.uniform(wlo, whi, (1500, 3)) - o
        sets.append((o.astype(F), d.astype(F), (10.0 ** rng.uniform(-3, np.log10(half), 1500)).astype(F)))
        for inst in insts:
            posed = NQ.posed(np.asarray(inst[0], F)[np.sort(inst[1])], inst[2])
            scale = float(np.abs(posed - posed.mean(axis=(0, 1))).max())
            _, go, gd, gr, _ = _grazing_sweeps(rng, posed, scale, 8)
            sets.append((go, gd, gr))
            sets.append(_extreme_sweeps(rng, inst, 12))
        o, d, r = (np.concatenate([s[k] for s in sets]) for k in range(3))
        tm = np.full(o.shape[0], np.inf, F)
        for j, inst in enumerate(insts):
            contact = WS.pair_contacts(inst, o, d, r, tm)
            counts, out_padded, out_bare, g_alone, g_all, kept = WS.top_figures(world, j, contact, o, d, r)
            assert counts.any(), (seed, j)
            assert kept[counts.any(axis=1)].all(), (seed, j)
            assert (g_all[counts] > 0).all()
            bare, padded = (out_bare / g_all)[counts].max(), (out_padded / np.maximum(g_alone, 2.0 ** -140))[counts].max()
            assert bare <= 0.25, (seed, j, bare)
            assert padded <= 0.25, (seed, j, padded)
            worst_bare, worst_padded, total = max(worst_bare, bare), max(worst_padded, padded), total + int(counts.sum())
    print("triples that count: %d; the largest observed / granted beyond the radius: %.3g without the padding, %.3g against the padded box"
          % (total, worst_bare, worst_padded))
    assert total > 100000


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

WORLD_SWEEP_ENTRIES = ("psm_world_sweep_sphere_dev", "psm_world_sweep_occluded_dev")
WORLD_SWEEP_METHODS = ("sphereCast", "sphereCastOccluded")


def test_library_exports_the_world_sweep_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in WORLD_SWEEP_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(psm_world\* world, const psm_sweep_query\* d_sweeps" % s, header), s
    assert "sweep queries over a world" in header and header.index("sweep queries over a world") > header.index("box queries over a world")
    assert "o' = inst_point(m, origin), d' =\n *     normalize3(inst_rotate(m, direct))" in header
    assert "lexicographically lowest (inst, tri)" in header
    for m in WORLD_SWEEP_METHODS:
        assert callable(getattr(psm.InstanceWorld, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.TriangleHierarchy):
            assert not hasattr(other, m), (other, m)
    assert "sphereCast" in psm.InstanceWorld.__doc__ and "have no sweeps; InstanceWorld has" in psm.TriangleHierarchy.sweepSphere.__doc__
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for m, s in zip(WORLD_SWEEP_METHODS, WORLD_SWEEP_ENTRIES):
        assert re.search(r"int %s\(const psm_sweep_query \*" % m, hpp) and "InstanceWorld::%s(" % m in inl and s + "(world," in inl
    dev = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "psm_world_dev.h")).read()
    assert "int world_sweep_launch(psm_ctx* c, bool any, uint32_t grid, const WorldArgs& a);" in dev
    assert "struct WorldBest {" in dev and "struct WorldRay {" in dev
    world = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "world.hip")).read()
    assert "struct WorldBest {" not in world and "struct WorldRay {" not in world


def test_world_sweep_refusals_that_need_no_device(psm):
    """no world: the code the other world queries give, before anything is looked at; the Python layer refuses mismatched
    arguments before any call is made"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    other = lib.psm_world_intersect_dev(None, None, ctypes.c_size_t(1), None, None)
    assert other != 0
    fn = lib.psm_world_sweep_sphere_dev
    assert fn(None, p, ctypes.c_size_t(1), p, p) == other and fn(None, None, ctypes.c_size_t(0), None, None) == other
    fn = lib.psm_world_sweep_occluded_dev
    assert fn(None, p, ctypes.c_size_t(1), p) == other and fn(None, None, ctypes.c_size_t(0), None) == other
    assert not any(buf)

    class NoCall:   # a world that cannot make a call
        ctx = None
        _scene = True

        def _launch_np(self, packed, out, name, *extra):
            raise AssertionError("a launch was made: %s %s %s" % (packed.shape, out, name))
        _query = psm.InstanceWorld._query
        sphereCast = psm.InstanceWorld.sphereCast
        sphereCastOccluded = psm.InstanceWorld.sphereCastOccluded
    o = np.zeros((3, 3), F)
    for call in (NoCall().sphereCast, NoCall().sphereCastOccluded):
        with pytest.raises(ValueError, match="3 against 2"):
            call(o, o[:2], 0.5)
        with pytest.raises(ValueError):
            call(o, o, np.zeros(2, F))                      # a radius per sweep: [n]
        with pytest.raises(ValueError):
            call(o, o, 0.5, np.zeros(4, F))
        with pytest.raises(TypeError):
            call(o, o)                                      # the radius has no default
    with pytest.raises(AssertionError, match=r"\(3, 8\) hits psm_bvh_sweep_sphere_dev"):      # (_call renames it for a world)
        NoCall().sphereCast(o, o, np.ones(3, F), 2.0)
    with pytest.raises(AssertionError, match=r"\(3, 8\) bool psm_bvh_sweep_occluded_dev"):
        NoCall().sphereCastOccluded(o, o, 0.25)


# The VGPRs and SGPRs each kernel reaches with the Makefile's flags, as ceilings under the 128 of __launch_bounds__(64, 4)
# (hipcc's figures for this code), and the LDS it declares (the 16-entry stack). Neither kernel fits the 80 VGPRs
# of six waves per SIMD, so (64, 6) was not taken.
WORLD_SWEEP_REGS = {"world_query_sweep": (94, 96), "world_query_sweep_any": (89, 80)}


def test_world_sweep_kernels_codegen():
    asm = csrc_asm("world_sweep.hip")
    assert asm.count(".amdhsa_kernel ") == 2
    for name, (vgprs, sgprs) in WORLD_SWEEP_REGS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9WorldArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= vgprs <= 128, (name, meta("vgpr_count"))
        assert meta("sgpr_count") <= sgprs, (name, meta("sgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name
        assert meta("group_segment_fixed_size") == 16 * 64 * 4 == 4096, name      # the stack
        assert "v_fma_mix_f32" in body, name                                      # the slab planes straight from the fp16 record
        assert "v_sqrt_f32" in body and "v_div_scale_f32" in body, name           # correctly rounded division and square root
    makefile = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "Makefile")).read()
    assert re.search(r"^world\.o world_box\.o world_sweep\.o: psm_world_dev\.h$", makefile, re.M)
    assert re.search(r"^sweep\.o world_sweep\.o: psm_sweep_dev\.h$", makefile, re.M)


def test_world_sweep_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "world_sweep_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_sweep_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
