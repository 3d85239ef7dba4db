"""CPU tests (no GPU) of the instance worlds (psm_world_*, world.hip; InstanceWorld): the numpy restatement of
boxes, padding, tree and two-level walk (world_query_model part (b)) answers bit for bit what the flat list answers (part (a)) --
on an adversarial soup, on a grid where it must also cull, on ties --; the padding bound holds with 4x headroom; the exports,
the refusals that need no device, the code generation of the seven kernels and the header layer."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import inside_query_model as IQ
import instance_query_model as NQ
import world_query_model as WQ
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
U = np.uint32


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    if a.dtype == np.float32:
        a, b = a.view(U), b.view(U)
    bad = np.nonzero(np.atleast_1d((a != b).reshape(a.shape[0], -1).any(axis=1)))[0]
    assert bad.size == 0, "%s: %d differ, first %d: %s against %s" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]])


def unit_box(scenes):
    return np.asarray(scenes._box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), F).reshape(-1, 3, 3)


def _shift(x, y, z):
    m = NQ.IDENTITY.copy()
    m[:, 3] = (x, y, z)
    return m


def soup_entries():
    """(mesh index, pose) of the adversarial soup over ONE mesh, the unit box with its triangles in the box's faces, at the
    identity pose and at translations only: touching boxes (shared faces), a box again at the same place, boxes offset by 1e3
    and by 1e-3"""
    shifts = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0), (0, 0, 0), (1e3, 0, 0), (1e3, 1e3, 1e3), (1e-3, 0, 0), (0, 0, 1 + 1e-3),
              (-1, -1, -1), (1e3 + 1, 0, 0)]
    return [(0, _shift(*s)) for s in shifts]


def soup_queries():
    """rays (o, d, tmin, tmax) and points p of the soup: axis-aligned rays along faces and edges, rays starting on a face,
    points on faces, the same offset by 1e3 and 1e-3"""
    o, d = [], []
    for base in ((0, 0, 0), (1e3, 0, 0), (1e-3, 0, 0)):
        b = np.asarray(base, np.float64)
        for ax in range(3):
            e = np.eye(3)[ax]
            for u in (0.0, 1.0, 0.5, 0.25):
                for v in (0.0, 1.0, 0.5):
                    s = np.zeros(3)
                    s[(ax + 1) % 3], s[(ax + 2) % 3] = u, v
                    for sign in (1.0, -1.0):
                        o.append(b + s - 3.0 * sign * e)      # along a face (u or v in {0, 1}), an edge (both) or through
                        d.append(sign * e)
                        o.append(b + s)                       # starting on a face
                        d.append(sign * e)
                        o.append(b + s + 0.5 * e)             # starting inside, in a face plane of the neighbours
                        d.append(sign * e)
    rng = np.random.RandomState(5)
    o += list(rng.uniform(-1, 3, (64, 3)))
    d += list(rng.normal(size=(64, 3)))
    o, d = np.asarray(o, F), np.asarray(d, F)
    p = np.concatenate([o, (o + F(0.5) * d).astype(F)])
    return o, d, p


@functools.lru_cache(maxsize=None)
def soup_case():
    """the soup with its flat answers: the windows and radii of the second pass sit exactly at a candidate's value"""
    scenes = __import__("importlib").import_module("prismarine-core_amd.scenes")
    box = unit_box(scenes)
    cand = np.arange(box.shape[0], dtype=np.int32)
    insts = [(box, cand, m) for _, m in soup_entries()]
    o, d, p = soup_queries()
    n = o.shape[0]
    per = WQ.per_instance_rays(insts, o, d, np.full(n, 0, F), np.full(n, np.inf, F))
    hits = WQ.flat_rays(per)[0]
    t = hits[:, 2].copy()
    tmin, tmax = np.zeros(n, F), np.full(n, np.inf, F)
    k = np.isfinite(t)
    tmax[k] = t[k]                                      # tmax exactly at the closest candidate's t
    tmin[k & (np.arange(n) % 2 == 0)] = t[k & (np.arange(n) % 2 == 0)]   # ... and the window a single value
    pp = WQ.per_instance_points(insts, p, np.full(p.shape[0], np.inf, F))
    dist = WQ.flat_points(pp)[0][:, 2].copy()
    rmax = np.where(np.arange(p.shape[0]) % 3 == 0, F(0.25), dist).astype(F)   # rmax exactly at the closest distance
    return box, insts, (o, d, tmin, tmax), (p, rmax)


def check_world_model(insts, rays, points, samples=(3,)):
    """(b) == (a) bit for bit on every kind; returns the entered lists by kind"""
    w = WQ.World(insts)
    o, d, tmin, tmax = rays
    n = o.shape[0]
    lo, hi = np.broadcast_to(np.asarray(tmin, F), (n,)).copy(), np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    per = WQ.per_instance_rays(insts, o, d, lo, hi)
    eh, ei, ea, ec = WQ.flat_rays(per)
    (gh, gi), ga, gc, ent_r = w.rays(o, d, lo, hi, per)
    _same(gh, eh, "intersect")
    _same(gi, ei, "intersect inst")
    _same(ga, ea, "occluded")
    _same(gc, ec, "countHits")
    p, rmax = points
    rm = np.broadcast_to(np.asarray(rmax, F), (p.shape[0],)).copy()
    pp = WQ.per_instance_points(insts, p, rm)
    ph, pi, pw = WQ.flat_points(pp)
    (qh, qi), qw, ent_p = w.points(p, rm, pp)
    _same(qh, ph, "closestPoint")
    _same(qi, pi, "closestPoint inst")
    _same(qw, pw, "within")
    par = WQ.per_instance_parities(insts, p, max(samples))
    gpar, ent_i = w.parities(p, max(samples), par)
    _same(gpar, WQ.flat_parities(par), "inside parities")
    return {"closest": ent_r[0], "any": ent_r[1], "count": ent_r[2], "point": ent_p[0], "within": ent_p[1], "inside": ent_i[0]}


def test_model_walk_equals_the_flat_answer_on_the_adversarial_soup():
    _, insts, rays, points = soup_case()
    o, d, tmin, tmax = rays
    check_world_model(insts, (o, d, np.zeros_like(tmin), np.full_like(tmax, np.inf)), (points[0], np.full_like(points[1], np.inf)))
    ent = check_world_model(insts, rays, points)
    assert WQ.average_entered(ent["closest"]) < len(insts)   # and it is a cull, not a pass-through


def test_model_ties_go_to_the_lowest_instance_wherever_it_sits_in_the_tree():
    """one hierarchy twice (and thrice) at one pose, at indices far apart in the list and in tree order"""
    box, _, rays, points = soup_case()
    cand = np.arange(box.shape[0], dtype=np.int32)
    far = [_shift(5 + 3 * k, 7 * (k % 3), -4 * k) for k in range(9)]
    poses = [far[0], far[1], far[2], _shift(0, 0, 0), far[3], far[4], far[5], far[6], _shift(0, 0, 0), far[7], far[8], _shift(0, 0, 0)]
    insts = [(box, cand, m) for m in poses]
    o, d, tmin, tmax = rays
    w = WQ.World(insts)
    (h, inst), _, _, _ = w.rays(o, d, np.zeros_like(tmin), np.full_like(tmax, np.inf))
    (ph, pinst), _, _ = w.points(points[0], np.full_like(points[1], np.inf))
    assert (inst >= 0).sum() > 100 and not np.isin(inst, (8, 11)).any() and (inst == 3).any()
    assert not np.isin(pinst, (8, 11)).any()
    check_world_model(insts, rays, points)


def grid_case(side=16, queries=96, seed=3):
    """side x side separated bodies (a 20-triangle icosphere of radius 0.3 at random rigid poses on a grid of pitch 2) and local
    queries: short rays and small radii around random bodies"""
    rng = np.random.RandomState(seed)
    ico = IQ.icosphere(0, 0.3)
    cand = np.arange(ico.shape[0], dtype=np.int32)
    insts = []
    for k in range(side * side):
        m = NQ.random_pose(rng, reflect=bool(k & 1), shift=0.0)
        m[:, 3] = (2.0 * (k % side), 2.0 * (k // side), 0.0)
        insts.append((ico, cand, m))
    at = rng.randint(0, side * side, queries)
    c = np.asarray([insts[k][2][:, 3] for k in at], F)
    o = (c + rng.uniform(-1, 1, (queries, 3))).astype(F)
    d = (c + rng.uniform(-0.3, 0.3, (queries, 3)) - o).astype(F)
    tmin, tmax = np.zeros(queries, F), rng.uniform(0.5, 3.0, queries).astype(F)
    p = (c + rng.uniform(-0.6, 0.6, (queries, 3))).astype(F)
    rmax = rng.uniform(0.1, 1.0, queries).astype(F)
    return insts, (o, d, tmin, tmax), (p, rmax)


def test_model_culls_on_a_grid_of_separated_bodies():
    insts, rays, points = grid_case()
    ent = check_world_model(insts, rays, points)
    for kind, e in ent.items():
        assert WQ.average_entered(e) <= 8.0, (kind, WQ.average_entered(e))


def test_padding_bound_has_four_times_headroom():
    """10 000 random poses and queries: the observed distance between a world point and the world image of its float32 move stays
    under the derived bound, and the derived bound under a quarter of what the padding and the query slack grant"""
    rng = np.random.RandomState(11)
    worst = 0.0
    for k in range(10000):
        scale = 10.0 ** rng.uniform(-3, 3)
        m = NQ.random_pose(rng, reflect=bool(k & 1), shift=scale)
        x = (m[:, 3] + rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-3, 3)).astype(F)
        seen, objmag = WQ.move_discrepancy(m, x)
        bound = WQ.move_bound(m, x, objmag)
        granted = float(WQ.WORLD_PAD) * max(objmag, float(np.abs(m[:, 3]).max())) + float(WQ.WORLD_QSLACK) * float(np.abs(x).max())
        assert seen <= bound, (k, seen, bound)
        assert bound <= 0.25 * granted, (k, bound, granted)
        worst = max(worst, seen / granted)
    assert worst < 0.25
    # the distances: |R^T d| = 1 +- 1.5e-5 under the pose check; the slacks hold it 4 times over (and more)
    assert 4 * 1.5e-5 <= float(WQ.WORLD_TSLACK) and 4 * 3e-5 <= float(WQ.WORLD_PSLACK)


def test_model_tree_is_a_tree_and_its_boxes_nest():
    insts, _, _ = grid_case(side=6, queries=1)
    w = WQ.World(insts)
    seen = []

    def down(link):   # -> lo, hi of the subtree
        if link < 0:
            seen.append(~link)
            return w.lo[~link], w.hi[~link]
        loL, hiL, lL, loR, hiR, lR = w.tree.nodes[link]
        a, b = down(lL), down(lR)
        assert np.array_equal(a[0], loL) and np.array_equal(a[1], hiL) and np.array_equal(b[0], loR) and np.array_equal(b[1], hiR)
        return np.fmin(loL, loR), np.fmax(hiL, hiR)
    down(0)
    assert sorted(seen) == list(range(36)) and len(w.tree.nodes) == 35 and 6 <= w.tree.depth <= 35
    assert (w.lo < w.hi).all()


# ---- host and build checks ------------------------------------------------------------------------------------------------------------

WORLD_EXPORTS = ["psm_world_create", "psm_world_destroy", "psm_world_set_instances", "psm_world_set_transforms", "psm_world_count"] + [
    "psm_world_%s_dev" % k for k in ("intersect", "occluded", "count_hits", "closest_point", "within", "inside", "signed_distance")]


def test_world_exports_and_python_surface(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for name in WORLD_EXPORTS:
        assert hasattr(lib, name) and name in psm.EXPORTS and re.search(r"\b%s\(" % name, header), name
    assert "#define PSM_WORLD_MAX_INSTANCES 65536" in header and psm.WORLD_MAX_INSTANCES == 65536
    assert psm.INSTANCE_DT.itemsize == ctypes.sizeof(psm.Instance) == 56
    for m in ("intersect", "occluded", "countHits", "closestPoint", "within", "inside", "signedDistance", "setTransform", "setTransforms",
              "transforms", "__len__", "setInstances", "refresh", "close"):
        assert callable(getattr(psm.InstanceWorld, m)), m


def test_world_refusals_that_need_no_device(psm):
    lib = psm.lib()
    INVALID = -1 if not hasattr(psm, "ERR_INVALID") else psm.ERR_INVALID
    assert lib.psm_world_create(None, ctypes.c_uint32(4)) is None
    assert lib.psm_world_count(None) == 0
    rcs = [lib.psm_world_destroy(None), lib.psm_world_set_instances(None, None, ctypes.c_uint32(0)),
           lib.psm_world_set_transforms(None, ctypes.c_uint32(0), ctypes.c_uint32(0), None)]
    for name in WORLD_EXPORTS[5:]:
        extra = (ctypes.c_uint32(3),) if name in ("psm_world_inside_dev", "psm_world_signed_distance_dev") else ()
        tail = (None,) if name in ("psm_world_intersect_dev", "psm_world_closest_point_dev", "psm_world_signed_distance_dev") else ()
        rcs.append(getattr(lib, name)(None, None, ctypes.c_size_t(1), *extra, None, *tail))
    assert all(rc != 0 for rc in rcs) and len(set(rcs)) == 1, rcs
    with pytest.raises(ValueError):   # the poses are checked before the library is asked
        bad = NQ.IDENTITY.copy()
        bad[0, 0] = 2.0
        psm._pose(bad, "InstanceWorld")


# the VGPRs each world kernel may reach with the Makefile's flags (closest / any / point / within / count / inside / sign). The
# lane's own hierarchy pointers and the world ray beside the object ray do not fit the 64 of the other families: the kernels are
# built with __launch_bounds__(64, 4), whose budget is 128
WORLD_KINDS = ("closest", "any", "point", "within", "count", "inside", "sign")
WORLD_VGPRS = dict(zip(WORLD_KINDS, (72, 68, 82, 78, 68, 66, 68)))


def test_world_kernels_codegen():
    asm = csrc_asm("world.hip")
    for kind, ceiling in WORLD_VGPRS.items():
        name = "world_query_" + kind
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9WorldArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= 128, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the 16 stack entries per lane in LDS
        assert meta("kernarg_segment_size") <= 88 + 256, name                 # (with the hidden arguments) the table is in memory
        if kind not in ("point", "within"):
            assert "v_fma_mix_f32" in body, name


def _kernel_digests(asm_path):
    """{kernel: sha256 of its normalised instruction stream and sizes}, by tools/kernel_diff.py's reading of the assembly"""
    import hashlib
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    return {name: hashlib.sha256(("\n".join(lines) + repr(sorted(sizes.items()))).encode()).hexdigest()
            for name, (lines, sizes) in kd.kernels(asm_path).items()}


def test_the_21_kernels_of_query_hip_are_unchanged(tmp_path):
    """query.hip's 21 kernels' instruction streams and sizes are those recorded from the commit before the worlds
    (tests/golden/query_kernels_before_worlds.json: tools/kernel_diff.py's normal form, hashed), whatever has moved between the
    file and the headers it shares with kbest.hip and world.hip since. The 15 ray kernels' digests were recorded anew when
    ray_axis's margin grew by 2^-12 (psm_query_dev.h, DESIGN.md 4.5: the one change of their code since); the 6 point kernels'
    are the first recording's."""
    import json
    out = tmp_path / "query.s"
    out.write_text(csrc_asm("query.hip"))
    now = _kernel_digests(str(out))
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "query_kernels_before_worlds.json")))
    assert len(before) == 21 and set(now) == set(before)
    assert [k for k in before if now[k] != before[k]] == []


def test_world_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "world_header")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_header.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
