"""CPU tests (no GPU) of the k-best queries of an instance world (psm_world_first_hits_dev / psm_world_nearest_dev, world.hip;
InstanceWorld.firstHits / nearest): the model (tests/world_kbest_query_model.py: per-instance rows merged by
(value, inst, tri)) at k = 1 is the flat answer of world_query_model bit for bit, its rows are prefixes of one another and
sorted, its counts are min(k, flat count), and ties across instances and triangles are listed by id; the library exports both
entry points, the two kernels compile within their ceilings, the 16 older kernels of kbest.hip and world.hip are the parent
commit's, the header layer compiles, and the list's insertion runs against std::sort under the sanitizers on the host."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np

import instance_query_model as NQ
import world_kbest_query_model as WK
import world_query_model as WQ
from test_gpu_world_query import _meshes, _posed_entries, _queries
from test_world_query_cpu import _kernel_digests, _same, _shift, soup_case
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
U = np.uint32
KMAX = 16


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, insts, (o, d, tmin, tmax), (p, rmax))]: the adversarial soup of test_world_query_cpu with its windows and radii
    exactly at a candidate's value, and the posed entries and queries of test_gpu_world_query at 2 and 33 instances"""
    _, insts, rays, points = soup_case()
    out = [("soup", insts, rays, points)]
    ico, tor = _meshes()
    meshes = [(ico, np.arange(ico.shape[0], dtype=np.int32)), (tor, np.arange(tor.shape[0], dtype=np.int32))]
    for n in (2, 33):
        entries, spread = _posed_entries(n, 100 + n)
        rays, points = _queries(np.random.RandomState(n), spread, 300)
        out.append(("posed %d" % n, [(meshes[k][0], meshes[k][1], m) for k, m in entries], rays, points))
    return out


@functools.lru_cache(maxsize=None)
def rows_at(which, k):
    """the model's (ray rows, inst, count), (point rows, inst, count) of case `which` at k -- computed once, never changed"""
    _, insts, (o, d, tmin, tmax), (p, rmax) = cases()[which]
    return WK.first_hits(insts, o, d, k, tmin, tmax), WK.nearest(insts, p, k, rmax)


@functools.lru_cache(maxsize=None)
def flat(which):
    _, insts, (o, d, tmin, tmax), (p, rmax) = cases()[which]
    n = o.shape[0]
    lo, hi = np.broadcast_to(np.asarray(tmin, F), (n,)).copy(), np.broadcast_to(np.asarray(tmax, F), (n,)).copy()
    rm = np.broadcast_to(np.asarray(rmax, F), (p.shape[0],)).copy()
    pp = WQ.per_instance_points(insts, p, rm)
    # the flat count of a point: the triangles of every instance within rmax, by the brute force of the per-instance k-best
    # model at a k no instance reaches (its counts are min(k, count): test_kbest_query_cpu)
    big = max(t.shape[0] for t, _, _ in insts)
    pc = np.sum([WK.KQ.nearest(t, c, NQ.move(m, p), big, rm)[1] for t, c, m in insts], axis=0, dtype=U)
    return WQ.flat_rays(WQ.per_instance_rays(insts, o, d, lo, hi)), WQ.flat_points(pp), pc


def test_model_at_k_1_is_the_flat_world_answer():
    for which, (name, _, _, _) in enumerate(cases()):
        (eh, ei, ea, ec), (ph, pi, pw), _ = flat(which)
        for k in (1, KMAX):
            (rows, inst, count), (prows, pinst, pcount) = rows_at(which, k)
            _same(rows[:, 0], eh, "%s: first hits slot 0, k = %d" % (name, k))
            _same(inst[:, 0], ei, "%s: first hits inst 0, k = %d" % (name, k))
            assert np.array_equal(count > 0, ea), name
            _same(prows[:, 0], ph, "%s: nearest slot 0, k = %d" % (name, k))
            _same(pinst[:, 0], pi, "%s: nearest inst 0, k = %d" % (name, k))
            assert np.array_equal(pcount > 0, pw), name
        assert (ei >= 0).sum() > 20 and (pi >= 0).sum() > 20, name


def test_model_rows_are_prefixes_sorted_and_counted():
    for which, (name, insts, _, _) in enumerate(cases()):
        (_, _, _, ec), _, pc = flat(which)
        (big, binst, bcount), (pbig, pbinst, pbcount) = rows_at(which, KMAX)
        for k in (1, 3):
            (rows, inst, count), (prows, pinst, pcount) = rows_at(which, k)
            _same(rows, big[:, :k], "%s: first hits prefix k = %d" % (name, k))
            _same(inst, binst[:, :k], "%s: first hits inst prefix k = %d" % (name, k))
            _same(prows, pbig[:, :k], "%s: nearest prefix k = %d" % (name, k))
            _same(pinst, pbinst[:, :k], "%s: nearest inst prefix k = %d" % (name, k))
            assert np.array_equal(count, np.minimum(ec, k)) and np.array_equal(pcount, np.minimum(pc, k)), (name, k)
        assert np.array_equal(bcount, np.minimum(ec, KMAX)) and np.array_equal(pbcount, np.minimum(pc, KMAX)), name
        # ascending in (t, inst, tri); a point's rows in (dist, ...) only weakly: two d2 may share a sqrtf
        t, tri, ins = big[:, :, 2], big.view(np.int32)[:, :, 3].astype(np.int64) & 0xffffffff, binst.astype(np.int64) & 0xffffffff
        live = np.arange(KMAX)[None, 1:] < bcount[:, None]
        with np.errstate(invalid="ignore"):
            eq = t[:, :-1] == t[:, 1:]
            asc = (t[:, :-1] < t[:, 1:]) | (eq & (ins[:, :-1] < ins[:, 1:])) | (eq & (ins[:, :-1] == ins[:, 1:]) & (tri[:, :-1] < tri[:, 1:]))
        assert (asc | ~live).all(), name
        plive = np.arange(KMAX)[None, 1:] < pbcount[:, None]
        assert ((pbig[:, :-1, 2] <= pbig[:, 1:, 2]) | ~plive).all(), name
        # the miss slots: {0, 0, +inf, -1} and inst = -1, exactly from the count on
        for rows, inst, count in ((big, binst, bcount), (pbig, pbinst, pbcount)):
            dead = np.arange(KMAX)[None] >= count[:, None]
            assert np.array_equal(rows.view(np.int32)[:, :, 3] < 0, dead) and np.array_equal(inst < 0, dead), name
            assert np.isinf(rows[:, :, 2][dead]).all() and not rows[:, :, :2][dead].any(), name
        if len(insts) > 2:   # (two bodies in a wide space: few rays meet three triangles)
            assert (bcount >= 3).sum() > 10 and (pbcount >= 3).sum() > 10, name


def test_model_ties_across_instances_are_listed_by_instance():
    """one mesh at one pose three times: every hit comes three times at a bit-equal value, inst 0, 1, 2; k cuts the group"""
    ico, _ = _meshes()
    cand = np.arange(ico.shape[0], dtype=np.int32)
    pose = NQ.random_pose(np.random.RandomState(3), shift=0.5)
    insts = [(ico, cand, pose)] * 3
    rng = np.random.RandomState(4)
    o = (pose[:, 3] + rng.uniform(-2, 2, (64, 3))).astype(F)
    d = (pose[:, 3] + rng.uniform(-0.3, 0.3, (64, 3)) - o).astype(F)
    rows, inst, count = WK.first_hits(insts, o, d, KMAX)
    assert (count >= 6).sum() > 30 and (count % 3 == 0).all()
    for s in range(0, 6, 3):
        full = count >= s + 3
        assert (inst[full, s:s + 3] == [0, 1, 2]).all()
        grp = rows[full, s:s + 3]
        assert (grp.view(U) == grp.view(U)[:, :1]).all()            # the three records of a group are bit-equal
    cut, cinst, ccount = WK.first_hits(insts, o, d, 4)
    full = count >= 6
    assert (ccount[full] == 4).all() and (cinst[full] == [0, 1, 2, 0]).all()
    _same(cut, rows[:, :4], "k = 4 cuts the second group")
    # points: rmax exactly at the closest distance, so a row holds the triangles that meet at the closest point (a face, an edge,
    # a vertex of the icosphere: 1, 2 or 5, fewer where their d2 round apart), each three times, inst ascending
    dist = WK.nearest(insts, o, 1)[0][:, 0, 2].copy()
    prows, pinst, pcount = WK.nearest(insts, o, KMAX, dist)
    ptri = prows.view(np.int32)[:, :, 3]
    assert (pcount % 3 == 0).all() and (pcount >= 3).all() and (pcount > 3).any() and (pcount < KMAX).all()
    for i in range(o.shape[0]):
        for t in set(ptri[i, :pcount[i]]):
            at = np.nonzero(ptri[i, :pcount[i]] == t)[0]
            assert list(pinst[i, at]) == [0, 1, 2] and (prows.view(U)[i, at] == prows.view(U)[i, at[0]]).all()
    cut, cinst, ccount = WK.nearest(insts, o, 4, dist)
    _same(cut, prows[:, :4], "nearest: k = 4 cuts a group")
    _same(cinst, pinst[:, :4], "nearest: k = 4 cuts a group, inst")


def test_model_ties_across_instances_and_triangles_and_the_zeros():
    """two meshes that hold the same triangle under different ids, at one pose, interleaved: (value, inst, tri) with the
    instance before the triangle; a ray that starts on the plane of two coincident triangles of opposite winding has t = +0 in
    one and -0 in the other, and the lower (inst, tri) still comes first"""
    tri = np.array([[[1, -1, -1], [1, 1, -1], [1, 0, 1]]], F)
    a = np.concatenate([tri, tri + F([1, 0, 0]), tri])              # ids 0 and 2 coincide
    b = np.concatenate([tri + F([1, 0, 0]), tri])                   # id 1 is the same triangle again
    insts = [(a, [0, 1, 2], NQ.IDENTITY), (b, [0, 1], NQ.IDENTITY), (a, [0, 1, 2], NQ.IDENTITY)]
    o, d = np.zeros((1, 3), F), F([[1, 0, 0]])
    rows, inst, count = WK.first_hits(insts, o, d, KMAX)
    assert count[0] == 8
    assert list(zip(inst[0, :8], rows.view(np.int32)[0, :8, 3])) == [(0, 0), (0, 2), (1, 1), (2, 0), (2, 2), (0, 1), (1, 0), (2, 1)]
    rows, inst, count = WK.first_hits(insts, o, d, 4)
    assert count[0] == 4 and list(zip(inst[0], rows.view(np.int32)[0, :, 3])) == [(0, 0), (0, 2), (1, 1), (2, 0)]
    prows, pinst, pcount = WK.nearest(insts, o, 3)
    assert list(zip(pinst[0], prows.view(np.int32)[0, :, 3])) == [(0, 0), (0, 2), (1, 1)]
    flip = tri[:, [0, 2, 1]]
    both = [(flip, [0], NQ.IDENTITY), (tri, [0], NQ.IDENTITY), (np.concatenate([tri, flip]), [0, 1], NQ.IDENTITY)]
    rows, inst, count = WK.first_hits(both, F([[1, 0, 0]]), d, 4, -1.0, 1.0)
    assert count[0] == 4 and (rows[0, :, 2] == 0).all() and len(set(np.signbit(rows[0, :, 2]))) == 2
    assert list(zip(inst[0], rows.view(np.int32)[0, :, 3])) == [(0, 0), (1, 0), (2, 0), (2, 1)]


WORLD_KBEST_EXPORTS = ("psm_world_first_hits_dev", "psm_world_nearest_dev")


def test_library_exports_the_world_kbest_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in WORLD_KBEST_EXPORTS:
        assert hasattr(lib, s) and s in psm.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert callable(psm.InstanceWorld.firstHits) and callable(psm.InstanceWorld.nearest)
    for flat_list in (psm.QueryScene, psm.InstancedScene):          # the flat lists have no k-best query
        assert not hasattr(flat_list, "firstHits") and not hasattr(flat_list, "nearest")
    lists = psm.QueryHitLists(np.zeros((3, 4, 4), F), np.zeros(3, U))
    assert lists.geom is None and lists.t.shape == (3, 4) and len(lists) == 3
    lists = psm.QueryHitLists(np.zeros((3, 4, 4), F), np.zeros(3, U), np.zeros((3, 4), np.int32))
    assert lists.geom.shape == (3, 4) and lists.tri.dtype == np.int32


def test_world_kbest_refusals_that_need_no_device(psm):
    """no world: the code the other world queries give, before anything is looked at"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    other = lib.psm_world_intersect_dev(None, None, ctypes.c_size_t(1), None, None)
    assert other != 0
    for s in WORLD_KBEST_EXPORTS:
        fn = getattr(lib, s)
        assert fn(None, p, ctypes.c_size_t(1), ctypes.c_uint32(1), p, p, p) == other
        assert fn(None, None, ctypes.c_size_t(0), ctypes.c_uint32(0), None, None, None) == other
        assert fn(None, p, ctypes.c_size_t(1), ctypes.c_uint32(17), p, p, p) == other


# The VGPRs the two kernels reach with the Makefile's flags (the ceilings), under the 128 of __launch_bounds__(64, 4), and the
# LDS they declare: the 16-entry stack; the list is dynamic, k x 768 B, and does not show here
WORLD_KBEST_VGPRS = {"world_query_first_hits": 88, "world_query_nearest": 89}


def test_world_kbest_kernels_codegen():
    asm = csrc_asm("world.hip")
    for name, ceiling in WORLD_KBEST_VGPRS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_9WorldArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= 128, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4 == 4096, name  # the stack; the list is the launch's k x 64 x 12 B
        if name == "world_query_first_hits":
            assert "v_fma_mix_f32" in body, name
    # by LDS alone a CU's 160 KB hold 33 / 22 / 16 / 10 waves at k = 1 / 4 / 8 / 16 (the kernels ask for 16)
    assert [160 * 1024 // (4096 + k * 64 * 12) for k in (1, 4, 8, 16)] == [33, 22, 16, 10]


def test_the_16_kernels_of_kbest_hip_and_world_hip_are_unchanged(tmp_path):
    """the instruction streams and sizes of kbest.hip's 2 and world.hip's 14 kernels are those recorded from the commit before the
    world's k-best queries (tests/golden/world_kbest_kernels_before.json: tools/kernel_diff.py's normal form, hashed). The digests
    of the 6 ray kernels among them (bvh_query_first_hits and the world's five) were recorded anew when ray_axis's margin grew by
    2^-12 (psm_query_dev.h, DESIGN.md 4.5: the one change of their code since); the 10 others' are the first recording's."""
    now = {}
    for src in ("kbest.hip", "world.hip"):
        out = tmp_path / src.replace(".hip", ".s")
        out.write_text(csrc_asm(src))
        now.update(_kernel_digests(str(out)))
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "world_kbest_kernels_before.json")))
    assert len(before) == 16 and set(before) <= set(now)
    assert [k for k in before if now[k] != before[k]] == []
    assert sorted(k for k in now if k not in before) == ["_ZN3psm19world_query_nearestENS_9WorldArgsE", "_ZN3psm22world_query_first_hitsENS_9WorldArgsE"]


def test_world_kbest_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "world_kbest_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_kbest_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)


def test_the_list_against_std_sort_under_the_sanitizers(tmp_path):
    """the kernels' own list (psm_world_klist.h) as a stand-alone host program with its own main, built with the address and
    undefined-behaviour sanitizers and run as a process of its own on the CPU: k = 1 .. 16, ties in every key word, -0, a list
    of exactly k slots"""
    exe = str(tmp_path / "world_klist_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "world_klist_host.cpp"), "-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0 and b" 0 bad" in done.stdout, done.stdout.decode(errors="replace")
