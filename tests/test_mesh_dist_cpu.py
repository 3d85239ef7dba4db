"""CPU tests (no GPU) of mesh clearance (psm_bvh_mesh_closest_dev / psm_bvh_mesh_within_dev / psm_bvh_mesh_clearance_dev,
mesh_dist.hip; TriangleHierarchy.meshClosest / meshWithin / meshClearance): the model
(tests/mesh_dist_query_model.py) on a lattice where all arithmetic is exact; the ties; the protocol around the shared word under
a few hundred random schedules; the word's packing, compiled for the host under the sanitizers; the exports, the header text, the
Python surface and the refusals that need no hierarchy; what mesh_dist.hip compiles to; and the header layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_dist_query_model as MD
import mesh_query_model as MQ
import tri_dist_query_model as TD
from point_query_model import _split
from test_gpu_mesh_query import POINT, lattice_case, lattice_soup, rotations, _pose
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
I = np.int32
MISS = [0.0, 0.0, np.inf, -1, 0.0, 0.0, -1, 0.0]   # u, v, dist, tri, s, t, other, 0 of a pose where no pair counts


def _is_miss(rec):
    return [rec[0], rec[1], rec[2], rec.view(I)[3], rec[4], rec[5], rec.view(I)[6], rec[7]] == MISS


def live(tris):
    """the triangles a build keeps, as far as these tests' inputs go: all but those with three equal vertices"""
    t = np.asarray(tris).reshape(-1, 3, 3)
    return np.nonzero(~((t[:, 0] == t[:, 1]).all(axis=1) & (t[:, 0] == t[:, 2]).all(axis=1)))[0]


# ---- the lattice: every operation exact ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lattice():
    tris, otris, poses = lattice_case()
    leaves, oleaves = live(tris), live(otris)
    assert oleaves.size == 130 and 130 not in oleaves
    return tris, leaves, otris, oleaves, poses, {r: MD.query(tris, leaves, otris, oleaves, poses, r) for r in (0.0, 0.125, 0.5, np.inf)}


def test_lattice_clearance_is_the_minimum_of_the_records(lattice):
    tris, leaves, otris, oleaves, poses, by_r = lattice
    for r, (hits, rec, within) in by_r.items():
        assert hits.shape == (6, 131, 8) and rec.shape == (6, 8) and within.shape == (6,)
        assert (hits.view(I)[:, 130, 3] == -1).all() and np.isinf(hits[:, 130, 2]).all()          # the dropped triangle
        for q in range(6):
            found = np.nonzero(hits.view(I)[q, :, 3] >= 0)[0]
            if found.size == 0:
                assert _is_miss(rec[q]) and not within[q]
                continue
            keys = [MD.key_of(hits[q, t, 2], t) for t in found]
            t_star = int(found[int(np.argmin(keys))])
            assert rec.view(I)[q, 6] == t_star and min(keys) == MD.key_of(rec[q, 2], t_star)
            assert np.array_equal(rec[q, :6].view(np.uint32), hits[q, t_star, :6].view(np.uint32)) and rec[q, 7] == 0
            assert within[q] and rec[q, 2] <= F(r)
            # the witness points are that far apart: exact on the lattice up to the division in the weights
            a, b = TD.points_of(tris, MQ.posed(otris, poses)[q, t_star][None], rec[q:q + 1])
            assert abs(np.linalg.norm(a[0].astype(np.float64) - b[0]) - rec[q, 2]) <= 1e-5
    inf = by_r[np.inf]
    assert inf[2].all() and (inf[1][:, 2] == 0).sum() >= 3 and (inf[1][:, 2] > 0).sum() >= 2       # poses that cut, poses out of reach
    assert not by_r[0.5][2].all() and by_r[0.0][2].sum() >= 3


def test_lattice_within_is_the_clearance_predicate(lattice):
    tris, leaves, otris, oleaves, poses, by_r = lattice
    for r, (hits, rec, within) in by_r.items():
        assert np.array_equal(within, rec.view(I)[:, 3] >= 0)
        assert np.array_equal(within, (hits.view(I)[:, :, 3] >= 0).any(axis=1))
        assert np.array_equal(within, by_r[np.inf][1][:, 2] <= F(r))                               # the pose's clearance decides
    for bad in (np.nan, -1.0):
        hits, rec, within = MD.query(tris, leaves, otris, oleaves, poses[:2], bad)
        assert not within.any() and all(_is_miss(x) for x in rec) and (hits.view(I)[:, :, 3] == -1).all()


# ---- ties ------------------------------------------------------------------------------------------------------------------------

def tie_cases():
    """[(name, tris, otris, poses, (tri, other) expected at pose 0)]: a triangle loaded twice into other -- the lower t wins --,
    a triangle loaded twice into bvh -- the lower tri wins --, and a triangle of other without an area lying ON bvh's mesh, which
    its build drops: it never wins. All on a lattice, at the identity and a shifted pose."""
    base = F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[2, 2, 0], [3, 2, 0], [2, 3, 0]], [[-2, 0, 1], [-2, 1, 1], [-3, 0, 1]]])
    near = F([[[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.75]]])                   # 0.5 above triangle 0
    far = F([[[5, 5, 5], [6, 5, 5], [5, 6, 5]]])
    poses = [np.eye(3, 4), _pose(np.eye(3), [0, 0, 0.25])]
    on_mesh = np.repeat(F([[[0.25, 0.25, 0]]]), 3, axis=1)                 # a point of triangle 0: no area, no leaf
    return [("other twice", base, np.concatenate([far, near, far, near]), poses, (0, 1)),
            ("bvh twice", np.concatenate([base[1:2], base[:1], base[2:], base[:1]]), np.concatenate([far, near]), poses, (1, 1)),
            ("dropped", base, np.concatenate([on_mesh, far, near, on_mesh]), poses, (0, 2))]


@pytest.mark.parametrize("case", tie_cases(), ids=lambda c: c[0])
def test_ties_go_to_the_lowest_id(case):
    name, tris, otris, poses, (tri, other) = case
    hits, rec, within = MD.query(tris, live(tris), otris, live(otris), poses)
    assert within.all()
    assert list(rec.view(I)[:, 3]) == [tri, tri] and list(rec.view(I)[:, 6]) == [other, other]
    assert list(rec[:, 2]) == [0.5, 0.75]
    if name == "other twice":
        assert np.array_equal(hits[:, 1].view(np.uint32), hits[:, 3].view(np.uint32))             # the same record twice
    if name == "dropped":
        assert (hits.view(I)[:, [0, 3], 3] == -1).all() and live(otris).tolist() == [1, 2]


# ---- the protocol ----------------------------------------------------------------------------------------------------------------

def _pair_dists(tris, leaves, otris, oleaves, poses, rmax):
    """per pose {t: the float32 dists of t's candidates that count, by ascending id}"""
    q = MQ.posed(otris, poses)
    v0, e1, e2 = _split(np.asarray(tris, F).reshape(-1, 3, 3)[leaves])
    out = []
    for qq in range(q.shape[0]):
        lanes = {}
        for t in oleaves:
            d2 = TD.tri_dist(v0, e1, e2, q[qq, t][None, 0], q[qq, t][None, 1], q[qq, t][None, 2])[0]
            with np.errstate(invalid="ignore"):
                d = np.sqrt(d2)
            lanes[int(t)] = [x for x in d if x <= F(rmax)]
        out.append(lanes)
    return out


def test_protocol_reaches_the_reduction_under_every_schedule():
    """Lanes in shuffled order, each reading a randomly stale snapshot of the word, publishing early or late: the final word is
    (the smallest dist, t*) of the model's reduction on every schedule"""
    rng = np.random.RandomState(5)
    soup = (rng.uniform(-1, 1, (60, 1, 3)) + rng.uniform(-0.2, 0.2, (60, 3, 3))).astype(F)
    osoup = (rng.uniform(-1, 1, (24, 1, 3)) + rng.uniform(-0.2, 0.2, (24, 3, 3))).astype(F)
    sposes = [_pose(r, t) for r, t in zip(rotations(rng, 3), [[0, 0, 0], [3, 0, 0], [0.2, -0.1, 0.4]])]
    cases = [(c[1], c[2], c[3], np.inf) for c in tie_cases()] + [(soup, osoup, sposes, np.inf), (soup, osoup, sposes, 0.05)]
    schedules = 0
    for tris, otris, poses, rmax in cases:
        leaves, oleaves = live(tris), live(otris)
        _, rec, _ = MD.query(tris, leaves, otris, oleaves, poses, rmax)
        for q, lanes in enumerate(_pair_dists(tris, leaves, otris, oleaves, poses, rmax)):
            want = MD.NONE if rec.view(I)[q, 3] < 0 else MD.key_of(rec[q, 2], rec.view(I)[q, 6])
            for seed in range(40):
                srng = np.random.RandomState(1000 * seed + q)
                order = {t: [lanes[t][k] for k in srng.permutation(len(lanes[t]))] for t in srng.permutation(list(lanes))}
                assert MD.simulate(order, srng, early=bool(seed % 2)) == want, (q, seed)
                schedules += 1
    assert schedules >= 300
    # a tie whose lower t runs last: it reads (0.5, 3) and must still publish (0.5, 1) -- the closed acceptance
    for seed in range(20):
        assert MD.simulate({3: [F(0.5)], 1: [F(0.75), F(0.5)]}, np.random.RandomState(seed)) == MD.key_of(0.5, 1)
    assert MD.simulate({2: [], 4: []}, np.random.RandomState(0)) == MD.NONE


# ---- the key ---------------------------------------------------------------------------------------------------------------------

def test_key_orders_as_dist_then_triangle(tmp_path):
    """psm_mesh_dist_key.h as a stand-alone host program with its own main under the address and undefined-behaviour sanitizers:
    its keys are the model's, and sorting by key sorts by (dist, t) for 0, denormals, equal dists and +inf; none is all-ones"""
    exe, fin, fout = (str(tmp_path / x) for x in ("mesh_dist_key_host", "records.bin", "keys.bin"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mesh_dist_key_host.cpp"), "-o", exe])
    rng = np.random.RandomState(9)
    dist = np.concatenate([F([0, 1e-45, 3e-45, 1.17549435e-38, 1.1754942e-38, 1, 1, 1, np.inf, np.inf, 3.4028235e38]),
                           rng.uniform(0, 4, 2000).astype(F), (10.0 ** rng.uniform(-44, 38, 2000)).astype(F)])
    dist = np.concatenate([dist, dist[:500]])                                   # equal dists under other ids
    rec = np.zeros(dist.size, np.dtype([("dist", "<f4"), ("t", "<u4")]))
    rec["dist"], rec["t"] = dist, rng.randint(0, 1 << 32, dist.size, dtype=np.uint64).astype(np.uint32)
    rec["t"][:8] = [0, 7, 0xffffffff, 5, 5, 2, 1, 0xffffffff]
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    keys = np.fromfile(fout, np.uint64)
    assert keys.size == rec.size and [int(k) for k in keys] == [MD.key_of(d, t) for d, t in zip(rec["dist"], rec["t"])]
    assert (keys != np.uint64(MD.NONE)).all() and int(keys.max()) < MD.NONE
    by_key, by_pair = np.argsort(keys, kind="stable"), np.lexsort((rec["t"], rec["dist"]))
    assert np.array_equal(rec[by_key], rec[by_pair])
    assert MD.key_of(0.0, 5) < MD.key_of(1e-45, 0) < MD.key_of(1.0, 0) < MD.key_of(1.0, 1) < MD.key_of(np.inf, 0) < MD.NONE


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

ENTRIES = ("psm_bvh_mesh_closest_dev", "psm_bvh_mesh_within_dev", "psm_bvh_mesh_clearance_dev")
METHODS = ("meshClosest", "meshWithin", "meshClearance")


def test_library_exports_mesh_clearance(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS, s
        assert re.search(r"\b%s\(psm_bvh\* bvh, psm_bvh\* other, const float\* poses, size_t p, float r(max)?, " % s, header), s
    assert re.search(r"float u, v, dist;[^}]*int32_t tri;\s+float s, t;\s+int32_t other;[^}]*float zero;\s+} psm_mesh_hit;", header)
    section = header[header.index("/* mesh clearance against a built hierarchy"):header.index("} psm_mesh_hit;")]
    for text in ("DESIGN.md 4.24", "BIT FOR BIT", "{0, 0, +inf, -1, 0, 0, -1, 0}", "{0, 0, +inf, -1, 0, 0, 0, 0}", "the lowest t", "comparing the float32 dist",
                 "(bits(dist) << 32) | t", "nobody waits", "d_hits not 16-byte aligned", "mesh query before build", "p == 0 returns PSM_OK and touches nothing",
                 "PSM_MESH_BOUND", "NaN or negative is not a refusal"):
        assert text in section, text
    covered = section[section.index("not covered:"):]
    for text in ("InstanceWorld", "QueryScene", "InstancedScene", "per-pose rmax", "k closest pairs", "dual-tree", "penetration depth", "graph capture"):
        assert text in covered, text
    dt = psm.MESH_HIT_DT
    assert dt.itemsize == 32 and [dt.fields[f][1] for f in ("u", "v", "dist", "tri", "s", "t", "other", "zero")] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [dt.fields[f][1] for f in ("u", "v", "dist", "tri", "s", "t")] == [psm.TRI_HIT_DT.fields[f][1] for f in ("u", "v", "dist", "tri", "s", "t")]
    for m in METHODS:
        assert callable(getattr(psm.TriangleHierarchy, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.InstanceWorld):                  # a single hierarchy's only
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "TriangleHierarchy.inl")).read()
    for m, s in zip(METHODS, ENTRIES):
        assert re.search(r"int %s\(TriangleHierarchy \* other, const glm::mat4 \* poses, size_t p, float r" % m, hpp)
        assert "TriangleHierarchy::%s(" % m in inl and s + "(bvh," in inl
    makefile = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "Makefile")).read()
    assert " mesh_dist.hip " in re.search(r"^SRC := (.*)$", makefile, re.M).group(1)
    assert re.search(r"^mesh_dist\.o: psm_mesh_dist_key\.h psm_mesh_dev\.h psm_tri_dist_dev\.h", makefile, re.M)
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "mesh_dist.hip")).read()
    for text in ("why the answer is fixed", "nobody waits", "__hip_atomic_load(word(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)", "atomicMin(word()",
                 "hipMemsetAsync(d_keys, 0xff"):
        assert text in src, text
    # (the knob is read once for every clearance entry point, beside the other shared host pieces: DESIGN.md 4.28)
    assert 'getenv("PSM_MESH_BOUND")' in open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "mesh.hip")).read() and "mesh_bound()" in src
    assert "asm(" not in src and "asm volatile" not in src                                     # plain HIP atomics throughout


def test_query_mesh_hits_views(psm):
    rec = TD.miss_records(6).reshape(2, 3, 8)
    rec[1, 2] = [0.25, 0.5, 2.0, 0, 0.125, 0.75, 0, 0]
    rec.view(I)[1, 2, 3] = 7
    hits = psm.QueryMeshHits(rec)
    assert hits.other is None and hits.tri.shape == (2, 3) and hits.tri.dtype == I and hits.tri[1, 2] == 7 and hits.tri[0, 0] == -1
    assert hits.dist[1, 2] == 2 and np.isinf(hits.dist[0]).all() and (hits.u[1, 2], hits.v[1, 2], hits.s[1, 2], hits.t[1, 2]) == (0.25, 0.5, 0.125, 0.75)
    assert len(hits) == 2 and hits.buffer is rec
    with pytest.raises(ValueError):
        hits.points(None, None, None)
    # per pose: `other` is slot 6; the witness points, held against the model's posed triangle
    tris, otris, poses = tie_cases()[0][1:4]
    _, crec, _ = MD.query(tris, live(tris), otris, live(otris), poses)
    pair = psm.QueryMeshHits(crec, True)
    assert pair.other.dtype == I and list(pair.other) == [1, 1] and list(pair.tri) == [0, 0] and pair.dist.shape == (2,)
    on_mesh, on_other = pair.points(tris, otris, poses)
    assert on_mesh.shape == (2, 3) and np.allclose(np.linalg.norm(on_mesh - on_other, axis=1), [0.5, 0.75])
    assert np.allclose(on_mesh[:, 2], 0) and np.allclose(on_other[:, 2], [0.5, 0.75])
    miss = TD.miss_records(2)
    miss.view(I)[:, 6] = -1
    a, b = psm.QueryMeshHits(miss, True).points(tris, otris, poses)
    assert np.isnan(a).all() and np.isnan(b).all()


def test_mesh_clearance_refusals_without_a_hierarchy(psm):
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for fn in (getattr(lib, s) for s in ENTRIES):                                 # no hierarchy: refused before anything is touched
        assert fn(None, None, p, ctypes.c_size_t(1), ctypes.c_float(1.0), p) == -1
        assert fn(None, None, None, ctypes.c_size_t(0), ctypes.c_float(1.0), None) == -1    # ... before p == 0 is answered, too
    assert not any(buf)

    class NoCall(psm.TriangleHierarchy):   # the Python layer refuses the poses, other and rmax before any call
        def __init__(self):
            self.ctx, self._h, self.triangleCount = None, None, 5

    th = NoCall()
    eye = np.eye(3, 4)
    scaled = eye.copy()
    scaled[:, :3] *= 1.01
    nan = eye.copy()
    nan[0, 3] = np.nan
    calls = (lambda m, r=1.0: th.meshClosest(th, m, r), lambda m, r=1.0: th.meshWithin(th, m, r), lambda m, r=1.0: th.meshClearance(th, m, r))
    for bad in (scaled, nan, [eye, scaled], np.eye(3), np.zeros((2, 2, 3, 4))):
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    for call in calls:
        with pytest.raises(ValueError, match="rmax must be one scalar"):
            call(eye, [1.0, 2.0])
    with pytest.raises(TypeError):
        th.meshClearance(object(), eye)


# What each kernel reaches with the Makefile's flags, as ceilings: VGPRs, SGPRs, the waves per SIMD its
# __launch_bounds__ ask for (what the unforced figure gives: 512 / VGPRs rounded up to 8), no scratch, no spills, no lane writes,
# the LDS of the 16-entry stack. The clearance kernel's four instances: the shared bound off (0), read in begin() alone (2),
# re-read before every leaf (6), and published early too (14: the default).
MESH_DIST_KERNELS = {"22bvh_query_mesh_closestE": (115, 96, 4), "21bvh_query_mesh_withinE": (145, 98, 3), "19bvh_query_mesh_pickE": (114, 88, 4),
                     "24bvh_query_mesh_clearanceILj0EEEv": (146, 96, 3), "24bvh_query_mesh_clearanceILj2EEEv": (148, 106, 3),
                     "24bvh_query_mesh_clearanceILj6EEEv": (150, 106, 3), "24bvh_query_mesh_clearanceILj14EEEv": (148, 106, 3)}


def test_mesh_dist_kernels_codegen():
    asm = csrc_asm("mesh_dist.hip")
    assert asm.count(".amdhsa_kernel ") == len(MESH_DIST_KERNELS) + 1            # and the fill kernel
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "mesh_dist.hip")).read()
    bounds = re.search(r"MD_CLOSEST_WAVES = (\d+), MD_WITHIN_WAVES = (\d+), MD_CLEAR_WAVES = (\d+), MD_PICK_WAVES = (\d+)", src)
    assert [int(x) for x in bounds.groups()] == [4, 3, 3, 4]
    for name, (vgprs, sgprs, waves) in MESH_DIST_KERNELS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%sNS_12MeshDistArgsE" % name)

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= vgprs and meta("sgpr_count") <= sgprs, (name, meta("vgpr_count"), meta("sgpr_count"))
        assert 512 // ((vgprs + 7) // 8 * 8) == waves, name                    # the bound asks for what the registers give
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4, name          # the stack
        assert "v_div_fixup_f32" in body and "v_sqrt_f32" in body and "v_pk_" not in body, name   # IEEE division and sqrtf, nothing paired
        clear = "clearance" in name
        assert ("global_atomic_umin_x2" in body) == clear, name               # the publication: one 64-bit atomic minimum
        loads = len(re.findall(r"global_load_dwordx2 [^\n]*sc1", body))       # agent-scope loads of the word
        assert (loads >= 1) == (clear and "Lj0E" not in name), (name, loads)


def test_mesh_clearance_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "mesh_dist_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "mesh_dist_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
