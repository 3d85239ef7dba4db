"""CPU tests (no GPU) of the mesh queries over an instance world (psm_world_mesh_overlaps_dev / psm_world_mesh_count_dev /
psm_world_mesh_triangles_dev, world_mesh.hip; InstanceWorld.overlapsMesh / countOnMesh / trianglesOnMesh).

The model (tests/world_mesh_query_model.py) is a composition of two models that are held elsewhere; the first three tests
exercise it alone -- rows and prefixes, skip, the identity world of one -- and pass without the feature. The rest fail without
it: psm_mesh_dev.h, psm_world_box_dev.h and psm_tri_dev.h chained as world_mesh.hip chains them, on the host under the
sanitizers, against the models record for record; the exports, the header text, the Python surface and the refusals that need
no device; what world_mesh.hip compiles to; the header layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import instance_query_model as NQ
import mesh_query_model as MQ
import tri_query_model as TQ
import world_box_query_model as WB
import world_mesh_query_model as WM
import world_tri_query_model as WT
from point_query_model import _split
from test_world_box_cpu import _pose, _rotation, _soup, general_world, lattice_world, signed_permutations
from util import ROOT, csrc_asm, kernel_asm, kernel_meta

F = np.float32
D = np.float64
U = np.uint32
KS = (1, 2, 3, 8, 16)


def _other(rng, n):
    """an `other` mesh around the origin with one dropped triangle (three equal vertices) in the middle of the load order"""
    t = _soup(rng, n + 1, 0.8)
    t[n // 2] = t[n // 2, :1]
    t[n] = [[-4, -4, 0.25], [4, -4, -0.25], [0, 4, 0.125]]   # ... and a last one through everything near the origin
    return t, np.delete(np.arange(n + 1), n // 2)


# ---- the model (these pass without the feature) ----------------------------------------------------------------------------------

def test_model_rows_are_ascending_prefixes_and_counts_agree():
    rng = np.random.RandomState(81)
    insts = general_world(82, 8)
    otris, oleaves = _other(rng, 40)
    poses = [_pose(_rotation(rng, j % 2 == 1), rng.uniform(-2, 2, 3) if j < 5 else [500.0, 0, 0]) for j in range(6)]
    flag, count, tri, inst, rcount = WM.query(insts, otris, oleaves, poses, 16)
    assert flag.shape == (6,) and count.shape == (6, 41) and tri.shape == inst.shape == (6, 41, 16) and rcount.shape == (6, 41)
    assert flag[:5].any() and not flag[5] and (count > 16).any() and ((count > 0) & (count < 16)).any()
    assert np.array_equal(flag, (count > 0).any(axis=1)) and np.array_equal(rcount, np.minimum(count, 16))
    assert (count[:, 20] == 0).all() and (tri[:, 20] == -1).all() and (inst[:, 20] == -1).all()      # the dropped triangle
    filled = tri >= 0
    assert np.array_equal(filled, np.arange(16)[None, None] < rcount[:, :, None]) and np.array_equal(filled, inst >= 0)
    key = inst.astype(np.int64) * (1 << 32) + tri
    assert ((key[:, :, :-1] < key[:, :, 1:]) | ~filled[:, :, 1:]).all()
    for k in KS:
        f, c, t, i, rc = WM.query(insts, otris, oleaves, poses, k)
        assert np.array_equal(f, flag) and np.array_equal(c, count) and np.array_equal(t, tri[:, :, :k]) and np.array_equal(i, inst[:, :, :k])
        assert np.array_equal(rc, np.minimum(count, k))
    # the contract's own statement: the world's triangle queries on the posed triangles
    q = MQ.posed(otris, poses)
    _, c2, t2, i2, _ = WT.flat(insts, q[:, oleaves].reshape(-1, 3, 3), 16)
    assert np.array_equal(c2.reshape(6, 40), count[:, oleaves]) and np.array_equal(t2.reshape(6, 40, 16), tri[:, oleaves])
    assert np.array_equal(i2.reshape(6, 40, 16), inst[:, oleaves])


def test_model_skip_is_the_shortened_list_reindexed():
    rng = np.random.RandomState(83)
    insts = lattice_world()[:10] + lattice_world()[48:]            # coincident members among them
    otris = (rng.randint(-2, 5, (30, 3, 3)) * 0.5).astype(F)
    oleaves = np.arange(30)
    poses = [_pose(r, t) for r, t in zip(signed_permutations()[5:9], ([0, 0, 0], [1, 0, -1], [0.5, 0.5, 0], [40, 0, 0]))]
    full = WM.query(insts, otris, oleaves, poses, 16)
    assert full[0][:3].all() and not full[0][3]
    for s in (0, 4, len(insts) - 1):
        got = WM.query(insts, otris, oleaves, poses, 16, skip=s)
        short = WM.query(insts[:s] + insts[s + 1:], otris, oleaves, poses, 16)
        assert np.array_equal(got[1], short[1]) and np.array_equal(got[2], short[2]) and np.array_equal(got[4], short[4])
        assert np.array_equal(got[3], np.where(short[3] >= s, short[3] + 1, short[3]))              # the indices kept
        assert not (got[3] == s).any() and (full[3] == s).any()
        # and it is the full answer with the skipped instance's pairs taken out (where the full rows are complete)
        whole = full[1] <= 16
        assert whole.any()
        lost = (full[3] == s).sum(axis=2)
        assert np.array_equal(got[1][whole], (full[1] - lost)[whole])
    assert not WM.query(insts[:1], otris, oleaves, poses, 4, skip=0)[1].any()                      # a world of one, skipped
    with pytest.raises(ValueError):
        WM.query(insts, otris, oleaves, poses, 4, skip=len(insts))


def test_model_identity_world_of_one_is_the_mesh_query():
    rng = np.random.RandomState(84)
    tris = _soup(rng, 150)
    cand = np.sort(rng.permutation(150)[:140])
    otris, oleaves = _other(rng, 50)
    poses = [_pose(_rotation(rng, j == 1), rng.uniform(-0.5, 0.5, 3)) for j in range(3)]
    flag, count, rows, rcount = MQ.query(tris, cand, otris, oleaves, poses, 16)
    got = WM.query([(tris, cand, NQ.IDENTITY, WB.plain_fit(tris))], otris, oleaves, poses, 16)
    assert flag.any() and (count > 0).sum() > 30
    assert np.array_equal(got[0], flag) and np.array_equal(got[1], count) and np.array_equal(got[2], rows) and np.array_equal(got[4], rcount)
    assert np.array_equal(got[3], np.where(rows >= 0, 0, -1))


# ---- the three device headers chained on the host ----------------------------------------------------------------------------------

def _host_records():
    """(mesh pose m[12], other's stored v0, e1, e2, the instance's pose w[12], the candidate's stored v0, e1, e2) float32 [n, 42]:
    lattice poses on both sides on lattice soups (exact), general rotations and reflections on both sides over six decades of
    size, each with candidates that are the posed query brought back into the instance (coincident, as rounding decides), that
    cross it and that share a vertex with it, and with random ones; some records with NaN and inf"""
    rng = np.random.RandomState(85)
    recs = []

    def add(m, src, w, cand):
        s, c = _split(src), _split(cand)
        n = src.shape[0]
        recs.append(np.concatenate([np.broadcast_to(np.asarray(m, D).reshape(1, 12), (n, 12)), *s,
                                    np.broadcast_to(np.asarray(w, D).reshape(1, 12), (n, 12)), *c], axis=1))

    def back(w, x):
        """world points [.., 3] (float64) in the instance's object space: R^T (x - T)"""
        return (x - w[:, 3]) @ w[:, :3]

    perms = signed_permutations()
    for j in range(6):                                                             # the lattice: every operation exact
        m = _pose(perms[rng.randint(48)], rng.randint(-4, 5, 3) / 8.0)
        w = _pose(perms[rng.randint(48)], rng.randint(-4, 5, 3) / 8.0)
        src = (np.clip(rng.randint(-8, 9, (120, 1, 3)) + rng.randint(-1, 2, (120, 3, 3)), -8, 8) / 8.0).astype(F)
        img = src.astype(D) @ m[:, :3].T + m[:, 3]
        add(m, src, w, back(w, img).astype(F))                                     # the image itself: coincident
        add(m, src, w, back(w, img[rng.permutation(120)]).astype(F))
        add(m, src, w, (np.clip(rng.randint(-8, 9, (120, 1, 3)) + rng.randint(-1, 2, (120, 3, 3)), -8, 8) / 8.0).astype(F))
        touch = img.copy()
        touch[:, 1:] = img[:, :1] + rng.randint(-2, 3, (120, 2, 3)) / 8.0          # shares v0, the rest elsewhere
        add(m, src, w, back(w, touch).astype(F))
    for mag in range(-3, 3):                                                       # general poses, six decades of size
        scale = 10.0 ** mag
        for reflect in (False, True):
            m = _pose(_rotation(rng, reflect), rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 2))
            w = _pose(_rotation(rng, not reflect), rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 2))
            src = ((rng.uniform(-1, 1, (150, 1, 3)) + rng.uniform(-0.2, 0.2, (150, 3, 3))) * scale).astype(F)
            img = src.astype(D) @ m[:, :3].T + m[:, 3]
            add(m, src, w, back(w, img).astype(F))                                 # near-coincident
            cross = img.mean(axis=1, keepdims=True) + rng.normal(size=(150, 3, 3)) * scale * 0.2
            add(m, src, w, back(w, cross).astype(F))                               # through the interior
            share = img.copy()
            share[:, 1:] = img[:, :1] + rng.normal(size=(150, 2, 3)) * scale * 0.2
            add(m, src, w, back(w, share).astype(F))                               # touching at a vertex, as rounding decides
            add(m, src, w, back(w, (rng.uniform(-1, 1, (150, 1, 3)) + rng.uniform(-0.5, 0.5, (150, 3, 3))) * scale + m[:, 3]).astype(F))
    rec = np.concatenate(recs).astype(F)
    rec[::97, 14] = np.nan                                                         # other's v0.z
    rec[1::97, 16] = np.inf                                                        # other's e1.y
    rec[2::97, 41] = -np.inf                                                       # the candidate's e2.z
    rec[3::97, 3] = np.float32(3e38)                                               # a translation next to overflow
    rec[3::97, 12] = np.float32(3e38)
    return rec


def test_query_and_candidate_on_the_host_are_the_models(tmp_path):
    """mesh_query_tri (psm_mesh_dev.h), fwd_point / fwd_vec (psm_world_box_dev.h) and tri_tri (psm_tri_dev.h), chained as
    world_mesh.hip's begin() and leaf() chain them, as a stand-alone host program with its own main, built with -ffp-contract=off
    and the address and undefined-behaviour sanitizers and run as a process of its own on the CPU: the query triangle and the
    posed candidate of every record are the models' bit for bit, and so is the flag"""
    hipcc = "/opt/rocm/bin/hipcc"
    exe, fin, fout, fposed = (str(tmp_path / x) for x in ("world_mesh_host", "records.bin", "flags.bin", "posed.bin"))
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "prismarine-core_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "world_mesh_host.cpp"), "-o", exe])
    rec = _host_records()
    assert rec.shape[1] == 42 and 5000 <= rec.shape[0] <= 12000
    rec.tofile(fin)
    done = subprocess.run([exe, fin, fout, fposed], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert done.returncode == 0, done.stdout.decode(errors="replace")
    got = np.fromfile(fout, np.uint8).astype(bool)
    posed = np.fromfile(fposed, F).reshape(-1, 18)
    want_q = MQ.pose_records(rec[:, :12], rec[:, 12:15], rec[:, 15:18], rec[:, 18:21])
    with np.errstate(all="ignore"):
        want_c = np.concatenate([MQ.fwd_point(rec[:, 21:33], rec[:, 33:36]), MQ.fwd_vec(rec[:, 21:33], rec[:, 36:39]),
                                 MQ.fwd_vec(rec[:, 21:33], rec[:, 39:42])], axis=1).astype(F)
    # (mesh_query_model's fwd_point / fwd_vec are world_box_query_model's: one pose of the second, record by record)
    for r in (0, 1000, rec.shape[0] - 1):
        pose = rec[r, 21:33].reshape(3, 4)
        assert np.array_equal(WB.fwd_point(pose, rec[r:r + 1, 33:36]).view(U), want_c[r:r + 1, 0:3].view(U))
        assert np.array_equal(WB.fwd_vec(pose, rec[r:r + 1, 36:39]).view(U), want_c[r:r + 1, 3:6].view(U))
    assert posed.shape[0] == rec.shape[0]
    bad = np.nonzero((posed[:, :9].view(U) != want_q.reshape(-1, 9).view(U)).any(axis=1))[0]
    assert bad.size == 0, "%d query triangles differ, first %d: %s against %s" % (bad.size, bad[0], posed[bad[0], :9], want_q[bad[0]])
    bad = np.nonzero((posed[:, 9:].view(U) != want_c.view(U)).any(axis=1))[0]
    assert bad.size == 0, "%d posed candidates differ, first %d: %s against %s" % (bad.size, bad[0], posed[bad[0], 9:], want_c[bad[0]])
    want = TQ.tri_tri(want_c[:, 0:3], want_c[:, 3:6], want_c[:, 6:9], want_q[:, 0], want_q[:, 1], want_q[:, 2])
    bad = np.nonzero(got != want)[0] if got.shape == want.shape else np.zeros(1, int)
    assert got.shape == want.shape and bad.size == 0, "%d flags differ, first %d: %s" % (bad.size, bad[0], rec[bad[0]])
    broken = ~(np.isfinite(want_q).reshape(-1, 9).all(axis=1) & np.isfinite(want_c).all(axis=1))
    assert 0.2 < want.mean() < 0.9 and broken.sum() > 100 and not want[broken].any()     # a non-finite image meets nothing


# ---- the library, the headers, the kernels ---------------------------------------------------------------------------------------

WORLD_MESH_ENTRIES = ("psm_world_mesh_overlaps_dev", "psm_world_mesh_count_dev", "psm_world_mesh_triangles_dev")
WORLD_MESH_METHODS = ("overlapsMesh", "countOnMesh", "trianglesOnMesh")


def test_library_exports_the_world_mesh_queries(psm):
    lib = psm.lib()
    header = open(os.path.join(ROOT, "include", "psm_hip.h")).read()
    for s in WORLD_MESH_ENTRIES:
        assert hasattr(lib, s) and s in psm.EXPORTS, s
        assert re.search(r"\b%s\(psm_world\* world, psm_bvh\* other, const float\* poses, size_t p, int32_t skip," % s, header), s
    section = header[header.index("/* mesh queries over a world"):header.index("int psm_world_mesh_overlaps_dev(")]
    section = re.sub(r"\n \*\s+", " ", section)                                                  # (as running text)
    for text in ("a = fwd_point(m, v0),  b = a + fwd_vec(m, e1),  c = a + fwd_vec(m, e2)", "BIT FOR BIT", "HOST memory", "WORLD space",
                 "its build dropped", "non-finite", "may be one of the world's own members", "entry s removed and the other indices KEPT",
                 "never by a filter after the test", "skip must be -1 or below psm_world_count()", "mesh query before build",
                 "other of another context", "a stale world", "named by its index", "skip out of range", "p x T >= 2^32",
                 "p == 0 returns PSM_OK and touches nothing", "an empty world and an other without leaves launch no query kernel",
                 "synchronises the context's stream ONCE", "CANNOT be captured into a graph", "PSM_MESH_SKIP",
                 "not covered: mesh queries over flat scenes and instanced lists", "a dual-tree walk", "intersection segments",
                 "more than one skipped instance", "k > PSM_QUERY_K_MAX; graph capture of the call"):
        assert text in section, text
    # 4.21's section keeps its sentence where it was, and points here after it
    mesh = header[header.index("/* mesh queries against a built hierarchy"):header.index("int psm_bvh_mesh_overlaps_dev(")]
    assert mesh.index("not covered: a mesh against a world") < mesh.index('"mesh queries over a world" below')
    for m in WORLD_MESH_METHODS:
        assert callable(getattr(psm.InstanceWorld, m)), m
        for other in (psm.QueryScene, psm.InstancedScene, psm.TriangleHierarchy):                 # a world's only
            assert not hasattr(other, m), (other, m)
    hpp = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.hpp")).read()
    inl = open(os.path.join(ROOT, "include", "Prismarine", "InstanceWorld.inl")).read()
    for m, s in zip(WORLD_MESH_METHODS, WORLD_MESH_ENTRIES):
        assert re.search(r"int %s\(TriangleHierarchy \* other, const glm::mat4 \* poses, size_t p, int skip," % m, hpp)
        assert "InstanceWorld::%s(" % m in inl and s + "(world," in inl
    makefile = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "Makefile")).read()
    assert " world_mesh.hip " in re.search(r"^SRC := (.*)$", makefile, re.M).group(1)
    deps = re.search(r"^world_mesh\.o: (.*)$", makefile, re.M).group(1).split()
    assert set(deps) >= {"psm_mesh_dev.h", "psm_query_dev.h", "psm_world_dev.h", "psm_world_box_dev.h", "psm_tri_dev.h", "psm_world_box_list.h"}


def test_world_mesh_refusals_that_need_no_device(psm):
    """no world: the code the other world queries give, before anything is looked at; the Python layer refuses k, skip and the
    poses before any call"""
    lib = psm.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one, none = ctypes.c_size_t(1), ctypes.c_int32(-1)
    code = lib.psm_world_intersect_dev(None, None, one, None, None)
    assert code != 0 and code == lib.psm_world_tri_count_dev(None, p, one, p)
    for fn in (lib.psm_world_mesh_overlaps_dev, lib.psm_world_mesh_count_dev):
        assert fn(None, None, p, one, none, p) == code
        assert fn(None, None, None, ctypes.c_size_t(0), none, None) == code                       # ... before p == 0 is answered, too
        assert fn(None, None, p, one, ctypes.c_int32(5), p) == code
    fn = lib.psm_world_mesh_triangles_dev
    assert fn(None, None, p, one, none, ctypes.c_uint32(1), p, p, p) == code
    assert fn(None, None, None, ctypes.c_size_t(0), none, ctypes.c_uint32(0), None, None, None) == code
    assert fn(None, None, p, one, none, ctypes.c_uint32(17), p, p, p) == code
    assert not any(buf)

    class Mesh(psm.TriangleHierarchy):   # a hierarchy that cannot make a call
        def __init__(self):
            self.ctx, self._h, self.triangleCount = None, None, 5

    class NoCall(psm.InstanceWorld):     # a world of three that cannot make a call
        def __init__(self):
            self.ctx, self._w = None, None
            self.hierarchies, self._handles = [Mesh(), Mesh(), Mesh()], [None, None, None]

        def close(self):
            pass

    world, mesh = NoCall(), Mesh()
    eye = np.eye(3, 4)
    for k in (0, 17, 1 << 20):
        with pytest.raises(psm.PsmError, match="psm_world_mesh_triangles_dev: k must be 1 .. 16"):
            world.trianglesOnMesh(mesh, eye, k)
    with pytest.raises(ValueError):
        world.trianglesOnMesh(mesh, eye, 2.5)
    calls = (lambda m, s=None: world.overlapsMesh(mesh, m, skip=s), lambda m, s=None: world.countOnMesh(mesh, m, skip=s),
             lambda m, s=None: world.trianglesOnMesh(mesh, m, 4, skip=s))
    for s in (3, -1, 1 << 20, 1.5, True):
        for call in calls:
            with pytest.raises(psm.PsmError, match="skip must be None or an instance index 0 .. 2"):
                call(eye, s)
    scaled = eye.copy()
    scaled[:, :3] *= 1.01
    nan = eye.copy()
    nan[0, 3] = np.nan
    for bad in (scaled, nan, [eye, scaled], np.eye(3), np.zeros((2, 2, 3, 4))):
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(TypeError):
        world.countOnMesh(object(), eye)
    with pytest.raises(TypeError):
        world.countOnMesh(world, eye)


# The VGPRs each kernel reaches with the Makefile's flags, as ceilings under the 128 of __launch_bounds__(64, 4), and the LDS it
# declares (the 16-entry stack; the key list is dynamic, k x 512 B, and does not show here)
WORLD_MESH_VGPRS = {"world_query_mesh_any": 101, "world_query_mesh_count": 100, "world_query_mesh_tris": 122}


def test_world_mesh_kernels_codegen():
    asm = csrc_asm("world_mesh.hip")
    assert asm.count(".amdhsa_kernel ") == 3
    for name, ceiling in WORLD_MESH_VGPRS.items():
        blk, body = kernel_asm(asm, "_ZN3psm%d%sENS_13WorldMeshArgsE" % (len(name), name))

        def meta(key):
            return kernel_meta(blk, key)
        assert meta("vgpr_count") <= ceiling <= 128, (name, meta("vgpr_count"))
        assert meta("vgpr_spill_count") == 0 and meta("sgpr_spill_count") == 0, name
        assert meta("private_segment_fixed_size") == 0 and "scratch_" not in body, name
        assert "v_writelane_b32" not in body, name                            # no SGPR parked in a VGPR lane either
        assert meta("group_segment_fixed_size") == 16 * 64 * 4 == 4096, name  # the stack; the list is the launch's k x 64 x 8 B
        assert not re.search(r"v_rcp_|v_rsq_|v_sqrt_|v_div_", body), name     # no division (the lane mapping's either), no square root
        assert "v_fma_f32" not in body and "v_fmac_f32" not in body, name     # nothing contracted: one rounding per operation
        assert ("ds_read_b64" in body and "ds_write_b64" in body) or name != "world_query_mesh_tris", name
    src = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "world_mesh.hip")).read()
    assert "asm(" not in src and "asm volatile" not in src                    # plain C++ throughout
    assert len(re.findall(r"__launch_bounds__\(QUERY_BLOCK, WORLD_MESH_WAVES\)", src)) == 3 and "WORLD_MESH_WAVES = 4;" in src
    # the list kernel's dynamic LDS is the launch's: k x 64 lanes x 8 B, on that kernel alone
    assert re.search(r"world_query_mesh_tris<<<grid, QUERY_BLOCK, \(size_t\)a\.w\.samples \* QUERY_BLOCK \* sizeof\(uint64_t\), c->stream>>>", src)
    assert len(re.findall(r"world_query_mesh_(?:any|count)<<<grid, QUERY_BLOCK, 0, c->stream>>>", src)) == 2
    # the pieces are used, not restated; skip is decided where an instance is entered
    for piece in ("v3 fwd_vec(", "v3 fwd_point(", "bool keep_top(", "void mesh_split(", "void mesh_query_tri(", "bool tri_tri(", "struct WorldBoxList"):
        assert piece not in src, piece
    for use in ("mesh_split(i, m.L, m.magic, q, j)", "mesh_query_tri(pose,", "enter_row(w, in)", "load_pose(w, (uint32_t)inst, p)", "tri_tri(v0, e1, e2, qa, qb, qc)",
                ": WorldBoxPrune", "WorldBoxList<QUERY_BLOCK> L;", "world_walk(m.w, q)"):
        assert use in src, use
    enter = src[src.index("PSM_D int enter(int in) {"):]
    assert enter.index("if (in == m.skip) return -1;") < enter.index("enter_row(w, in)") < enter.index("leaf(r.sorted_tri[0])")
    assert src.count("m.skip") == 1


def test_world_mesh_header_layer_compiles_and_links(tmp_path):
    exe = str(tmp_path / "world_mesh_query_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-DPSM_NO_SYSTEM_GLM",
                           os.path.join(ROOT, "tests", "cpp", "world_mesh_query_host.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "prismarine-core_amd"), "-lpsm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "prismarine-core_amd")])
    assert os.path.exists(exe)
