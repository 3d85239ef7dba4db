"""CPU tests (no GPU) of the host path the eleven grid entry points share (psm_grid_* and psm_grid_world_*: grid.hip,
grid_dist.hip, world.hip): folding the four host functions onto one set of pieces moved no kernel -- the 28
kernels of the five files are the commit before's, by digest and by name --, each shared text is written once, the hand-written
copies are gone, and the Python grid methods are the commit before's by signature and docstring."""
import glob
import hashlib
import inspect
import json
import os
import re

from test_world_query_cpu import _kernel_digests
from util import ROOT, csrc_asm

CSRC = os.path.join(ROOT, "prismarine-core_amd", "csrc")
KERNELS = {"grid.hip": 4, "grid_dist.hip": 3, "world_grid.hip": 3, "world_grid_dist.hip": 2, "world.hip": 16}
BEFORE = json.load(open(os.path.join(ROOT, "tests", "golden", "grid_kernels_before.json")))
SIGNATURES = {
    "TriangleHierarchy.voxelize": "(self, origin, cell, dims, solid=False, samples=3, as_torch=False)",
    "TriangleHierarchy.voxelCounts": "(self, origin, cell, dims, as_torch=False)",
    "TriangleHierarchy.distanceField": "(self, origin, cell, dims, rmax=inf, signed=False, samples=3, nearest=True, as_torch=False)",
    "InstanceWorld.voxelize": "(self, origin, cell, dims, solid=False, samples=3, as_torch=False)",
    "InstanceWorld.voxelCounts": "(self, origin, cell, dims, as_torch=False)",
    "InstanceWorld.voxelInstances": "(self, origin, cell, dims, as_torch=False)",
    "InstanceWorld.distanceField": "(self, origin, cell, dims, rmax=inf, signed=False, samples=3, nearest=True, as_torch=False)",
}


def _hip():
    return {os.path.basename(f): open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def test_the_28_kernels_of_the_grid_files_and_world_hip_are_unchanged(tmp_path):
    """the instruction streams and sizes of the kernels of grid.hip, grid_dist.hip, world_grid.hip, world_grid_dist.hip and
    world.hip are those recorded from the commit before the shared host path (tests/golden/grid_kernels_before.json:
    tools/kernel_diff.py's normal form, hashed), and there is no kernel more or less"""
    now = {}
    for src, count in KERNELS.items():
        out = tmp_path / src.replace(".hip", ".s")
        out.write_text(csrc_asm(src))
        found = _kernel_digests(str(out))
        assert len(found) == count and not set(found) & set(now), src
        now.update(found)
    before = BEFORE["kernels"]
    assert len(before) == 28 and set(now) == set(before)
    assert [k for k in before if now[k] != before[k]] == []


def test_each_shared_text_is_written_once():
    """the refusals and the two state texts the four host functions used to restate exist once over csrc/*.hip (samples' text
    once over the grid paths: query.hip has the point queries' own), and the grid paths format no message of their own"""
    hip = _hip()
    everything = "".join(hip.values())
    for text in (": invalid grid: %s", "rmax must be >= 0", "grid query before build", "grid query: hierarchy deeper than the query stack"):
        assert everything.count(text) == 1, text
    paths = "".join(hip[f] for f in ("grid.hip", "grid_dist.hip", "world.hip", "world_grid.hip", "world_grid_dist.hip"))
    assert paths.count("samples must be 1, 3 or 5") == 1
    assert everything.count("samples must be 1, 3 or 5") == 2 and hip["query.hip"].count("samples must be 1, 3 or 5") == 1
    # the NULL pointer and the alignment texts are the posed-mesh pieces' (mesh.hip), not restated for the grids
    for f in ("grid.hip", "grid_dist.hip"):
        assert "NULL pointer\"" not in hip[f] and "-byte aligned\"" not in hip[f] and "snprintf" not in hip[f], f
    host = open(os.path.join(CSRC, "psm_query_host.h")).read()
    for piece in ("int grid_front(", "int grid_built(", "int grid_slabs(", "int slabs_for("):
        assert piece in host, piece
    for f, calls in (("grid.hip", 2), ("grid_dist.hip", 1), ("world.hip", 2)):   # (grid.hip: the definition and grid_query())
        assert hip[f].count("grid_front(") == calls, f


def test_the_hand_written_copies_are_gone():
    """a grid's nine numbers are copied into kernel arguments by grid_args and world_grid_args alone, how a world's walk starts
    is said once, and the slab loop is the shared iterator's"""
    hip = _hip()
    headers = {os.path.basename(f): open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*.h")))}
    fill = "g.ox = grid->origin[0]"
    assert sum(t.count(fill) for t in hip.values()) + sum(t.count(fill) for t in headers.values()) == 2
    for text, name in ((headers["psm_grid_dev.h"], "grid_args"), (hip["world.hip"], "world_grid_args")):
        body = text[text.index(" %s(const psm_grid* grid" % name):]
        assert fill in body[:body.index("return g;")], name
    assert hip["world.hip"].count("== 1 ? ~0 : 0") == 1 and hip["world.hip"].count("= world_start(w)") == 5   # (the grids' through world_grid_args)
    loops = sum(len(re.findall(r"for \(uint64_t first = 0; first < ", t)) for t in list(hip.values()) + list(headers.values()))
    assert loops == 1 and "for (uint64_t first = 0; first < bricks; first += slab)" in headers["psm_query_host.h"]
    assert sum(t.count("GRID_SLAB_BRICKS / 2u") for t in hip.values()) == 1     # the signed scheme's sizing


def test_the_python_grid_methods_are_unchanged_and_share_two_helpers(psm):
    """TriangleHierarchy._grid_call and InstanceWorld._grid_call are gone; the seven public grid methods keep their signatures and
    their docstrings (SHA-256 recorded from the commit before in tests/golden/grid_kernels_before.json)"""
    assert not hasattr(psm.TriangleHierarchy, "_grid_call") and not hasattr(psm.InstanceWorld, "_grid_call")
    assert callable(psm._voxel_call) and callable(psm._distance_call)
    assert sorted(BEFORE["docstrings"]) == sorted(SIGNATURES) and len(SIGNATURES) == 7
    for name, signature in SIGNATURES.items():
        cls, method = name.split(".")
        f = getattr(getattr(psm, cls), method)
        assert str(inspect.signature(f)) == signature, name
        assert hashlib.sha256(f.__doc__.encode()).hexdigest() == BEFORE["docstrings"][name], name


def test_the_header_layer_has_one_distance_read_back():
    inl = {f: open(os.path.join(ROOT, "include", "Prismarine", f)).read() for f in ("TriangleHierarchy.inl", "InstanceWorld.inl")}
    assert "worldDistanceReadBack" not in "".join(inl.values())
    assert inl["TriangleHierarchy.inl"].count("inline int distanceReadBack(") == 1 and "inline int distanceReadBack(" not in inl["InstanceWorld.inl"]
    assert inl["TriangleHierarchy.inl"].count("return distanceReadBack(") == 2 and inl["InstanceWorld.inl"].count("return distanceReadBack(") == 2
