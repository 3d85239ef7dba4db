"""CPU tests (no GPU) of the host path the twelve posed-mesh entry points share (psm_bvh_mesh_* and psm_world_mesh_*: mesh.hip,
mesh_dist.hip, world.hip): folding the four host functions onto one set of pieces moved no kernel -- the 38
kernels of the five files are the commit before's, by digest and by name -- and each shared text is written once."""
import glob
import json
import os
import re

from test_world_query_cpu import _kernel_digests
from util import ROOT, csrc_asm

CSRC = os.path.join(ROOT, "prismarine-core_amd", "csrc")
KERNELS = {"mesh.hip": 3, "mesh_dist.hip": 8, "world_mesh.hip": 3, "world_mesh_dist.hip": 8, "world.hip": 16}


def test_the_38_kernels_of_the_posed_mesh_files_and_world_hip_are_unchanged(tmp_path):
    """the instruction streams and sizes of the kernels of mesh.hip, mesh_dist.hip, world_mesh.hip, world_mesh_dist.hip and
    world.hip are those recorded from the commit before the shared host path (tests/golden/posed_mesh_kernels_before.json:
    tools/kernel_diff.py's normal form, hashed), and there is no kernel more or less"""
    now = {}
    for src, count in KERNELS.items():
        out = tmp_path / src.replace(".hip", ".s")
        out.write_text(csrc_asm(src))
        found = _kernel_digests(str(out))
        assert len(found) == count and not set(found) & set(now), src
        now.update(found)
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "posed_mesh_kernels_before.json")))
    assert len(before) == 38 and set(now) == set(before)
    assert [k for k in before if now[k] != before[k]] == []


def test_each_shared_text_is_written_once():
    """the two knobs are read in one place each and the refusals the four host functions used to restate exist once, over
    csrc/*.hip; one constant bounds the answers of a call"""
    hip = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*.hip"))))
    for text in ('getenv("PSM_MESH_SKIP")', 'getenv("PSM_MESH_BOUND")', "more than 2^32 answers", "pose %zu %s",
                 "leaf count exceeds its triangle count"):
        assert hip.count(text) == 1, text
    everything = hip + "".join(open(f).read() for f in sorted(glob.glob(os.path.join(CSRC, "*.h"))))
    defined = [name for name in ("MESH_QUERIES_MAX", "WORLD_MESH_ANSWERS_MAX") if re.search(r"constexpr\s+\w+\s+%s\s*=" % name, everything)]
    assert len(defined) == 1, defined
    host = open(os.path.join(CSRC, "psm_query_host.h")).read()
    assert "poses_for" not in everything and "mesh_keys_for" not in everything and "int mesh_upload(" in host
