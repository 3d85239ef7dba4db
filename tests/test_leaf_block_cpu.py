"""The leaf block of the traversal loop in hipcc's gfx950 assembly (no GPU needed): one packed pass per block.

A lane that reaches accepted leaves parks its triangle pair; once enough lanes are parked the wave runs the block
(trace.hip, rt_traverse). The pair's second test runs in a helper lane at the same time as the first tests, so the block
issues the triangle test's body once, not twice: the helper pulls the ray by ds_bpermute and the owner pulls the result back.
The block lies between the node step (its first v_fma_mix_f32) and the solo gear (its first v_readfirstlane / v_readlane);
the triangle test is the one IEEE divide there (tri_test's 1 / det)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMED = ("_ZN3psm11rt_traverseILb0ELb0ELb1EEEvNS_8TravArgsE", "_ZN3psm11rt_traverseILb0ELb0ELb0EEEvNS_8TravArgsE")


def _kernels(tmp_path):
    flags = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", flags, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = str(tmp_path / "trace.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + [f for f in cxx if not f.startswith("-W")] +
                          ["-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "prismarine-core_amd", "csrc", "trace.hip")],
                          stderr=subprocess.DEVNULL)
    lines = open(out).read().split("\n")
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN3psm\w+:", l)]
    ends = [i for i, l in enumerate(lines) if l.startswith(".Lfunc_end")]
    return {name: lines[st:en] for (st, name), en in zip(starts, ends) if name in TIMED}


def _leaf_block(body):
    first = next(i for i, l in enumerate(body) if "v_fma_mix_f32" in l)          # the node step
    solo = next(i for i in range(first, len(body)) if re.match(r"\tv_read(first)?lane", body[i]))   # the solo gear
    # the block's entry: behind the wave's decision (its lane counts, s_bcnt1) and the two scalar exits (keep stepping, solo gear)
    a = next(i for i in range(first, solo) if body[i].startswith("\ts_bcnt1"))
    for _ in range(2):
        a = next(i for i in range(a, solo) if body[i].startswith("\ts_cbranch_scc1")) + 1
    return first, a, solo


def test_leaf_block_runs_one_packed_pass(tmp_path):
    kern = _kernels(tmp_path)
    assert sorted(kern) == sorted(TIMED)
    for name, body in kern.items():
        first, a, solo = _leaf_block(body)
        divs = [i for i in range(first, solo) if body[i].startswith("\tv_div_fixup_f32") and body[i].rstrip().endswith("1.0")]
        assert len(divs) == 1, (name, divs)                       # one tri_test body in the loop
        div = divs[0]
        assert a < div, name
        perm = [i for i in range(a, solo) if body[i].startswith("\tds_bpermute_b32")]
        before = [i for i in perm if i < div]
        after = [i for i in perm if i > div]
        # the helper's triangle and ray (1 + 3 + 3) before the test, the owner's d, u, v after it
        assert len(before) == 7 and len(after) == 3, (name, before, after)
        # one pass: no branch behind the test leads back into it (the serial block looped over its body a second time)
        labels = {l.split(":")[0]: i for i, l in enumerate(body) if l.startswith(".LBB")}
        for i in range(div, solo):
            m = re.match(r"\ts_(cbranch_\w+|branch) (\.LBB\w+)", body[i])
            if m:
                assert not (before[0] <= labels[m.group(2)] <= div), (name, body[i])
        # the block up to the owner's last pull: pairing, pulls, the test and the first test's acceptance -- 142 VALU in both
        # kernels (the serial block: 124 from its entry to the end of a pass, and its 111-instruction body again whenever a
        # lane of the wave had a pair)
        valu = sum(1 for l in body[a:after[-1] + 1] if l.startswith("\tv_"))
        assert valu <= 150, (name, valu)
