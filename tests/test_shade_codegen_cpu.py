"""Code-generation guard of the shading kernel that needs no GPU: hipcc's gfx950 build of shade.hip with the Makefile's flags,
its resource-usage remarks and its assembly. rt_shade<false, false, false> is the instantiation the benchmark runs (no
textures, one hierarchy, ordinary materials); the frame is bound by vector-instruction issue, so what the
kernel is worth is the vector instructions it issues at the occupancy it had. The test counts instruction classes only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_ZN3psm8rt_shadeILb0ELb0ELb0EEEvNS_9ShadeArgsE"

# The same kernel of the parent commit (c1deaa7: before the per-triangle shading record, the baked material constants and light
# centres, the exact skips and the wave-level queue locator), measured by shade_figures() below on that commit's shade.hip with
# ROCm 7.2's hipcc (AMD clang 22.0.0git, roc-7.2.0): 63 VGPRs, no scratch, 2516 vector instructions. The proposal this change
# answers counted 2509 for it with a script of its own; the bound is the lower of the two. (This tree: 62 VGPRs, 2289.)
PARENT_VGPRS = 63
PARENT_VALU = 2509


def shade_figures(source, out_dir):
    """{vgprs, scratch, valu} of rt_shade<false, false, false> in `source`: VGPRs and scratch bytes per lane from the
    kernel-resource-usage remarks, the static count of vector instructions (lines that start with v_) from the kernel's label to
    its s_endpgm"""
    flags = open(os.path.join(ROOT, "prismarine-core_amd", "csrc", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", flags, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "-fno-slp-vectorize" in cxx and "-ffp-contract=off" in cxx
    out = os.path.join(str(out_dir), "shade.s")
    res = subprocess.run(["/opt/rocm/bin/hipcc"] + [f for f in cxx if not f.startswith("-W")] +
                         ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", out, source],
                         stderr=subprocess.PIPE, universal_newlines=True, check=True)
    remarks = res.stderr.split("\n")
    at = [i for i, l in enumerate(remarks) if "Function Name: " + KERNEL in l]
    assert len(at) == 1, "no resource-usage remark for " + KERNEL
    blk = "\n".join(remarks[at[0]:at[0] + 12])
    fig = {"vgprs": int(re.search(r"remark:\s+VGPRs: (\d+)", blk).group(1)),
           "scratch": int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
           "vgpr_spills": int(re.search(r"VGPRs Spill: (\d+)", blk).group(1))}
    lines = open(out).read().split("\n")
    start = [i for i, l in enumerate(lines) if l.startswith(KERNEL + ":")][0]
    end = [i for i, l in enumerate(lines) if i > start and l.startswith(".Lfunc_end")][0]
    last = [i for i in range(start, end) if lines[i].startswith("\ts_endpgm")][-1]
    fig["valu"] = sum(1 for l in lines[start:last] if l.startswith("\tv_"))
    return fig


def test_rt_shade_keeps_its_registers_and_issues_fewer_vector_instructions(tmp_path):
    fig = shade_figures(os.path.join(ROOT, "prismarine-core_amd", "csrc", "shade.hip"), tmp_path)
    print(fig)
    assert fig["vgprs"] <= PARENT_VGPRS, fig           # 8 waves per SIMD, as before
    assert fig["scratch"] == 0 and fig["vgpr_spills"] == 0, fig
    assert fig["valu"] < PARENT_VALU, fig
