#!/usr/bin/env python3
"""Compare the kernels of two `hipcc -S --cuda-device-only` outputs: kernel_diff.py OLD.s NEW.s

A kernel is `same` when its body (from its label to its .amdhsa_kernel block) holds the same instructions and directives once
comments are stripped and the local labels (.LBB<f>_<n>, .Ltmp<n>, .Lfunc_*) are renumbered in the order they appear, and its
register and segment sizes agree. Prints one line per kernel with the instruction and VGPR counts of both sides; exits 1 when
a kernel differs or is on one side only."""
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")
SIZES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_size")


def kernels(path):
    """{name: (body lines, {size: value})} in file order"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        name, desc = m.group(1), m.group(2)
        body = text[text.index("\n" + name + ":") + 1:m.start()]
        names = {}
        lines = []
        for line in body.split("\n"):
            line = line.split(";")[0].rstrip()
            if line:
                lines.append(LABEL.sub(lambda l: names.setdefault(l.group(0), ".L%d" % len(names)), line))
        sizes = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, desc).group(1)) for k in SIZES}
        out[name] = (lines, sizes)
    return out


def instructions(lines):
    return sum(1 for l in lines if l.startswith("\t") and not l.lstrip().startswith("."))


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    bad = 0
    for name in list(old) + [k for k in new if k not in old]:
        if name not in old or name not in new:
            print("%-52s only in %s" % (name, old_path if name in old else new_path))
            bad += 1
            continue
        (lo, so), (ln, sn) = old[name], new[name]
        same = lo == ln and so == sn
        bad += not same
        print("%-52s %-7s instructions %5d -> %5d  VGPRs %3d -> %3d" % (name, "same" if same else "differs", instructions(lo), instructions(ln),
                                                                        so["next_free_vgpr"], sn["next_free_vgpr"]))
    print("%d kernels, %d differ" % (len(set(old) | set(new)), bad))
    return 1 if bad or not old else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
