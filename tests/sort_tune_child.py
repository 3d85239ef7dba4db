"""A fresh process for the PSM_SORT_TUNE tests (test_gpu_parity.py): the variable is read when a context is created.
usage: python sort_tune_child.py rejected | layouts S CAP"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import sort_layouts as LY
import sort_local_model as M

psm = importlib.import_module("prismarine-core_amd")
N = 20000


def check(rs, keys, shape):
    rng = np.random.RandomState(keys.size)
    keys = keys[rng.permutation(keys.size)]
    vals = rng.randint(0, 2 ** 32, size=keys.size, dtype=np.int64).astype(np.uint32)
    order = np.argsort(keys, kind="stable")
    overflow = M.overflows(keys, 48, shape)
    try:
        gk, gv = rs.sort_arrays(keys, vals)
        assert np.array_equal(gk, keys[order]) and np.array_equal(gv, vals[order])
        assert rs.getAlgorithm() == (2, 0 if overflow else 2), (rs.getAlgorithm(), overflow)
    finally:
        rs.setAlgorithm(2)
    return overflow


ctx = psm.Context(0)
rs = psm.RadixSort(ctx)
if sys.argv[1] == "rejected":   # the default shapes must be in force: a bin of 3 072 keys behind 1 023 fits them, one of 3 073 does not
    rng = np.random.RandomState(2)
    for big in (3072, 3073):
        bins = np.concatenate([np.arange(1023), np.full(big, 5000), 6000 + rng.randint(0, 3000, N - 1023 - big)]).astype(np.uint64)
        keys = (bins << np.uint64(48)) | rng.randint(0, 2 ** 48, size=N, dtype=np.int64).astype(np.uint64)
        assert check(rs, keys, (1024, 4096)) == (big == 3073)
    print("sorted 2 x %d keys" % N)
else:
    S, CAP = int(sys.argv[2]), int(sys.argv[3])
    ran = over = 0
    for name in LY.NAMES:
        if name.startswith("long_at_") or name == "two_long":
            for c0 in LY.stretches(name, N, S, CAP).values():
                over += check(rs, LY.layout(name, N, S, CAP, c0, 48, seed=ran), (S, CAP))
                ran += 1
    print("sorted %d layouts, %d overflowed" % (ran, over))
ctx.close()
