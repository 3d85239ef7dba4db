"""radix_local works in place; these tests pin the argument that lets it (sort.hip, "In place"): EVERY state of keys[] that a
neighbouring workgroup can load shows, at every position, a key of the bin that the sorted array has there.

The device cannot show a bad interleaving on demand, so the kernel is restated as generators (sort_local_model.py) and the
tests choose the interleaving: every overflow workgroup held at each of its yield points while all others run to their end,
and seeded random schedules. `legacy=True` is the kernel as it was (local_slow over the whole chunk, small bins included):
the same schedules must catch it, or they prove nothing.
"""
import numpy as np
import pytest

import sort_layouts as LY
import sort_local_model as M

N = 20000
SHAPES = [(1024, 4096), (2048, 4096)]
# one layout each for the other instantiated shapes (5120 keys of LDS; 6144 under 512 threads): the model has no thread count
EXTRA = [(3072, 5120, "small_total_S_minus_1"), (3072, 5120, "two_long"), (4096, 6144, "small_total_S_minus_1"), (4096, 6144, "long_at_half")]


def _cases():
    out = []
    for S, CAP in SHAPES:
        for pshift in (48, 47):
            for name in LY.NAMES:
                out.append(pytest.param(name, S, CAP, pshift, id="%s-%d-%d-%d" % (name, S, CAP, pshift)))
    for S, CAP, name in EXTRA:
        out.append(pytest.param(name, S, CAP, 48, id="%s-%d-%d-48" % (name, S, CAP)))
    return out


class Case:
    """one layout in its middle placement: partitioned keys, random values, the expected result"""

    def __init__(self, keys, pshift, S, CAP, seed=5):
        self.S, self.CAP, self.pshift = S, CAP, pshift
        vals = np.random.RandomState(seed).randint(0, 2 ** 32, size=keys.size, dtype=np.int64).astype(np.uint32)
        self.keys, self.vals = M.partition(keys, vals, pshift)
        order = np.argsort(self.keys, kind="stable")
        self.ek, self.ev = self.keys[order], self.vals[order]
        self.ebins = M.key_bins(self.ek, pshift)
        assert np.array_equal(self.ebins, M.key_bins(self.keys, pshift))   # the input is partitioned by bin

    def launch(self, legacy=False):
        return M.Launch(self.keys, self.vals, self.S, self.CAP, self.pshift, legacy=legacy)

    def bins_hold(self, L):
        """after a yield: does every position of keys[] hold a key of the bin the sorted array has there? (Only the positions the
        step stored into are compared: the others held at the yield before, and the input does by construction.)"""
        if L.stored is None:
            return True
        lo, hi = L.stored
        return bool((M.key_bins(L.keys[lo:hi], self.pshift) == self.ebins[lo:hi]).all())

    def sorted(self, L):
        return np.array_equal(L.keys, self.ek) and np.array_equal(L.vals, self.ev)


_cache = {}


def _case(name, S, CAP, pshift):
    key = (name, S, CAP, pshift)
    if key not in _cache:
        st = LY.stretches(name, N, S, CAP)
        c0 = st.get("middle", st.get("end", st.get("first")))
        _cache[key] = Case(LY.layout(name, N, S, CAP, c0, pshift, seed=len(_cache)), pshift, S, CAP)
    return _cache[key]


def _directed(case, legacy=False, strict=True):
    """Every overflow workgroup, held after k = 0, 1, ... of its yields while all the others run to their end, then let go.
    Returns (runs, runs in which a bin moved, runs that ended unsorted); with strict, asserts that both are 0."""
    plain = M.run(case.launch(legacy))
    slow = list(plain.slow)
    runs = moved = unsorted = 0
    for c in slow:
        k = 0
        while True:
            L = case.launch(legacy)
            gens = L.workgroups()
            ok = True
            held = True
            for _ in range(k):
                try:
                    next(gens[c])
                except StopIteration:
                    held = False
                    break
                ok = ok and case.bins_hold(L)
            if not held:
                break   # k is past the workgroup's last yield: every hold point has been tried
            for g in gens[:c] + gens[c + 1:] + [gens[c]]:
                for _ in g:
                    ok = ok and case.bins_hold(L)
            runs += 1
            moved += not ok
            unsorted += not case.sorted(L)
            if strict:
                assert ok, "workgroup %d held after %d yields: a key left the positions of its bin" % (c, k)
                assert case.sorted(L), "workgroup %d held after %d yields: not the stable order" % (c, k)
            k += 1
    return slow, runs, moved, unsorted


@pytest.mark.parametrize("name,S,CAP,pshift", _cases())
def test_directed_schedules(name, S, CAP, pshift):
    case = _case(name, S, CAP, pshift)
    slow, runs, _, _ = _directed(case)
    L = M.run(case.launch())
    assert case.sorted(L)
    assert (L.overflow != 0) == bool(slow)
    if name not in ("end_at_window_minus_1",):
        assert slow, "this layout is meant to take the overflow path"
        assert runs >= 8 * len(slow)
    if name == "two_long":
        assert len(slow) == 2


@pytest.mark.parametrize("name,S,CAP,pshift", _cases())
def test_random_schedules(name, S, CAP, pshift):
    """200 seeded interleavings: the bin invariant after every yield of every workgroup, the stable order at the end."""
    case = _case(name, S, CAP, pshift)
    for seed in range(200):
        rng = np.random.RandomState(1000 + seed)
        L = case.launch()
        bad = []

        def after(c, label):
            if not case.bins_hold(L):
                bad.append((c, label))

        M.run(L, pick=lambda live: rng.randint(len(live)), after=after)
        assert not bad, "seed %d: a key left the positions of its bin after %r" % (seed, bad[0])
        assert case.sorted(L), "seed %d" % seed


def _bin_of_3073():
    """the keys of test_hybrid_sort_chunk_edges[bin_of_3073] (test_gpu_parity.py): 1 023 one-key bins, then a bin of 3 073"""
    rng = np.random.RandomState(11)
    low = rng.randint(0, 2 ** 48, size=N, dtype=np.int64).astype(np.uint64)
    bins = np.concatenate([np.arange(1023), np.full(3073, 5000), 6000 + rng.randint(0, 3000, N - 1023 - 3073)])
    keys = ((bins.astype(np.uint64) << np.uint64(48)) | low)[rng.permutation(N)]
    return Case(keys, 48, 1024, 4096)


def test_bin_of_3073_directed_and_random():
    case = _bin_of_3073()
    slow, runs, moved, unsorted = _directed(case)
    assert slow == [0] and runs > 20


def test_the_schedules_catch_the_legacy_overflow_path():
    """Teeth: local_slow over the whole chunk (legacy=True) interleaves the chunk's bins in keys[] from its second executed pass
    on; the directed schedules on bin_of_3073 must see bins move AND a wrong result, and the plain in-order run must not (which
    is why no run on a device noticed)."""
    case = _bin_of_3073()
    plain = M.run(case.launch(legacy=True))
    assert case.sorted(plain) and plain.overflow != 0 and plain.slow == [0]
    slow, runs, moved, unsorted = _directed(case, legacy=True, strict=False)
    assert slow == [0]
    assert moved > 0, "the bin invariant held in all %d directed runs of the legacy path" % runs
    assert unsorted > 0, "all %d directed runs of the legacy path ended sorted" % runs
    # the state the issue describes: after two executed passes keys[] holds the chunk ordered by its low digits
    L = case.launch(legacy=True)
    g = L.workgroups()[0]
    for label in g:
        if label == "slow: pass 1, end":
            break
    wrong = M.key_bins(L.keys[:4096], 48) != case.ebins[:4096]
    assert wrong.sum() > 1000


def test_model_overflow_word_matches_the_chunk_edge_cases():
    """the flags test_hybrid_sort_chunk_edges carries by hand, from the model"""
    rng = np.random.RandomState(3)
    low = rng.randint(0, 2 ** 48, size=N, dtype=np.int64).astype(np.uint64)
    for big, want in ((3072, False), (3073, True)):
        bins = np.concatenate([np.arange(1023), np.full(big, 5000), 6000 + rng.randint(0, 3000, N - 1023 - big)])
        assert M.overflows((bins.astype(np.uint64) << np.uint64(48)) | low) == want
    assert M.overflows(np.full(N, 77 << 48, np.uint64))
    assert not M.overflows((np.arange(N, dtype=np.uint64) // np.uint64(512)) << np.uint64(48))
    assert not M.overflows(np.full(4096, 5, np.uint64))
