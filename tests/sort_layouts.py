"""Key layouts around radix_local's overflow path (a chunk whose last bin runs past the workgroup's window), shared by the
model's tests (test_sort_local_cpu.py) and the device's (test_gpu_parity.py).

A layout is a run of small bins that starts exactly on a stretch boundary, a0 = c0 S, followed by one LONG bin; the rest of
the array is filler (bins of a few keys). layout() returns the keys ordered by bin -- what the hybrid sort's two global
passes make of any permutation of them. Bin numbers stay below 32 768, so the keys are valid for pshift 48 and for 47
(Morton codes: bit 63 clear).

NAMES:
  long_at_0 / _1 / _half / _last    one-key bins up to offset 0, 1, S/2, S - 1 of the stretch, then a bin of CAP + 500 keys
  two_long                          two such bins, each behind small bins of its own stretch: two overflow workgroups in one launch
  long_to_end                       the long bin runs to the end of the array (the binary search for its end ends at n)
  end_at_window_minus_1 / end_at_window / end_past_window
                                    the long bin ends at a0 + CAP - 1, a0 + CAP, a0 + CAP + 1: the workgroup sees a bin's end only
                                    INSIDE its window, so the first fits LDS and the other two do not (the model says which)
  small_total_S_minus_1             bins of 1..40 keys that total S - 1 before the long bin: the largest first part
  long_equal_small_differ           a long bin of ONE key value behind small bins that differ in every low digit
  small_equal_long_differs          the reverse: small bins of one low value, a long bin that differs in every low digit
  long_differs_in_1 / _2 / _3 / _6  the long bin's keys differ in that many digits: odd counts leave local_slow's result in the
                                    scratch buffer (copied back), even ones in keys[]
"""
import numpy as np

NAMES = ["long_at_0", "long_at_1", "long_at_half", "long_at_last", "two_long", "long_to_end",
         "end_at_window_minus_1", "end_at_window", "end_past_window", "small_total_S_minus_1",
         "long_equal_small_differ", "small_equal_long_differs",
         "long_differs_in_1", "long_differs_in_2", "long_differs_in_3", "long_differs_in_6"]


def _sizes(rng, total, most):
    """bin sizes in [1, most] that add up to `total`"""
    out = []
    while total > 0:
        s = min(int(rng.randint(1, most + 1)), total)
        out.append(s)
        total -= s
    return out


def _feature(name, S, CAP, rng):
    """[(bin sizes, kind of low bits)] from a0 on; kind: 'rand', 'const', or a digit count; None = filler up to the next stretch but one"""
    long_ = CAP + 500
    ones = lambda o: ([1] * o, "rand")
    if name.startswith("long_at_"):
        o = {"0": 0, "1": 1, "half": S // 2, "last": S - 1}[name[8:]]
        return [ones(o), ([long_], "rand")]
    if name == "two_long":
        return [(_sizes(rng, S // 2, 5), "rand"), ([long_], "rand"), None, (_sizes(rng, S // 3, 5), "rand"), ([long_], "rand")]
    if name == "long_to_end":
        return [ones(S // 2), ([-1], "rand")]
    if name.startswith("end_"):
        o = S // 2
        return [ones(o), ([CAP - o + {"at_window_minus_1": -1, "at_window": 0, "past_window": 1}[name[4:]]], "rand")]
    if name == "small_total_S_minus_1":
        return [(_sizes(rng, S - 1, 40), "rand"), ([long_], "rand")]
    if name == "long_equal_small_differ":
        return [(_sizes(rng, S // 2, 40), "rand"), ([long_], "const")]
    if name == "small_equal_long_differs":
        return [(_sizes(rng, S // 2, 40), "const"), ([long_], "rand")]
    if name.startswith("long_differs_in_"):
        return [ones(S // 2), ([long_], int(name[16:]))]
    raise KeyError(name)


def _length(feature, S):
    at = 0
    for seg in feature:
        if seg is None:
            at = ((at + S - 1) // S + 1) * S
        else:
            at += sum(s for s in seg[0] if s > 0)
    return at


def stretches(name, n, S, CAP):
    """{where: c0}: the stretches to place the layout in -- the first, a middle one, and the last in which the whole layout still
    fits (a long bin that STARTS in the array's very last stretch cannot run past its window); equal ones listed once"""
    if name == "long_to_end":
        return {"end": (n - CAP - 700) // S}
    last = (n - 1 - _length(_feature(name, S, CAP, np.random.RandomState(0)), S)) // S
    assert last >= 0, "the layout does not fit %d keys" % n
    out = {}
    for where, c0 in (("first", 0), ("middle", last // 2), ("last", last)):
        if c0 not in out.values():
            out[where] = c0
    return out


def layout(name, n, S, CAP, c0, pshift=48, seed=0):
    rng = np.random.RandomState(seed)
    feature = _feature(name, S, CAP, rng)
    most = 2 * max(4, -(-n // 12000)) - 1
    sizes, kinds = [], []

    def fill(total):
        s = _sizes(rng, total, most)
        sizes.extend(s); kinds.extend(["rand"] * len(s))

    fill(c0 * S)
    at = c0 * S
    for seg in feature:
        if seg is None:
            to = ((at + S - 1) // S + 1) * S
            fill(to - at)
            at = to
            continue
        for s in seg[0]:
            s = n - at if s < 0 else s
            sizes.append(s); kinds.append(seg[1])
            at += s
    assert at <= n
    fill(n - at)
    sizes = np.array(sizes, np.int64)
    assert sizes.sum() == n and sizes.size < 32768
    bins = np.repeat(np.arange(sizes.size, dtype=np.uint64), sizes)
    low = rng.randint(0, 2 ** 62, size=n, dtype=np.int64).astype(np.uint64)
    const = np.uint64(0x5A5A1234ABCD77)
    start = np.concatenate([[0], np.cumsum(sizes)])
    for b, kind in enumerate(kinds):
        if kind == "rand":
            continue
        s, e = int(start[b]), int(start[b + 1])
        if kind == "const":
            low[s:e] = const
        else:   # random in the lowest `kind` digits only
            m = np.uint64((1 << (8 * kind)) - 1)
            low[s:e] = (low[s:e] & m) | (const & ~m)
    low &= np.uint64((1 << pshift) - 1)
    return (bins << np.uint64(pshift)) | low
