"""A plain model of one radix_local launch (prismarine-core_amd/csrc/sort.hip), numpy and Python only.

The hybrid sort's last kernel works IN PLACE: workgroup c reads the window [c S - 1, c S + CAP) of keys[] while its
neighbours may already be writing into it. Whether that is safe is a property of the ORDER of the kernel's global loads
and stores, which no run on a device can pin down. So this file restates the kernel as one Python generator per workgroup
over the shared arrays keys, vals, altk, altv; a generator yields wherever another workgroup's loads or stores could come
in between, and a test is free to interleave the generators as it likes (tests/test_sort_local_cpu.py).

It is a reading of the kernel and must stay one: nothing here calls the library, and every step names the lines of
sort.hip it restates (the function names below are the kernel's).

  workgroup(c):                                                          radix_local
    a = c S, winN = min(CAP, n - a), win1 = min(winN, S + 1024)            "the window", `win1`
    snapshot keys[a - 1] and keys[a, a + win1)                    YIELD    the first `L.sk[j] = keys[a + j]` loop, `bin_before`
    lo = first bin edge of the snapshot, hi = first one at j >= S          "the chunk: from the first bin boundary ..."
    if hi is none, win1 < winN and lo < S:
        snapshot keys[a + win1, a + winN)                         YIELD    "the rest of the window"
        hi = first edge in [win1, winN)
    js = lo; none or >= S: return (no chunk)                               `if (js == 0xFFFFFFFFu || js >= S) return`
    je = hi; none and the array ends inside the window: je = winN
    je still none -- the overflow path:                                    "the chunk's last bin runs past the window"
        binary search over keys[] for the long bin's end          YIELD    after every probe `keys[mid]`
        jl = first key of the long bin in the snapshot, jl in [js, S)      `atomicMin(&L.hi, j)` over [js, S)
        local_slow over the LONG BIN ALONE, [a + jl, end)                  `local_slow(L, ..., a + jl, m)`
        overflow += its length (never 0)                                   `__hip_atomic_fetch_add(overflow, m, ...)`
        jl == js: return (nothing precedes the long bin); else je = jl and go on: the small bins are an LDS chunk
      (legacy=True, the kernel before this model was written: local_slow over the WHOLE chunk [a + js, end), return)
    the LDS chunk [js, je): keys from the snapshot, vals[a + js, a + je) YIELD  `k[i] = L.sk[js + q]`, `v[i] = vals[gs + q]`
    no digit differs: return                                               `if (diff == 0ull) return`
    stable LSD passes over the digits that differ, in LDS                  the `for (int p = 0; p < 8; p++)` loop
    write back keys and vals [a + js, a + je)          YIELD half way and at the end   the last loop of the kernel

  local_slow(gs, m):                                                     local_slow
    OR of key ^ keys[gs] over keys[gs, gs + m)                   YIELD    the `dif |=` loop
    per digit that differs, src and dst swapping between (keys, vals) and (altk, altv):
        stable scatter of src[gs, gs + m) by the digit into dst[gs, gs + m)
                                                        YIELD half way and at the end   the `dk[pos] = k[i]` stores
    result in the scratch buffers (odd number of passes): copy back   YIELD half way and at the end   `if (sk != keys)`

The kernel's stores within one loop have no order among themselves; "half way" is one of the states a neighbour can see, and
the invariant the tests check -- every position of keys[] holds a key of the bin that the sorted array has there -- does not
depend on which half goes first, only on which positions a loop may write at all.

Before every yield the generator notes in Launch.stored which range of keys[] its last step stored into (None: it only
loaded), so that a check of keys[] after every yield need not look at positions that cannot have changed.

What the host can observe besides the arrays: Launch.overflow, the pinned word (non-zero: the context falls back to the
eight passes).
"""
import numpy as np

NONE = 0xFFFFFFFF


def key_bins(k, pshift):
    """key_bin: the bin of a key, key >> pshift (pshift 64, the single-chunk launch: every key in bin 0)"""
    k = np.asarray(k, np.uint64)
    if pshift >= 64:
        return np.zeros(k.shape, np.uint64)
    return k >> np.uint64(pshift)


def partition(keys, vals, pshift):
    """What sort_hybrid's two global passes leave: ordered by bin, input order inside a bin."""
    order = np.argsort(key_bins(keys, pshift), kind="stable")
    return keys[order], vals[order]


def default_shape(n):
    """sort_hybrid's choice of (S, CAP, pshift offset is the caller's): small sorts 1 024 of 4 096, large ones 2 048 of 4 096;
    up to 4 096 keys one chunk and no bins (pshift 64, and no overflow word)"""
    if n <= 4096:
        return 4096, 4096
    return (1024, 4096) if n <= (1 << 19) else (2048, 4096)


class Launch:
    """The shared state of one radix_local launch over keys that the global passes have partitioned by bin."""

    def __init__(self, keys, vals, S, CAP, pshift, legacy=False):
        self.keys = np.array(keys, np.uint64)
        self.vals = np.array(vals, np.uint32)
        self.n = int(self.keys.size)
        self.altk = np.zeros(self.n, np.uint64)
        self.altv = np.zeros(self.n, np.uint32)
        self.S, self.CAP, self.pshift, self.legacy = int(S), int(CAP), int(pshift), bool(legacy)
        self.overflow = 0
        self.slow = []   # the workgroups that took the overflow path
        self.stored = None   # the range [lo, hi) of keys[] that the step before the latest yield stored into, or None

    def grid(self):
        return (self.n + self.S - 1) // self.S

    def workgroups(self):
        return [self.workgroup(c) for c in range(self.grid())]

    # ---------------------------------------------------------------------------------------------------- local_slow
    def local_slow(self, gs, m):
        keys, vals = self.keys, self.vals
        diff = int(np.bitwise_or.reduce(keys[gs:gs + m] ^ keys[gs]))
        self.stored = None
        yield "slow: diff"
        sk, sv, dk, dv = keys, vals, self.altk, self.altv
        for p in range(8):
            shift = 8 * p
            if (diff >> shift) & 255 == 0:
                continue
            k = sk[gs:gs + m].copy()   # (the kernel reads src tile by tile; nobody writes src[gs, gs + m) during the pass)
            v = sv[gs:gs + m].copy()
            pos = np.empty(m, np.int64)
            pos[np.argsort(((k >> np.uint64(shift)) & np.uint64(255)).astype(np.uint8), kind="stable")] = np.arange(m)
            h = m // 2
            dk[gs + pos[:h]] = k[:h]; dv[gs + pos[:h]] = v[:h]
            self.stored = (gs, gs + m) if dk is keys else None
            yield "slow: pass %d, half" % p
            dk[gs + pos[h:]] = k[h:]; dv[gs + pos[h:]] = v[h:]
            self.stored = (gs, gs + m) if dk is keys else None
            yield "slow: pass %d, end" % p
            sk, sv, dk, dv = dk, dv, sk, sv
        if sk is not keys:
            h = m // 2
            keys[gs:gs + h] = sk[gs:gs + h]; vals[gs:gs + h] = sv[gs:gs + h]
            self.stored = (gs, gs + h)
            yield "slow: copy back, half"
            keys[gs + h:gs + m] = sk[gs + h:gs + m]; vals[gs + h:gs + m] = sv[gs + h:gs + m]
            self.stored = (gs + h, gs + m)
            yield "slow: copy back, end"

    # --------------------------------------------------------------------------------------------------- radix_local
    def workgroup(self, c):
        keys, vals = self.keys, self.vals
        n, S, CAP, pshift = self.n, self.S, self.CAP, self.pshift
        a = c * S
        if a >= n:
            return
        winN = min(CAP, n - a)
        win1 = min(winN, S + 1024)
        sk = np.zeros(CAP, np.uint64)
        sk[:win1] = keys[a:a + win1]
        bin_before = int(key_bins(keys[a - 1], pshift)) if a > 0 else 0
        self.stored = None
        yield "window: first part"
        b = key_bins(sk[:win1], pshift)
        edge = np.empty(win1, bool)
        edge[0] = (a == 0) or int(b[0]) != bin_before
        edge[1:] = b[1:] != b[:-1]
        e = np.flatnonzero(edge)
        lo = int(e[0]) if e.size else NONE
        e = e[e >= S]
        hi = int(e[0]) if e.size else NONE
        if hi == NONE and win1 < winN and lo < S:
            sk[win1:winN] = keys[a + win1:a + winN]
            self.stored = None
            yield "window: the rest"
            b = key_bins(sk[win1 - 1:winN], pshift)
            e = np.flatnonzero(b[1:] != b[:-1])
            if e.size:
                hi = win1 + int(e[0])
        js = lo
        if js == NONE or js >= S:
            return
        je = hi
        if je == NONE and a + winN >= n:
            je = winN
        if je == NONE:
            self.slow.append(c)
            lbin = int(key_bins(sk[winN - 1], pshift))
            lo, hi = a + winN, n
            while lo < hi:
                mid = lo + ((hi - lo) >> 1)
                later = int(key_bins(keys[mid], pshift)) > lbin
                self.stored = None
                yield "search: probe %d" % mid
                if later:
                    hi = mid
                else:
                    lo = mid + 1
            if self.legacy:
                gs, m = a + js, lo - (a + js)
                yield from self.local_slow(gs, m)
                self.overflow += m
                return
            jl = js + int(np.flatnonzero(key_bins(sk[js:S], pshift) == np.uint64(lbin))[0])
            m = lo - (a + jl)
            yield from self.local_slow(a + jl, m)
            self.overflow += m
            if jl == js:
                return
            je = jl
        size, gs = je - js, a + js
        k = sk[js:je].copy()
        v = vals[gs:gs + size].copy()
        self.stored = None
        yield "chunk: values"
        diff = int(np.bitwise_or.reduce(k ^ k[0]))
        if diff == 0:
            return
        for p in range(8):
            shift = 8 * p
            if (diff >> shift) & 255 == 0:
                continue
            o = np.argsort(((k >> np.uint64(shift)) & np.uint64(255)).astype(np.uint8), kind="stable")
            k, v = k[o], v[o]
        h = size // 2
        keys[gs:gs + h] = k[:h]; vals[gs:gs + h] = v[:h]
        self.stored = (gs, gs + h)
        yield "chunk: write back, half"
        keys[gs + h:gs + size] = k[h:]; vals[gs + h:gs + size] = v[h:]
        self.stored = (gs + h, gs + size)
        yield "chunk: write back, end"


def run(launch, pick=None, after=None):
    """Runs every workgroup of `launch` to its end. pick(live) chooses the index (into `live`, the list of workgroup numbers
    still running) of the workgroup that takes the next step -- default: each in turn to its end, lowest first; after(c, label)
    is called after every yield."""
    gens = dict(enumerate(launch.workgroups()))
    live = sorted(gens)
    while live:
        i = pick(live) if pick else 0
        c = live[i]
        try:
            label = next(gens[c])
        except StopIteration:
            live.pop(i)
            continue
        if after:
            after(c, label)
    return launch


def overflows(keys, pshift=48, shape=None):
    """Does the hybrid sort of these (unsorted) keys raise the overflow word? -- the model's answer, by running it."""
    keys = np.asarray(keys, np.uint64)
    S, CAP = shape or default_shape(keys.size)
    if shape is None and keys.size <= 4096:
        return False   # one chunk of at most CAP keys: the array ends inside the window, and there is no overflow word
    pk, pv = partition(keys, np.zeros(keys.size, np.uint32), pshift)
    return run(Launch(pk, pv, S, CAP, pshift)).overflow != 0
