"""NumPy reference of frequent-condition counting (K1 / K2, rdfind_amd/csrc/counts.inl) and the inputs that aim at its
size-dependent branches (pure NumPy, no GPU; nothing here is sized by |V|).

``reference`` restates the stage from its definition with ``np.unique``: per position the values that occur at least
``ms`` times, and the binary keys ``bt << 62 | v1 << 31 | v2`` of the triples whose two values are frequent, with their
counts.  tests/test_fc_ref.py checks it against the Python oracle and the C oracle; tests/test_gpu_fc.py compares the
HIP kernels with it element for element.

``mix64`` / ``b2_bucket`` / ``b2_home`` restate the hash K2 groups its records by.  They only *aim* inputs (which bucket
and which table slot a key lands in); no expected value is computed from them, and every test that relies on the aim
asks rdf_test_fc_report for proof that the branch ran.

The shape builders return ``(s, p, o, V)``; their docstrings say which branch they are after.
"""
import numpy as np

from tests.prim_ref import mix64

U64 = np.uint64
NONE32 = 0xFFFFFFFF


# ---- reference ---------------------------------------------------------------------------------------------------

def bin_keys(bt, v1, v2):
    return (U64(bt) << U64(62)) | (np.asarray(v1, U64) << U64(31)) | np.asarray(v2, U64)


class Ref:
    """freq[pos]: ascending frequent values of position pos (0 s, 1 p, 2 o); ukeys: the frequent unary keys
    pos * V + value in rank order; n_binary_keys: distinct candidate binary keys; bkeys: the frequent ones, ascending."""

    def __init__(self, s, p, o, V, ms):
        ms = max(int(ms), 1)  # a support of 0 counts as 1
        cols = [np.asarray(c, np.uint32) for c in (s, p, o)]
        self.V, self.ms, self.freq = V, ms, []
        for c in cols:
            vals, cnt = np.unique(c, return_counts=True)
            self.freq.append(vals[cnt >= ms].astype(np.uint32))
        self.n3 = [int(f.shape[0]) for f in self.freq]
        self.fval = np.concatenate(self.freq) if cols[0].shape[0] else np.zeros(0, np.uint32)
        self.ukeys = np.concatenate([U64(t * V) + f.astype(U64) for t, f in enumerate(self.freq)])
        fs, fp, fo = (np.isin(c, f) for c, f in zip(cols, self.freq))
        s_, p_, o_ = cols
        keys = np.concatenate([bin_keys(2, s_[fs & fp], p_[fs & fp]),   # o[s,p]
                               bin_keys(1, s_[fs & fo], o_[fs & fo]),   # p[s,o]
                               bin_keys(0, p_[fp & fo], o_[fp & fo])])  # s[p,o]
        self.cand, self.cand_cnt = np.unique(keys, return_counts=True)
        self.n_binary_keys = int(self.cand.shape[0])
        self.bkeys = self.cand[self.cand_cnt >= ms]

    def rank_bit(self, keys):
        """(rank, bit) the device must hold for the unary keys: the index among ukeys, NONE32 / 0 for the others."""
        keys = np.asarray(keys, U64)
        at = np.searchsorted(self.ukeys, keys)
        hit = (at < self.ukeys.shape[0]) & (self.ukeys[np.minimum(at, max(self.ukeys.shape[0] - 1, 0))] == keys) \
            if self.ukeys.shape[0] else np.zeros(keys.shape[0], bool)
        return np.where(hit, at, NONE32).astype(np.uint32), hit.astype(np.uint32)


def reference(s, p, o, V, ms):
    return Ref(s, p, o, V, ms)


def probe_keys(ref, s, p, o, k1_bits):
    """The unary keys a test looks up: every frequent key and its two neighbours, t * V - 1 and t * V, 0, 3V - 1, and
    the first and last key of every K1 bucket (2^k1_bits keys) that holds a key of the input."""
    V = ref.V
    K = 3 * V
    present = np.unique(np.concatenate([np.asarray(s, U64), U64(V) + np.asarray(p, U64), U64(2 * V) + np.asarray(o, U64)]))
    bk = np.unique(present >> U64(k1_bits)).astype(np.int64)
    first = bk << k1_bits
    last = np.minimum(((bk + 1) << k1_bits) - 1, K - 1)
    f = ref.ukeys.astype(np.int64)
    edges = np.array([0, V - 1, V, 2 * V - 1, 2 * V, K - 1], np.int64)
    allk = np.concatenate([f, f - 1, f + 1, edges, first, last, first - 1, last + 1])
    return np.unique(allk[(allk >= 0) & (allk < K)]).astype(U64)


# ---- the hash K2 groups by (aiming only) -------------------------------------------------------------------------

def b2_bucket(keys, bits):
    return (mix64(keys) >> U64(64 - bits)).astype(np.int64)


def b2_home(keys, T):
    return (mix64(keys) & U64(T - 1)).astype(np.int64)


# ---- shapes ------------------------------------------------------------------------------------------------------

def _column(counts, rng):
    """A column holding value v counts[v] times, in random order."""
    col = np.repeat(np.fromiter(counts.keys(), np.uint32, len(counts)), np.fromiter(counts.values(), np.int64, len(counts)))
    rng.shuffle(col)
    return col


def boundary(V, fa, fb, ms=3, seed=0):
    """K1 at the s / p / o boundaries V and 2V: the values 0 and V - 1 occur in every position; key V - 1 (subject
    V - 1) is frequent iff ``fa`` and key V (predicate 0) iff not ``fa``; key 2V - 1 (predicate V - 1) is frequent iff
    ``fb`` and key 2V (object 0) iff not ``fb``.  Every value's count is exactly ms (frequent) or ms - 1 (not); each
    position holds as many of the one kind as of the other.  V = 1 has one key per position: every count is ms when
    ``fa``, else ms - 1.  V = 2 has room for fa == fb only."""
    rng = np.random.default_rng(seed)
    if V == 1:
        z = np.zeros(ms if fa else ms - 1, np.uint32)
        return z, z.copy(), z.copy(), 1
    if V == 2:
        assert fa == fb
        flags = [{1: fa, 0: not fa}, {0: not fa, 1: fb}, {0: not fb, 1: fb}]
    else:
        assert V >= 4
        flags = [{V - 1: fa, 0: not fa}, {0: not fa, V - 1: fb}, {0: not fb, V - 1: fb}]
        for f in flags:  # values 1 and V - 2 bring the position to two frequent and two infrequent values
            need = 2 - sum(f.values())
            f[1] = need > 0
            f[V - 2] = need > 1
    cols = [_column({v: ms if fr else ms - 1 for v, fr in f.items()}, rng) for f in flags]
    assert len({c.shape[0] for c in cols}) == 1
    return cols[0], cols[1], cols[2], V


def threshold_counts(n, ms, pinned, V, rng):
    """{value: count}: counts of exactly ms or ms - 1 that sum to n, about as many of each; ``pinned`` = {value: frequent?}
    is part of it, the other values are random in [0, V)."""
    j = (-n) % ms  # j values at ms - 1 and k at ms: k * ms + j * (ms - 1) = n
    j += ms * max(0, (n // (2 * ms - 1) - j) // ms)
    k = (n - j * (ms - 1)) // ms
    assert k >= 0 and k * ms + j * (ms - 1) == n and k + j <= V
    pf = sum(pinned.values())
    assert pf <= k and len(pinned) - pf <= j
    others = np.setdiff1d(rng.permutation(V)[: k + j + len(pinned)], np.fromiter(pinned.keys(), np.int64, len(pinned)),
                          assume_unique=False)[: k + j - len(pinned)]
    rng.shuffle(others)
    counts = {int(v): ms if fr else ms - 1 for v, fr in pinned.items()}
    for i, v in enumerate(others):
        counts[int(v)] = ms if i < k - pf else ms - 1
    assert sum(counts.values()) == n
    return counts


def multi_slice(V, pv, fa, n=70000, ms=24, seed=0):
    """One predicate ``pv`` in n = 70 000 triples: its K1 bucket holds more than two counting slices of records, so it is
    counted in slices and ranked by k_u2_finish.  Subjects and objects have counts of exactly ms and ms - 1; subject
    V - 1 and object V - 1 are frequent iff ``fa``, subject 0 and object 0 iff not."""
    rng = np.random.default_rng(seed)
    s = _column(threshold_counts(n, ms, {V - 1: fa, 0: not fa}, V, rng), rng)
    o = _column(threshold_counts(n, ms, {0: not fa, V - 1: fa}, V, rng), rng)
    return s, np.full(n, pv, np.uint32), o, V


def k1_bucket_lens(s, p, o, V, bits):
    keys = np.concatenate([np.asarray(s, np.int64), V + np.asarray(p, np.int64), 2 * V + np.asarray(o, np.int64)])
    return np.bincount(keys >> bits, minlength=(3 * V + (1 << bits) - 1) >> bits)


def k1_slice_starts(lens, slice_records=1 << 15):
    """Record offsets at which k_u2_count's slices start (bucket start + len * j / nsl)."""
    out, start = [], 0
    for ln in lens.tolist():
        nsl = max(1, -(-ln // slice_records))
        out += [start + ln * j // nsl for j in range(nsl)]
        start += ln
    return out


VECTOR_LENS = (1, 7, 8, 9, 19)  # 19 = 8 * 2 + 3


def vector_edges(seed=0, ms=2):
    """K1 buckets of 1, 7, 8, 9 and 8k + 3 records (V = 5 * 2^14: five buckets per position), the sizes rotated from
    position to position so that the buckets start at different offsets from a 16-byte boundary: k_u2_count's short
    path, and its vector body with and without head and tail.  Counts are ms and ms - 1."""
    rng = np.random.default_rng(seed)
    V = 5 << 14
    cols = []
    for t in range(3):
        col = []
        for b in range(5):
            ln = VECTOR_LENS[(b + 2 * t) % 5]
            vals = (b << 14) + rng.permutation(1 << 14)[: ln]  # distinct values of the bucket, used up in turn
            if t == 0 and b == 0:
                vals[0] = 0
            if t == 2 and b == 4:
                vals[0] = V - 1
            left, i = ln, 0
            while left:
                c = min(left, ms if i % 2 == 0 else ms - 1)
                col += [int(vals[i])] * c
                left -= c
                i += 1
        col = np.array(col, np.uint32)
        rng.shuffle(col)
        cols.append(col)
    return cols[0], cols[1], cols[2], V


def big_v(V=180_000_001, seed=0, ms=3):
    """|V| past the 14-bit range (ceil(3V / 2^14) > 2^15 buckets): K1 takes 15 key bits per bucket.  A few thousand
    triples with values at 0, 2^15 - 1, 2^15, V - 1 (each side of V and 2V frequent in one position and not in the
    next) and random ones, counts ms and ms - 1."""
    rng = np.random.default_rng(seed)
    n = 3000
    pins = [{0: False, (1 << 15) - 1: True, 1 << 15: False, V - 1: True, V - 2: False, 1: True},
            {0: True, (1 << 15) - 1: False, 1 << 15: True, V - 1: False, V - 2: True, 1: False},
            {0: False, (1 << 15) - 1: True, 1 << 15: True, V - 1: True, V - 2: False, 1: False}]
    cols = []
    for pin in pins:
        j = (-n) % ms
        j += ms * max(0, (n // (2 * ms - 1) - j) // ms)
        k = (n - j * (ms - 1)) // ms
        counts = {v: ms if fr else ms - 1 for v, fr in pin.items()}
        kf, jf = k - sum(pin.values()), j - (len(pin) - sum(pin.values()))
        others = rng.integers(2, V - 2, size=kf + jf + 64)
        others = np.array([v for v in dict.fromkeys(others.tolist()) if v not in pin][: kf + jf])
        for i, v in enumerate(others):
            counts[int(v)] = ms if i < kf else ms - 1
        assert sum(counts.values()) == n
        cols.append(_column(counts, rng))
    return cols[0], cols[1], cols[2], V


def support_edges(seed=0):
    """n = 50 triples of one predicate: with ms = n it alone is frequent, with ms = n + 1 nothing is."""
    rng = np.random.default_rng(seed)
    n, V = 50, 65
    return (rng.integers(0, V, n).astype(np.uint32), np.full(n, 64, np.uint32), rng.integers(0, 8, n).astype(np.uint32), V)


# K2 ----------------------------------------------------------------------------------------------------------------

RUN_LENS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130)
RUNS_MS = 140


def _to_roles(a, b, c, pair):
    """Columns (a, b) hold the pair under test and c the third value; ``pair`` names the positions of a and b."""
    return {"po": (c, a, b), "so": (a, c, b), "sp": (a, b, c)}[pair]


def runs(pair="po", seed=0, ms=RUNS_MS):
    """K2's run merging (wave_runs4): equal pairs in adjacent rows.  Two first values (0 and 1) and one second value per
    run length; pair (0, x) totals exactly ms and pair (1, x) ms - 1.  Each pair has one main run of its length: starting
    at a multiple of 64 rows or crossing one, in turn, and three of them crossing a multiple of 1024; every other main run
    is broken by a row whose second value is infrequent (an inactive lane inside the run).  The rest of each total is spread in pieces of 1
    to 5 rows.  The third value is unique per row, so only this pair type has candidates.  The input ends in rows of
    pair (0, 0) at a row count that is no multiple of 64: the inactive lanes after the end carry the same key.
    ``pair``: which two positions hold the pair."""
    rng = np.random.default_rng(seed)
    keys = [(f, x) for x in range(len(RUN_LENS)) for f in (0, 1)]
    total = {k: ms - k[0] for k in keys}
    breaker = len(RUN_LENS)  # second value of the breaking rows: occurs fewer than ms times
    mains, n_break = [], 0
    specs = []
    for i, k in enumerate(keys):
        L = RUN_LENS[k[1]]
        rows = [k] * L
        if L >= 2 and i % 2 == 1:
            rows.insert(L // 2, (k[0], breaker))
            n_break += 1
        specs.append((L, rows))
    # run index -> (a multiple of 1024, the rows of the run before it): lengths 3, 63 and the first piece of the broken 130
    cross1024 = {4: (1024, 1), 16: (2048, 32), 23: (3072, 20)}
    for i, (at, before) in cross1024.items():
        mains.append((at - before, specs[i][1]))

    def clash(start, ln):
        for st, rr in mains:
            if start < st + len(rr) and st < start + ln:
                return st + len(rr)
        return None

    cursor = 0
    for i, (L, rows) in enumerate(specs):
        if i in cross1024:
            continue
        while True:
            if i % 2 == 0 or L < 2:
                start = -(-cursor // 64) * 64                       # starts at a multiple of 64
            else:
                start = (cursor + L) // 64 * 64 + 64 - (L + 1) // 2  # crosses one
            nxt = clash(start, len(rows))
            if nxt is None:
                break
            cursor = nxt
        mains.append((start, rows))
        cursor = start + len(rows)
    cursor = max(st + len(rr) for st, rr in mains)
    tail = [(0, 0)] * 3
    N = sum(total.values()) + n_break
    if N % 64 == 0:
        N, n_break = N + 1, n_break + 1
        extra_breaker = True
    else:
        extra_breaker = False
    assert cursor + len(tail) <= N and n_break < ms
    rows = [None] * N
    for start, rr in mains:
        rows[start: start + len(rr)] = rr
    rows[N - 3:] = tail
    left = dict(total)
    for r in rows:
        if r is not None and r in left:
            left[r] -= 1
    pieces = []
    for k, c in left.items():
        while c:
            q = min(c, int(rng.integers(1, 6)))
            pieces.append([k] * q)
            c -= q
    if extra_breaker:
        pieces.append([(1, breaker)])
    order = rng.permutation(len(pieces))
    stream = [r for i in order for r in pieces[i]]
    it = iter(stream)
    rows = [r if r is not None else next(it) for r in rows]
    assert next(it, None) is None
    a = np.array([r[0] for r in rows], np.uint32)
    b = np.array([r[1] for r in rows], np.uint32)
    c = np.arange(100, 100 + N, dtype=np.uint32)
    s, p, o = _to_roles(a, b, c, pair)
    return s, p, o, 100 + N


HOT_ROWS = 60000


def hot_key(seed=0, ms=3, n_mates=8):
    """One (p, o) pair in 60 000 adjacent rows: 15 000 records of count 4 in one K2 bucket, which is counted in several
    slices whose partials fc_sum_pairs adds up.  ``n_mates`` other pairs whose hash shares the hot key's top 12 bits (its
    bucket under every form at this size) have totals of ms and ms - 1, in single rows far apart.  Subjects are unique."""
    rng = np.random.default_rng(seed)
    hp, ho = 5, 7
    hot = bin_keys(0, [hp], [ho])
    P, O = np.meshgrid(np.arange(0, 64), np.arange(100, 4100), indexing="ij")
    cand = bin_keys(0, P.ravel(), O.ravel())
    mates = cand[b2_bucket(cand, 12) == b2_bucket(hot, 12)[0]][: n_mates]
    assert mates.shape[0] == n_mates
    rows = []  # (p, o) of the rows outside the hot run
    for i, k in enumerate(mates.tolist()):
        mp, mo = (k >> 31) & 0x7FFFFFFF, k & 0x7FFFFFFF
        tot = ms if i % 2 == 0 else ms - 1
        rows += [(mp, mo)] * tot
        # the mate's values are frequent whatever its own total: ms rows with another partner each
        rows += [(mp, 5000 + i)] * ms + [(63 + i, mo)] * ms
    rows = [rows[i] for i in rng.permutation(len(rows))]
    half = len(rows) // 2
    allrows = rows[:half] + [(hp, ho)] * HOT_ROWS + rows[half:]
    p = np.array([r[0] for r in allrows], np.uint32)
    o = np.array([r[1] for r in allrows], np.uint32)
    n = p.shape[0]
    s = np.arange(6000, 6000 + n, dtype=np.uint32)
    return s, p, o, 6000 + n


CROWD_BITS = 2   # the colliding keys share the top 2 hash bits: one counting bucket with and without a split bit
CROWD_T = 128    # ... and the home slot of a table of 128 slots (33 to 64 records in the slice)


def crowded(seed=0, m=40):
    """A crowded K2 table: ``m`` >= 34 (p, o) pairs whose keys share a counting bucket and the home slot of its table of
    128 slots.  Keys with one home slot need as many probes as there are, so the last ones pass the 32-probe limit and
    go to the spill list although the bucket has one slice.  ms = 2 and subjects are unique.  Most pairs sit in two
    adjacent rows (one record of count 2); every fourth one in two rows far apart (two records), every fifth one in one
    row (total ms - 1).  Further pairs with totals ms and ms - 1 that share a value with a colliding pair lie in other
    buckets (chosen by their hash), so the table keeps its size."""
    rng = np.random.default_rng(seed)
    P, O = np.meshgrid(np.arange(0, 200), np.arange(200, 400), indexing="ij")
    cand = bin_keys(0, P.ravel(), O.ravel())
    grp = b2_bucket(cand, CROWD_BITS) * CROWD_T + b2_home(cand, CROWD_T)
    best = np.bincount(grp).argmax()
    keys = cand[grp == best][: m]
    assert keys.shape[0] == m >= 34
    top = int(b2_bucket(keys[:1], 1)[0])  # the 1-bit bucket the others must stay out of

    def away(p=None, o=None):  # a partner from a range of its own whose pair hashes to the other 1-bit bucket
        for d in range(1000, 3000):
            k = bin_keys(0, [p if p is not None else d], [o if o is not None else d])
            if int(b2_bucket(k, 1)[0]) != top and (d not in used):
                used.add(d)
                return (p if p is not None else d, o if o is not None else d)
        raise AssertionError("no partner")

    used = set()
    adjacent, apart, n_records = [], [], 0
    for i, k in enumerate(keys.tolist()):
        kp, ko = (k >> 31) & 0x7FFFFFFF, k & 0x7FFFFFFF
        if i % 5 == 4:      # total 1 = ms - 1; its values are made frequent by pairs in the other bucket
            apart += [(kp, ko)]
            adjacent += [[away(p=kp)] * 2, [away(o=ko)] * 2]
            n_records += 1
        elif i % 4 == 3:    # total 2 in two records
            apart += [(kp, ko), (kp, ko)]
            n_records += 2
        else:
            adjacent.append([(kp, ko)] * 2)
            n_records += 1
        if i % 3 == 0:      # neighbours in the other bucket: totals ms and ms - 1
            adjacent.append([away(p=kp)] * 2)
            q = away(o=ko)
            apart.append(q)
            adjacent.append([away(p=q[0])] * 2)  # (q's new value is frequent, q itself is not)
    assert 32 < n_records <= 64
    rng.shuffle(apart)
    blocks = [adjacent[i] for i in rng.permutation(len(adjacent))]
    rows = []
    for i, blk in enumerate(blocks):  # the far-apart rows between the adjacent pairs, never next to their twin
        rows += blk
        if i < len(apart):
            rows.append(apart[i])
    assert len(apart) <= len(blocks)
    p = np.array([r[0] for r in rows], np.uint32)
    o = np.array([r[1] for r in rows], np.uint32)
    n = p.shape[0]
    s = np.arange(4000, 4000 + n, dtype=np.uint32)
    return s, p, o, 4000 + n
