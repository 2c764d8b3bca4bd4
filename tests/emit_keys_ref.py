"""A restatement of K3's emission with key items (RDFIND_EMIT_KEYS), for tests/test_emit_keys_cpu.py and
tests/test_gpu_emit_keys.py.

The rule: a frequent binary key (a = va, b = vb) determines two unary records, the capture of a = va projected on b
joined on vb and the capture of b = vb projected on a joined on va.  A triple that holds the key does not write them; the
key writes them once, as an emission item of its own behind the triples, under the same projection and selection tests.
The distinct record set stays what the plain emission gives.

Records are (capture, join value) pairs; a capture is (projected attribute, ((attribute, value), ...)).  Attributes are
0 s, 1 p, 2 o.  The emission drops repeats of four unary kinds (p[s], s[p], o[p], p[o]) per iteration of 256 items of a
block, exactly (an LDS table); everything else is written as often as it is emitted.
"""
from collections import Counter

import numpy as np

BLOCK = 256
EMIT_GRID = 8192
REPEATING = {(1, 0), (0, 1), (2, 1), (1, 2)}  # (projected, condition attribute) of the kinds the iteration table sees
KINDS = ((0, 1), (0, 2), (1, 2))  # binary key kinds: (s, p), (s, o), (p, o)


def frequent(arr, ms):
    """(frequent unary conditions {(attribute, value)}, frequent binary keys {(a, b, va, vb)}) at support ms."""
    ms = max(int(ms), 1)
    tr = [tuple(int(x) for x in t) for t in np.asarray(arr).reshape(-1, 3).tolist()]
    un = Counter((a, t[a]) for t in tr for a in range(3))
    fu = {k for k, c in un.items() if c >= ms}
    bi = Counter((a, b, t[a], t[b]) for t in tr for a, b in KINDS if (a, t[a]) in fu and (b, t[b]) in fu)
    return fu, {k for k, c in bi.items() if c >= ms}


def windows(n_items, grid_cap=None):
    """The (first, last + 1) item ranges of the emission's iterations: eg = min(ceil(items / 256), cap) blocks of
    per = ceil(items / eg) contiguous items, each in iterations of 256."""
    if n_items == 0:
        return []
    cap = min(int(grid_cap), EMIT_GRID) if grid_cap else EMIT_GRID
    eg = max(1, min((n_items + BLOCK - 1) // BLOCK, cap))
    per = (n_items + eg - 1) // eg
    out = []
    for b in range(eg):
        lo, hi = b * per, min((b + 1) * per, n_items)
        out += [(i, min(i + BLOCK, hi)) for i in range(lo, hi, BLOCK)]
    return out


def triple_records(t, fu, fb, proj, keys_on):
    """(records the triple writes, records it leaves to the key items), in the kernel's order."""
    out, cut = [], []
    for x in (2, 1, 0):  # records joined on the object, the predicate, the subject
        if x not in proj:
            continue
        a, b = [y for y in range(3) if y != x]
        for c, other in ((a, b), (b, a)):
            if (c, t[c]) not in fu:
                continue
            lo, hi = min(x, c), max(x, c)  # the key of the condition's and the projected attribute's values
            rec = ((x, ((c, t[c]),)), t[x])
            (cut if keys_on and (lo, hi, t[lo], t[hi]) in fb else out).append(rec)
        if (a, b, t[a], t[b]) in fb:
            out.append(((x, ((a, t[a]), (b, t[b]))), t[x]))
    return out, cut


def key_records(key, proj):
    a, b, va, vb = key
    out = []
    if b in proj:
        out.append(((b, ((a, va),)), vb))
    if a in proj:
        out.append(((a, ((b, vb),)), va))
    return out


def model(arr, ms, projection="spo", keys_on=True, grid_cap=None, table_keys=None):
    """What the one-pass emission of the input does.  table_keys: the keys of the lookup table when they are not all
    frequent keys (--use-ars: the keys no rule implies).  Returns a dict: n_records (what the triples emit before the
    rule), sorted (records into the sort), suppressed, key_items, keys_per_kind, distinct (the record set)."""
    arr = np.asarray(arr).reshape(-1, 3)
    tr = [tuple(int(x) for x in t) for t in arr.tolist()]
    proj = {"spo".index(ch) for ch in projection}
    fu, fb = frequent(arr, ms)
    if table_keys is not None:
        fb = set(table_keys)
    keys = sorted(fb) if keys_on and tr else []
    n = len(tr)
    n_records = suppressed = n_sorted = 0
    distinct = set()
    written = []
    for t in tr:
        out, cut = triple_records(t, fu, fb, proj, bool(keys))
        n_records += len(out) + len(cut)
        suppressed += len(cut)
        written.append(out)
    for lo, hi in windows(n + len(keys), grid_cap):
        seen = set()
        for i in range(lo, hi):
            if i >= n:
                recs = key_records(keys[i - n], proj)
                n_sorted += len(recs)
                distinct.update(recs)
                continue
            for rec in written[i]:
                (x, cond), _ = rec
                if len(cond) == 1 and (x, cond[0][0]) in REPEATING:
                    if rec in seen:
                        continue
                    seen.add(rec)
                n_sorted += 1
                distinct.add(rec)
    per_kind = {k: sum(1 for key in fb if key[:2] == k) for k in KINDS}
    return {"n_records": n_records, "sorted": n_sorted, "suppressed": suppressed, "key_items": len(keys),
            "keys_per_kind": per_kind, "distinct": distinct}


# ---- shapes: the smallest inputs at which the rule can go wrong -----------------------------------------------------

def shape_exact(n=1024):
    """n triples (s_i, P, X), distinct subjects, support 2: one frequent key (p = P, o = X).  Every triple has 5 records
    (o[p]@X, p[o]@P, s[p]@s_i, s[o]@s_i, s[p,o]@s_i); the first two repeat across all triples."""
    arr = np.stack([np.arange(n), np.full(n, n), np.full(n, n + 1)], 1).astype(np.uint32)
    return arr, n + 2, 2


def shape_kinds():
    """One frequent key of each kind at support 3, every value distinct (two values of a key never share a join range
    of one join value each): (s = 0, p = 1) with 4 objects, (s = 10, o = 11) under 4 predicates, (p = 20, o = 21) for 4
    subjects; and a few triples that share one value with a key without holding it."""
    t = [(0, 1, 2 + j) for j in range(4)] + [(10, 12 + j, 11) for j in range(4)] + [(22 + j, 20, 21) for j in range(4)]
    t += [(0, 20, 30), (10, 1, 31), (32, 1, 21), (0, 12, 11), (22, 20, 2)]
    return np.array(t, np.uint32), 33, 3


def shape_no_keys():
    """Frequent predicates only: no binary key, B = 0, and records exist."""
    n = 60
    arr = np.stack([np.arange(n), 200 + np.arange(n) % 3, 100 + np.arange(n)], 1).astype(np.uint32)
    return arr, 203, 2


def shape_more_keys(n, seed=0):
    """Support 1 on n random triples over few terms: nearly three keys per triple, B > n.  The key items fill whole
    blocks; the block that holds the last triples holds the first key items (unless n is a multiple of its size)."""
    rng = np.random.default_rng(4100 + n + seed)
    nv = max(6, n // 2)
    arr = np.stack([rng.integers(0, nv, n), rng.integers(0, nv // 3 + 1, n), rng.integers(0, nv, n)], 1).astype(np.uint32)
    return arr, nv, 1


def shape_empty():
    return np.zeros((0, 3), np.uint32), 1, 1


SHAPES = {
    "kinds": shape_kinds,
    "no_keys": shape_no_keys,
    "empty": shape_empty,
    "more_keys_200": lambda: shape_more_keys(200),
    "more_keys_100": lambda: shape_more_keys(100),
    "more_keys_300": lambda: shape_more_keys(300),
}
PROJECTIONS = ("s", "p", "o", "sp", "so", "po", "spo")
