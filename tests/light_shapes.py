"""Near-miss inputs for the light pass (test infrastructure; plain numpy, no GPU).

The "sets over subjects" model.  Every triple is (x, P_k, fresh object) with every object id unique, so at
``--support 2`` no ``o`` condition and no ``(s, p)`` or ``(p, o)`` condition is frequent.  Under projection ``s`` the
frequent captures are then exactly ``s[p=P_k]``; the join set of ``s[p=P_k]`` is ``S_k``, the subjects that have
predicate ``P_k``; a subject's capture group is ``{k : x in S_k}``; a dependent has ``|S_k|`` groups; its candidates are
the members of its smallest group; and ``s[p=P_a] < s[p=P_b]`` holds iff ``S_a`` is a subset of ``S_b``.

A shape is a dependent ``D = {0..m-1}``, ``n_true`` strict supersets ``D + extras``, ``n_sub`` subsets (``D`` minus two
subjects each: ``D`` is *their* true ref), near-misses ``N_i = (D - {x_i}) + extras`` that lack exactly one subject of
``D``, and a few unrelated sets.  ``D`` has the smallest capture id and one true superset the largest of the plain
form, so a true ref sits at the first and at the last place of the member lists that are searched.  The near-misses
are dependents themselves: their own refs and misses run the same
device code from ``m - 1`` groups.  Every set has >= 2 subjects and every subject >= 2 predicates, so all of it is
frequent at support 2.

How positions map to the device's data (read in rdfind_hip.hip, g_sort_support / k_dgrp, and kernels.inl,
k_light_body): the kept records are sorted by (compact capture, join value) and groups are numbered in join-value
order, so a dependent's ``dgrp`` list ascends in group id = in join value = in term id.  Subjects get the term ids
``0..n_subjects-1`` with ``D`` first, so **position i of D's group list is subject i**: k_light reads it in lane
``i % 64``, slot ``(i / 64) % LIGHT_IT`` of the window ``i / (64 LIGHT_IT)``, in segment ``i / LIGHT_SEG``.  (A heavy
group keeps its place in the list, tagged; the pivot and the second pivot are blanked in place.)  A near-miss that
lacks subject ``x_i`` has the later subjects one position earlier.  Compact capture ids ascend with the external ones,
i.e. with the predicate's term id: candidates ascend by set index.

The miss positions are the point: 0, 63, 64, 127, 128, 191, 192, 255, 256 (lane and slot edges of a LIGHT_IT x 64
window), 2047 / 2048 and 4095 / 4096 (segment edges), ``m - 1``, and a seeded random remainder, as far as ``m`` allows.
Only missed positions have groups smaller than the rest (the subsets drop miss positions too), so D's pivot and its
second pivot, the two smallest groups, are both miss positions by construction (``Shape.pivots`` computes them; the
CPU tests assert it).  Two equal near-misses (one position missed by two identical sets) give the dedup classes a member.
The twins carry four extras, a group count no other set of the shape has: the dedup pass offers a dependent one
candidate representative, the smallest id with its (support, group count, heavy mask, signature) key, and the 512-bit
signature is saturated from ~2000 groups on, so among sets of equal size only a class that holds the smallest id of its
size is found (k_dup_insert; the trues T_1 = T_3 of the multi-segment shapes are equal sets and are not).

Heavy columns.  The library turns the groups of the top quarter-octave size buckets into bit columns while they number
at most HMAX = 64 (heavy_threshold_from_hist), so without further sets a shape has either none or an unpredictable
set of them.  ``ballast=True`` adds 64 ballast subjects of ``D`` (none of them a miss position) that also sit in enough
extra "ballast sets" to be at least twice as large as every other group: they take all 64 columns under the default
heavy setting and under RDFIND_HEAVY_MIN=2, and the missed positions stay light.  The no-ballast form is run with
RDFIND_HEAVY_MIN=1073741824 (no columns: every miss is found by a light search).

Packed edges.  light_plan packs a dependent with ``ng <= 32`` groups when its pivot has at least ``ng`` members, or
with ``ng <= 512`` groups of which at most 16 are light.  A strict superset of a 32-group set has 33 groups, so the
shapes that must prove "no k_light item" have no supersets of ``D``: their true inclusions are ``(subset, D)``, and all
near-misses share one extra subject (a second extra would be a small pivot group).  A dependent has at most HMAX heavy
groups, so "at most 16 light" means at most 80 groups: the second rule's edge is m = 80 / 81 (64 ballast + 16 / 17
light groups), and its 512-group bound cannot be reached by any input.

Shared objects.  With fresh objects no binary condition is frequent, so the minimality rules of the explicit path never
see a near-miss.  ``shared_objects=True`` gives every triple of set ``k`` the one object ``O_k`` instead: ``s[p=P_k]``,
``s[o=O_k]`` and ``s[p=P_k,o=O_k]`` then share the join set ``S_k`` (three twins per set with equal group lists), every
inclusion and every near-miss exists in nine capture combinations, and the rules remove about two thirds of the raw
rows.  Subjects, positions and misses are those of the plain form, so the position model above still holds (private
predicates keep their fresh objects).  The expected rows of this form come from the oracles alone.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

HMAX = 64  # kernels.hpp
LIGHT_SEG = 2048
LIGHT_PACK_MAXG = 32
LIGHT_PACK_NL = 16
LIGHT_SMALL = 31
WINDOW_EDGES = (0, 63, 64, 127, 128, 191, 192, 255, 256)
SEGMENT_EDGES = (2047, 2048, 4095, 4096)
NO_HEAVY = "1073741824"


@dataclass
class Shape:
    name: str
    m: int
    sets: list  # S_k as sorted int64 arrays; set k is predicate P_k
    kind: list  # per set: "D", "true", "sub", "near", "ballast", "other"
    miss: list  # per set: the missed position of a near-miss, else -1
    ballast: np.ndarray  # ballast subjects (empty without)
    n_subjects: int
    s: np.ndarray = field(default=None, repr=False)
    p: np.ndarray = field(default=None, repr=False)
    o: np.ndarray = field(default=None, repr=False)
    num_terms: int = 0
    min_support: int = 2
    n_pred: int = 0  # predicates: the sets' and the private ones
    shared_objects: bool = False

    def obj(self, k: int) -> int:
        """Term id of O_k, the one object of set k in the shared-object form."""
        assert self.shared_objects
        return self.n_subjects + self.n_pred + k

    @property
    def n(self):
        return int(self.s.shape[0])

    def pred(self, k: int) -> int:
        """Term id of P_k = the external capture id of s[p=P_k] (type 0 of the id layout)."""
        return self.n_subjects + k

    def idx(self, kind: str):
        return [k for k, x in enumerate(self.kind) if x == kind]

    def membership(self) -> np.ndarray:
        """bool [n_sets, n_subjects]"""
        mem = np.zeros((len(self.sets), self.n_subjects), bool)
        for k, sk in enumerate(self.sets):
            mem[k, sk] = True
        return mem

    def inclusions(self) -> np.ndarray:
        """Sorted packed keys (P_a << 32 | P_b) of {(a, b): a != b, S_a subset of S_b}, by set algebra alone."""
        mem = self.membership().astype(np.float32)
        size = mem.sum(1)
        inter = mem @ mem.T  # exact: counts < 2^24
        a, b = np.nonzero(inter == size[:, None])
        keep = a != b
        key = ((a[keep] + self.n_subjects).astype(np.uint64) << np.uint64(32)) | (b[keep] + self.n_subjects).astype(np.uint64)
        return np.sort(key)

    def pair_key(self, a: int, b: int) -> np.uint64:
        return np.uint64((self.pred(a) << 32) | self.pred(b))

    def group_sizes(self) -> np.ndarray:
        """Members of every subject's capture group under projection s."""
        return np.bincount(np.concatenate(self.sets), minlength=self.n_subjects)

    def heavy_subjects(self, heavy_min: int) -> np.ndarray:
        """The subjects whose groups become bit columns (projection s): heavy_threshold_from_hist restated."""
        gs = self.group_sizes()
        b = _size_bucket(gs)
        hist = np.bincount(b, minlength=256)
        cum, best = 0, -1
        for q in range(255, -1, -1):
            cum += hist[q]
            if cum > HMAX:
                break
            if hist[q]:
                best = q
        if best < 0:
            return np.zeros(0, np.int64)
        return np.nonzero((b >= best) & (gs >= heavy_min))[0]

    def pivots(self, k: int, heavy=()):
        """(pivot subject, second pivot subject or -1) of set k: the smallest groups by (size, id); the second pivot is
        the smallest light one other than the pivot."""
        gs = self.group_sizes()
        sub = self.sets[k]
        order = sub[np.lexsort((sub, gs[sub]))]
        piv = int(order[0])
        hv = set(int(x) for x in heavy)
        rest = [int(x) for x in order[1:] if int(x) not in hv]
        return piv, (rest[0] if rest else -1)

    def plan(self, heavy=()):
        """Per set (projection s): (groups, light groups, pivot size, packed) as light_plan decides."""
        gs = self.group_sizes()
        hv = np.zeros(self.n_subjects, bool)
        hv[np.asarray(heavy, np.int64)] = True
        out = []
        for sk in self.sets:
            ng, nl, sz = len(sk), int((~hv[sk]).sum()), int(gs[sk].min())
            packed = (ng <= LIGHT_PACK_MAXG and ng <= max(sz, 4)) or (ng <= 512 and nl <= LIGHT_PACK_NL)
            out.append((ng, nl, sz, packed))
        return out


def _size_bucket(n):
    """Quarter-octave size buckets (kernels.inl size_bucket)."""
    n = np.asarray(n, np.int64)
    msb = np.floor(np.log2(np.maximum(n, 1))).astype(np.int64)
    frac = np.where(msb >= 2, (n >> np.maximum(msb - 2, 0)) & 3, (n << np.maximum(2 - msb, 0)) & 3)
    return np.where(n == 0, 0, msb * 4 + frac)


def miss_positions(m: int, n_near: int, rng, avoid=()) -> list:
    """n_near distinct positions of D's group list: the window and segment edges that fit and m - 1 first, then a
    seeded random remainder."""
    avoid = set(int(x) for x in avoid)
    want = [q for q in WINDOW_EDGES + SEGMENT_EDGES + (m - 1,) if q < m and q not in avoid]
    pos = list(dict.fromkeys(want))[:n_near]
    free = np.array([q for q in range(m) if q not in avoid and q not in set(pos)], np.int64)
    extra = rng.choice(free, size=min(max(n_near - len(pos), 0), len(free)), replace=False)
    return pos + sorted(int(x) for x in extra)


def make(name: str, m: int, n_true: int, n_near: int, *, n_sub: int = 0, ballast: bool = False, one_extra: bool = False,
         n_other: int = 3, private_from: int = -1, seed: int = 1, shared_objects: bool = False) -> Shape:
    """Build a shape.  one_extra: every near-miss adds the same single extra subject (the packed-edge shapes).  One
    near-miss is repeated as an identical set (equal group lists for the dedup classes).  private_from >= 0: every
    subject of D from that position on also has a predicate of its own (one triple: an infrequent condition, so
    projection s sees nothing of it); under projection spo it keeps the p[s=x] captures of the subjects of D, which
    otherwise all have the same predicates, from including each other (m^2 rows).  shared_objects: one object per set
    instead of one per triple (the module's docstring)."""
    rng = np.random.default_rng(seed)
    D = np.arange(m, dtype=np.int64)
    bal = np.zeros(0, np.int64)
    if ballast:
        assert m >= HMAX + 2
        # not on an edge position: the interesting positions stay light
        edges = set(q for q in WINDOW_EDGES + SEGMENT_EDGES + (m - 1,) if q < m)
        free = np.array([q for q in range(m) if q not in edges], np.int64)
        if len(free) < HMAX:  # (m = 80 / 81: the light positions are what is left)
            free = np.arange(m, dtype=np.int64)[: HMAX]
        bal = np.sort(rng.choice(free, size=HMAX, replace=False)) if len(free) > HMAX else free
    pos = miss_positions(m, n_near, rng, avoid=bal)
    n_extra = 1 if one_extra else 6
    x0 = m  # extras' subject ids
    other0 = x0 + n_extra
    sets, kind, miss = [D], ["D"], [-1]
    for j in range(max(n_true - 1, 0)):
        e = x0 + np.array(sorted({j % n_extra, (j * 2 + 1) % n_extra}), np.int64)
        sets.append(np.concatenate([D, e]))
        kind.append("true")
        miss.append(-1)
    for j in range(n_sub):
        drop = sorted({pos[(3 * j + 1) % len(pos)], pos[(3 * j + 2) % len(pos)]})  # miss positions: see the pivots
        sets.append(np.setdiff1d(D, np.array(drop, np.int64)))
        kind.append("sub")
        miss.append(-1)
    for j, q in enumerate(pos):
        e = x0 + (np.array([0], np.int64) if one_extra else np.array(sorted({j % n_extra, (j // n_extra + j + 3) % n_extra}), np.int64))
        if j == len(pos) - 1 and not one_extra:
            e = x0 + np.arange(4, dtype=np.int64)  # the twins: a group count no other set has (see the docstring)
        sets.append(np.concatenate([np.delete(D, q), e]))
        kind.append("near")
        miss.append(int(q))
    if pos:  # an identical twin of the last near-miss
        sets.append(sets[-1].copy())
        kind.append("near")
        miss.append(int(pos[-1]))
    # unrelated sets: a slice of D with other subjects, and sets of other subjects alone
    assert n_other == 0 or n_other >= 3
    n_os = 5 if n_other else 0
    others = other0 + np.arange(n_os, dtype=np.int64)
    for j in range(n_other):
        part = D[j::3][: max(2, min(m // 3, 40))] if j % 2 == 0 else np.zeros(0, np.int64)
        sets.append(np.concatenate([part, others[np.arange(n_os) != (j % n_os)]]))
        kind.append("other")
        miss.append(-1)
    if n_true:  # the last true superset has the largest capture id: the last member of every light group of D
        sets.append(np.concatenate([D, x0 + np.array([2, 4], np.int64)]))
        kind.append("true")
        miss.append(-1)
    n_subjects = other0 + n_os
    if ballast:
        gs = np.bincount(np.concatenate(sets), minlength=n_subjects)
        nb = max(int(gs.max()) + 8, 72)  # ballast groups: more than twice any other group and >= 64 members
        for _ in range(nb):
            sets.append(bal.copy())
            kind.append("ballast")
            miss.append(-1)
    sets = [np.sort(x) for x in sets]
    sh = Shape(name, m, sets, kind, miss, bal, n_subjects)
    sizes = np.array([len(x) for x in sets])
    priv = np.arange(private_from, m, dtype=np.int64) if 0 <= private_from < m else np.zeros(0, np.int64)
    n_pred = len(sets) + len(priv)
    sh.s = np.concatenate(sets + [priv]).astype(np.uint32)
    sh.p = np.concatenate([np.repeat(n_subjects + np.arange(len(sets)), sizes),
                           n_subjects + len(sets) + np.arange(len(priv))]).astype(np.uint32)
    if shared_objects:  # O_k per set; the private predicates' triples keep objects of their own
        sh.o = (n_subjects + n_pred + np.concatenate([np.repeat(np.arange(len(sets)), sizes),
                                                      len(sets) + np.arange(len(priv))])).astype(np.uint32)
        n_obj = len(sets) + len(priv)
    else:
        sh.o = (n_subjects + n_pred + np.arange(sh.s.shape[0])).astype(np.uint32)
        n_obj = sh.s.shape[0]
    perm = rng.permutation(sh.s.shape[0])  # triples in no particular order
    sh.s, sh.p, sh.o = sh.s[perm], sh.p[perm], sh.o[perm]
    sh.num_terms = int(n_subjects + n_pred + n_obj)
    sh.n_pred, sh.shared_objects = n_pred, bool(shared_objects)
    assert min(len(x) for x in sets) >= 2 and np.bincount(np.concatenate(sets), minlength=n_subjects).min() >= 2
    return sh


# name -> (make arguments, the class of the shape).  n_true + n_near (+ the twin) + D = the candidates of D's pivot.
SPECS = {
    # packed edges: 32 | 33 groups (rule 1), 80 | 81 groups with 16 | 17 light (rule 2, ballast + RDFIND_HEAVY_MIN=2)
    "pack32": (dict(m=32, n_true=0, n_near=31, n_sub=3, one_extra=True, n_other=0), "packed"),
    "pack33": (dict(m=33, n_true=0, n_near=31, n_sub=3, one_extra=True, n_other=0), "packed_over"),
    "pack80h": (dict(m=80, n_true=0, n_near=14, n_sub=2, one_extra=True, n_other=0, ballast=True), "packed"),
    "pack81h": (dict(m=81, n_true=0, n_near=14, n_sub=2, one_extra=True, n_other=0, ballast=True), "packed_over"),
    # one segment, every light group <= LIGHT_SMALL members
    "small300": (dict(m=300, n_true=5, n_near=20, n_sub=2), "one_seg"),
    # one segment, many candidates: D's pivot group has at most n_true + n_near + n_sub members: both sides of a chunk of 64 candidates and of a last chunk of fewer than 8 octets
    "cand63": (dict(m=301, n_true=6, n_near=55, n_sub=2), "one_seg"),
    "cand64": (dict(m=300, n_true=6, n_near=56, n_sub=2), "one_seg"),
    "cand65": (dict(m=299, n_true=6, n_near=57, n_sub=2), "one_seg"),
    "cand129": (dict(m=300, n_true=8, n_near=119, n_sub=2), "one_seg"),
    # two and three segments, two and three chunks
    "seg2": (dict(m=2049, n_true=6, n_near=64, n_sub=2, private_from=300), "multi_seg"),
    "seg3": (dict(m=4100, n_true=8, n_near=121, n_sub=2, private_from=300), "multi_seg"),
}
# (the shapes whose miss positions must stay light under the default heavy setting get a ballast form)
BALLAST_FORMS = ("small300", "cand63", "cand64", "cand65", "cand129", "seg2", "seg3")
_CACHE: dict = {}


def shape(name: str, ballast: bool = False, shared_objects: bool = False) -> Shape:
    """The named shape, built once per process.  ballast: its form for the default heavy setting (64 columns taken by
    ballast subjects); without: the form for RDFIND_HEAVY_MIN=NO_HEAVY.  The pack80h / pack81h shapes always carry
    ballast (they run under RDFIND_HEAVY_MIN=2).  shared_objects: one object per set (name suffix "+o"): the same sets,
    subjects and seed as the plain form."""
    key = (name, bool(ballast), bool(shared_objects))
    if key not in _CACHE:
        kw = dict(SPECS[name][0])
        if ballast:
            kw["ballast"] = True
        _CACHE[key] = make(name + ("+b" if ballast else "") + ("+o" if shared_objects else ""),
                           seed=len(name) * 131 + kw["m"], shared_objects=shared_objects, **kw)
    return _CACHE[key]


def shape_class(name: str) -> str:
    return SPECS[name][1]
