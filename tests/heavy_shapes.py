"""Edge inputs for the heavy columns and the mask classes (test infrastructure; plain numpy, no GPU).

The "sets over subjects" model of tests/light_shapes.py, turned towards the heavy path.  Every triple is
(x, P_k, fresh object); under projection ``s`` at support 2 the captures are ``s[p=P_k]`` with join set ``S_k``, a
subject's capture group is the set of captures that hold it, and ``s[p=P_a] < s[p=P_b]`` iff ``S_a`` is a subset of
``S_b``.  The groups of the top quarter-octave size buckets become the bit columns of ``hmask`` while they number at
most HMAX (``Shape.heavy_subjects``, the rule restated in tests/light_shapes.py); a dependent all of whose subjects are
heavy is *heavy-only*; the heavy-only dependents with the same subject set ``m`` form a *class*; the class's pivot is
the smallest group of ``m`` by (size, subject id), and its list ``L(m)`` holds the members of the pivot group whose
subjects include all of ``m``, ascending by capture id.  With unary captures only no rule removes a ref, so
``L'(m) = L(m)``, each member's refs are ``L'(m)`` minus itself, and the result is the same in all four modes.

Column numbers are handed out in atomicAdd order on the device, so no shape aims at a bit position: where every bit
position is wanted, every column is missed once.

Each shape carries its own model (``HShape``): the heavy subjects and the threshold under its RDFIND_HEAVY_MIN, the
classes with members, pivot groups, lists and the members' own positions, the counts the device reports
(``class_stats``), and the rows by set algebra over groups of equal sets (``rows``; nothing is sized sets x sets).

Families.

A. Columns and threshold.  ``cols64`` / ``cols64x9``: 64 heavy subjects H; the dependent H itself (a mask of 64 ones;
   1 member, or 9: two tiles of CLS_DT = 8); for every j the heavy-only near-miss ``H - {h_j}`` (63 columns, alone in
   its class) and the near-miss ``(H - {h_j}) + {a light subject}``, which is not heavy-only and meets the mask test as
   a candidate of the explicit path and of the class lists; true supersets ``H + {light}``; sub-masks of 2 and 3
   columns.  ``cols6`` is the same generator with 6 columns (small enough for the Python restatement of mode
   (1, raw)).  ``thr_*``: group-size histograms that put one edge of the threshold rule in force each.
B. List lengths and emission.  ``emit16k`` / ``emit32k``: three heavy subjects with every predicate, K long captures
   (the three plus a private subject: pivot = the private group of one, no refs, cheap) and M members on the three
   alone: one class, one list of K + M refs (two / three CLS_LS segments), M runs of K + M - 1 refs.  K + M is even, so
   a run is odd and consecutive runs start at every residue mod 64 of the output.  The predicates are numbered so that
   the members sit at chosen places of the list.  ``emit300`` is the same generator at K = 301, where both oracles
   check the set algebra.  ``lists_small``: disjoint two-subject classes with list lengths 1 (three of them: the
   member alone), 2, 32, 33, 63, 64, 65, 128, 129 and 1, 7, 8, 9, 17 members, every subject heavy under
   RDFIND_HEAVY_MIN=2.

C, D. Shared objects (``r3_shape`` / ``SShape`` below): triples (h, P, O_j) make s[p=P,o=O_j] a frequent binary capture,
   a parent of s[p=P] and of s[o=O_j].  One input carries R3 inside a class (parent lists on both sides of
   PARENT_SCAN_MAX with the covering parent at chosen places) and binary heavy-only dependents with class lists of 63,
   64, 65 and 129 entries.  Its expected rows are the C oracle's; its model gives the parent lists, the places in the
   pivot groups, the lists L'(m) and the counts the device reports.
   ``r3`` also holds the marks' edges (a chunk with six long components, a component run across a chunk cut, an R in a
   last partly filled chunk) and a binary dependent with a mask of its own; ``r3s`` is the same generator reduced to
   706 triples, for the cells whose only oracle is the Python restatement ((1, raw), association rules).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import light_shapes as L
from tests.light_shapes import HMAX, _size_bucket

CLS_DT = 8  # kernels.inl
CLS_LS = 16384
WAVE = 64
DEFAULT_HEAVY_MIN = 64  # switches.hpp


@dataclass
class HShape(L.Shape):
    heavy_min: int = DEFAULT_HEAVY_MIN  # the RDFIND_HEAVY_MIN the shape runs under
    algebra_raw_s2l: bool = False  # mode (1, raw) expects rows(): the Python restatement takes too long at this size
    want: dict = field(default_factory=dict)  # what the generator promises; the CPU tests assert it from the model

    def group_sizes(self) -> np.ndarray:  # (computed once: the searches below ask for it per set)
        if "_gs" not in self.__dict__:
            self.__dict__["_gs"] = super().group_sizes()
        return self.__dict__["_gs"]

    # -- heavy columns ------------------------------------------------------------------------------------------------
    def heavy(self) -> np.ndarray:
        return self.heavy_subjects(self.heavy_min)

    def threshold(self) -> int:
        """heavy_threshold as the library reports it: the smallest size of the lowest bucket the rule takes, at least
        RDFIND_HEAVY_MIN; 0 when the rule takes no bucket."""
        top = self.heavy_subjects(1)
        if not top.size:
            return 0
        best = int(_size_bucket(self.group_sizes()[top]).min())
        n = np.arange(1, 1 << 20)
        return max(int(n[_size_bucket(n) == best][0]), self.heavy_min)

    # -- classes ------------------------------------------------------------------------------------------------------
    def groups_of(self) -> list:
        """Per subject: the sets that hold it, ascending (the capture group's members in device order)."""
        if "_grp" not in self.__dict__:
            sizes = np.array([len(x) for x in self.sets])
            owner = np.repeat(np.arange(len(self.sets)), sizes)
            subj = np.concatenate(self.sets)
            order = np.lexsort((owner, subj))
            cut = np.searchsorted(subj[order], np.arange(self.n_subjects + 1))
            self.__dict__["_grp"] = [owner[order[cut[x]:cut[x + 1]]] for x in range(self.n_subjects)]
        return self.__dict__["_grp"]

    def _holds(self, cand: np.ndarray, x: int) -> np.ndarray:
        """cand[i] holds subject x."""
        g = self.groups_of()[x]
        if g.size < 64:
            return np.isin(cand, g, assume_unique=True)
        cache = self.__dict__.setdefault("_gmask", {})
        if x not in cache:
            cache[x] = np.zeros(len(self.sets), bool)
            cache[x][g] = True
        return cache[x][cand]

    def supersets(self, sub: np.ndarray) -> np.ndarray:
        """The sets that hold every subject of sub, ascending: the smallest group, filtered by the others."""
        gs = self.group_sizes()
        order = sub[np.lexsort((sub, gs[sub]))]
        cand = self.groups_of()[int(order[0])]
        for x in order[1:]:
            cand = cand[self._holds(cand, int(x))]
        return cand

    def heavy_only(self) -> list:
        hv = np.zeros(self.n_subjects, bool)
        hv[self.heavy()] = True
        return [k for k, sk in enumerate(self.sets) if hv[sk].all()]

    def classes(self) -> list:
        """One dict per class: mask (the subjects), members (set indices, ascending), pivot (subject), group (the pivot
        group's sets), L (the list), selfpos (member -> its place in L)."""
        if "_cls" in self.__dict__:
            return self.__dict__["_cls"]
        by_mask: dict = {}
        for k in self.heavy_only():
            by_mask.setdefault(self.sets[k].tobytes(), []).append(k)
        out = []
        for ks in by_mask.values():
            sub = self.sets[ks[0]]
            piv, _ = self.pivots(ks[0])
            lst = self.supersets(sub)
            pos = np.searchsorted(lst, ks)
            assert (lst[pos] == ks).all()  # with unary captures alone a member is always in its own list
            out.append(dict(mask=sub, members=ks, pivot=piv, group=self.groups_of()[piv], L=lst,
                            selfpos=dict(zip(ks, pos.tolist()))))
        self.__dict__["_cls"] = out
        return out

    def class_stats(self) -> dict:
        """What the device reports for the class path (rdf_cind_stats and rdf_test_paths)."""
        cl = self.classes()
        lens = [len(c["L"]) for c in cl]
        return dict(
            n_classes=len(cl), n_class_members=sum(len(c["members"]) for c in cl),
            n_class_cinds=sum(len(c["members"]) * (len(c["L"]) - 1) for c in cl),
            n_class_chunks=sum(-(-len(c["group"]) // WAVE) for c in cl),
            n_emit_tiles=sum(-(-len(c["members"]) // CLS_DT) * -(-len(c["L"]) // CLS_LS) for c in cl),
            max_class_list=max(lens, default=0), n_multi_seg_lists=sum(n > CLS_LS for n in lens))

    # -- the result by set algebra -----------------------------------------------------------------------------------
    def rows(self):
        """(sorted dep << 32 | ref keys, supports in that order) of {(a, b): a != b, S_a subset of S_b}; support |S_a|.
        Equal sets are grouped: one superset search per distinct set."""
        distinct: dict = {}
        for k, sk in enumerate(self.sets):
            distinct.setdefault(sk.tobytes(), []).append(k)
        deps, refs = [], []
        for ks in distinct.values():
            sup = self.supersets(self.sets[ks[0]])
            for k in ks:
                r = sup[sup != k]
                deps.append(np.full(r.size, k, np.int64))
                refs.append(r)
        dep, ref = np.concatenate(deps), np.concatenate(refs)
        size = np.array([len(x) for x in self.sets], np.uint32)
        key = ((dep + self.n_subjects).astype(np.uint64) << np.uint64(32)) | (ref + self.n_subjects).astype(np.uint64)
        order = np.argsort(key, kind="stable")
        return key[order], size[dep][order]


def rows_struct(keys: np.ndarray, sup: np.ndarray) -> np.ndarray:
    """Packed rows as the dep / ref / support array the checker's checksum takes."""
    out = np.zeros(keys.shape[0], dtype=[("dep", "<u4"), ("ref", "<u4"), ("support", "<u4")])
    out["dep"], out["ref"], out["support"] = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF), sup
    return out


def _finish(name: str, sets: list, kind: list, n_subjects: int, seed: int, **kw) -> HShape:
    """Triples of the sets (set k is predicate P_k), in no particular order, every object fresh."""
    sets = [np.sort(np.asarray(x, np.int64)) for x in sets]
    assert len(sets) == len(kind) and min(len(x) for x in sets) >= 2  # every capture is frequent at support 2
    assert all(np.unique(x).size == x.size for x in sets)
    sh = HShape(name, 0, sets, kind, [-1] * len(sets), np.zeros(0, np.int64), n_subjects, **kw)
    assert sh.group_sizes().min() >= 1  # every subject id is a term that occurs: group ids ascend with subject ids
    sizes = np.array([len(x) for x in sets])
    rng = np.random.default_rng(seed)
    s = np.concatenate(sets)
    p = np.repeat(n_subjects + np.arange(len(sets)), sizes)
    perm = rng.permutation(s.shape[0])
    sh.s, sh.p = s[perm].astype(np.uint32), p[perm].astype(np.uint32)
    sh.o = (n_subjects + len(sets) + np.arange(s.shape[0])).astype(np.uint32)
    sh.num_terms = int(n_subjects + len(sets) + s.shape[0])
    return sh


# ---------------------------------------------------------------------------------------------------------------------
# family A

N_LIGHT = 4
SUBMASKS = ((0, 1), (-2, -1), (0, -1), (0, 1, 2), (-3, -2, -1))  # columns by index into H (2 and 3 of them)


def cols(name: str, nh: int, n_full: int, seed: int = 7) -> HShape:
    """nh heavy subjects H = 0..nh-1, N_LIGHT light ones behind them."""
    H = np.arange(nh, dtype=np.int64)
    light = nh + np.arange(N_LIGHT, dtype=np.int64)
    sets, kind = [], []
    mid = (nh // 2 - 1, nh // 2) if nh >= 8 else None  # (nh = 64: columns 31 | 32, whatever bits they get)
    for cols_ in SUBMASKS + ((mid,) if mid else ()):
        sets.append(H[list(cols_)])
        kind.append("submask")
    for _ in range(n_full):
        sets.append(H)
        kind.append("full")
    for j in range(nh):
        sets.append(np.delete(H, j))
        kind.append("near_heavy")
    for j in range(nh):
        sets.append(np.concatenate([np.delete(H, j), light[[j % N_LIGHT]]]))
        kind.append("near_light")
    for a in light:
        sets.append(np.concatenate([H, [a]]))
        kind.append("true")
    # (fewer than HMAX groups in all: the rule takes every bucket, and only the minimum keeps the light subjects light)
    sh = _finish(name, sets, kind, nh + N_LIGHT, seed, heavy_min=DEFAULT_HEAVY_MIN if nh == HMAX else 10)
    sh.want = dict(n_heavy=nh, H=H, light=light)
    return sh


def threshold(name: str, sizes: list, heavy_min: int, n_heavy: int, thr: int, seed: int = 3) -> HShape:
    """Subjects with the given group sizes: subject x has the predicates P_0 .. P_{sizes[x] - 1}."""
    sizes = np.asarray(sizes, np.int64)
    sets = [np.nonzero(sizes > k)[0] for k in range(int(sizes.max()))]
    sh = _finish(name, sets, ["chain"] * len(sets), len(sizes), seed, heavy_min=heavy_min)
    assert sh.group_sizes().tolist() == sizes.tolist()
    sh.want = dict(n_heavy=n_heavy, threshold=thr)
    return sh


# name -> (group sizes as (count, size) runs, RDFIND_HEAVY_MIN, expected columns, expected threshold).  Sizes 64 .. 79
# share bucket 24, 80 .. 95 are bucket 25, 48 .. 55 bucket 22; the 9 groups of 8 keep the walk from running out.
THRESHOLDS = {
    "thr_top64": ([(64, 64), (9, 8)], 2, 64, 64),
    "thr_top65": ([(65, 64), (9, 8)], 2, 0, 0),
    "thr_60p4": ([(60, 64), (4, 48), (9, 8)], 2, 64, 48),
    "thr_60p5": ([(60, 64), (5, 48), (9, 8)], 2, 60, 64),
    "thr_ends_in": ([(30, 80), (20, 79), (14, 64), (5, 63)], 2, 64, 64),  # 64 and 79 at the ends of the lowest bucket taken
    "thr_ends_out": ([(60, 80), (3, 79), (2, 64), (5, 63)], 2, 60, 80),  # ... and of the first one refused
    "thr_min70": ([(30, 80), (20, 79), (14, 64), (5, 63)], 70, 50, 70),  # RDFIND_HEAVY_MIN inside bucket 24: the 64s stay light
    "thr_min_default": ([(10, 100), (5, 63), (9, 8)], DEFAULT_HEAVY_MIN, 10, 64),  # every bucket taken; the default minimum cuts
}


# ---------------------------------------------------------------------------------------------------------------------
# family B

def emit(name: str, K: int, member_pos: tuple, M: int, seed: int = 11, algebra: bool = True) -> HShape:
    """Three heavy subjects 0, 1, 2 under all K + M predicates; the members (sets {0, 1, 2}) at the list places
    member_pos (negative: from the end) and at seeded random ones up to M of them; every other predicate is a long
    capture {0, 1, 2, a private subject}."""
    n = K + M
    assert n % 2 == 0  # an odd run: consecutive runs start at every residue mod 64
    rng = np.random.default_rng(seed)
    pos = sorted({q % n for q in member_pos})
    assert len(pos) == len(member_pos) <= M
    free = np.setdiff1d(np.arange(n), pos)
    pos = np.sort(np.concatenate([pos, rng.choice(free, size=M - len(pos), replace=False)]).astype(np.int64))
    is_member = np.zeros(n, bool)
    is_member[pos] = True
    H = np.arange(3, dtype=np.int64)
    private = 3 + np.cumsum(~is_member) - 1
    sets = [H if is_member[k] else np.concatenate([H, [private[k]]]) for k in range(n)]
    kind = ["member" if x else "long" for x in is_member]
    sh = _finish(name, sets, kind, 3 + K, seed, algebra_raw_s2l=algebra)
    sh.want = dict(n_heavy=3, member_pos=pos, list_len=n, edges=sorted(q % n for q in member_pos))
    return sh


EMIT16K_POS = (0, 1, 31, 32, 33, 16351, 16352, 16383, 16384, 16385, -2, -1)
EMIT32K_POS = (0, 16383, 16384, 16385, 32767, 32768, 32769, -2, -1)

LIST_SPECS = ((1, 1), (2, 1), (32, 7), (33, 8), (63, 9), (64, 17), (65, 1), (128, 8), (129, 9))  # (list length, members)


def lists_small(name: str = "lists_small", seed: int = 5) -> HShape:
    """Class c > 0 has the subjects {2c, 2c + 1}, its members are that set, and its list is filled up with strict
    supersets {2c, 2c + 1, z}, z a subject of another class.  The list of length 1 is a set of two subjects of different
    classes: nothing else holds both."""
    nc = len(LIST_SPECS)
    n_subjects = 2 * nc
    lone = [c for c, (ln, _) in enumerate(LIST_SPECS) if ln == 1]
    lone_subjects = np.array([x for c in lone for x in (2 * c, 2 * c + 1)], np.int64)
    sets, kind = [], []
    for c, (ln, nm) in enumerate(LIST_SPECS):
        if ln == 1:
            continue
        own = np.array([2 * c, 2 * c + 1], np.int64)
        others = np.setdiff1d(np.arange(n_subjects), np.concatenate([own, lone_subjects]))
        for _ in range(nm):
            sets.append(own)
            kind.append("member")
        for j in range(ln - nm):
            sets.append(np.concatenate([own, others[[(j * 5 + c) % others.size]]]))
            kind.append("filler")
    for c in lone:  # the pair, and each of the two with a subject of another class: three lists of one (no filler holds
        # a lone subject), and both lone groups have two members, so they are columns under RDFIND_HEAVY_MIN=2
        sets += [np.array([2 * c, 2 * c + 1], np.int64), np.array([2 * c, 2 * ((c + 1) % nc)], np.int64),
                 np.array([2 * c + 1, 2 * ((c + 2) % nc)], np.int64)]
        kind += ["lone"] * 3
    sh = _finish(name, sets, kind, n_subjects, seed, heavy_min=2)
    sh.want = dict(n_heavy=n_subjects)
    return sh


# ---------------------------------------------------------------------------------------------------------------------
# families C and D: shared objects, hence binary captures

PARENT_SCAN_MAX = 32  # kernels.inl
R3_QS = (1, 31, 32, 33, 64, 65, 200)
D_LISTS = (63, 64, 65, 129)


@dataclass
class SShape:
    """An input with shared objects and its capture-level model under projection ``s`` at support 2: the captures
    s[p=P], s[o=O], s[p=P,o=O] in device order (unary before binary, each by ascending key), their join sets, the
    parents of every unary capture in plist order, and the subjects' groups."""
    name: str
    n_subjects: int
    s: np.ndarray
    p: np.ndarray
    o: np.ndarray
    num_terms: int
    mask: tuple  # the class m the R3 variants are built around
    preds: dict  # predicate term id -> dict(q=parents, variant=..., cover=[indices into its parent list])
    min_support: int = 2
    heavy_min: int = 2

    @property
    def n(self):
        return int(self.s.shape[0])

    def model(self) -> dict:
        if "_m" in self.__dict__:
            return self.__dict__["_m"]
        by = {"p": {}, "o": {}, "po": {}}
        for x, pp, oo in zip(self.s.tolist(), self.p.tolist(), self.o.tolist()):
            by["p"].setdefault((pp,), set()).add(x)
            by["o"].setdefault((oo,), set()).add(x)
            by["po"].setdefault((pp, oo), set()).add(x)
        caps = [dict(kind=k, key=key, subj=tuple(sorted(v))) for k in ("p", "o", "po")
                for key, v in sorted(by[k].items()) if len(v) >= self.min_support]
        index = {(c["kind"], c["key"]): i for i, c in enumerate(caps)}
        cu = sum(c["kind"] != "po" for c in caps)
        parents = [[] for _ in caps]
        for i, c in enumerate(caps):  # ascending binary id: a unary capture's parents in plist order
            if c["kind"] == "po":
                parents[index[("p", c["key"][:1])]].append(i)
                parents[index[("o", c["key"][1:])]].append(i)
        groups = [[] for _ in range(self.n_subjects)]
        for i, c in enumerate(caps):
            for x in c["subj"]:
                groups[x].append(i)
        self.__dict__["_m"] = dict(caps=caps, index=index, cu=cu, parents=parents, groups=groups)
        return self.__dict__["_m"]

    def group_sizes(self):
        return np.array([len(g) for g in self.model()["groups"]])

    def heavy(self):
        """Every subject: at most HMAX groups in all, each of at least RDFIND_HEAVY_MIN = 2 members."""
        gs = self.group_sizes()
        assert len(gs) <= HMAX and gs.min() >= self.heavy_min
        return np.arange(self.n_subjects)

    def threshold(self) -> int:
        """Every bucket is taken: the smallest size of the lowest one, at least RDFIND_HEAVY_MIN."""
        best = int(_size_bucket(self.group_sizes()).min())
        n = np.arange(1, 1 << 20)
        return max(int(n[_size_bucket(n) == best][0]), self.heavy_min)

    def pivot(self, subj) -> int:
        gs = self.group_sizes()
        return min(subj, key=lambda x: (gs[x], x))

    def covers(self, i, m) -> bool:
        return set(m) <= set(self.model()["caps"][i]["subj"])

    def class_list(self, m, clean: bool) -> list:
        """L'(m): the pivot group's captures that cover m; clean: minus the unary ones with a parent that covers m (R3)."""
        M = self.model()
        out = []
        for i in M["groups"][self.pivot(m)]:
            if not self.covers(i, m):
                continue
            if clean and i < M["cu"] and any(self.covers(x, m) for x in M["parents"][i]):
                continue
            out.append(i)
        return out

    def class_stats(self, clean: bool, binary_classed: bool) -> dict:
        """Every capture is heavy-only here.  The members are the unary captures; with binary_classed (the class path
        of strategy 1) the binary captures' masks are classes too."""
        M = self.model()
        masks = {}
        for i, c in enumerate(M["caps"]):
            if i < M["cu"] or binary_classed:
                masks.setdefault(c["subj"], []).append(i)
        gs = self.group_sizes()
        st = dict(n_classes=len(masks), n_class_members=M["cu"], n_class_cinds=0,
                  n_class_chunks=sum(-(-int(gs[self.pivot(m)]) // WAVE) for m in masks), scan_chunks=0, absent=[])
        for m, ids in masks.items():
            lst = self.class_list(m, clean)
            for i in ids:
                if i < M["cu"]:
                    st["n_class_cinds"] += len(lst) - (i in lst)
                    if i not in lst:
                        st["absent"].append(i)
        st["scan_chunks"] = sum(-(-int(gs[self.pivot(c["subj"])]) // WAVE) for c in M["caps"][M["cu"]:])
        return st


N_LACKPIV = 12  # predicates whose only binary in m's pivot group is the covering one: >= 6 of them share a chunk
N_TAIL_FILL = 64  # plain members of the tail class: its R stands at place 64, in the group's last chunk of three


def r3_shape(name: str = "r3", qs=R3_QS, d_lists=D_LISTS, n_spare: int = 40, full: bool = True, seed: int = 13) -> SShape:
    """The class m = {0, 1}; spare subjects 2 ..; for every q of qs and every variant a predicate P whose unary
    capture R = s[p=P] covers m (two triples with fresh objects) and has q parents s[p=P,o=O_j], the objects ascending
    with j.  A parent covers m (join set {0, 1}) or lacks exactly one column of it (join set {0, spare} / {1, spare},
    alternating).  Variants: none covers; exactly one, the first, the last, the 32nd or the 33rd of plist; two, the first
    and the last; all (q <= 33).  Plain members of m (fresh objects), and one member whose own single parent covers m.

    Family D: for every k of d_lists two subjects of their own under one predicate with k shared objects: k binary
    dependents s[p=P,o=O] with the same mask, whose list holds them, their components s[p=P] and s[o=O] (trivial refs;
    R2 / R3 clear them under --clean-implied, leaving exactly k entries) and each other.

    full (the shape r3; without, a reduced input small enough for the Python restatement):
    * the predicates are numbered so that the R of three cleared variants with 200 parents sit at places 0, 63 and 64
      of m's pivot group (the s[p=.] captures come first in a group), every covering binary in a later chunk;
    * `all65`: 65 covering parents of one predicate, consecutive in the pivot group: the run of binaries sharing
      component 0 crosses from lane 63 of one chunk into lane 0 of the next wherever it starts;
    * `lackpiv` x N_LACKPIV: 33 parents, one covering, the others {0, spare}: they lack the pivot subject 1 (group 0 is
      the larger one), so of each predicate only the covering binary is in the pivot group, and these stand next to
      each other: one chunk holds >= 6 binaries with distinct components of more than PARENT_SCAN_MAX parents;
    * the tail class {e0, e1} (two subjects of their own): N_TAIL_FILL plain members, then R with 33 parents, the last
      covering, the others {e0, spare}: the pivot group of e1 is 64 members, R at place 64, its covering s[o=O] and
      binary at 65 and 66: R, cleared by the marks, lies in the last, partly filled chunk with the binary that clears it;
    * one binary dependent whose mask {0, 2, 3} no unary capture has (its object is shared by a second predicate, its
      predicate has one more subject): a class that exists only where the binary dependents are classed."""
    nd = len(d_lists)
    ns = 2 + n_spare + 2 * nd + (2 if full else 0)
    specs = []
    for q in qs:
        var = [("none", []), ("first", [0]), ("last", [q - 1])]
        if q >= 33:
            var += [("p32", [31]), ("p33", [32])]
        if q >= 64:
            var += [("two", [0, q - 1])]
        if q <= 33:
            var += [("all", list(range(q)))]
        specs += [(q, v, cov) for v, cov in var]
    if full:
        specs = specs[-1:] + specs[:-1]  # (200, two) first: place 0; (200, p32) and (200, p33) last: places 63 and 64
    n_members = 65 - len(specs) if full else 3
    extra = ([(65, "all65", list(range(65)))] + [(33, "lackpiv", [16])] * N_LACKPIV) if full else []
    n_pred = len(specs) + n_members + 1 + nd + len(extra) + ((N_TAIL_FILL + 1 + 2) if full else 0)
    P0 = ns
    O0 = ns + n_pred
    tri, preds, obj, spare = [], {}, O0, 0
    fresh = []  # (s, p) triples that get a fresh object each

    def parents(P, q, cov, pair=(0, 1), lack=None):
        nonlocal obj, spare
        for j in range(q):
            if j in cov:
                subj = pair
            else:
                subj = (pair[j % 2] if lack is None else lack, 2 + spare % n_spare)
                spare += 1
            tri.extend((x, P, obj) for x in subj)
            obj += 1

    for k, (q, v, cov) in enumerate(specs):
        P = P0 + ((0 if k == 0 else n_members + k) if full else k)  # full: the plain members take the predicates 1 .. n_members
        preds[P] = dict(q=q, variant=v, cover=cov)
        fresh += [(0, P), (1, P)]
        parents(P, q, cov)
    for k in range(n_members):
        Pm = P0 + (1 + k if full else len(specs) + k)
        fresh += [(0, Pm), (1, Pm)]
    PX = P0 + len(specs) + n_members  # the member with a covering parent of its own
    preds[PX] = dict(q=1, variant="member_covered", cover=[0])
    parents(PX, 1, [0])
    d0 = 2 + n_spare
    for c, k in enumerate(d_lists):
        parents(PX + 1 + c, k, list(range(k)), pair=(d0 + 2 * c, d0 + 2 * c + 1))
    sh_extra = {}
    if full:
        P = PX + 1 + nd
        for q, v, cov in extra:
            preds[P] = dict(q=q, variant=v, cover=cov)
            fresh += [(0, P), (1, P)]
            parents(P, q, cov, lack=0 if v == "lackpiv" else None)
            P += 1
        e0, e1 = ns - 2, ns - 1
        for _ in range(N_TAIL_FILL):
            fresh += [(e0, P), (e1, P)]
            P += 1
        fresh += [(e0, P), (e1, P)]
        parents(P, 33, [32], pair=(e0, e1), lack=e0)
        sh_extra["tail"] = dict(pair=(e0, e1), P=P)
        P += 1
        tri.extend((x, P, obj) for x in (0, 2, 3))  # the binary with a mask of its own
        fresh += [(4, P)]
        tri.append((5, P + 1, obj))
        sh_extra["unique"] = dict(mask=(0, 2, 3), key=(P, obj))
        obj += 1
        assert P + 2 == P0 + n_pred
    for x, P in fresh:
        tri.append((x, P, obj))
        obj += 1
    arr = np.array(tri, np.uint32)
    arr = arr[np.random.default_rng(seed).permutation(arr.shape[0])]
    sh = SShape(name, ns, arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy(), int(obj), (0, 1), preds)
    sh.__dict__["d_pairs"] = [(d0 + 2 * c, d0 + 2 * c + 1) for c in range(nd)]
    sh.__dict__["d_lists"] = tuple(d_lists)
    sh.__dict__.update(sh_extra)
    return sh


# ---------------------------------------------------------------------------------------------------------------------
BUILDERS = {
    "cols6": lambda: cols("cols6", 6, 2),
    "cols64": lambda: cols("cols64", HMAX, 1),
    "cols64x9": lambda: cols("cols64x9", HMAX, 9),
    "emit300": lambda: emit("emit300", 301, (0, 1, 31, 32, 33, -2, -1), 9, algebra=False),
    "emit16k": lambda: emit("emit16k", 16401, EMIT16K_POS, 65),
    "emit32k": lambda: emit("emit32k", 32801, EMIT32K_POS, 9),
    "lists_small": lists_small,
}
SHARED = {"r3": r3_shape,
          "r3s": lambda: r3_shape("r3s", qs=(1, 32, 33), d_lists=(5,), n_spare=6, full=False)}
for _name, (_runs, _hm, _nh, _thr) in THRESHOLDS.items():
    BUILDERS[_name] = (lambda a=_name, b=_runs, c=_hm, d=_nh, e=_thr:
                       threshold(a, [sz for cnt, sz in b for _ in range(cnt)], c, d, e))
FAMILY_A = ("cols6", "cols64", "cols64x9") + tuple(THRESHOLDS)
FAMILY_B = ("emit300", "emit16k", "emit32k", "lists_small")
_CACHE: dict = {}


def shape(name: str):
    """The named shape, built once per process."""
    if name not in _CACHE:
        _CACHE[name] = (SHARED[name] if name in SHARED else BUILDERS[name])()
    return _CACHE[name]
