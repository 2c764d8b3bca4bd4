"""A rank model for the near-miss, heavy and class shapes in sharded mode (test infrastructure; plain numpy, no GPU).

The sharded protocol (rdfind_amd/distributed.py) gives every join value an owner rank: the balanced table of the hot
values (rdfind_hip.hip sh_phase16 / sh_phase18), else a hash.  Under projection ``s`` the join values of the shapes of
tests/light_shapes.py and tests/heavy_shapes.py are their subjects, so the owner of a subject decides on which rank its
capture group lives, and with it what the exchange has to do for a dependent: how many ranks hold a light group of it
(``nrl``), and whether the one subject a near-miss lacks sits on the rank that draws the candidates (the holder) or on
another, where only the verify pass of that rank can reject the pair.

The owner functions are imported from tests/shard_sim.py (``hot_owner_table``, ``shard_of``, ``key_owner``,
``dep_owner``), not restated.  They aim and audit the inputs: tests/test_shard_shapes_cpu.py asserts from this model
that the inputs contain what the protocol must reject, and tests/test_gpu_sharded_shapes.py asserts the heavy columns per
rank and the class counts from it.  No expected row comes from here: the rows are the oracle's.

The holder of a dependent is elected on quarter-octave size buckets with a hashed tie-break (kernels.inl holder_key),
which this model does not restate: it names the rank of the globally smallest group by (size, subject) only as a
description, and everything asserted on the device that depends on the holder is either an inequality or holds
whichever rank is elected (the ``vedge`` shapes below).

``vedge63`` / ``vedge64`` / ``vedge65`` / ``vedge129``: a dependent ``D`` of 40 subjects whose verify pairs at world 2
under the default owners number exactly 63, 64, 65 and 129 whichever rank holds ``D``: ``n_true`` true supersets (no
one includes another: each adds its own pair of extra subjects), and two pairs of near-misses, each pair missing one
subject owned by rank 0 and one owned by rank 1.  The holder rejects the near-miss of each pair whose missed subject it
owns and sends the other with the trues to the other rank, which must reject it: n_true + 2 verify pairs.  One pair has
the smallest and one the largest capture ids of D's refs, so a rejected pair is the first and the last candidate of the
verify pass.  The missed positions are chosen by this model (a seeded search) and asserted by the CPU test.  The shapes
also hold every two-subject set over six further subjects: of six subjects two share an owner at world 2 and at world 3
under any owner function, so under every setting some dependent has a light group on one rank only (nrl = 1), which the
other light shapes, whose sets spread over all ranks, do not offer.
"""
from __future__ import annotations

import numpy as np

from tests import heavy_shapes as H
from tests import light_shapes as L
from tests.shard_sim import HOT_CAP, HOT_DIV, dep_owner, hot_owner_table, key_owner, shard_of

_OWN: dict = {}


def slice_sizes(n: int, world: int, slices: bool = True) -> list:
    """Triples per rank: ``rank::world`` slices of the rows, or the row ranges the library cuts from a replicated input
    (rdfind_hip.hip sh_slice)."""
    if slices:
        return [len(range(r, n, world)) for r in range(world)]
    return [n * (r + 1) // world - n * r // world for r in range(world)]


def subject_owners(sh, world: int, hot_balance: bool = True, slices: bool = True) -> np.ndarray:
    """Owner rank of every subject 0 .. n_subjects - 1 under projection s.  hot_balance: the default (the hot table
    first); without: RDFIND_HOT_BALANCE=0, the hash alone.  The table is fed what sh_phase16 submits: every rank's
    slice size, and from each key owner (key_owner of key = position * V + value, position 0 for subjects) the summed
    occurrence counts of its keys that reach its own threshold, the HOT_CAP largest."""
    key = (sh.name, bool(getattr(sh, "shared_objects", False)), world, hot_balance, slices)
    if key in _OWN:
        return _OWN[key]
    ns = sh.n_subjects
    table = {}
    if hot_balance and world > 1:
        V = sh.num_terms
        occ = np.bincount(sh.s.astype(np.int64), minlength=V)  # occurrences at the projected position
        sizes = slice_sizes(sh.n, world, slices)
        words = []
        subj = np.nonzero(occ)[0].tolist()
        kown = [key_owner(k, world) for k in subj]
        for r in range(world):
            thr = max(1, 1 * sizes[r] // (3 * HOT_DIV))
            cand = sorted(((int(occ[k]), k) for k, q in zip(subj, kown) if q == r and occ[k] >= thr),
                          key=lambda x: (-x[0], x[1]))[:HOT_CAP]
            words.append((0xFFFFFFFF << 32) | sizes[r])
            words += [(k << 32) | c for c, k in cand]
        table = hot_owner_table(words, V, world, 1)
    own = np.array([table[x] if x in table else shard_of(x, world) for x in range(ns)], np.int64)
    _OWN[key] = own
    return own


def heavy_set(sh, heavy_min) -> np.ndarray:
    """The heavy subjects under the RDFIND_HEAVY_MIN the cell runs with (None: the default; decided on the whole input,
    which is what the gathered histogram must reproduce)."""
    if isinstance(sh, H.SShape) or hasattr(sh, "heavy_min"):
        return np.asarray(sh.heavy(), np.int64)
    hm = H.DEFAULT_HEAVY_MIN if heavy_min is None else int(heavy_min)
    return sh.heavy_subjects(hm)


def heavy_per_rank(sh, world: int, heavy_min=None, **kw) -> list:
    """Heavy columns per rank: the heavy subjects each rank owns."""
    own = subject_owners(sh, world, **kw)
    return np.bincount(own[heavy_set(sh, heavy_min)], minlength=world).tolist()


def bucket_groups_per_rank(sh, world: int, size_lo: int, size_hi: int, **kw) -> list:
    """Groups with size_lo <= members <= size_hi per rank (one quarter-octave bucket of the local histograms)."""
    own = subject_owners(sh, world, **kw)
    gs = sh.group_sizes()
    return np.bincount(own[(gs >= size_lo) & (gs <= size_hi)], minlength=world).tolist()


def facts(sh, world: int, heavy_min=L.NO_HEAVY, **kw) -> list:
    """Per set k of a light shape: dict(groups = groups per rank, nrl = ranks with a light group, light = light groups
    per rank, smallest = rank of the globally smallest group by (size, subject), miss_rank = owner of the subject a
    near-miss lacks, else -1)."""
    own = subject_owners(sh, world, **kw)
    hv = np.zeros(sh.n_subjects, bool)
    hv[heavy_set(sh, heavy_min)] = True
    gs = sh.group_sizes()
    out = []
    for k, sk in enumerate(sh.sets):
        light = np.bincount(own[sk[~hv[sk]]], minlength=world)
        piv = int(sk[np.lexsort((sk, gs[sk]))][0])
        out.append(dict(groups=np.bincount(own[sk], minlength=world).tolist(), light=light.tolist(),
                        nrl=int((light > 0).sum()), smallest=int(own[piv]),
                        miss_rank=int(own[sh.miss[k]]) if sh.miss[k] >= 0 else -1))
    return out


def miss_ranks(sh, world: int, **kw) -> list:
    """Near-misses of D per rank that owns the missed subject."""
    f = facts(sh, world, **kw)
    return np.bincount([f[k]["miss_rank"] for k in sh.idx("near")], minlength=world).tolist()


def misses_off_every_holder(sh, world: int, **kw) -> bool:
    """Misses of D on at least two ranks: whichever rank holds D, some near-miss lacks a subject of another rank, so the
    holder keeps the pair and a verify pass must reject it."""
    return sum(1 for x in miss_ranks(sh, world, **kw) if x) >= 2


def class_model(sh, clean: bool = True) -> dict:
    """n_classes and n_class_members of a heavy / class shape as a sharded run reports them (the binary dependents are
    not classed in sharded mode)."""
    st = sh.class_stats(clean, False) if isinstance(sh, H.SShape) else sh.class_stats()
    return dict(n_classes=st["n_classes"], n_class_members=st["n_class_members"])


def member_owners(sh, world: int) -> list:
    """Class members (heavy-only unary dependents) per owner rank; dep_owner takes the compact capture id, which under
    projection s with unary captures alone is the set's index (captures ascend with the predicate's term id)."""
    assert not isinstance(sh, H.SShape)
    ks = [k for c in sh.classes() for k in c["members"]]
    return np.bincount([dep_owner(int(k), world) for k in ks], minlength=world).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# verify-count edges

VEDGE = {"vedge63": 63, "vedge64": 64, "vedge65": 65, "vedge129": 129}
VEDGE_M, VEDGE_EXTRAS, VEDGE_PAIRS, VEDGE_OTHERS = 40, 17, 2, 6
_CACHE: dict = {}


def _vedge_build(name: str, n_true: int, pos, seed: int) -> L.Shape:
    """pos = ((a0, b0), (a1, b1)): the missed positions of the two near-miss pairs."""
    m, D = VEDGE_M, np.arange(VEDGE_M, dtype=np.int64)
    x0 = m  # extras of the trues: every true its own pair of them, so no true includes another
    z = x0 + VEDGE_EXTRAS  # the one extra subject of every near-miss: their smallest group, hence their pivot
    o0 = z + 1  # subjects of the unrelated sets
    pairs = [(a, b) for a in range(VEDGE_EXTRAS) for b in range(a + 1, VEDGE_EXTRAS)]
    assert n_true <= len(pairs)
    near = lambda q: np.concatenate([np.delete(D, q), [z]])
    sets, kind, miss = [D], ["D"], [-1]
    for q in pos[0]:  # the smallest capture ids among D's refs
        sets.append(near(q)), kind.append("near"), miss.append(int(q))
    for j in range(n_true):
        a, b = pairs[(j * 7) % len(pairs)]  # (7 and 136 are coprime: distinct pairs, every extra in several sets)
        sets.append(np.concatenate([D, [x0 + a, x0 + b]])), kind.append("true"), miss.append(-1)
    for a in range(VEDGE_OTHERS):  # every two-subject set over the other subjects: see the docstring
        for b in range(a + 1, VEDGE_OTHERS):
            sets.append(o0 + np.array([a, b], np.int64)), kind.append("other"), miss.append(-1)
    for q in pos[1]:  # ... and the largest
        sets.append(near(q)), kind.append("near"), miss.append(int(q))
    n_subjects = o0 + VEDGE_OTHERS
    sets = [np.sort(x) for x in sets]
    sh = L.Shape(name, m, sets, kind, miss, np.zeros(0, np.int64), n_subjects)
    sizes = np.array([len(x) for x in sets])
    rng = np.random.default_rng(seed)
    s = np.concatenate(sets)
    p = np.repeat(n_subjects + np.arange(len(sets)), sizes)
    perm = rng.permutation(s.shape[0])
    sh.s, sh.p = s[perm].astype(np.uint32), p[perm].astype(np.uint32)
    sh.o = (n_subjects + len(sets) + np.arange(s.shape[0])).astype(np.uint32)
    sh.n_pred = len(sets)
    sh.num_terms = int(n_subjects + len(sets) + s.shape[0])
    assert sh.group_sizes().min() >= 2
    return sh


def vedge(name: str) -> L.Shape:
    """The named verify-edge shape: the smallest seeded choice of missed positions for which this model says that each
    near-miss pair misses one subject of rank 0 and one of rank 1 (world 2, default owners, rank::world slices)."""
    if name in _CACHE:
        return _CACHE[name]
    n_true = VEDGE[name] - VEDGE_PAIRS
    rng = np.random.default_rng(VEDGE[name])
    for trial in range(200):
        q = rng.choice(VEDGE_M, size=4, replace=False)
        sh = _vedge_build(name, n_true, ((int(q[0]), int(q[1])), (int(q[2]), int(q[3]))), seed=VEDGE[name])
        _OWN.pop((sh.name, False, 2, True, True), None)
        own = subject_owners(sh, 2)
        if sorted(own[q[:2]].tolist()) == [0, 1] and sorted(own[q[2:]].tolist()) == [0, 1]:
            _CACHE[name] = sh
            return sh
    raise AssertionError(f"{name}: no choice of missed positions splits over the two ranks")


def vedge_verify_pairs(sh) -> int:
    """Verify pairs of D at world 2 under the default owners, whichever rank holds D: its true supersets plus, of each
    near-miss pair, the one whose missed subject the holder does not own."""
    own = subject_owners(sh, 2)
    f = facts(sh, 2)
    d = sh.idx("D")[0]
    assert f[d]["nrl"] == 2
    counts = set()
    for holder in (0, 1):
        counts.add(len(sh.idx("true")) + sum(1 for k in sh.idx("near") if own[sh.miss[k]] != holder))
    assert len(counts) == 1
    return counts.pop()


def light_shape(name: str, ballast: bool = False, shared_objects: bool = False):
    """A light shape by name: tests/light_shapes.py's or a verify-edge shape."""
    if name in VEDGE:
        assert not ballast and not shared_objects
        return vedge(name)
    return L.shape(name, ballast, shared_objects)
