"""tests/group_kv_ref.py pinned: its pair sort against tests/prim_ref.py's stable bit-field sort, and its group build
against the oracle's join lines (oracle/rdfind_oracle.py join_lines / line_captures) on small random triples."""
import random

import numpy as np

import group_kv_ref
import prim_ref
from oracle import rdfind_oracle as ro


def test_pair_sort_is_prim_refs_stable_sort_of_the_packed_pairs():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 17, 500):
        for lo, hi in ((0, 1), (0, 9), (3, 12), (0, 23), (0, 32), (7, 7)):
            keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            if n > 4:
                keys[: n // 2] = keys[n // 2: 2 * (n // 2)]  # equal keys: stability shows
            vals = np.arange(n, dtype=np.uint32)
            sk, sv = group_kv_ref.pair_sort(keys, vals, lo, hi)
            packed = keys.astype(np.uint64) | (vals.astype(np.uint64) << np.uint64(32))
            want = prim_ref.sort_bits(packed, lo, hi) if hi > lo else packed
            assert np.array_equal(sk, (want & np.uint64(0xFFFFFFFF)).astype(np.uint32)), (n, lo, hi)
            assert np.array_equal(sv, (want >> np.uint64(32)).astype(np.uint32)), (n, lo, hi)


def test_pair_sort_is_stable():
    keys = np.array([5, 1, 5, 1, 5, 0], np.uint32)
    sk, sv = group_kv_ref.pair_sort(keys, np.arange(6), 0, 3)
    assert sk.tolist() == [0, 1, 1, 5, 5, 5] and sv.tolist() == [5, 1, 3, 0, 2, 4]


def _oracle_case(seed, n, nv, ms):
    rnd = random.Random(seed)
    triples = [(rnd.randrange(nv), rnd.randrange(3), rnd.randrange(nv)) for _ in range(n)]
    ufc = ro.frequent_unary_conditions(triples, ms)
    bfc = ro.frequent_binary_conditions(triples, ufc, ms)
    lines = ro.join_lines(triples, ufc, bfc)
    caps_of = {}
    for jv, line in lines.items():
        unary, binary = ro.line_captures(line)
        caps_of[jv] = {c.key() for c in unary | binary}
    return caps_of


def test_group_build_is_the_oracles_join_lines_restricted_to_frequent_captures():
    for seed, n, nv, ms in ((1, 60, 6, 2), (2, 200, 9, 3), (3, 400, 12, 5), (4, 30, 4, 1)):
        caps_of = _oracle_case(seed, n, nv, ms)
        ids = {c: i for i, c in enumerate(sorted({c for s in caps_of.values() for c in s}))}
        ncap, joinbits = max(len(ids), 1), 5
        assert nv <= 1 << joinbits
        recs = [(ids[c] << joinbits) | jv for jv, s in caps_of.items() for c in s]
        rnd = random.Random(seed)
        recs = sorted(recs + [rnd.choice(recs) for _ in range(len(recs) // 2)])  # K3 emits a record more than once
        r = group_kv_ref.group_kv(np.array(recs, np.uint64), joinbits, ncap, ms, nv)
        # supports: the join lines a capture occurs in
        want_sup = np.zeros(ncap, np.uint32)
        for s in caps_of.values():
            for c in s:
                want_sup[ids[c]] += 1
        assert np.array_equal(r["support"], want_sup)
        freq = [i for i in range(ncap) if want_sup[i] >= ms]
        comp = {i: k for k, i in enumerate(freq)}
        # groups: one per join value with a frequent capture, ascending; members = its frequent captures, ascending
        want_groups = [(jv, sorted(comp[ids[c]] for c in caps_of[jv] if ids[c] in comp)) for jv in sorted(caps_of)]
        want_groups = [(jv, m) for jv, m in want_groups if m]
        assert r["G"] == len(want_groups) and r["Jf"] == sum(len(m) for _, m in want_groups)
        for g, (jv, members) in enumerate(want_groups):
            assert r["gmap"][jv] == g
            assert r["gcap"][int(r["goff"][g]): int(r["goff"][g + 1])].tolist() == members
        assert {jv for jv in range(nv) if r["gmap"][jv] != group_kv_ref.PATTERN} == {jv for jv, _ in want_groups}
        # dependent -> groups: compact capture d's groups are those of its join values, ascending
        assert r["doff"].shape[0] == len(freq) + 1 and r["doff"][-1] == r["Jf"]
        for d, i in enumerate(freq):
            mine = [g for g, (jv, m) in enumerate(want_groups) if d in m]
            assert r["dgrp"][int(r["doff"][d]): int(r["doff"][d + 1])].tolist() == mine
