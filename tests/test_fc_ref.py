"""tests/fc_ref.py on the CPU: the NumPy reference of frequent-condition counting against the Python oracle and the C
oracle on small random inputs, and the aimed shapes against what their docstrings promise (run lengths and places, bucket
sizes, shared buckets and home slots).  The hash restatement is checked against tests/shard_sim.py's scalar one."""
import random

import numpy as np
import pytest

from oracle import c_oracle
from oracle import rdfind_oracle as orc
from tests import fc_ref as F
from tests import shard_sim

BT_OF_TYPE = {orc.S | orc.P: 2, orc.S | orc.O: 1, orc.P | orc.O: 0}


@pytest.mark.parametrize("seed", range(12))
def test_reference_vs_oracles(seed):
    rng = random.Random(seed)
    n, nv, ms = rng.randrange(1, 300), rng.randrange(1, 50), rng.choice([0, 1, 2, 3, 5])
    arr = np.array([(rng.randrange(nv), rng.randrange(nv // 3 + 1), rng.randrange(nv)) for _ in range(n)], np.uint32)
    s, p, o = arr[:, 0], arr[:, 1], arr[:, 2]
    ref = F.reference(s, p, o, nv, ms)
    triples = [tuple(int(x) for x in r) for r in arr]
    ufc = orc.frequent_unary_conditions(triples, max(ms, 1))
    for pos, t in enumerate((orc.S, orc.P, orc.O)):
        assert ref.freq[pos].tolist() == sorted(ufc[t])
    bfc = orc.frequent_binary_conditions(triples, ufc, max(ms, 1))
    want = sorted((BT_OF_TYPE[t] << 62) | (v1 << 31) | v2 for t, v1, v2 in bfc)
    assert ref.bkeys.tolist() == want
    _, keys, st = c_oracle.run(s, p, o, nv, max(ms, 1))  # (the library reads a support of 0 as 1; the oracles take it as given)
    assert st["n_freq_unary"] == ref.n3
    assert st["n_binary_keys"] == ref.n_binary_keys
    assert st["n_freq_binary"] == len(want) and np.array_equal(np.sort(keys), ref.bkeys)
    rank, bit = ref.rank_bit(np.arange(3 * nv))
    assert rank[bit == 1].tolist() == list(range(sum(ref.n3))) and (rank[bit == 0] == F.NONE32).all()
    assert np.array_equal(np.flatnonzero(bit), ref.ukeys.astype(np.int64))
    assert np.array_equal(ref.fval, (ref.ukeys % np.uint64(nv)).astype(np.uint32))


def test_hash_restatement():
    keys = F.bin_keys(0, np.arange(50), np.arange(100, 150))
    assert F.mix64(keys).tolist() == [shard_sim.mix64(int(k)) for k in keys]
    assert F.b2_bucket(keys, 5).tolist() == [shard_sim.mix64(int(k)) >> 59 for k in keys]


def exact_counts(cols, ms):
    for c in cols:
        assert set(np.unique(c, return_counts=True)[1].tolist()) <= {ms, ms - 1}


@pytest.mark.parametrize("V", [2, 63, 16385])
def test_boundary_shape(V):
    for fa, fb in ((True, True), (False, False)) + (((True, False), (False, True)) if V > 2 else ()):
        s, p, o, _ = F.boundary(V, fa, fb)
        exact_counts((s, p, o), 3)
        for c in (s, p, o):
            assert {0, V - 1} <= set(c.tolist())
        _, bit = F.reference(s, p, o, V, 3).rank_bit([V - 1, V, 2 * V - 1, 2 * V])
        assert bit.tolist() == [fa, not fa, fb, not fb]


def test_multi_slice_and_vector_shapes():
    for V, pv, inside in ((6000, 0, True), (40000, 10000, False)):
        s, p, o, _ = F.multi_slice(V, pv, True)
        exact_counts((s, o), 24)
        lens = F.k1_bucket_lens(s, p, o, V, 14)
        hot = (V + pv) >> 14
        assert lens[hot] > 2 << 15
        assert ((V >> 14) == hot and (2 * V >> 14) == hot) == inside
        assert any(x % 8 for x in F.k1_slice_starts(lens))
    s, p, o, V = F.vector_edges()
    exact_counts((s, p, o), 2)
    lens = F.k1_bucket_lens(s, p, o, V, 14).tolist()
    assert sorted(lens) == sorted(F.VECTOR_LENS * 3) and any(x % 8 for x in np.cumsum(lens))
    s, p, o, V = F.big_v()
    exact_counts((s, p, o), 3)
    assert (3 * V + (1 << 14) - 1) >> 14 > 1 << 15
    for c in (s, p, o):
        assert {0, (1 << 15) - 1, 1 << 15, V - 1} <= set(c.tolist())


@pytest.mark.parametrize("pair", ["po", "so", "sp"])
def test_runs_shape(pair):
    s, p, o, V = F.runs(pair)
    n = s.shape[0]
    assert n % 64 and n <= 4096  # one partition block: lanes are rows modulo 64
    a, b = {"po": (p, o), "so": (s, o), "sp": (s, p)}[pair]
    ref = F.reference(s, p, o, V, F.RUNS_MS)
    assert ref.n_binary_keys == 24 and np.sort(ref.cand_cnt).tolist() == [F.RUNS_MS - 1] * 12 + [F.RUNS_MS] * 12
    key = a.astype(np.int64) * 1000 + b
    heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    ends = np.r_[heads[1:], n]
    lens = ends - heads
    active = b[heads] < len(F.RUN_LENS)
    assert set(F.RUN_LENS) <= set(lens[active].tolist())
    long = active & (lens >= 2)
    assert (heads[long] % 64 == 0).any()
    assert (heads[long] // 64 != (ends[long] - 1) // 64).any()
    assert sum(heads[long] // 1024 != (ends[long] - 1) // 1024) >= 3
    # a breaking row sits between two pieces of one key
    brk = np.flatnonzero(~active)
    brk = brk[(brk > 0) & (brk < len(heads) - 1)]
    assert (key[heads[brk - 1]] == key[heads[brk + 1]]).sum() >= 5
    assert a[-1] == 0 and b[-1] == 0  # the rows past the end read as pair (0, 0) too


def test_hot_and_crowded_shapes():
    s, p, o, V = F.hot_key()
    keys = F.bin_keys(0, p, o)
    run = np.flatnonzero(keys == F.bin_keys(0, [5], [7])[0])
    assert run.shape[0] == F.HOT_ROWS and run[-1] - run[0] == F.HOT_ROWS - 1
    ref = F.reference(s, p, o, V, 3)
    mates = ref.cand[F.b2_bucket(ref.cand, 12) == F.b2_bucket(keys[run[:1]], 12)[0]]
    tot = ref.cand_cnt[np.isin(ref.cand, mates)]
    assert (tot == 3).sum() >= 4 and (tot == 2).sum() >= 4
    s, p, o, V = F.crowded()
    ref = F.reference(s, p, o, V, 2)
    assert ref.n3[0] == 0 and 3 * s.shape[0] <= 2048  # only po keys; two first-level buckets
    grp = F.b2_bucket(ref.cand, F.CROWD_BITS) * F.CROWD_T + F.b2_home(ref.cand, F.CROWD_T)
    best = np.bincount(grp).argmax()
    crowd = ref.cand[grp == best]
    assert crowd.shape[0] >= 34
    same1 = ref.cand[F.b2_bucket(ref.cand, 1) == F.b2_bucket(crowd[:1], 1)[0]]
    assert np.array_equal(same1, crowd)  # nothing else in the 1-bit bucket: the table has 128 slots
    tot = ref.cand_cnt[np.isin(ref.cand, crowd)]
    assert set(tot.tolist()) == {1, 2}
