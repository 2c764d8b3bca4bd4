"""The key-value form of the one-pass group build (RDFIND_GROUP_KV, default on): the kept records as u32 joins and
captures, their stable pair sort (primitives.hip radix_sort_pairs_u32) and the group passes over the sorted joins,
row-exact against tests/group_kv_ref.py.  The pair sort runs on caller data through rdf_test_radix_pairs, the whole
chain (k_fresh_bounds, k_keep_scatter_kv, the pair sort, k_group_flags_kv, k_group_build_kv, k_dgrp_kv) through
rdf_test_group_kv; every device array lies between canaries and the inputs are compared with what was uploaded.  The
record tile is T = rdf_test_record_tile() records, the radix tile 4096 keys; the shapes put runs, group heads and
capture boundaries on and next to both.  The last tests run the whole pipeline under both values of the switch."""
import zlib

import numpy as np
import pytest

from rdfind_amd import _lib, synth
from tests import group_kv_ref as R
from tests import light_shapes

pytestmark = pytest.mark.gpu

RT = 4096  # primitives.hip RS_TILE
SIZES = (0, 1, 2, RT - 1, RT, RT + 1, 3 * RT + 5)
BITS = (1, 8, 9, 10, 18, 19, 23, 27, 28, 32)  # 1-4 passes, digits of <= 8 and of 9 bits
PASSES = {1: 1, 8: 1, 9: 1, 10: 2, 18: 2, 19: 3, 23: 3, 27: 3, 28: 4, 32: 4}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T(ctx):
    t = ctx.test_record_tile()
    assert t >= 256 and t % 256 == 0
    return t


def rng_for(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def check_pairs(ctx, keys, vals, lo, hi, what):
    keys = np.asarray(keys, np.uint32)
    vals = np.asarray(vals, np.uint32)
    sk, sv, ok = ctx.test_radix_pairs(keys, vals, lo, hi)
    assert ok, ("a canary was overwritten, the input changed or a single pass touched its scratch", what)
    rk, rv = R.pair_sort(keys, vals, lo, hi)
    assert np.array_equal(sk, rk), what
    assert np.array_equal(sv, rv), what


def test_pass_counts_cover_one_to_four(ctx):
    assert {b: ctx.lib.rdf_test_radix_passes(b) for b in BITS} == PASSES


@pytest.mark.parametrize("bits", BITS)
def test_pair_sort_sizes_and_bits(ctx, bits):
    top = (1 << bits) - 1
    for n in SIZES:
        rng = rng_for("pairs", bits, n)
        keys = rng.integers(0, top + 1, n, dtype=np.uint64).astype(np.uint32)
        if n > 1:
            keys[n // 2] = top  # the largest key of the range is there
            keys[: n // 3] = keys[n // 3: 2 * (n // 3)]  # equal keys far apart: the index values show the order kept
        check_pairs(ctx, keys, np.arange(n), 0, bits, (bits, n, "index values"))


@pytest.mark.parametrize("bits", (1, 9, 18, 23, 32))
def test_pair_sort_key_orders(ctx, bits):
    top = (1 << bits) - 1
    for n in (2, RT + 1, 3 * RT + 5):
        rng = rng_for("orders", bits, n)
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        asc = np.sort(rng.integers(0, top + 1, n, dtype=np.uint64)).astype(np.uint32)
        check_pairs(ctx, np.full(n, top, np.uint32), np.arange(n), 0, bits, (bits, n, "all keys equal"))
        check_pairs(ctx, asc, vals, 0, bits, (bits, n, "sorted"))
        check_pairs(ctx, asc[::-1].copy(), np.arange(n), 0, bits, (bits, n, "reversed"))


def test_pair_sort_bit_field_above_zero(ctx):
    # bits outside [lo, hi) are carried along and decide nothing
    n = 2 * RT + 7
    keys = rng_for("field").integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for lo, hi in ((5, 14), (12, 32), (3, 3)):
        check_pairs(ctx, keys, np.arange(n), lo, hi, (lo, hi))


# ---- the chain ---------------------------------------------------------------------------------------------------

JB = 12  # join bits of most chain shapes: V <= 4096, two passes of 6 bits


def recs(pairs, joinbits=JB):
    """Sorted records of (capture, join) pairs, as given (repeats stay)."""
    a = np.array([(c << joinbits) | j for c, j in pairs], np.uint64) if len(pairs) else np.zeros(0, np.uint64)
    return np.sort(a)


def check_chain(ctx, keys, joinbits, ncap, ms, V, what):
    assert (np.diff(keys.astype(np.int64)) >= 0).all()
    got = ctx.test_group_kv(keys, joinbits, ncap, ms, V)
    assert got["canaries_ok"], ("a canary around a device buffer was overwritten", what)
    ref = R.group_kv(keys, joinbits, ncap, ms, V)
    assert (got["Jf"], got["G"]) == (ref["Jf"], ref["G"]), what
    for name in ("support", "doff", "dgrp", "goff", "gcap", "gmap"):
        assert np.array_equal(got[name], ref[name]), (what, name)
    return ref


def grid_records(n_caps, joins, joinbits=JB):
    """Every capture 0 .. n_caps - 1 with every join of `joins`."""
    c = np.repeat(np.arange(n_caps, dtype=np.uint64), len(joins))
    j = np.tile(np.asarray(joins, np.uint64), n_caps)
    return (c << np.uint64(joinbits)) | j


@pytest.mark.parametrize("which", ["0", "1", "T-1", "T", "T+1", "4095", "4097"])
def test_chain_sizes(ctx, T, which):
    """Jf kept records exactly: frequent captures of 3-5 joins between infrequent ones of 1-2 (ms = 3), records repeated."""
    jf = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "4095": RT - 1, "4097": RT + 1}[which]
    rng = rng_for("chain_sizes", jf)
    ms = 3 if jf != 1 else 1  # (one kept record: a capture of one join, frequent at ms = 1, and nothing infrequent)
    sizes = [3] * (jf // 3 - 1) + [3 + jf % 3] if jf >= 3 else [1] * jf
    pairs, cap = [], 0
    for k in sizes or [0] * 40:
        if ms == 3 and (k == 0 or rng.integers(0, 2)):  # an infrequent capture first
            pairs += [(cap, int(j)) for j in rng.choice(1 << JB, int(rng.integers(1, 3)), replace=False)]
            cap += 1
        pairs += [(cap, int(j)) for j in rng.choice(1 << JB, k, replace=False)]
        cap += k > 0
    keys = recs(pairs)
    keys = np.sort(np.concatenate([keys, rng.choice(keys, keys.shape[0] // 3 + 2)]))
    ref = check_chain(ctx, keys, JB, cap + 1, ms, 1 << JB, which)
    assert ref["Jf"] == jf


def test_chain_one_group_holds_every_record(ctx, T):
    keys = grid_records(3 * T + 5, [77])
    ref = check_chain(ctx, keys, JB, 3 * T + 5, 1, 100, "one group")
    assert ref["G"] == 1 and ref["Jf"] == 3 * T + 5


def test_chain_every_record_its_own_group(ctx, T):
    n = T + 9
    keys = (np.arange(n, dtype=np.uint64) << np.uint64(JB)) | np.arange(n, dtype=np.uint64)[::-1]
    ref = check_chain(ctx, keys, JB, n, 1, 1 << JB, "own groups")
    assert ref["G"] == ref["Jf"] == n


def test_chain_group_and_capture_over_three_tiles(ctx, T):
    # capture 1 holds 3 T + 40 joins (its kept records span three whole record tiles); join 3 is in 3 T + 20 captures
    # (its group spans three tiles of the join-sorted records)
    joinbits = 14
    big_cap = (np.uint64(1) << np.uint64(joinbits)) | np.arange(4, 3 * T + 44, dtype=np.uint64)
    big_grp = (np.arange(2, 3 * T + 22, dtype=np.uint64) << np.uint64(joinbits)) | np.uint64(3)
    keys = np.sort(np.concatenate([big_cap, big_grp, big_grp[:50]]))
    ref = check_chain(ctx, keys, joinbits, 3 * T + 22, 1, 1 << joinbits, "three tiles")
    assert ref["goff"][1] - ref["goff"][0] == 3 * T + 20
    check_chain(ctx, keys, joinbits, 3 * T + 22, 2, 1 << joinbits, "three tiles, only the large capture frequent")


def test_chain_group_heads_on_tile_edges(ctx, T):
    # single-capture groups except join 0, whose group ends at record T - 2: heads at T - 1 (a tile's last record) and at
    # T (the next tile's first)
    first = grid_records(T - 1, [0])
    rest = (np.uint64(T) << np.uint64(JB)) | np.arange(1, T + 3, dtype=np.uint64)
    keys = np.sort(np.concatenate([first, rest]))
    ref = check_chain(ctx, keys, JB, T + 1, 1, 1 << JB, "heads on edges")
    assert list(ref["goff"][:4]) == [0, T - 1, T, T + 1]


def test_chain_joins_with_gaps_and_the_last_value(ctx, T):
    V = 3000  # 12 join bits, V not a power of two; join V - 1 occurs, most values do not
    joins = [0, 7, 8, 1023, 1024, 2047, V - 1]
    keys = grid_records(T // 4 + 3, joins)
    ref = check_chain(ctx, keys, JB, T // 4 + 3, 2, V, "gaps")
    assert ref["G"] == len(joins) and ref["gmap"][V - 1] == len(joins) - 1 and ref["gmap"][V - 2] == R.PATTERN
    # ... and V = 2^joinbits with its last value, 23 join bits (three passes, as the flagship workload)
    jb = 23
    keys = np.sort(np.concatenate([grid_records(50, [(1 << jb) - 1, 1 << 22, 9], jb), grid_records(3, [4, 5], jb)]))
    ref = check_chain(ctx, keys, jb, 50, 3, 1 << jb, "23 bits")
    assert ref["gmap"][(1 << jb) - 1] == 4 and ref["G"] == 5


def test_chain_alternating_frequent_and_infrequent_captures(ctx, T):
    rng = rng_for("alternate")
    pairs = []
    for c in range(T + 50):
        k = 4 if c % 2 == 0 else int(rng.integers(1, 3))  # even captures frequent (ms = 3)
        pairs += [(c, int(j)) for j in rng.choice(200, k, replace=False)]
    ref = check_chain(ctx, recs(pairs), JB, T + 50, 3, 200, "alternating")
    assert ref["Jf"] == 4 * ((T + 51) // 2)


def test_chain_duplicate_records_across_a_tile_edge(ctx, T):
    # records T - 3 .. T + 3 are one key, and a second run of one key covers a whole tile and both its edges
    head = grid_records(1, range(T - 3))
    run = np.full(7, (1 << JB) | 9, np.uint64)
    mid = (np.uint64(2) << np.uint64(JB)) | np.arange(0, T - 4 - 7 + T, dtype=np.uint64)[: T - 9]
    long_run = np.full(T + 5, (3 << JB) | 1, np.uint64)
    tail = grid_records(6, [9, 1, 11])[3:] + np.uint64(3 << JB)
    keys = np.concatenate([head, run, mid, long_run, tail])
    keys = np.sort(keys)
    assert keys[T - 1] == keys[T] == run[0] and keys[T - 4] != run[0]
    for ms in (1, 2):
        check_chain(ctx, keys, JB, 12, ms, 1 << JB, ("duplicates", ms))


# ---- the whole pipeline under both values of the switch -----------------------------------------------------------

STATS = ("n_records", "n_frequent_records", "n_groups", "n_captures", "n_unary_captures", "n_heavy_groups")


@pytest.fixture(scope="module")
def both():
    """RDFIND_GROUP_KV value -> context (the switch is read when a context is created)."""
    mp = pytest.MonkeyPatch()
    made = {}
    for v in ("1", "0"):
        mp.setenv("RDFIND_GROUP_KV", v)
        made[v] = _lib.Context(0)
        mp.undo()
    yield made
    for c in made.values():
        c.close()


def _inputs():
    d = synth.config("c1", 0.02)
    yield "c1", d.s, d.p, d.o, d.num_terms, d.min_support, "spo"
    sh = light_shapes.shape("seg2")
    yield "seg2", sh.s, sh.p, sh.o, sh.num_terms, sh.min_support, "s"


def test_pipeline_same_result_under_both_forms(both):
    for name, s, p, o, nv, ms, proj in _inputs():
        res = {}
        for v, g in both.items():
            g.set_triples(s, p, o, nv)
            g.run(ms, proj)
            res[v] = (tuple(g.groups[k] for k in STATS), g.cind_count(), g.checksum())
            assert g.test_paths()["group_form"] == {"1": "kv", "0": "u64"}[v], (name, v)
        assert res["1"] == res["0"], name
        assert res["1"][0][1] > 0 and res["1"][1] > 0, name  # kept records and CINDs: the comparison is not empty


def test_range_build_reports_no_form(monkeypatch):
    monkeypatch.setenv("RDFIND_GROUP_RANGE", "500")
    d = synth.config("c1", 0.02)
    with _lib.Context(0) as g:
        g.set_triples(d.s, d.p, d.o, d.num_terms)
        g.run(d.min_support)
        assert g.test_paths()["group_form"] is None and g.groups["n_join_ranges"] > 1
