"""Frequent-condition counting (K1 / K2, rdfind_amd/csrc/counts.inl) on its own, at the shapes where its branches change.

Every case runs rdf_frequent_conditions only and compares what the stage leaves on the device with the NumPy reference of
tests/fc_ref.py: U, the s / p / o split and fval element for element (rdf_test_copy_frequent_unary); the rank and the
frequency bit (rdf_test_unary_lookup) of every frequent key, its two neighbours, the keys around V and 2V, 0, 3V - 1 and
the first and last key of every K1 bucket the input touches; the sorted frequent binary keys element for element,
n_binary_keys and n_frequent_binary.  Where a case is after a branch, rdf_test_fc_report (the stage ran under
rdf_test_fc_trace) must say that the branch ran; the shapes are aimed in tests/fc_ref.py and checked on the CPU by
tests/test_fc_ref.py.  Contexts of forced forms are created under the form's switches.
"""
import functools
import time

import numpy as np
import pytest

from rdfind_amd import _lib
from tests import fc_ref as F

pytestmark = pytest.mark.gpu

SWITCHES = ("RDFIND_COUNT_PATHS", "RDFIND_U1_RADIX_MIN", "RDFIND_B2_SPLIT", "RDFIND_B2_RADIX_MIN")
# form -> (environment, K1 form, K2 form)
FORMS = {
    "default": ({}, "partitioned", "plain"),
    "u1radix": ({"RDFIND_U1_RADIX_MIN": "1"}, "radix", "plain"),
    "b2split": ({"RDFIND_B2_SPLIT": "2"}, "partitioned", "split"),
    "b2radix": ({"RDFIND_B2_RADIX_MIN": "1"}, "partitioned", "radix"),
    "b2nosplit": ({"RDFIND_B2_SPLIT": "0"}, "partitioned", "plain"),
    "atomic": ({"RDFIND_COUNT_PATHS": "atomic"}, "atomic", "atomic"),
}
K1_FORMS = ("default", "u1radix", "atomic")

_CTX = {}


def new_context(monkeypatch, form):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form][0].items():
        monkeypatch.setenv(k, v)
    c = _lib.Context(0)  # (the switches are read at creation and held by value)
    c.test_fc_trace(True)
    return c


def context(monkeypatch, form):
    if form not in _CTX:
        _CTX[form] = new_context(monkeypatch, form)
    return _CTX[form]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    while _CTX:
        _CTX.popitem()[1].close()


@functools.lru_cache(maxsize=None)
def shape(name, *args):
    return getattr(F, name)(*args)


@functools.lru_cache(maxsize=None)
def ref_of(ms, name, *args):
    s, p, o, V = shape(name, *args)
    return F.reference(s, p, o, V, ms)


def check(ctx, form, ms, name, *args):
    """One frequent-condition stage on shape(name, *args) against the reference; returns the stage's report."""
    s, p, o, V = shape(name, *args)
    ref = ref_of(ms, name, *args)
    what = (form, ms, name) + args
    ctx.set_triples(s, p, o, V)
    st = ctx.frequent_conditions(ms)
    rep = ctx.test_fc_report()
    assert rep["traced"] and (rep["k1_form"], rep["k2_form"]) == FORMS[form][1:], (what, rep)
    assert (rep["k2_sub"] >= 1) == (form == "b2split"), (what, rep)
    fval, n3 = ctx.test_copy_frequent_unary()
    assert n3 == ref.n3 == st["n_frequent_unary"], what
    assert fval.shape[0] == sum(ref.n3) and np.array_equal(fval, ref.fval), what
    k1_bits = rep["k1_bits"] or 14
    assert form == "atomic" or rep["k1_buckets"] == (3 * V + (1 << k1_bits) - 1) >> k1_bits, (what, rep)
    keys = F.probe_keys(ref, s, p, o, k1_bits)
    rank, bit, ok = ctx.test_unary_lookup(keys)
    want_rank, want_bit = ref.rank_bit(keys)
    assert ok, what
    bad = np.flatnonzero((rank != want_rank) | (bit != want_bit))
    assert bad.size == 0, (what, [(int(keys[i]), int(rank[i]), int(want_rank[i]), int(bit[i])) for i in bad[:8]])
    assert st["n_binary_keys"] == ref.n_binary_keys, what
    assert st["n_frequent_binary"] == ref.bkeys.shape[0], what
    got = ctx.binary_keys()
    assert got.shape == ref.bkeys.shape and np.array_equal(got, ref.bkeys), what
    return rep


# ---- K1 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 5461, 5462, 8192, 10923, 16384, 16385])
@pytest.mark.parametrize("form", K1_FORMS)
def test_k1_boundaries(monkeypatch, form, V):
    """Each side of V and of 2V frequent and not, in every arrangement |V| has room for; counts of exactly ms, ms - 1."""
    ctx = context(monkeypatch, form)
    arrangements = [(True, True), (False, False)] + ([(True, False), (False, True)] if V > 2 else [])
    for fa, fb in arrangements:
        rep = check(ctx, form, 3, "boundary", V, fa, fb)
        assert form == "atomic" or rep["k1_bits"] == 14


@pytest.mark.parametrize("V,pv,fa", [(6000, 0, True), (6000, 5999, False), (40000, 10000, True)])
@pytest.mark.parametrize("form", K1_FORMS)
def test_k1_multi_slice(monkeypatch, form, V, pv, fa):
    """A K1 bucket of several counting slices (summed in cntg, ranked by k_u2_finish), with both boundaries inside it
    (V = 6000) and outside (V = 40 000, where the bucket holds the hot predicate alone and its slices start at records
    that are no multiple of 8).  ms = n and n + 1 decide on the hot key's exact count."""
    ctx = context(monkeypatch, form)
    n = shape("multi_slice", V, pv, fa)[0].shape[0]
    for ms in (24, n, n + 1):
        rep = check(ctx, form, ms, "multi_slice", V, pv, fa)
        assert form == "atomic" or (rep["k1_multi"] >= 1 and rep["k1_slices"] >= rep["k1_buckets"] + 2), rep
        assert ref_of(ms, "multi_slice", V, pv, fa).n3[1] == (1 if ms <= n else 0)


@pytest.mark.parametrize("form", ["default", "u1radix"])
def test_k1_vector_edges(monkeypatch, form):
    """Buckets of 1, 7, 8, 9 and 19 records at different offsets: k_u2_count's short path, head, vector body, tail."""
    rep = check(context(monkeypatch, form), form, 2, "vector_edges")
    assert rep["k1_buckets"] == 15 and rep["k1_multi"] == 0


@pytest.mark.parametrize("form", K1_FORMS)
def test_support_edges(monkeypatch, form):
    """ms = 0 (read as 1), 1, n (the one predicate alone) and n + 1 (nothing: U = 0, B = 0)."""
    ctx = context(monkeypatch, form)
    n = shape("support_edges")[0].shape[0]
    for ms in (0, 1, n, n + 1):
        check(ctx, form, ms, "support_edges")
    assert ref_of(0, "support_edges").n3 == ref_of(1, "support_edges").n3
    assert ref_of(n, "support_edges").n3 == [0, 1, 0]
    assert ctx.test_copy_frequent_unary()[0].shape[0] == 0 and ctx.fc["n_frequent_binary"] == 0  # (ms = n + 1 ran last)


@pytest.mark.parametrize("form", ["default", "u1radix"])
def test_k1_15bit_buckets(monkeypatch, form):
    """|V| = 180 000 001: more than 2^15 buckets of 2^14 keys, so K1 takes 15 key bits per bucket (BITS = 15).  The
    stage alone; the context holds 6.1 GiB for the call and gives it back.
    Measured on one MI355X (the test prints the line; profiles/gpu_fc_tests.log): over the runs measured the whole test took at
    most 0.03 s in the partitioned form and at most 0.25 s in the radix form, so both forms stay cases of one test."""
    ctx = new_context(monkeypatch, form)
    try:
        t0 = time.perf_counter()
        rep = check(ctx, form, 3, "big_v")
        print(f"\nk1_15bit[{form}]: {time.perf_counter() - t0:.2f} s, {ctx.device_bytes() / 2**30:.1f} GiB held")
        assert rep["k1_bits"] == 15 and rep["k1_buckets"] > 1 << 14
        ctx.release_scratch()
    finally:
        ctx.close()


# ---- K2 ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", ["po", "so", "sp"])
@pytest.mark.parametrize("form", ["default", "b2split", "b2radix", "atomic"])
def test_k2_runs(monkeypatch, form, pair):
    """Runs of 1 to 130 equal pairs in adjacent rows, at and across multiples of 64 and 1024 rows, some broken by an
    inactive row; totals of exactly ms and ms - 1 (wave_runs4's pieces of 1 to 4, b2_pack's count bits 30 and 61)."""
    check(context(monkeypatch, form), form, F.RUNS_MS, "runs", pair)


@pytest.mark.parametrize("form", ["default", "b2split", "b2radix", "b2nosplit", "atomic"])
def test_k2_hot_key(monkeypatch, form):
    """15 000 records of one key in one bucket: several slices, every partial through the spill list and fc_sum_pairs,
    with bucket mates at totals ms and ms - 1."""
    rep = check(context(monkeypatch, form), form, 3, "hot_key")
    assert form == "atomic" or (rep["k2_multi"] >= 1 and rep["k2_spill"] > 0), rep


@pytest.mark.parametrize("form", ["default", "b2split", "b2radix"])
def test_k2_crowded_table(monkeypatch, form):
    """40 keys with one home slot in a table of 128: the 32-probe refusal in a bucket of one slice."""
    rep = check(context(monkeypatch, form), form, 2, "crowded")
    assert rep["k2_spill"] > 0 and rep["k2_multi"] == 0, rep
