"""The rule of K3's key items (RDFIND_EMIT_KEYS) on the CPU: the restatement of tests/emit_keys_ref.py keeps the distinct
record set and n_records, and the shapes of tests/test_gpu_emit_keys.py hold what they claim (both oracles)."""
import numpy as np
import pytest

from oracle import c_oracle as C, rdfind_oracle as R
from tests import emit_keys_ref as K

ATTR = {0: R.S, 1: R.P, 2: R.O}


def oracle_keys(arr, ms):
    tr = [tuple(x) for x in arr.tolist()]
    uf = R.frequent_unary_conditions(tr, ms)
    return uf, R.frequent_binary_conditions(tr, uf, ms)


@pytest.mark.parametrize("name", list(K.SHAPES) + ["exact"])
def test_shapes_hold_what_they_claim(name):
    arr, nv, ms = K.shape_exact() if name == "exact" else K.SHAPES[name]()
    on = K.model(arr, ms)
    off = K.model(arr, ms, keys_on=False)
    # the Python oracle's frequent conditions are the model's, kind by kind; the C oracle counts the same keys and the
    # same emitted records
    uf, bf = oracle_keys(arr, ms)
    fu, fb = K.frequent(arr, ms)
    assert {(a, v) for a in range(3) for v in uf[ATTR[a]]} == fu
    assert {(ATTR[a] | ATTR[b], va, vb) for a, b, va, vb in fb} == set(bf)
    _, st = C.run_set(arr[:, 0], arr[:, 1], arr[:, 2], nv, ms, 1, True)
    assert st["n_freq_binary"] == len(fb) == sum(on["keys_per_kind"].values())
    assert st["n_records"] == on["n_records"] == off["n_records"]
    assert st["n_unique"] == len(on["distinct"])
    # the rule keeps the record set and never adds to the sort
    assert on["distinct"] == off["distinct"]
    assert on["sorted"] <= off["sorted"] and off["suppressed"] == 0 and off["key_items"] == 0
    n = arr.shape[0]
    if name == "exact":
        assert on["keys_per_kind"] == {(0, 1): 0, (0, 2): 0, (1, 2): 1}
        assert (on["n_records"], on["sorted"], on["suppressed"], on["key_items"]) == (5 * n, 3 * n + 2, 2 * n, 1)
        assert off["sorted"] == 3 * n + 2 * len(K.windows(n))
        for grid in (1, 4):
            assert K.model(arr, ms, grid_cap=grid)["sorted"] == 3 * n + 2
            assert K.model(arr, ms, keys_on=False, grid_cap=grid)["sorted"] == 3 * n + 2 * len(K.windows(n, grid))
    elif name == "kinds":
        assert on["keys_per_kind"] == {(0, 1): 1, (0, 2): 1, (1, 2): 1}
        assert on["suppressed"] == 2 * 4 * 3 and on["key_items"] == 3
        for a, b, va, vb in fb:  # every value distinct: a key's two records fall into different join ranges
            assert va != vb
    elif name == "no_keys":
        assert len(fb) == 0 and on["n_records"] > 0 and on["sorted"] == off["sorted"]
    elif name == "empty":
        assert on["n_records"] == on["sorted"] == on["key_items"] == 0
    else:
        B = len(fb)
        assert B > n
        w = K.windows(n + B)
        assert sum(1 for lo, hi in w if lo >= n) >= 1  # iterations of key items only ...
        assert any(lo < n < hi for lo, hi in w)        # ... and one with the last triples and the first key items
        if n + B > 2 * K.BLOCK:  # one block (RDFIND_EMIT_GRID=1): the key items cross its iterations' boundaries
            assert any(lo > n and lo % K.BLOCK == 0 for lo, hi in K.windows(n + B, 1))


@pytest.mark.parametrize("name", ["kinds", "more_keys_200", "more_keys_300", "no_keys"])
def test_projection_subsets_keep_the_record_set(name):
    arr, nv, ms = K.SHAPES[name]()
    for proj in K.PROJECTIONS:
        on, off = K.model(arr, ms, proj), K.model(arr, ms, proj, keys_on=False)
        assert on["distinct"] == off["distinct"], proj
        assert on["n_records"] == off["n_records"] and on["sorted"] <= off["sorted"], proj
        # only records of the projected attributes exist, the key items' included
        assert {x for (x, _), _ in on["distinct"]} <= {"spo".index(ch) for ch in proj}, proj
        _, st = C.run_set(arr[:, 0], arr[:, 1], arr[:, 2], nv, ms, 1, True, proj)
        assert (st["n_records"], st["n_unique"]) == (on["n_records"], len(on["distinct"])), proj


def test_random_inputs_against_the_oracle_counts():
    rng = np.random.default_rng(77)
    for _ in range(40):
        n, nv, ms = int(rng.integers(1, 300)), int(rng.integers(2, 40)), int(rng.integers(1, 4))
        arr = np.stack([rng.integers(0, nv, n), rng.integers(0, nv // 3 + 1, n), rng.integers(0, nv, n)], 1).astype(np.uint32)
        on, off = K.model(arr, ms), K.model(arr, ms, keys_on=False)
        _, st = C.run_set(arr[:, 0], arr[:, 1], arr[:, 2], nv, ms, 1, True)
        assert on["distinct"] == off["distinct"]
        assert (st["n_records"], st["n_unique"], st["n_freq_binary"]) == (on["n_records"], len(on["distinct"]), on["key_items"])
