"""The near-miss shapes (tests/light_shapes.py) and the C oracle pinned against plain set inclusion, on the CPU.

This is the independent reference of tests/test_gpu_light_shapes.py: under projection ``s`` the 1/1 CINDs of a shape
are the inclusions among its sets ``S_k``, computed here with numpy alone, so a device bug cannot hide behind an oracle
quirk.  The structural facts each shape promises (which light path its dependents take, where the misses sit) are
asserted from the sets too."""
import numpy as np
import pytest

from tests import light_shapes as L
from tests.parity import shape_rows

FORMS = [(name, b) for name in L.SPECS for b in ((False, True) if name in L.BALLAST_FORMS else (False,))]
IDS = [n + ("+b" if b else "") for n, b in FORMS]


def heavy_of(sh):
    """The bit-column subjects of the setting the form runs under: RDFIND_HEAVY_MIN=2 for the pack80h / pack81h
    shapes, the default (64) for a ballast form, none for the others (RDFIND_HEAVY_MIN=NO_HEAVY)."""
    if not len(sh.ballast):
        return np.zeros(0, np.int64)
    return sh.heavy_subjects(2 if sh.name.startswith("pack8") else 64)


@pytest.mark.parametrize("name,ballast", FORMS, ids=IDS)
def test_oracle_is_set_inclusion(name, ballast):
    sh = L.shape(name, ballast)
    inc = sh.inclusions()
    sizes = {sh.pred(k): len(x) for k, x in enumerate(sh.sets)}
    raw, raw_sup = shape_rows(sh, 0, False, "s")
    np.testing.assert_array_equal(raw, inc)  # strategy 0 raw: exactly {(a, b): a != b, S_a subset of S_b}
    assert [sizes[int(k) >> 32] for k in raw] == raw_sup.tolist()  # support = |S_a|
    d = sh.idx("D")[0]
    near = [sh.pair_key(d, k) for k in sh.idx("near")]
    true = [sh.pair_key(d, k) for k in sh.idx("true")] + [sh.pair_key(k, d) for k in sh.idx("sub")]
    assert near and true
    assert np.isin(true, raw).all()
    for strategy, clean in ((1, True), (0, True), (0, False)):
        keys, _ = shape_rows(sh, strategy, clean, "s")
        assert np.isin(keys, inc).all(), (strategy, clean)  # the clean modes: a subset
        assert not np.isin(near, keys).any(), (strategy, clean)  # no (D, near-miss) anywhere
    # every near-miss lacks exactly one subject of D, at the position it names
    for k in sh.idx("near"):
        lack = np.setdiff1d(sh.sets[d], sh.sets[k])
        assert lack.tolist() == [sh.miss[k]]


@pytest.mark.parametrize("name,ballast", FORMS, ids=IDS)
def test_shape_structure(name, ballast):
    sh = L.shape(name, ballast)
    cls = L.shape_class(name)
    m, d = sh.m, sh.idx("D")[0]
    assert sh.sets[d].tolist() == list(range(m))  # position i of D's group list is subject i
    assert min(len(x) for x in sh.sets) >= 2 and sh.group_sizes().min() >= 2  # everything is frequent at support 2
    assert np.unique(sh.o).size == sh.n  # fresh objects
    heavy = heavy_of(sh)
    if len(sh.ballast):  # exactly the ballast takes the HMAX columns: the miss positions stay light
        assert sorted(heavy.tolist()) == sh.ballast.tolist() and len(heavy) == L.HMAX
    else:
        assert sh.heavy_subjects(1 << 30).size == 0
    missed = sorted({q for q in sh.miss if q >= 0})
    assert not set(missed) & set(sh.ballast.tolist())
    light_d = [q for q in range(m) if q not in set(heavy.tolist())]
    want = [q for q in L.WINDOW_EDGES + L.SEGMENT_EDGES + (m - 1,) if q < m and q in light_d]
    if cls in ("one_seg", "multi_seg"):
        assert set(want) <= set(missed), (want, missed)
        assert m - 1 in missed and {0, 63, 64, 127, 128, 191, 192, 255, 256} <= set(missed)
    if cls == "multi_seg":
        assert {2047, 2048} <= set(missed) and (m <= 4096 or {4095, 4096} <= set(missed))
    assert len(missed) > len(want) or cls.startswith("packed")  # ... and a random remainder
    twins = [q for q in missed if sh.miss.count(q) > 1]
    assert len(twins) == 1  # two identical near-misses: a dedup class of two
    a, b = [k for k in sh.idx("near") if sh.miss[k] == twins[0]]
    assert sh.sets[a].tolist() == sh.sets[b].tolist()
    # D's pivot and second pivot are miss positions
    piv, p2 = sh.pivots(d, heavy)
    assert piv in missed and p2 in missed, (piv, p2)
    # the light path of every dependent, as light_plan decides from (groups, light groups, pivot size)
    plan = sh.plan(heavy)
    ng, nl, sz, packed = plan[d]
    assert ng == m
    k_light = [k for k, (g, l, z, pk) in enumerate(plan) if l and not pk]
    if cls == "packed":  # no dependent takes k_light: n_light_items == 0 < n_packed_octets
        assert packed and not k_light
        assert (m == L.LIGHT_PACK_MAXG and nl == m) or (nl == L.LIGHT_PACK_NL and ng == L.HMAX + nl)
    elif cls == "packed_over":  # one group more: D itself is a k_light dependent
        assert not packed and d in k_light
        assert (m == L.LIGHT_PACK_MAXG + 1 and nl == m) or (nl == L.LIGHT_PACK_NL + 1 and ng == L.HMAX + nl)
    else:
        assert not packed and d in k_light and m > 80
        nseg = [-(-plan[k][0] // L.LIGHT_SEG) for k in k_light]
        assert (max(nseg) == 1) if cls == "one_seg" else (max(nseg) == -(-m // L.LIGHT_SEG) > 1)
    if name == "small300":  # every light group has at most LIGHT_SMALL members: the staged rows can run
        gs = sh.group_sizes()
        lightg = np.setdiff1d(np.arange(sh.n_subjects), heavy)
        assert gs[lightg].max() <= L.LIGHT_SMALL
        assert sz >= 16  # ... with a sweep's worth of candidates alive (LIGHT_SWEEP_MIN)
    want_piv = {"cand63": 63, "cand64": 64, "cand65": 65, "cand129": 129}
    if name in want_piv:  # D's pivot group around one chunk of 64, and a last chunk of one octet
        assert sz == want_piv[name]
    if cls == "multi_seg":
        assert sz > 64  # multi-chunk and multi-segment at once
        assert 150_000 <= sh.n <= 600_000


def test_miss_positions_cover_the_edges():
    rng = np.random.default_rng(0)
    pos = L.miss_positions(4100, 40, rng)
    assert pos[:14] == [0, 63, 64, 127, 128, 191, 192, 255, 256, 2047, 2048, 4095, 4096, 4099]
    assert len(set(pos)) == 40 and max(pos) < 4100
    few = L.miss_positions(33, 10, rng, avoid=(0,))
    assert few[0] == 32 and 0 not in few and len(set(few)) == 10


# ---------------------------------------------------------------------------------------------------------------------
# the shared-object form: one object O_k per set, so s[p=P_k], s[o=O_k] and s[p=P_k,o=O_k] share the join set S_k

SHARED = ("pack32", "pack33", "small300", "cand64", "cand65")


def _ids(cinds, sh, bkeys):
    """Sorted packed (dep << 32 | ref) capture-id keys of oracle Cind tuples (the id layout of rdfind_amd/codes.py)."""
    from rdfind_amd import codes
    V = sh.num_terms

    def cap(code, v1, v2):
        if v2 is None:
            return codes.UNARY_TYPE_INDEX[code] * V + v1
        k = (codes.BINARY_TYPE_INDEX[code] << 62) | (v1 << 31) | v2
        j = int(np.searchsorted(bkeys, np.uint64(k)))
        assert j < len(bkeys) and int(bkeys[j]) == k
        return 6 * V + j

    return np.sort(np.array([(cap(dt, d1, d2) << 32) | cap(rt, r1, r2) for dt, d1, d2, rt, r1, r2, _ in cinds], np.uint64))


@pytest.mark.parametrize("name", SHARED)
def test_shared_objects_oracles_agree_and_rules_act(name):
    """The C oracle equals the Python restatement in all four modes under projection s (the restatement's join lines
    are built once and shared by its modes), the rules remove rows, no (D, near-miss) pair exists in any of the nine
    capture combinations, and of every true inclusion exactly the combinations the rules keep are present.

    Which combinations the rules keep, from the rules (oracle/rdfind_oracle.py remove_implied, s2l_exact_raw), with
    a = S_a's captures (u1 = s[p=P_a], u2 = s[o=O_a], b = s[p=P_a,o=O_a]) and S_a a subset of S_b: all nine (x_a, y_b)
    are valid.  R1 drops (b_a, u_b) because (u1_a, u_b) is a 1/1 CIND; R4 drops (b_a, b_b) because (u1_a, b_b) is a 1/2
    CIND; R3 drops (u_a, u_b) because (u_a, b_b) is a 1/2 CIND whose ref has u_b as a component; V12 stays whole.  So
    the clean modes keep the two (u_a, b_b) and drop seven, the exact raw S2L mode (V11 + V12 + V21 - R1 + V22 - R4)
    keeps the six with a unary dependent, and strategy 0 raw keeps all nine (its literal `implies` filter only drops a
    binary ref whose first value is the dependent's second: a predicate is no object here)."""
    from oracle import c_oracle as C, rdfind_oracle as R
    from tests.parity import shared_captures

    sh, plain = L.shape(name, shared_objects=True), L.shape(name)
    assert sh.name == plain.name + "+o" and sh.shared_objects and not plain.shared_objects
    # the same subjects, sets and misses as the plain form: the position model still holds
    assert np.array_equal(sh.s, plain.s) and np.array_equal(sh.p, plain.p) and sh.miss == plain.miss
    assert all(np.array_equal(a, b) for a, b in zip(sh.sets, plain.sets))
    assert np.unique(sh.o).size == len(sh.sets) and sh.num_terms == sh.n_subjects + 2 * len(sh.sets)
    for k in (0, len(sh.sets) - 1):  # one object per set
        assert set(sh.o[sh.p == sh.pred(k)].tolist()) == {sh.obj(k)}
    ms = sh.min_support
    tr = list(zip(sh.s.tolist(), sh.p.tolist(), sh.o.tolist()))
    uf = R.frequent_unary_conditions(tr, ms)
    bf = R.frequent_binary_conditions(tr, uf, ms)
    lines = R.join_lines(tr, uf, bf, "s")
    raw0 = R.all_at_once(lines, ms, False)
    py = {(0, False): R.cind_set(raw0),
          (0, True): R.cind_set(R.remove_implied(*R.split_by_arity(raw0))),  # what all_at_once(clean) does with them
          (1, True): R.cind_set(R.small_to_large(lines, bf, ms, True)),
          (1, False): R.cind_set(R.all_at_once(lines, ms, False, literal_implies=False))}  # the C oracle's (1, raw) is V
    _, bkeys, _ = C.run(sh.s, sh.p, sh.o, sh.num_terms, ms, 0, False, "s")
    keys = {}
    for mode, exp in py.items():
        got, _ = C.run_set(sh.s, sh.p, sh.o, sh.num_terms, ms, mode[0], mode[1], "s")
        assert got == exp, (name, mode)
        if mode != (1, False):
            rows, _ = shape_rows(sh, mode[0], mode[1], "s")  # what the device tests compare with
            np.testing.assert_array_equal(rows, _ids(exp, sh, bkeys))
        keys[mode] = _ids(exp, sh, bkeys)
    # the device's (1, raw) is the exact raw S2L output of V
    s2l_raw = _ids(R.cind_set(R.s2l_exact_raw([R.Cind(*x) for x in py[(1, False)]])), sh, bkeys)
    if name in ("pack32", "pack33", "small300"):  # (the shapes whose (1, raw) the device tests run)
        np.testing.assert_array_equal(shape_rows(sh, 1, False, "s")[0], s2l_raw)
    V = keys[(1, False)]
    assert len(keys[(1, True)]) < len(V) and len(keys[(0, True)]) < len(keys[(0, False)])  # the rules act
    assert len(s2l_raw) < len(V)
    for k in (keys[(1, True)], keys[(0, True)], keys[(0, False)], s2l_raw):
        assert np.isin(k, V).all()
    cap = shared_captures(sh)
    pair = lambda a, i, b, j: np.uint64((int(cap[a, i]) << 32) | int(cap[b, j]))
    d = sh.idx("D")[0]
    near = [pair(d, i, k, j) for k in sh.idx("near") for i in range(3) for j in range(3)]
    assert len(near) == 9 * len(sh.idx("near")) and not np.isin(near, V).any()  # absent from V: from every mode
    true = [(d, k) for k in sh.idx("true")] + [(k, d) for k in sh.idx("sub")]
    assert true
    for a, b in true:
        nine = {(i, j): pair(a, i, b, j) for i in range(3) for j in range(3)}
        assert np.isin(list(nine.values()), V).all() and np.isin(list(nine.values()), keys[(0, False)]).all()
        for i, j in nine:
            kept_clean, kept_s2l = i < 2 and j == 2, i < 2
            assert bool(np.isin(nine[i, j], keys[(1, True)])) == kept_clean, (a, b, i, j)
            assert bool(np.isin(nine[i, j], keys[(0, True)])) == kept_clean, (a, b, i, j)
            assert bool(np.isin(nine[i, j], s2l_raw)) == kept_s2l, (a, b, i, j)


def test_expected_checksum_is_the_oracles():
    """parity.expected_checksum over the materialised rows = the streamed C oracle's checksum (the library's mix)."""
    from oracle import c_oracle as C
    from tests.parity import expected_checksum

    sh = L.shape("pack33", shared_objects=True)
    for strategy, clean in ((1, True), (0, False)):
        k, s = shape_rows(sh, strategy, clean, "s")
        st = C.stream(sh.s, sh.p, sh.o, sh.num_terms, sh.min_support, strategy, clean, "s")
        assert (len(k), expected_checksum(k, s)) == (st["n_cinds"], st["checksum"])
    assert expected_checksum(np.zeros(0, np.uint64), np.zeros(0, np.uint32)) == 0
