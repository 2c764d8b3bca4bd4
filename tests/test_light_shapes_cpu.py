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
