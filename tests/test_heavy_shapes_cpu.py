"""The heavy and class shapes (tests/heavy_shapes.py) pinned on the CPU: the set algebra of every shape's model equals
both oracles in all four modes, and every edge a shape is built for is asserted from its model, so that
tests/test_gpu_heavy_shapes.py compares the device with rows and counts that do not depend on the device."""
import numpy as np
import pytest

from tests import heavy_shapes as H
from tests.light_shapes import HMAX, _size_bucket
from tests.parity import shape_rows

MODES = [(0, False), (0, True), (1, True), (1, False)]


@pytest.mark.parametrize("name", list(H.BUILDERS))
def test_set_algebra_is_the_oracle(name):
    """rows() = the materializing C oracle in (0, raw), (0, clean), (1, clean) and the Python restatement in (1, raw):
    with unary captures alone no rule removes anything.  emit16k / emit32k are too large for the Python restatement;
    their (1, raw) rows are rows() itself, proven here on the same generator at K = 301 (emit300)."""
    sh = H.shape(name)
    assert sh.algebra_raw_s2l == (name in ("emit16k", "emit32k"))
    keys, sup = sh.rows()
    assert keys.size and np.unique(keys).size == keys.size
    for strategy, clean in MODES[:3] if sh.algebra_raw_s2l else MODES:
        ek, es = shape_rows(sh, strategy, clean, "s")
        np.testing.assert_array_equal(ek, keys, err_msg=str((name, strategy, clean)))
        np.testing.assert_array_equal(es, sup, err_msg=str((name, strategy, clean)))


def test_large_emit_shapes_use_the_proven_generator():
    for name in ("emit16k", "emit32k"):
        assert H.shape(name).algebra_raw_s2l and H.shape(name).kind.count("member") >= 9
    small, big = H.shape("emit300"), H.shape("emit16k")
    assert sorted(set(small.kind)) == sorted(set(big.kind)) == ["long", "member"]
    assert small.want["edges"][:5] == big.want["edges"][:5] == [0, 1, 31, 32, 33]


@pytest.mark.parametrize("name", list(H.BUILDERS))
def test_heavy_columns_of_every_shape(name):
    """The columns and the threshold the restated rule gives are the ones the shape was built for; every set is a
    frequent capture; objects are fresh."""
    sh = H.shape(name)
    assert len(sh.heavy()) == sh.want["n_heavy"] <= HMAX
    if "threshold" in sh.want:
        assert sh.threshold() == sh.want["threshold"]
    assert np.unique(sh.o).size == sh.n and min(len(x) for x in sh.sets) >= 2
    st = sh.class_stats()
    assert st["n_class_members"] == len(sh.heavy_only())
    assert st["n_class_cinds"] <= sh.rows()[0].size


@pytest.mark.parametrize("name,n_full", [("cols64", 1), ("cols64x9", 9), ("cols6", 2)])
def test_cols_edges(name, n_full):
    sh = H.shape(name)
    Hs, light = sh.want["H"], sh.want["light"]
    nh = len(Hs)
    assert sorted(sh.heavy().tolist()) == Hs.tolist()  # exactly H takes columns; the light subjects stay light
    gs = sh.group_sizes()
    assert gs[light].max() * 2 < gs[Hs].min()
    if nh == HMAX:  # one more group in the walk would be too many: the light bucket is refused by the count
        assert sh.heavy_min == H.DEFAULT_HEAVY_MIN <= gs[Hs].min()
    cls = {tuple(c["mask"].tolist()): c for c in sh.classes()}
    full = cls[tuple(Hs.tolist())]
    assert len(full["mask"]) == nh and len(full["members"]) == n_full == sh.kind.count("full")
    assert [sh.kind[k] for k in full["L"]] == ["full"] * n_full + ["true"] * len(light)  # nothing else covers the mask
    assert -(-n_full // H.CLS_DT) == (2 if n_full == 9 else 1)
    # the heavy-only near-misses: nh - 1 columns each, alone in their class, every column missed once
    near_h = sh.idx("near_heavy")
    missed = []
    for k in near_h:
        c = cls[tuple(sh.sets[k].tolist())]
        assert c["members"] == [k] and len(c["mask"]) == nh - 1
        missed += np.setdiff1d(Hs, sh.sets[k]).tolist()
        assert not np.isin(k, full["L"]) and np.isin(k, full["group"]) == (full["pivot"] in sh.sets[k])
    assert sorted(missed) == Hs.tolist()
    # ... and in the full class's pivot group every one but the pivot column's own is a candidate that fails the mask test
    assert sum(int(k in full["group"]) for k in near_h) == nh - 1
    # the near-misses with a light subject are not heavy-only, miss every column once, and are candidates (members of
    # the pivot group) of a true superset on the explicit path and of the full class
    near_l = sh.idx("near_light")
    assert not set(near_l) & set(sh.heavy_only())
    assert sorted(np.setdiff1d(Hs, sh.sets[k]).item() for k in near_l) == Hs.tolist()
    seen = set()
    for t in sh.idx("true"):
        assert t not in sh.heavy_only()
        piv, _ = sh.pivots(t)
        assert piv in light  # the explicit path: the candidates are the light subject's group
        for k in sh.groups_of()[piv]:
            if sh.kind[k] == "near_light":
                assert np.setdiff1d(sh.sets[t], sh.sets[k]).size == 1  # lacks exactly one column, nothing else
                seen.add(int(k))
    assert seen == set(near_l)
    assert sum(int(k in full["group"]) for k in near_l) == nh - 1
    # sub-masks of 2 and 3 columns: classes of their own, support = popcount
    sub = sh.idx("submask")
    assert sorted({len(sh.sets[k]) for k in sub}) == [2, 3]
    keys, sup = sh.rows()
    for k in sub:
        c = cls[tuple(sh.sets[k].tolist())]
        assert c["members"] == [k] and len(c["L"]) > n_full + len(light)
        assert set(sup[(keys >> np.uint64(32)) == np.uint64(sh.pred(k))].tolist()) == {len(sh.sets[k])}


def test_threshold_edges():
    b = _size_bucket
    assert b(64) == b(79) == 24 and b(80) == 25 and b(63) == 23 and b(48) == 22
    hist = lambda sh: np.bincount(_size_bucket(sh.group_sizes()), minlength=256)
    h = hist(H.shape("thr_top64"))
    assert h[24] == 64 == len(H.shape("thr_top64").heavy())  # 64 groups in the top bucket: all of them
    h = hist(H.shape("thr_top65"))
    assert h[24] == 65 and h[25:].sum() == 0 and len(H.shape("thr_top65").heavy()) == 0  # 65: no columns at all
    sh = H.shape("thr_60p4")
    h = hist(sh)
    assert (h[24], h[23], h[22]) == (60, 0, 4) and len(sh.heavy()) == 64  # the next non-empty bucket fits
    sh = H.shape("thr_60p5")
    h = hist(sh)
    assert (h[24], h[23], h[22]) == (60, 0, 5) and len(sh.heavy()) == 60  # ... or does not
    sh = H.shape("thr_ends_in")
    gs = sh.group_sizes()
    assert sorted(set(gs[sh.heavy()].tolist())) == [64, 79, 80] and 63 in gs  # both ends of bucket 24 are in
    sh = H.shape("thr_ends_out")
    gs = sh.group_sizes()
    assert set(gs[sh.heavy()].tolist()) == {80} and {64, 79} <= set(gs.tolist())  # both ends of bucket 24 are out
    sh = H.shape("thr_min70")
    gs = sh.group_sizes()
    light = np.setdiff1d(np.arange(sh.n_subjects), sh.heavy())
    assert sh.heavy_min == sh.threshold() == 70 and 64 in gs[light] and b(64) == b(79) and 79 in gs[sh.heavy()]
    sh = H.shape("thr_min_default")
    assert sh.heavy_min == H.DEFAULT_HEAVY_MIN == sh.threshold() and 63 in sh.group_sizes()


@pytest.mark.parametrize("name,nseg", [("emit300", 1), ("emit16k", 2), ("emit32k", 3)])
def test_emit_edges(name, nseg):
    sh = H.shape(name)
    (c,) = sh.classes()
    n = sh.want["list_len"]
    assert c["mask"].tolist() == [0, 1, 2] == sorted(sh.heavy().tolist()) and len(c["L"]) == n == len(sh.sets)
    assert -(-n // H.CLS_LS) == nseg
    members = c["members"]
    assert members == sh.idx("member") and len(members) == (65 if name == "emit16k" else 9)
    # the members' own places in the list are the wanted edges and a seeded remainder
    pos = [c["selfpos"][k] for k in members]
    assert pos == sh.want["member_pos"].tolist() == members  # (every predicate is in the list: place = set index)
    assert set(sh.want["edges"]) <= set(pos)
    if name == "emit16k":
        assert {0, 1, 31, 32, 33, 16351, 16352, 16383, 16384, 16385, n - 2, n - 1} <= set(pos) and len(pos) > 12
        assert _size_bucket(sh.group_sizes()[:3]).tolist() == [56] * 3
    if name == "emit32k":
        assert {0, 16383, 16384, 16385, 32767, 32768, 32769, n - 2, n - 1} == set(pos)
    # the long captures are not heavy-only and cost nothing: their pivot is a private group of one
    for k in sh.idx("long")[:50] + sh.idx("long")[-50:]:
        piv, _ = sh.pivots(k)
        assert sh.group_sizes()[piv] == 1 and k not in sh.heavy_only()
    # a run has an odd number of refs: the member runs, consecutive in the output, start at every residue mod 64
    n_run = n - 1
    assert n_run % 2 == 1
    starts = {(i * n_run) % 64 for i in range(len(members))}
    assert len(starts) == min(len(members), 64)
    if name == "emit16k":
        assert starts == set(range(64))
    st = sh.class_stats()
    assert st["n_class_cinds"] == len(members) * n_run == sh.rows()[0].size
    assert st["n_emit_tiles"] == -(-len(members) // H.CLS_DT) * nseg
    assert st["max_class_list"] == n and st["n_multi_seg_lists"] == (nseg > 1)
    assert st["n_class_chunks"] == -(-n // 64)
    if name == "emit16k":
        assert 65_000 <= sh.n <= 66_000 and st["n_class_cinds"] > 1_000_000


def test_lists_small_edges():
    sh = H.shape("lists_small")
    assert len(sh.heavy()) == sh.n_subjects == 18 and len(sh.heavy_only()) == len(sh.sets)  # every dependent is classed
    cl = sh.classes()
    got = {(len(c["L"]), len(c["members"])) for c in cl}
    assert set(H.LIST_SPECS) <= got, sorted(got)
    assert {ln for ln, _ in H.LIST_SPECS} == {1, 2, 32, 33, 63, 64, 65, 128, 129}
    assert {nm for _, nm in H.LIST_SPECS} == {1, 7, 8, 9, 17}  # both sides of CLS_DT = 8, and two tiles plus one
    lone = [c for c in cl if len(c["L"]) == 1]
    assert lone and all(len(c["members"]) == 1 for c in lone)  # the member alone: an empty run


# ---------------------------------------------------------------------------------------------------------------------
# families C and D (shared objects)

EXTRA_VARIANTS = ("member_covered", "all65", "lackpiv")


@pytest.mark.parametrize("name", ["r3", "r3s"])
def test_r3_parent_lists_and_covering_places(name):
    """Every R = s[p=P] of the shape has the parent count it was built for, on both sides of PARENT_SCAN_MAX; the parents
    that cover m stand where the variant says (first, last, 32nd, 33rd of plist, two, all, none), every other parent
    lacks exactly one column of m; R is in L'(m) exactly when no parent covers."""
    sh = H.shape(name)
    qs = H.R3_QS if name == "r3" else (1, 32, 33)
    M = sh.model()
    m = sh.mask
    lst_clean, lst_raw = sh.class_list(m, True), sh.class_list(m, False)
    seen = set()
    for P, spec in sh.preds.items():
        r = M["index"][("p", (P,))]
        par = M["parents"][r]
        assert len(par) == spec["q"] and all(M["caps"][x]["key"][0] == P for x in par)
        assert [M["caps"][x]["key"][1] for x in par] == sorted(M["caps"][x]["key"][1] for x in par)  # plist order
        assert [j for j, x in enumerate(par) if sh.covers(x, m)] == spec["cover"]
        for j, x in enumerate(par):
            if j not in spec["cover"]:
                assert len(set(m) - set(M["caps"][x]["subj"])) == 1
        assert sh.covers(r, m) and r in lst_raw and (r in lst_clean) == (not spec["cover"])
        if spec["variant"] not in EXTRA_VARIANTS:
            seen.add((spec["q"], spec["variant"]))
    assert {q for q, _ in seen} == set(qs) and min(qs) <= H.PARENT_SCAN_MAX < max(qs)
    assert {32, 33} <= set(qs) and {31, 32, 33} <= set(H.R3_QS)  # the parent scan's last entry, its limit, and the first list left to the marks
    for q in qs:
        want = {"none", "first", "last"} | ({"p32", "p33"} if q >= 33 else set()) | ({"two"} if q >= 64 else set()) \
            | ({"all"} if q <= 33 else set())
        assert {v for qq, v in seen if qq == q} == want, q
    assert "member_covered" in {s["variant"] for s in sh.preds.values()}


def test_r3_pivot_group_places():
    """R at places 0, 63 and 64 of the class's pivot group, all three cleared by the marks (more than
    PARENT_SCAN_MAX parents, one covering); every covering binary lies in a later chunk than its R; the two covering
    binaries of a `two` variant lie in different chunks; the member with a covering parent is absent from its own list."""
    sh = H.shape("r3")
    M = sh.model()
    m = sh.mask
    g = M["groups"][sh.pivot(m)]
    place = {c: i for i, c in enumerate(g)}
    at = {}
    split_two = 0
    for P, spec in sh.preds.items():
        r = M["index"][("p", (P,))]
        at[place[r]] = spec
        cov = [x for x in M["parents"][r] if sh.covers(x, m)]
        assert all(place[x] // H.WAVE > place[r] // H.WAVE for x in cov)
        if spec["variant"] == "two":
            split_two += place[cov[0]] // H.WAVE != place[cov[1]] // H.WAVE
            assert spec["q"] < 200 or place[cov[0]] // H.WAVE != place[cov[1]] // H.WAVE  # two chunks clear one R
    for q in (0, 63, 64):
        assert at[q]["q"] > H.PARENT_SCAN_MAX and at[q]["cover"], q
    assert split_two >= 1
    assert len(g) % H.WAVE != 0  # a last, partly filled chunk
    st = sh.class_stats(True, True)
    px = [P for P, s in sh.preds.items() if s["variant"] == "member_covered"][0]
    assert M["index"][("p", (px,))] in st["absent"] and M["caps"][M["index"][("p", (px,))]]["subj"] == m
    assert not sh.class_stats(False, True)["absent"]  # raw: every member is in its own list


def test_r3_binary_dependents_and_lists():
    """Family D: every capture is heavy-only, the binary ones included; the binary dependents of the D pairs have clean
    lists of exactly 63, 64, 65 and 129 entries (themselves), and raw lists that also hold both components of each."""
    sh = H.shape("r3")
    M = sh.model()
    assert len(sh.heavy()) == sh.n_subjects <= HMAX and len(M["caps"]) > M["cu"] > 0
    assert sh.__dict__["d_lists"] == H.D_LISTS == (63, 64, 65, 129)
    for pair, k in zip(sh.__dict__["d_pairs"], H.D_LISTS):
        clean, raw = sh.class_list(pair, True), sh.class_list(pair, False)
        assert len(clean) == k and all(i >= M["cu"] for i in clean)
        assert len(raw) == 2 * k + 1 and sum(i < M["cu"] for i in raw) == k + 1
    # one binary dependent has a mask that no unary capture has: its class exists only where the binaries are classed
    u = sh.__dict__["unique"]
    assert M["caps"][M["index"][("po", u["key"])]]["subj"] == u["mask"]
    assert all(c["subj"] != u["mask"] for c in M["caps"][:M["cu"]])
    assert sh.class_stats(True, True)["n_classes"] == sh.class_stats(True, False)["n_classes"] + 1
    assert sh.class_stats(True, True)["scan_chunks"] > 0


def test_r3_mark_edges():
    """k_class_mark's edges, from the model's group places.  (a) one chunk of m's pivot group holds >= 6 covering
    binaries with distinct components of more than PARENT_SCAN_MAX parents: wave_merge<u64, 4> runs out of rounds.
    (b) the 65 covering binaries of `all65` are consecutive and cross from lane 63 of a chunk into lane 0 of the next:
    the head at a chunk start.  (c) the tail class: R at place 64 of a pivot group of 67, cleared by the marks (33
    parents) from the binary at place 66 of the same, last and partly filled chunk."""
    sh = H.shape("r3")
    M = sh.model()
    m = sh.mask
    piv = sh.pivot(m)
    g = M["groups"][piv]
    place = {c: i for i, c in enumerate(g)}
    long_heads = {}  # chunk -> the distinct long components (s[p=P]) of its covering binaries
    for i in g:
        c = M["caps"][i]
        if i >= M["cu"] and sh.covers(i, m) and len(M["parents"][M["index"][("p", c["key"][:1])]]) > H.PARENT_SCAN_MAX:
            long_heads.setdefault(place[i] // H.WAVE, set()).add(c["key"][0])
    assert max(len(v) for v in long_heads.values()) >= 6
    lack = [P for P, s in sh.preds.items() if s["variant"] == "lackpiv"]
    assert len(lack) == H.N_LACKPIV
    for P in lack:  # of each only the covering binary is in the pivot group: the others lack the pivot subject
        par = M["parents"][M["index"][("p", (P,))]]
        assert len(par) == 33 and sum(x in place for x in par) == 1 == sum(sh.covers(x, m) for x in par)
        assert all(piv not in M["caps"][x]["subj"] for x in par if not sh.covers(x, m))
    (p65,) = [P for P, s in sh.preds.items() if s["variant"] == "all65"]
    run = [place[x] for x in M["parents"][M["index"][("p", (p65,))]]]
    assert len(run) == 65 and run == list(range(run[0], run[0] + 65))
    assert any(a % H.WAVE == 63 and b % H.WAVE == 0 for a, b in zip(run, run[1:]))
    tail = sh.__dict__["tail"]
    tp = sh.pivot(tail["pair"])
    tg = M["groups"][tp]
    r = M["index"][("p", (tail["P"],))]
    cov = [x for x in M["parents"][r] if sh.covers(x, tail["pair"])]
    assert len(tg) == H.N_TAIL_FILL + 3 and tg.index(r) == 64 and len(M["parents"][r]) == 33 > H.PARENT_SCAN_MAX
    assert len(cov) == 1 and tg.index(cov[0]) == 66 and len(tg) % H.WAVE == 3
    assert r in sh.class_list(tail["pair"], False) and r not in sh.class_list(tail["pair"], True)


def test_r3s_is_pinned_to_both_oracles():
    """The reduced shape, the same generator at a size the Python restatement can take: in mode (1, raw) the restatement's
    rows are a subset of the C oracle's (0, raw) rows and hold the model's number of rows with a unary dependent, raw
    lists that hold binaries and their components included; the clean modes of both strategies agree with the model."""
    sh = H.shape("r3s")
    M = sh.model()
    assert sh.n < 1000 and len(M["caps"]) > M["cu"] > 0 and sh.__dict__["d_lists"] == (5,)
    k1r, _ = shape_rows(sh, 1, False, "s")
    k0r, _ = shape_rows(sh, 0, False, "s")
    assert np.isin(k1r, k0r).all()
    unary = lambda k: int(((k >> np.uint64(32)) < np.uint64(6 * sh.num_terms)).sum())
    assert unary(k1r) == unary(k0r) == sh.class_stats(False, True)["n_class_cinds"]
    for strategy in (0, 1):
        k, _ = shape_rows(sh, strategy, True, "s")
        assert unary(k) == sh.class_stats(True, True)["n_class_cinds"]
    raw_list = sh.class_list(sh.__dict__["d_pairs"][0], False)
    assert len(raw_list) == 11 and sum(i >= M["cu"] for i in raw_list) == 5


@pytest.mark.parametrize("name", ["r3", "r3s"])
def test_r3_model_counts_the_oracles_unary_rows(name):
    """The model's L'(m) (mask test, then R3 by covering parents) gives the oracle's number of rows with a unary
    dependent, clean and raw: the class counts the GPU test asserts do not come from the device."""
    sh = H.shape(name)
    for clean in (True, False):
        keys, _ = shape_rows(sh, 0, clean, "s")
        unary = int(((keys >> np.uint64(32)) < np.uint64(6 * sh.num_terms)).sum())
        assert unary == sh.class_stats(clean, True)["n_class_cinds"], clean
    k1, s1 = shape_rows(sh, 1, True, "s")
    k0, s0 = shape_rows(sh, 0, True, "s")
    assert k1.size and k0.size
