"""What the shapes must contain before a sharded GPU run of them means anything, asserted from the rank model
(tests/shard_shapes.py; the owner functions are those of tests/shard_sim.py).  tests/test_gpu_sharded_shapes.py runs
the shapes; here, on the CPU, each condition is a property of the inputs: the subjects a near-miss lacks lie on other
ranks than the one that draws the candidates, a dependent's groups lie on every rank, the segment, column and threshold
edges fall where the sharded code decides, and the verify-edge shapes have the verify counts they are named after."""
import numpy as np
import pytest

from tests import heavy_shapes as H
from tests import light_shapes as L
from tests import shard_shapes as S

LIGHT = ("pack32", "pack33", "small300", "cand63", "cand64", "cand65", "cand129", "seg2", "seg3", "pack80h", "pack81h")
SETTINGS = [(w, hb) for w in (2, 3) for hb in (True, False)]
SET_IDS = [f"w{w}-{'hot' if hb else 'hash'}" for w, hb in SETTINGS]


def forms(name):
    """(shape, RDFIND_HEAVY_MIN it runs under) of every form the GPU matrix runs."""
    if name in S.VEDGE:
        return [(S.vedge(name), L.NO_HEAVY)]
    if name.startswith("pack8"):
        return [(L.shape(name), 2)]
    out = [(L.shape(name), L.NO_HEAVY)]
    if name in ("small300", "cand65", "seg3"):
        out.append((L.shape(name, True), None))
    if name in ("pack33", "small300", "cand65"):
        out.append((L.shape(name, shared_objects=True), L.NO_HEAVY))
    if name in ("small300", "cand65"):
        out.append((L.shape(name, True, True), None))
    return out


@pytest.mark.parametrize("world,hot", SETTINGS, ids=SET_IDS)
@pytest.mark.parametrize("name", LIGHT + tuple(S.VEDGE))
def test_rank_spread(name, world, hot):
    """The missed subjects of D's near-misses lie on at least two ranks (whichever rank holds D, a verify pass on
    another must reject a pair the holder kept), at world 2 on both; D's groups lie on every rank."""
    for sh, hm in forms(name):
        f = S.facts(sh, world, heavy_min=hm, hot_balance=hot)
        d = sh.idx("D")[0]
        mr = S.miss_ranks(sh, world, heavy_min=hm, hot_balance=hot)
        assert sum(1 for x in mr if x) >= 2 and S.misses_off_every_holder(sh, world, heavy_min=hm, hot_balance=hot), (sh.name, mr)
        if world == 2:
            assert min(mr) >= 1, (sh.name, mr)
        assert min(f[d]["groups"]) >= 1, (sh.name, f[d]["groups"])
        # the missed subjects are light (the verify pass is a light pass): D has a light group on every rank
        assert f[d]["nrl"] == world, (sh.name, f[d]["light"])
        # replicated input: the row ranges have the sizes of the slices here, so the owners are the same
        assert S.slice_sizes(sh.n, world, False) == sorted(S.slice_sizes(sh.n, world, True))
        assert (S.subject_owners(sh, world, hot, False) == S.subject_owners(sh, world, hot, True)).all()


@pytest.mark.parametrize("world,hot", SETTINGS, ids=SET_IDS)
def test_every_nrl_occurs(world, hot):
    """Dependents with a light group on one rank only, on two and, at world 3, on three: need = 1, 2, 3 in
    k_mult_flags.  The two-subject sets of the verify-edge shapes give the small values under every setting."""
    seen = set()
    for name in LIGHT + tuple(S.VEDGE):
        for sh, hm in forms(name):
            seen |= {x["nrl"] for x in S.facts(sh, world, heavy_min=hm, hot_balance=hot)}
    assert set(range(1, world + 1)) <= seen, seen
    for name in S.VEDGE:  # ... and each of these shapes alone has a one-rank dependent: a two-subject set on one owner
        sh = S.vedge(name)
        f = S.facts(sh, world, hot_balance=hot)
        one = [k for k in sh.idx("other") if f[k]["nrl"] == 1]
        assert one and all(len(sh.sets[k]) == 2 for k in one), name


@pytest.mark.parametrize("hot", [True, False], ids=["hot", "hash"])
def test_all_subjects_are_hot_by_default(hot):
    """In the small shapes every subject reaches n / (R 4096) occurrences: the balanced table decides every owner by
    default and the hash decides none, so both settings must run."""
    sh = L.shape("cand64")
    a, b = S.subject_owners(sh, 3, True), S.subject_owners(sh, 3, False)
    assert (a != b).any()
    load = np.bincount(a, weights=np.bincount(sh.s.astype(np.int64), minlength=sh.num_terms)[: sh.n_subjects], minlength=3)
    assert load.max() - load.min() <= sh.group_sizes().max()  # balanced: largest first to the least loaded rank


@pytest.mark.parametrize("hot", [True, False], ids=["hot", "hash"])
def test_seg3_is_multi_segment_at_world_2_only(hot):
    """seg3 at world 2: some rank holds more than LIGHT_SEG groups of D and of a near-miss, so the verify pass, which
    skips no pivot, runs multi-segment; at world 3 no rank does."""
    sh = L.shape("seg3")
    f = S.facts(sh, 2, hot_balance=hot)
    d = sh.idx("D")[0]
    assert max(f[d]["light"]) > L.LIGHT_SEG, f[d]["light"]
    assert any(max(f[k]["light"]) > L.LIGHT_SEG for k in sh.idx("near"))
    assert max(max(x["light"]) for x in S.facts(sh, 3, hot_balance=hot)) <= L.LIGHT_SEG
    # (the ballast form has 64 of D's groups as columns: 2018 light groups per rank, one segment, beside the heavy masks)
    assert max(S.facts(L.shape("seg3", True), 2, heavy_min=None, hot_balance=hot)[d]["light"]) <= L.LIGHT_SEG
    sh = L.shape("seg2")  # two segments on one GPU, one per rank when sharded
    assert max(max(x["light"]) for x in S.facts(sh, 2, hot_balance=hot)) <= L.LIGHT_SEG < sh.m


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["cols64", "cols64x9", "thr_top64", "thr_60p4"])
def test_columns_split_over_the_ranks(name, world):
    """Every rank holds at least one of the 64 columns and none holds them all: the bit bases (collective 2) and the
    summed masks (collective 3) carry the result."""
    sh = H.shape(name)
    per = S.heavy_per_rank(sh, world)
    assert sum(per) == sh.want["n_heavy"] == 64 and min(per) >= 1 and max(per) < 64, per


# name -> smallest group size of the bucket the global rule refuses (tests/heavy_shapes.py THRESHOLDS)
REFUSED = {"thr_top65": 64, "thr_60p5": 48, "thr_ends_out": 64}


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_bucket_fits_locally(name, world):
    """Down to the bucket the global histogram refuses (more than 64 groups in all) every rank sees at most 64 groups
    of its own: a rank that decided on its local histogram would take columns the global rule refuses."""
    sh = H.shape(name)
    lo = REFUSED[name]
    per = S.bucket_groups_per_rank(sh, world, lo, 1 << 30)
    assert sum(per) > 64 >= max(per) and min(per) >= 1, per
    assert len(sh.heavy()) == sh.want["n_heavy"] < sum(per)
    local = [np.nonzero((S.subject_owners(sh, world) == r))[0] for r in range(world)]
    gs = sh.group_sizes()
    for r, mine in enumerate(local):  # the rule on the rank's own groups takes more columns than the rank may have
        hist = np.bincount(L._size_bucket(gs[mine]), minlength=256)
        cum, best = 0, -1
        for q in range(255, -1, -1):
            cum += hist[q]
            if cum > L.HMAX:
                break
            if hist[q]:
                best = q
        alone = int(((L._size_bucket(gs[mine]) >= best) & (gs[mine] >= sh.heavy_min)).sum()) if best >= 0 else 0
        assert alone > S.heavy_per_rank(sh, world)[r], (name, r, alone)


@pytest.mark.parametrize("name", ["cols64x9", "emit16k", "lists_small"])
def test_class_members_have_owners_on_two_ranks(name):
    for world in (2, 3):
        per = S.member_owners(H.shape(name), world)
        assert sum(per) == S.class_model(H.shape(name))["n_class_members"] and sum(1 for x in per if x) >= 2, per


@pytest.mark.parametrize("name", list(S.VEDGE))
def test_vedge_verify_counts(name):
    """The verify pairs of D at world 2 under the default owners are 63 / 64 / 65 / 129 whichever rank holds D: both
    sides of one chunk of 64 candidates and a last chunk of one octet.  No other dependent receives as many."""
    sh = S.vedge(name)
    want = S.VEDGE[name]
    assert S.vedge_verify_pairs(sh) == want == len(sh.idx("true")) + S.VEDGE_PAIRS
    own = S.subject_owners(sh, 2)
    near = sh.idx("near")
    assert len(near) == 2 * S.VEDGE_PAIRS
    for pair in (near[:2], near[2:]):  # each pair misses one subject of each rank
        assert sorted(own[[sh.miss[k] for k in pair]].tolist()) == [0, 1]
    d = sh.idx("D")[0]
    inc = sh.inclusions()
    refs = np.sort(inc[(inc >> np.uint64(32)) == np.uint64(sh.pred(d))] & np.uint64(0xFFFFFFFF))
    assert refs.tolist() == [sh.pred(k) for k in sh.idx("true")]  # D's refs are its trues alone
    # candidates ascend by capture id: a near-miss pair before the first true and one behind the last
    assert max(near[:2]) < min(sh.idx("true")) and min(near[2:]) > max(sh.idx("true"))
    for k in near:
        assert np.setdiff1d(sh.sets[d], sh.sets[k]).tolist() == [sh.miss[k]]
    # every other dependent has a pivot group of fewer members than D has verify pairs: D's count is the maximum
    gs = sh.group_sizes()
    for k in range(len(sh.sets)):
        if k != d:
            assert gs[sh.sets[k]].min() < want - 1, (name, k)
    # D's smallest groups are missed positions, with 1 + n_true + 3 members
    assert gs[sh.sets[d]].min() == len(sh.idx("true")) + 4 and sh.pivots(d)[0] in [sh.miss[k] for k in near]
    assert sh.heavy_subjects(1 << 30).size == 0 and sh.n < 6000


@pytest.mark.parametrize("name", list(S.VEDGE))
def test_vedge_oracle_is_set_inclusion(name):
    """The verify-edge shapes pinned like the near-miss shapes (tests/test_light_shapes_cpu.py): strategy 0 raw is
    exactly the inclusions among the sets, the other modes a subset, no (D, near-miss) pair anywhere."""
    from tests.parity import shape_rows
    sh = S.vedge(name)
    inc = sh.inclusions()
    raw, raw_sup = shape_rows(sh, 0, False, "s")
    np.testing.assert_array_equal(raw, inc)
    sizes = {sh.pred(k): len(x) for k, x in enumerate(sh.sets)}
    assert [sizes[int(k) >> 32] for k in raw] == raw_sup.tolist()
    d = sh.idx("D")[0]
    near = [sh.pair_key(d, k) for k in sh.idx("near")]
    for strategy, clean in ((1, True), (0, True), (1, False)):
        keys, _ = shape_rows(sh, strategy, clean, "s")
        assert np.isin(keys, inc).all() and not np.isin(near, keys).any(), (strategy, clean)
    assert np.unique(sh.o).size == sh.n and min(len(x) for x in sh.sets) >= 2
