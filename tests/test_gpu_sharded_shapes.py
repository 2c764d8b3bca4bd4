"""The near-miss, heavy, class and rule shapes through the sharded exchange: 2 and 3 ranks on the one GPU of the test
box (gloo), row-exact against the oracle, with proof from rdf_test_shard_report that the exchange did the rejecting.

tests/light_shapes.py and tests/heavy_shapes.py build the inputs, tests/shard_shapes.py says on which rank every
subject's group lives, and tests/test_shard_shapes_cpu.py asserts from it that the inputs hold what the protocol must
reject: candidates that have every join value of a dependent but one, that one on a rank other than the holder's.  The
holder's light pass keeps such a pair, k_route_survivors sends it to the rank with the missing value, that rank's verify
pass (sh_phase15) must reject it, and k_mult_flags on the owner must drop the pair for the missing report.

One spawn per test: a worker per rank runs a list of cells (shape, mode, projection, rules on / off, switches), one
context per switch set (the switches are read when a context is created), and returns per cell its rows (decoded by
parity.device_rows, ids checked first), count, checksum, statistics and shard report.  The parent opens no context:
the expectation is the oracle's rows (parity.shape_rows).  Per cell the ranks' rows are pairwise disjoint and their
sorted union equals the oracle's, row for row and support for support; the counts sum to its length and the checksums
sum mod 2^64 to the checksum of the expected rows.

Modes: all four under projection ``s``; mode (1, raw), whose only oracle is the Python restatement, on the shapes
tests/test_gpu_light_shapes.py runs it on (RAW_S2L_SHAPES), the verify-edge shapes and the small shared-object forms.

After a rank process ends on a signal, is terminated at its limit or reports a HIP error, every later test of this file
skips: nothing more of it starts on the card.
"""
import os
import queue

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import heavy_shapes as H
from tests import light_shapes as L
from tests import shard_shapes as S
from tests.parity import expected_checksum, shape_rows
from tests.test_gpu_sharded import _free_port

pytestmark = pytest.mark.gpu

MODES = [(1, True), (0, True), (0, False), (1, False)]
MODES3 = MODES[:3]
RAW_S2L = ("pack32", "pack33", "pack80h", "pack81h", "small300") + tuple(S.VEDGE)  # tests/test_gpu_light_shapes.py + vedge
NO_HEAVY = {"RDFIND_HEAVY_MIN": L.NO_HEAVY}
Q_TIMEOUT = 180
_FAULT = []  # reasons; non-empty: a rank faulted, hung or reported a HIP error


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    if _FAULT:
        pytest.skip(f"an earlier sharded run of this file faulted or hung: {_FAULT[0]}")


def get_shape(key):
    kind, name, ballast, shared = key
    return H.shape(name) if kind == "H" else S.light_shape(name, ballast, shared)


def light(name, ballast=False, shared=False):
    return ("L", name, ballast, shared)


def heavy(name):
    return ("H", name, False, False)


def cell(key, strategy, clean, env, projection="s", use_ars=False):
    return (key, strategy, clean, projection, use_ars, tuple(sorted(env.items())))


def _cells_worker(rank, world, port, cells, q, slices):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rdfind_amd import _lib, distributed
    from tests.parity import device_rows

    out, ctx, cur_env, cur_shape, set_keys = [], None, None, None, []
    try:
        for key, strategy, clean, proj, use_ars, env in cells:
            if ctx is None or env != cur_env:  # the switches are read when a context is created
                if ctx is not None:
                    ctx.close()
                for k in set_keys:
                    os.environ.pop(k, None)
                set_keys = [k for k, _ in env]
                os.environ.update(dict(env))
                ctx, cur_env, cur_shape = _lib.Context(0), env, None
            if key != cur_shape:
                sh = get_shape(key)
                if slices:
                    ctx.set_triples(sh.s[rank::world], sh.p[rank::world], sh.o[rank::world], sh.num_terms)
                else:
                    ctx.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
                cur_shape = key
            gs, cs = distributed.run_sharded(ctx, sh.min_support, proj, clean, strategy, local_slice=slices,
                                             use_ars=use_ars)
            item = {"report": ctx.test_shard_report(), "n": ctx.cind_count(), "checksum": ctx.checksum(),
                    "groups": {k: int(gs[k]) for k in ("n_heavy_groups", "heavy_threshold", "n_join_ranges")},
                    "cinds": {k: int(cs[k]) for k in ("n_classes", "n_class_members", "n_explicit_raw")}}
            item["keys"], item["sup"] = device_rows(ctx)
            item["expanded"] = (ctx.cind_count(), ctx.checksum())  # after the rows were expanded: must be unchanged
            if use_ars:
                item["rules"] = sorted(map(tuple, ctx.copy_association_rules().tolist()))
                item["decoded"] = _lib.decoded_to_set(ctx.decoded_cinds())
            out.append(item)
        if ctx is not None:
            ctx.close()
        q.put((rank, out))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, repr(e) + "\n" + traceback.format_exc()[-1500:]))
        try:  # a peer already in its next cell stops at that cell's first header instead of waiting for this rank
            distributed.agree(1, 0, 0, None, None, distributed.exchange_device())
        except Exception:
            pass
    finally:
        dist.destroy_process_group()


def run_cells(world, cells, slices=True):
    """{rank: [item per cell]}.  The spawn's own limits: Q_TIMEOUT per answer, the workers joined, then terminated."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cells_worker, args=(r, world, port, cells, q, slices)) for r in range(world)]
    for p in procs:
        p.start()
    res, failed = {}, None
    try:
        for _ in procs:
            try:
                r, item = q.get(timeout=Q_TIMEOUT)
            except queue.Empty:
                _FAULT.append(f"no answer from a rank within {Q_TIMEOUT} s")
                raise AssertionError(_FAULT[-1])
            if isinstance(item, str):
                if "hip" in item.lower():
                    _FAULT.append(f"rank {r} reported a HIP error")
                failed = failed or f"rank {r}: {item}"
                break  # its peers stop at the next header (PeerFailure)
            res[r] = item
    finally:
        for p in procs:
            p.join(timeout=60 if len(res) == world else 10)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
                _FAULT.append("a rank process was terminated at its limit")
            elif p.exitcode is not None and p.exitcode < 0:
                _FAULT.append(f"a rank process ended on signal {-p.exitcode}")
    assert failed is None, failed
    assert not _FAULT, _FAULT
    return res


def expected_rows(sh, strategy, clean, proj):
    ek, es = shape_rows(sh, strategy, clean, proj)
    return ek, es, expected_checksum(ek, es)


def check_rows(world, parts, sh, strategy, clean, proj, what):
    """Disjoint parts whose sorted union is the oracle's rows; counts and checksums sum to the oracle's."""
    ek, es, eh = expected_rows(sh, strategy, clean, proj)
    keys = np.concatenate([p["keys"] for p in parts])
    sup = np.concatenate([p["sup"] for p in parts])
    assert np.unique(keys).size == keys.size, (what, "a row on two ranks")
    order = np.argsort(keys, kind="stable")
    gk, gs = keys[order], sup[order]
    assert gk.size == ek.size and (gk == ek).all(), (what, gk.size, ek.size,
                                                    {"device_only": np.setdiff1d(gk, ek)[:4].tolist(),
                                                     "oracle_only": np.setdiff1d(ek, gk)[:4].tolist()})
    np.testing.assert_array_equal(gs, es, err_msg=str(what))
    assert [p["n"] for p in parts] == [p["keys"].size for p in parts], what
    assert all(p["expanded"] == (p["n"], p["checksum"]) for p in parts), (what, "count or checksum changed by the expansion")
    assert sum(p["n"] for p in parts) == ek.size, what
    assert sum(p["checksum"] for p in parts) % (1 << 64) == eh, what


def rsum(parts, field):
    return sum(p["report"][field] for p in parts)


def check_exchange(world, parts, sh, env, what, hot=True):
    """What the report must say about the exchange of a light or shared-object cell."""
    rep = [p["report"] for p in parts]
    assert [(r["rank"], r["nranks"]) for r in rep] == [(k, world) for k in range(world)], what
    # every word sent arrives: reports at the owners, verify words at the verifiers
    assert rsum(parts, "verify_sent") == rsum(parts, "verify_received"), what
    assert rsum(parts, "reports_sent") == rsum(parts, "reports_received") == rsum(parts, "holder_survivors"), what
    for r in rep:
        assert r["routed_words"] == r["reports_sent"] + r["verify_sent"] and r["verify_kept"] <= r["verify_received"], what
        assert r["owner_kept"] == r["unary_own"] + r["binary_own"], what
    assert rsum(parts, "owner_reports") == rsum(parts, "holder_survivors") + rsum(parts, "verify_kept"), what
    assert len({r["unary_gathered"] for r in rep}) == 1 and rep[0]["unary_gathered"] == rsum(parts, "unary_own"), what
    hm = dict(env).get("RDFIND_HEAVY_MIN")
    if S.misses_off_every_holder(sh, world, heavy_min=hm, hot_balance=hot):
        # a verify pass rejected pairs a holder kept ...
        assert rsum(parts, "verify_received") - rsum(parts, "verify_kept") > 0, what
        # ... and the owners dropped them: reports that never became a need-complete pair (every kept pair has its
        # holder's report, so the holders' survivors beyond the kept pairs are the pairs with a report missing)
        assert rsum(parts, "owner_reports") - rsum(parts, "owner_kept") > 0, what
        assert rsum(parts, "holder_survivors") - rsum(parts, "owner_kept") > 0, what


def light_cells(names, ballast_names=(), shared=False, env=NO_HEAVY, raw=RAW_S2L):
    out = []
    for name in names:
        e = {"RDFIND_HEAVY_MIN": "2"} if name.startswith("pack8") else env
        for strategy, clean in (MODES if name in raw else MODES3):
            out.append(cell(light(name, False, shared), strategy, clean, e))
    for name in ballast_names:  # the default heavy setting: the 64 columns go to the ballast
        for strategy, clean in MODES3:
            out.append(cell(light(name, True, shared), strategy, clean, {k: v for k, v in env.items() if k != "RDFIND_HEAVY_MIN"}))
    return out


def run_light(world, cells, slices=True, hot=True):
    res = run_cells(world, cells, slices)
    fan = False
    for i, (key, strategy, clean, proj, use_ars, env) in enumerate(cells):
        sh = get_shape(key)
        what = (sh.name, world, "slices" if slices else "replicated", strategy, clean, dict(env))
        parts = [res[r][i] for r in range(world)]
        check_rows(world, parts, sh, strategy, clean, proj, what)
        check_exchange(world, parts, sh, env, what, hot)
        assert all((p["report"]["hot_entries"] > 0) == hot for p in parts), what
        fan |= any(p["report"]["verify_sent"] > p["report"]["holder_survivors"] for p in parts)
        if key[1] in S.VEDGE and world == 2 and hot and slices:
            # the most verify pairs one dependent received: D's, whichever rank holds it
            got = [p["report"]["max_verify_per_dep"] for p in parts]
            assert None not in got and max(got) == S.VEDGE[key[1]] == S.vedge_verify_pairs(sh), (what, got)
    return res, fan


SMALL = ("pack32", "pack33", "small300", "cand63", "cand64", "cand65", "cand129", "pack80h", "pack81h") + tuple(S.VEDGE)
SMALL_BALLAST = ("small300", "cand65")
SEG = ("seg2", "seg3")
SEG_BALLAST = ("seg3",)
CONFIGS = [(2, True, True), (3, True, True), (2, False, True), (2, True, False)]  # (world, slices, default owners)
CONFIG_IDS = ["w2-slices", "w3-slices", "w2-replicated", "w2-slices-hash"]


def test_process_start_cost():
    """An empty cell list at world 3: what every test below pays before its first cell (its duration is the measure)."""
    res = run_cells(3, [])
    assert res == {0: [], 1: [], 2: []}


@pytest.mark.parametrize("world,slices,hot", CONFIGS, ids=CONFIG_IDS)
def test_light_small(world, slices, hot):
    env = NO_HEAVY if hot else dict(NO_HEAVY, RDFIND_HOT_BALANCE="0")
    cells = light_cells(SMALL, SMALL_BALLAST, env=env)
    if not hot:  # (pack80h / pack81h run under their own heavy minimum)
        cells = [c[:5] + (tuple(sorted(dict(c[5], RDFIND_HOT_BALANCE="0").items())),) for c in cells]
    _, fan = run_light(world, cells, slices, hot)
    # world 3: a dependent with light groups on three ranks sends two verify words per survivor
    assert fan == (world == 3), (world, fan)


@pytest.mark.parametrize("world,slices,hot", CONFIGS, ids=CONFIG_IDS)
def test_light_segments(world, slices, hot):
    """seg2 / seg3: at world 2 a rank holds more than LIGHT_SEG groups of seg3's D, so the verify pass is
    multi-segment; the ballast form of seg3 adds the heavy masks of 64 columns spread over the ranks."""
    env = NO_HEAVY if hot else dict(NO_HEAVY, RDFIND_HOT_BALANCE="0")
    run_light(world, light_cells(SEG, SEG_BALLAST, env=env), slices, hot)


@pytest.mark.parametrize("world", [2, 3])
def test_shared_objects(world):
    """The shared-object forms: collective 8 feeds the unary dependents' pairs to the explicit rules (k_rules_explicit ->
    rule_keep -> member, k_rules_mark), which here see near-misses in nine capture combinations."""
    cells = light_cells(("pack33", "small300", "cand65"), ("small300", "cand65"), shared=True,
                        raw=("pack33", "small300"))
    res, _ = run_light(world, cells)
    for i, c in enumerate(cells):  # binary dependents exist and stay with their owners; the unary ones are gathered
        assert sum(res[r][i]["report"]["binary_own"] for r in range(world)) > 0, c
        assert res[0][i]["report"]["unary_gathered"] > 0, c


def test_shared_objects_association_rules():
    """small300 with shared objects and --use-ars (projection spo, the oracle of tests/test_gpu_ars.py): o=O_k <=> p=P_k
    are rules; one more all-reduce; the rules are equal on every rank and equal to the oracle's."""
    from tests.parity import ars_expected

    sh = L.shape("small300", shared_objects=True)
    modes = [(1, True), (0, False)]
    cells = [cell(light("small300", shared=True), s, c, NO_HEAVY, "spo", True) for s, c in modes]
    res = run_cells(2, cells)
    for i, (strategy, clean) in enumerate(modes):
        rules, cinds = ars_expected(sh, strategy, clean)
        assert len(rules) >= 2 * len(sh.sets)
        parts = [res[r][i] for r in range(2)]
        assert all(p["rules"] == rules for p in parts), (strategy, clean)
        union = set().union(*(p["decoded"] for p in parts))
        assert sum(len(p["decoded"]) for p in parts) == len(union), (strategy, clean)
        assert union == cinds, (strategy, clean)


def heavy_env(sh):
    return {} if sh.heavy_min == H.DEFAULT_HEAVY_MIN else {"RDFIND_HEAVY_MIN": str(sh.heavy_min)}


def check_heavy(world, parts, sh, clean, use_ars, what):
    rep = [p["report"] for p in parts]
    per = S.heavy_per_rank(sh, world)
    total = len(sh.heavy())
    assert [r["heavy_columns"] for r in rep] == per and sum(per) == total, (what, [r["heavy_columns"] for r in rep], per)
    assert [r["heavy_base"] for r in rep] == np.concatenate([[0], np.cumsum(per)[:-1]]).tolist(), what
    assert all(p["groups"]["n_heavy_groups"] == total for p in parts), what  # the gathered histogram's count
    assert all(p["groups"]["heavy_threshold"] == sh.threshold() for p in parts), what
    m = S.class_model(sh, clean)
    want_cls = 0 if use_ars else m["n_classes"]
    assert [p["cinds"]["n_classes"] for p in parts] == [want_cls] * world == [r["n_classes"] for r in rep], what
    assert rsum(parts, "n_class_members") == (0 if use_ars else m["n_class_members"]), what
    assert rsum(parts, "n_class_members") == sum(p["cinds"]["n_class_members"] for p in parts), what
    if not use_ars and not isinstance(sh, H.SShape):
        assert [r["n_class_members"] for r in rep] == S.member_owners(sh, world), what


def run_heavy(world, cells):
    res = run_cells(world, cells)
    contributed = set()
    for i, (key, strategy, clean, proj, use_ars, env) in enumerate(cells):
        sh = get_shape(key)
        what = (sh.name, world, strategy, clean, "ars" if use_ars else "")
        parts = [res[r][i] for r in range(world)]
        check_rows(world, parts, sh, strategy, clean, proj, what)
        check_heavy(world, parts, sh, clean, use_ars, what)
        if use_ars:
            assert all(p["rules"] == [] for p in parts), what  # fresh objects: no rule
        n = sum(1 for p in parts if p["report"]["n_list_entries"] > 0)
        if n >= 2:
            contributed.add(key[1])
        if key[1] in ("cols64x9", "emit16k") and not use_ars:
            assert sum(1 for p in parts if p["report"]["n_class_members"] > 0) >= 2, what
    return res, contributed


HEAVY_SMALL = ("cols6", "cols64", "cols64x9", "lists_small", "emit300", "r3s") + tuple(H.THRESHOLDS)


@pytest.mark.parametrize("world", [2, 3])
def test_heavy_and_class_small(world):
    """Columns numbered from a per-rank bit base (collective 2) and summed (collective 3), the threshold from the
    gathered histogram, the class holder elected by every member alike, the class lists from one all-gather."""
    cells = []
    for name in HEAVY_SMALL:
        sh = H.shape(name)
        cells += [cell(heavy(name), s, c, heavy_env(sh)) for s, c in MODES]
    sh = H.shape("cols64")
    cells += [cell(heavy("cols64"), s, c, heavy_env(sh), "s", True) for s, c in MODES]
    _, contributed = run_heavy(world, cells)
    assert contributed, "no cell in which two ranks contributed class list entries"


@pytest.mark.parametrize("world", [2, 3])
def test_heavy_and_class_large(world):
    """emit16k (a class list of two CLS_LS segments gathered from the ranks; (1, raw) against its set algebra) and r3
    (R3 inside the classes, binary heavy-only dependents; without (1, raw), whose only oracle takes minutes here)."""
    cells = [cell(heavy("emit16k"), s, c, {}) for s, c in MODES]
    cells += [cell(heavy("r3"), s, c, heavy_env(H.shape("r3"))) for s, c in MODES3]
    run_heavy(world, cells)


def test_join_ranges():
    """A rank's join shard built in join-value ranges (RDFIND_GROUP_RANGE=300 records): seg2 and r3s at world 2."""
    rng = {"RDFIND_GROUP_RANGE": "300"}
    cells = [cell(light("seg2"), s, c, dict(NO_HEAVY, **rng)) for s, c in ((1, True), (0, False))]
    n_light = len(cells)
    cells += [cell(heavy("r3s"), s, c, dict(heavy_env(H.shape("r3s")), **rng)) for s, c in MODES]
    res = run_cells(2, cells)
    for i, (key, strategy, clean, proj, use_ars, env) in enumerate(cells):
        sh = get_shape(key)
        what = (sh.name, "ranges", strategy, clean)
        parts = [res[r][i] for r in range(2)]
        check_rows(2, parts, sh, strategy, clean, proj, what)
        assert any(p["groups"]["n_join_ranges"] > 1 for p in parts), what
        if i < n_light:
            check_exchange(2, parts, sh, env, what)
        else:
            check_heavy(2, parts, sh, clean, False, what)
