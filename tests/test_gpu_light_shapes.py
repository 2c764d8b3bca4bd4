"""The light pass on near-miss inputs that reach every one of its branches, with proof that they ran.

tests/light_shapes.py builds inputs whose dependents have a chosen number of groups and candidates and whose candidates
miss exactly one group at a chosen position of the dependent's group list (lane, slot and segment edges); a wrong
membership answer at that position changes the result.  tests/test_light_shapes_cpu.py pins the oracle's rows of these
inputs against plain set inclusion.  Here every shape runs under every switch set of the light pass, in the modes
(1, clean), (0, clean), (0, raw), under projections ``s`` and ``spo``, row-exact against the C oracle, and
rdf_test_paths must report what the shape and the switch set demand (conditions, not measurements).

Mode (1, raw) has only the Python restatement as its oracle (slow on large inputs): it runs on the packed-edge shapes
and the smallest one-segment shape only.

Heavy settings: a shape's plain form runs under RDFIND_HEAVY_MIN=1073741824 (no bit columns: every miss is found by a
light search), its ballast form under the default setting (the 64 columns go to ballast subjects, the miss positions
stay light); pack80h / pack81h, the edge of light_plan's second rule, under RDFIND_HEAVY_MIN=2.

The matrix is sparse by one rule: a switch set that only k_light reads (``KLIGHT_ONLY``) is left out on the two shapes
that have no k_light item under projection ``s`` (class "packed": pack32, pack80h); everything else is run.

The instrumented variant of the library (librdfind_hip_stats.so, per-item records of k_light) proves the branches
inside k_light: one child process per switch family (RDFIND_HIP_LIB is read at import), one light pass only (a second
pass would overwrite the dump).
"""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from rdfind_amd import _lib
from tests import light_shapes as L
from tests.parity import assert_shape_rows
from tests.test_gpu import DEFAULT_FORMS, compact_matches, expected_set, forms, gpu_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(1, True), (0, True), (0, False)]
RAW_S2L_SHAPES = ("pack32", "pack33", "pack80h", "pack81h", "small300")  # mode (1, False): the Python restatement
DENSE_ALL = {"RDFIND_DENSE": "1000000", "RDFIND_DENSE_MIN": "2"}  # every light group of >= 2 members gets a bitmap

# name -> environment.  RDFIND_DENSE is a divisor: "dense_c" (RDFIND_DENSE=1) asks for groups of C / 1 members, which no
# group of these shapes reaches (parity only); the sets that must produce bitmap rows use the divisor of
# test_dense_bitmap_paths_parity, under which every light group of >= RDFIND_DENSE_MIN members gets one.
SWITCH_SETS = {
    "defaults": {},
    "stage0": {"RDFIND_STAGE": "0"},
    "stage1": {"RDFIND_STAGE": "1"},
    "hiocc": {"RDFIND_STAGE": "0", "RDFIND_LIGHT_HIOCC": "1"},
    "nofilters": {"RDFIND_SIG": "0", "RDFIND_PIV2": "0", "RDFIND_PIVX": "0"},
    "filters_packed": {"RDFIND_SIG": "1", "RDFIND_PIV2": "1"},
    "pivx4": {"RDFIND_STAGE": "0", "RDFIND_PIVX_N": "4", "RDFIND_PIVX_PACKED": "1"},
    "sweep0": {"RDFIND_SWEEP_F": "0"},
    "sweep_all": {"RDFIND_SWEEP_F": "1000000000"},
    "light2": {"RDFIND_LIGHT2": "1"},
    "dense_c": {"RDFIND_DENSE": "1", "RDFIND_DENSE_MIN": "2"},
    "dense": dict(DENSE_ALL),
    "dense_stage0": dict(DENSE_ALL, RDFIND_STAGE="0"),
    "order1": {"RDFIND_LIGHT_ORDER": "1"},
    "order0": {"RDFIND_LIGHT_ORDER": "0"},
    "side0": {"RDFIND_LIGHT_SIDE": "0"},
    "dedup0": {"RDFIND_LIGHT_DEDUP": "0"},
    "dedup_all": {"RDFIND_LIGHT_DEDUP": "1", "RDFIND_DUP_MIN": "1"},
    "twopass_k3": {"RDFIND_EMIT_ONEPASS": "0"},
}
# On the one-segment shapes (~300 groups in a 512-bit signature) the signature and the pivots kill almost every near-miss
# before a window sees it; the window paths also run with the prefilters off, so that the near-misses die where the
# switch under test decides (the multi-segment shapes saturate the signature and reach the windows either way).
NOFILTERS = SWITCH_SETS["nofilters"]
for _name in ("stage0", "stage1", "hiocc", "sweep0", "sweep_all", "light2", "dense", "dense_stage0"):
    SWITCH_SETS["nf_" + _name] = dict(SWITCH_SETS[_name], **NOFILTERS)
KLIGHT_ONLY = ("stage0", "stage1", "hiocc", "sweep0", "sweep_all", "light2", "dense_stage0", "order1", "order0",
               "nf_stage0", "nf_stage1", "nf_hiocc", "nf_sweep0", "nf_sweep_all", "nf_light2", "nf_dense_stage0")
MULTI_CHUNK = ("cand65", "cand129", "seg2", "seg3")  # D's pivot group has more than 64 members


def cells():
    """(switch set, shape) pairs of the matrix and the ones the rule leaves out."""
    run, skipped = [], []
    for sw in SWITCH_SETS:
        for name in L.SPECS:
            (skipped if sw in KLIGHT_ONLY and L.shape_class(name) == "packed" else run).append((sw, name))
    return run, skipped


def heavy_forms(name):
    """(ballast form?, RDFIND_HEAVY_MIN or None) under which the shape runs."""
    if name.startswith("pack8"):
        return [(False, "2")]  # (these two always carry their ballast)
    return [(False, L.NO_HEAVY)] + ([(True, None)] if name in L.BALLAST_FORMS else [])


_CTX = {}  # (switch set, heavy_min) -> Context; the contexts of one switch set at a time


def context(monkeypatch, sw, env, heavy_min):
    """A context created under the switch set's environment (the switches are read at creation and held by value);
    kept while the tests of that switch set run, so a test pays for its runs, not for the context's buffers."""
    for key in [k for k in _CTX if k[0] != sw]:
        _CTX.pop(key).close()
    if (sw, heavy_min) not in _CTX:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        if heavy_min is not None:
            monkeypatch.setenv("RDFIND_HEAVY_MIN", heavy_min)
        else:
            monkeypatch.delenv("RDFIND_HEAVY_MIN", raising=False)
        _CTX[(sw, heavy_min)] = _lib.Context(0)
    return _CTX[(sw, heavy_min)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    while _CTX:
        _CTX.popitem()[1].close()


def check_paths(t, sw, name, proj, strategy, what):
    """What rdf_test_paths must report for this shape under this switch set."""
    env = SWITCH_SETS[sw]
    cls = L.shape_class(name)
    WI, WP, WM = t["n_light_items"], t["n_packed_octets"], t["n_mseg_chunks"]
    assert t["k3_form"] == ("twopass" if env.get("RDFIND_EMIT_ONEPASS") == "0" else "onepass"), what
    assert t["k1_form"] == DEFAULT_FORMS[0], what
    sig_on, piv2_on = env.get("RDFIND_SIG", "2") != "0", env.get("RDFIND_PIV2", "1") != "0"
    assert (t["sig_on"], t["piv2_on"]) == (sig_on, piv2_on), what
    if "RDFIND_STAGE" in env:
        assert t["light_stage"] == (env["RDFIND_STAGE"] == "1"), what
    if env.get("RDFIND_LIGHT_HIOCC") == "1":
        assert t["light_hiocc"] and not t["light_stage"], what
    assert not (t["light_hiocc"] and t["light_stage"]), what
    two = env.get("RDFIND_LIGHT2") == "1"
    assert t["light_two_pass"] == (two and WI > 0), what
    if not two:
        assert t["light_side"] == (env.get("RDFIND_LIGHT_SIDE") != "0" and WI > 0 and WP > 0), what
        assert t["n_light_survivors"] == 0, what
    order = env.get("RDFIND_LIGHT_ORDER")
    assert t["light_ordered"] == (WI > 0 and (t["light_stage"] if order is None else order != "0")), what
    pivx_on = piv2_on and env.get("RDFIND_PIVX", "1") != "0"
    if WI:
        assert (t["light_npx"] in (1, 4)) if pivx_on else t["light_npx"] == 0, what
    if WP and not pivx_on:
        assert t["packed_npx"] == 0, what
    if env.get("RDFIND_LIGHT_DEDUP") == "0" or strategy == 0:
        assert t["n_dedup_members"] == 0, what
    elif sw == "dedup_all":  # the identical near-misses are a class of two
        assert t["n_dedup_members"] > 0, what
    if env.get("RDFIND_DENSE") == "1000000":
        assert t["dense_on"] and t["n_dense"] > 0, what
    if proj != "s":
        return
    # projection s: the captures are the shape's sets alone, so the work is what tests/test_light_shapes_cpu.py derives
    if WI and pivx_on:  # small groups: the pivot pass keeps one extra pivot, whatever RDFIND_PIVX_N asks for
        assert t["light_npx"] == 1 and not (t["light_hiocc"] and "RDFIND_LIGHT_HIOCC" not in env), what
    if WP and pivx_on:
        assert t["packed_npx"] == (1 if env.get("RDFIND_PIVX_PACKED") == "1" else 0), what
    if cls == "packed":
        assert WI == 0 < WP and WM == 0, what
    elif cls == "packed_over":
        assert WI > 0 and WM == 0, what
    elif cls == "one_seg":
        assert WI > 0 and WM == 0, what
    else:
        assert WM > 0 and t["n_multi_items"] > 0 and WI > WM, what
    if two and name in MULTI_CHUNK:
        assert t["n_light_survivors"] > 0, what


RUN, SKIPPED = cells()


@pytest.mark.parametrize("sw,name", RUN, ids=[f"{a}-{b}" for a, b in RUN])
def test_shape_matrix(monkeypatch, sw, name):
    """Row-exact parity and the path report for one (switch set, shape) cell: both heavy forms, the three modes (and
    (1, raw) on the small shapes), projections s and spo."""
    modes = MODES + ([(1, False)] if name in RAW_S2L_SHAPES else [])
    for ballast, heavy_min in heavy_forms(name):
        sh = L.shape(name, ballast)
        g = context(monkeypatch, sw, SWITCH_SETS[sw], heavy_min)
        g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
        for proj in ("s", "spo"):
            for strategy, clean in modes:
                what = (sw, sh.name, proj, strategy, clean)
                g.run(sh.min_support, proj, clean, strategy)
                t = g.test_paths()
                print("paths", json.dumps({"cell": what, **{k: (int(v) if not isinstance(v, str) else v) for k, v in t.items()
                                                            if v is not None}}))
                assert_shape_rows(g, sh, strategy, clean, proj, what)
                assert compact_matches(g, sh.num_terms), what
                check_paths(t, sw, name, proj, strategy, what)


def test_matrix_is_sparse_by_rule():
    """The cells left out are exactly the k_light-only switch sets on the shapes without a k_light item."""
    assert sorted(set(b for _, b in SKIPPED)) == ["pack32", "pack80h"]
    assert sorted(set(a for a, _ in SKIPPED)) == sorted(KLIGHT_ONLY)
    assert len(RUN) + len(SKIPPED) == len(SWITCH_SETS) * len(L.SPECS)


def test_k3_count_and_write_form_random(monkeypatch):
    """K3 as count pass + write pass (RDFIND_EMIT_ONEPASS=0, g_emit_range with cache == 0) on the usual small random
    inputs: the form is reported, the result is the oracle's and the group build counts the same records as the
    one-pass form of a default context."""
    monkeypatch.setenv("RDFIND_EMIT_ONEPASS", "0")
    g = _lib.Context(0)
    monkeypatch.delenv("RDFIND_EMIT_ONEPASS")
    g0 = _lib.Context(0)
    try:
        rng = random.Random(4100)
        for _ in range(30):
            n = rng.randrange(1, 600)
            nv = rng.randrange(2, 60)
            ms = rng.randrange(1, 4)
            arr = np.array([(rng.randrange(nv), rng.randrange(nv // 3 + 1), rng.randrange(nv)) for _ in range(n)],
                           dtype=np.uint32)
            for strategy, clean in MODES:
                assert gpu_set(g, arr, nv, ms, strategy, clean) == expected_set(arr, nv, ms, strategy, clean), (n, nv, ms)
                assert forms(g)[2] == "twopass"
                gpu_set(g0, arr, nv, ms, strategy, clean)
                assert forms(g0) == DEFAULT_FORMS
                assert g.groups["n_records"] == g0.groups["n_records"], (n, nv, ms)
                assert (g.cind_count(), g.checksum()) == (g0.cind_count(), g0.checksum())
    finally:
        g.close()
        g0.close()


# ---------------------------------------------------------------------------------------------------------------------
# the shared-object form (tests/light_shapes.py): one object per set, so every set has three captures with equal group
# lists, frequent binary conditions exist and the minimality rules of the explicit path see the near-misses

SHARED_FORMS = [("pack32", False), ("pack33", False), ("small300", False), ("cand64", False), ("cand65", False),
                ("cand65", True), ("small300", True)]
ALL_MODES = MODES + [(1, False)]


DUP_MIN = 256  # switches.hpp RDFIND_DUP_MIN: the shortest group list that looks for an equal one by default


def check_shared_paths(t, sh, name, sw, strategy, what):
    """Every dependent has two twins with equal group lists.  With the dedup classes on for every list (the switch set
    dedup_all) members must be found; by default the classes are looked for only where the light pass stages its rows
    and only among lists of at least DUP_MIN groups (d_light_dedup), so the report says 0 wherever that rules them out."""
    if strategy != 1:
        assert t["n_dedup_members"] == 0, what
    elif sw == "dedup_all" or (t["light_stage"] and sh.m >= DUP_MIN):
        assert t["n_dedup_members"] > 0, what
    elif not t["light_stage"] or len(max(sh.sets, key=len)) < DUP_MIN:
        assert t["n_dedup_members"] == 0, what
    if L.shape_class(name) == "packed":
        assert t["n_packed_octets"] > 0, what
    else:
        assert t["n_light_items"] > 0, what


@pytest.mark.parametrize("sw", ["defaults", "dedup_all"])
@pytest.mark.parametrize("name,ballast", SHARED_FORMS, ids=[n + ("+b" if b else "") + "+o" for n, b in SHARED_FORMS])
def test_shared_objects_four_modes(monkeypatch, name, ballast, sw):
    """Row-exact in all four modes under projection s (rows decoded by parity.device_rows, ids checked first): the
    explicit rules (k_rules_explicit -> rule_keep -> member, k_rules_mark) on inputs full of near-misses, in the default
    setting and with the dedup classes on for every group list."""
    sh = L.shape(name, ballast, shared_objects=True)
    g = context(monkeypatch, sw, SWITCH_SETS[sw], None if ballast else L.NO_HEAVY)
    g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    for strategy, clean in ALL_MODES:
        what = (sh.name, sw, "s", strategy, clean)
        g.run(sh.min_support, "s", clean, strategy)
        t = g.test_paths()
        print("paths", json.dumps({"cell": what, "n_dedup_members": int(t["n_dedup_members"]), "light_stage": bool(t["light_stage"]),
                                   "n_light_items": int(t["n_light_items"]), "n_packed_octets": int(t["n_packed_octets"])}))
        assert_shape_rows(g, sh, strategy, clean, "s", what)
        assert compact_matches(g, sh.num_terms), what
        check_shared_paths(t, sh, name, sw, strategy, what)


def test_shared_objects_spo(monkeypatch):
    """small300 with shared objects under projection spo."""
    sh = L.shape("small300", shared_objects=True)
    g = context(monkeypatch, "defaults", {}, L.NO_HEAVY)
    g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    for strategy, clean in MODES:
        what = (sh.name, "spo", strategy, clean)
        g.run(sh.min_support, "spo", clean, strategy)
        t = g.test_paths()
        assert_shape_rows(g, sh, strategy, clean, "spo", what)
        assert compact_matches(g, sh.num_terms), what
        assert t["n_light_items"] > 0, what


def test_shared_objects_association_rules(monkeypatch):
    """small300 with shared objects and association rules on: o=O_k <=> p=P_k are rules (the oracle of
    tests/test_gpu_ars.py, projection spo)."""
    from tests.parity import ars_expected
    from tests.test_gpu_ars import gpu_run
    sh = L.shape("small300", shared_objects=True)
    g = context(monkeypatch, "defaults", {}, L.NO_HEAVY)
    arr = np.stack([sh.s, sh.p, sh.o], axis=1)
    for strategy, clean in ((1, True), (0, False)):
        rules, cinds = ars_expected(sh, strategy, clean)
        got, got_rules = gpu_run(g, arr, sh.num_terms, sh.min_support, strategy, clean)
        assert len(rules) > 0 and sorted(map(tuple, got_rules.tolist())) == rules, (strategy, clean)
        assert got == cinds, (strategy, clean)


def test_shard_report_needs_a_sharded_run():
    """rdf_test_shard_report (the report tests/test_gpu_sharded_shapes.py reads) is a state error without a completed
    sharded run; a one-GPU run does not count."""
    sh = L.shape("pack32")
    with _lib.Context(0) as g:
        with pytest.raises(_lib.RdfError):
            g.test_shard_report()
        g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
        g.run(sh.min_support, "s", True, 1)
        with pytest.raises(_lib.RdfError):
            g.test_shard_report()


# ---------------------------------------------------------------------------------------------------------------------
# the branches inside k_light (the instrumented variant)

STATS_LIB = os.path.join(ROOT, "rdfind_amd", "librdfind_hip_stats.so")
# family -> (environment, shapes).  Plain forms under RDFIND_HEAVY_MIN=NO_HEAVY, projection s, mode (1, clean).  The sweep
# families run with the prefilters off: a sweep needs LIGHT_SWEEP_MIN candidates alive at the window.
STATS_FAMILIES = {
    "sweep_all": (dict(NOFILTERS, RDFIND_SWEEP_F="1000000000"), ("cand64", "seg2", "seg3")),
    "sweep0_stage0": (dict(NOFILTERS, RDFIND_SWEEP_F="0", RDFIND_STAGE="0"), ("cand64", "small300")),
    "stage1": ({"RDFIND_STAGE": "1"}, ("small300",)),
    "dense": (DENSE_ALL, ("cand129",)),
    "nofilters": (NOFILTERS, ("cand64", "cand65")),
}


def run_stats_child(family, tmp_path):
    env_sw, names = STATS_FAMILIES[family]
    env = dict(os.environ, RDFIND_HIP_LIB=STATS_LIB, RDFIND_LIGHT_DUMP=str(tmp_path / "items.bin"),
               RDFIND_HEAVY_MIN=L.NO_HEAVY, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_sw)
    env.pop("RDFIND_LIGHT2", None)
    out = subprocess.run([sys.executable, "-m", "tests.light_stats_child", *names], cwd=ROOT, env=env, check=True,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120).stdout
    return {r["shape"]: r for r in (json.loads(ln[6:]) for ln in out.splitlines() if ln.startswith("STATS "))}


@pytest.mark.parametrize("family", list(STATS_FAMILIES))
def test_k_light_branches_ran(monkeypatch, tmp_path, family):
    """Per-item records of the instrumented k_light on the shapes: the branch the family is about ran (or, switched
    off, did not), and the instrumented build computes what the product build computes."""
    assert os.path.exists(STATS_LIB), "the default make target builds the instrumented variant"
    env_sw, names = STATS_FAMILIES[family]
    rec = run_stats_child(family, tmp_path)
    g = context(monkeypatch, "stats-" + family, env_sw, L.NO_HEAVY)  # the product build under the same switches
    for name in names:
        sh = L.shape(name)
        g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
        g.run(sh.min_support, "s", True, 1)
        r = rec[name]
        print("stats", json.dumps(r))
        assert (r["n_cinds"], r["checksum"]) == (g.cind_count(), g.checksum()), (family, name)
        assert r["items"] == g.test_paths()["n_light_items"] > 0, (family, name)
        if family == "sweep_all":
            assert r["sweep"] > 0, name
            if L.shape_class(name) == "multi_seg":
                assert r["max_nseg"] == -(-sh.m // L.LIGHT_SEG) > 1 and r["ser"] > 0, name
        elif family == "sweep0_stage0":
            assert r["sweep"] == 0 and r["bat"] > 0 and r["rows"] == 0, name
        elif family == "stage1":
            assert r["rows"] > 0, name
        elif family == "dense":
            assert r["dser"] > 0, name
        elif family == "nofilters":  # a near-miss died in a window, not in a prefilter
            assert r["killed_in_window"] > 0, name

