"""The heavy columns and the mask classes on inputs that sit on their edges, row-exact, with proof that the path ran.

tests/heavy_shapes.py builds the inputs and carries their models; tests/test_heavy_shapes_cpu.py pins the models
against both oracles and asserts every edge from them.  Here every shape runs in the four modes (strategy 0 / 1 x raw /
clean) under projection ``s``; family A also runs with association rules on, where the unary heavy-only dependents take
k_heavy_eval / k_heavy_mark / k_heavy_write instead of the classes.  Each run

* first takes the compact hand-over (copy_result_compact): the checker's expansion of it must give the device's count
  and checksum and the expected ones -- the class part is still compact then (k_class_checksum);
* then the rows themselves, sorted packed (dep, ref) keys and supports against the oracle's (assert_shape_rows): this is
  what runs k_class_emit;
* afterwards count and checksum, now of the expanded rows, must be unchanged;
* and asserts from the shape's model what the run reports: the columns and the threshold, the classes, their members
  and refs, no heavy work items (there is no binary heavy-only dependent), and rdf_test_paths' class fields.

The expected rows are the C oracle's; in mode (1, raw) the Python restatement's, and for emit16k / emit32k, too large for
that, the model's set algebra (equal to both oracles on the same generator at K = 301, on the CPU).

The shape r3 (families C and D: shared objects, hence binary captures, R3 inside the classes and binary heavy-only
dependents) has cells of its own at the end of the file: the class path and the pivot scan, projections s and spo, a
paged run with a one-byte budget, RDFIND_HCLASS=0 and the heavy-bits form.  Its reduced form r3s runs what only the
Python restatement can check: mode (1, raw) and the four modes with association rules on.

Rows are decoded by parity.device_rows from the raw id-records, every id checked before it is used.
"""
import json

import numpy as np
import pytest

from oracle import c_oracle as C
from rdfind_amd import _lib
from tests import heavy_shapes as H
from tests.parity import assert_shape_rows, device_rows, packed, shape_rows

pytestmark = pytest.mark.gpu

MODES = [(1, True), (1, False), (0, True), (0, False)]
SHAPES = [n for n in H.BUILDERS]
_CTX: dict = {}  # RDFIND_HEAVY_MIN -> Context (the switch is read at creation and held by value)


def context(monkeypatch, heavy_min):
    if heavy_min not in _CTX:
        if heavy_min == H.DEFAULT_HEAVY_MIN:
            monkeypatch.delenv("RDFIND_HEAVY_MIN", raising=False)
        else:
            monkeypatch.setenv("RDFIND_HEAVY_MIN", str(heavy_min))
        _CTX[heavy_min] = _lib.Context(0)
    return _CTX[heavy_min]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    while _CTX:
        _CTX.popitem()[1].close()


def expected(sh, strategy, clean):
    """(keys, supports, count, checksum) of the oracle's rows."""
    ek, es = shape_rows(sh, strategy, clean, "s")
    return ek, es, int(ek.shape[0]), C.checksum_rows(H.rows_struct(ek, es))


def assert_host_decode(g, sh, strategy, clean, proj, what):
    """The library's own host decode (rdf_copy_cinds) gives the same rows: once per shape, after device_rows has checked
    every id of this result."""
    ek, es = shape_rows(sh, strategy, clean, proj)
    gk, gs = packed(g.copy_cinds())
    np.testing.assert_array_equal(gk, ek, err_msg=str(what))
    np.testing.assert_array_equal(gs, es, err_msg=str(what))


def run_cell(g, sh, strategy, clean, use_ars=False):
    """One run and its three checks; returns (group stats, cind stats, path report)."""
    what = (sh.name, strategy, clean, "ars" if use_ars else "")
    g.run(sh.min_support, "s", clean, strategy, use_ars=use_ars)
    groups, cinds = g.last_stats()
    t = g.test_paths()
    print("paths", json.dumps({"cell": what, **{k: v for k, v in t.items() if k.startswith(("n_class", "n_emit", "max_", "n_multi_seg", "hclassed"))},
                               **{k: cinds[k] for k in ("n_classes", "n_class_members", "n_class_cinds", "n_heavy_chunks")},
                               **{k: groups[k] for k in ("n_heavy_groups", "heavy_threshold")}}))
    _, _, n_exp, h_exp = expected(sh, strategy, clean)
    parts = g.copy_result_compact()  # before any row accessor: the class part is handed over unexpanded
    n, h, _ = C.checksum_compact(parts, sh.num_terms)
    assert (n, h) == (g.cind_count(), g.checksum()) == (n_exp, h_exp), what
    assert_shape_rows(g, sh, strategy, clean, "s", what)  # expands the class part
    assert (g.cind_count(), g.checksum()) == (n_exp, h_exp), what
    if (strategy, clean, use_ars) == (1, True, False):
        assert_host_decode(g, sh, strategy, clean, "s", what)
    assert groups["n_heavy_groups"] == len(sh.heavy()) == sh.want["n_heavy"], what
    assert groups["heavy_threshold"] == sh.threshold(), what
    return groups, cinds, t


@pytest.mark.parametrize("name", SHAPES)
def test_shape_four_modes(monkeypatch, name):
    sh = H.shape(name)
    st = sh.class_stats()
    g = context(monkeypatch, sh.heavy_min)
    g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    for strategy, clean in MODES:
        what = (name, strategy, clean)
        _, cinds, t = run_cell(g, sh, strategy, clean)
        for k in ("n_classes", "n_class_members", "n_class_cinds"):
            assert cinds[k] == st[k], (what, k)
        assert cinds["n_heavy_chunks"] == 0, what  # no binary heavy-only dependent in these families
        for k in ("n_class_chunks", "n_emit_tiles", "max_class_list", "n_multi_seg_lists"):
            assert t[k] == st[k], (what, k)
        assert t["hclassed"] == (strategy == 1), what
    if name == "emit16k":
        assert t["max_class_list"] > 16384 and t["n_multi_seg_lists"] >= 1
    if name == "emit32k":
        assert t["max_class_list"] > 2 * 16384 and t["n_emit_tiles"] == 6


@pytest.mark.parametrize("name", ["cols6", "lists_small"])
def test_hclass_off_is_reported(monkeypatch, name):
    """RDFIND_HCLASS=0 (binary heavy-only dependents keep the pivot scan): the report says so in every mode, and the
    unary classes are what they were."""
    sh = H.shape(name)
    st = sh.class_stats()
    monkeypatch.setenv("RDFIND_HCLASS", "0")
    monkeypatch.setenv("RDFIND_HEAVY_MIN", str(sh.heavy_min))
    with _lib.Context(0) as g:
        g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
        for strategy, clean in MODES:
            _, cinds, t = run_cell(g, sh, strategy, clean)
            assert not t["hclassed"], (name, strategy, clean)
            assert (cinds["n_classes"], t["n_class_chunks"], t["n_emit_tiles"]) == \
                (st["n_classes"], st["n_class_chunks"], st["n_emit_tiles"]), (name, strategy, clean)


@pytest.mark.parametrize("name", H.FAMILY_A)
def test_family_a_with_association_rules(monkeypatch, name):
    """--use-ars: a class list is not per-dependent, so every heavy-only dependent takes the pivot scan (k_heavy_*).
    The shapes have fresh objects, hence no frequent binary condition and no rule: the rows are the plain ones."""
    sh = H.shape(name)
    g = context(monkeypatch, sh.heavy_min)
    g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    scan_chunks = sum(len(c["members"]) * -(-len(c["group"]) // H.WAVE) for c in sh.classes())
    for strategy, clean in MODES:
        what = (name, strategy, clean, "ars")
        _, cinds, t = run_cell(g, sh, strategy, clean, use_ars=True)
        assert g.copy_association_rules().shape[0] == 0, what
        assert (cinds["n_classes"], cinds["n_class_members"], cinds["n_class_cinds"]) == (0, 0, 0), what
        assert cinds["n_heavy_chunks"] == scan_chunks and (scan_chunks > 0) == bool(sh.heavy_only()), what
        assert not t["hclassed"] and (t["n_class_chunks"], t["n_emit_tiles"], t["max_class_list"]) == (0, 0, 0), what


# ---------------------------------------------------------------------------------------------------------------------
# families C and D: the shape with shared objects (binary captures), tests/heavy_shapes.py r3_shape.  Expected rows: the
# C oracle's.  Mode (1, raw) and the runs with association rules have only the Python restatement as their oracle, which
# takes minutes on r3: they run on r3s, the same generator reduced (q in {1, 32, 33}, one D pair, 706 triples).

R3_MODES = [(1, True), (0, True), (0, False)]


def r3_expected(sh, strategy, clean, proj):
    ek, es = shape_rows(sh, strategy, clean, proj)
    return ek, es, int(ek.shape[0]), C.checksum_rows(H.rows_struct(ek, es))


def r3_bin_chunks(sh, clean):
    """Work items of the classed binary dependents: chunks of 64 of their class's list."""
    M = sh.model()
    lens = {}
    for c in M["caps"][M["cu"]:]:
        if c["subj"] not in lens:
            lens[c["subj"]] = len(sh.class_list(c["subj"], clean))
    return sum(-(-lens[c["subj"]] // H.WAVE) for c in M["caps"][M["cu"]:])


def r3_cell(g, sh, strategy, clean, proj, what):
    """Compact hand-over, rows, count and checksum again; returns (groups, cinds, paths)."""
    g.run(sh.min_support, proj, clean, strategy)
    groups, cinds = g.last_stats()
    t = g.test_paths()
    print("paths", json.dumps({"cell": what, **{k: int(v) for k, v in t.items() if k.startswith(("n_class", "n_emit", "max_", "n_multi_seg", "hclassed"))},
                               **{k: cinds[k] for k in ("n_classes", "n_class_members", "n_class_cinds", "n_heavy_chunks")},
                               **{k: groups[k] for k in ("n_heavy_groups", "heavy_threshold")}}))
    _, _, n_exp, h_exp = r3_expected(sh, strategy, clean, proj)
    parts = g.copy_result_compact()
    n, h, _ = C.checksum_compact(parts, sh.num_terms)
    assert (n, h) == (g.cind_count(), g.checksum()) == (n_exp, h_exp), what
    assert_shape_rows(g, sh, strategy, clean, proj, what)
    assert (g.cind_count(), g.checksum()) == (n_exp, h_exp), what
    if (strategy, clean) == (1, True):
        assert_host_decode(g, sh, strategy, clean, proj, what)
    return groups, cinds, t


def r3_check_paths(sh, groups, cinds, t, clean, classed, what):
    """classed: the binary dependents read the class lists (strategy 1 with RDFIND_HCLASS on); else the pivot scan."""
    st = sh.class_stats(clean, classed)
    assert groups["n_heavy_groups"] == sh.n_subjects == len(sh.heavy()) and groups["heavy_threshold"] == sh.threshold(), what
    assert t["hclassed"] == classed, what
    for k in ("n_classes", "n_class_members", "n_class_cinds"):
        assert cinds[k] == st[k], (what, k)
    assert t["n_class_chunks"] == st["n_class_chunks"], what
    assert cinds["n_heavy_chunks"] == (r3_bin_chunks(sh, clean) if classed else st["scan_chunks"]) > 0, what


@pytest.mark.parametrize("name,proj", [("r3", "s"), ("r3", "spo"), ("r3s", "s"), ("r3s", "spo")])
def test_r3_modes(monkeypatch, name, proj):
    """R3 inside the classes (parent scan and marks) and the binary heavy-only dependents: the class path under strategy
    1, the pivot scan (k_heavy_eval / k_heavy_mark / k_heavy_write) under strategy 0.  The reduced shape r3s runs all
    four modes: in (1, raw) the raw class lists, which hold binaries and their components, meet the Python restatement."""
    sh = H.shape(name)
    g = context(monkeypatch, sh.heavy_min)
    g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    for strategy, clean in (MODES if name == "r3s" else R3_MODES):
        what = (name, proj, strategy, clean)
        groups, cinds, t = r3_cell(g, sh, strategy, clean, proj, what)
        if proj == "s":  # the model is that of projection s
            r3_check_paths(sh, groups, cinds, t, clean, strategy == 1, what)
        else:
            assert cinds["n_heavy_chunks"] > 0 and t["hclassed"] == (strategy == 1), what


@pytest.mark.parametrize("strategy,clean", MODES)
def test_r3s_with_association_rules(monkeypatch, strategy, clean):
    """Family C with --use-ars (projection spo, the Python oracle of tests/test_gpu_ars.py): every object of the shape
    occurs under one predicate, so o=O => p=P are rules; the heavy-only dependents, those with parents included, take
    k_heavy_eval / k_heavy_mark / k_heavy_write instead of the classes."""
    from tests.test_gpu_ars import expected as ars_expected, gpu_run
    sh = H.shape("r3s")
    g = context(monkeypatch, sh.heavy_min)
    arr = np.stack([sh.s, sh.p, sh.o], axis=1)
    got, rules = gpu_run(g, arr, sh.num_terms, sh.min_support, strategy, clean)
    _, cinds = g.last_stats()
    t = g.test_paths()
    assert got == ars_expected([tuple(x) for x in arr.tolist()], sh.min_support, strategy, clean), (strategy, clean)
    assert rules.shape[0] > 0 and cinds["n_classes"] == 0 and cinds["n_heavy_chunks"] > 0 and not t["hclassed"]


def test_r3_hclass_off(monkeypatch):
    """RDFIND_HCLASS=0: strategy 1 keeps the pivot scan for the binary heavy-only dependents."""
    sh = H.shape("r3")
    monkeypatch.setenv("RDFIND_HCLASS", "0")
    monkeypatch.setenv("RDFIND_HEAVY_MIN", str(sh.heavy_min))
    with _lib.Context(0) as g:
        g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
        for clean in (True,):
            what = ("r3", "hclass0", 1, clean)
            groups, cinds, t = r3_cell(g, sh, 1, clean, "s", what)
            r3_check_paths(sh, groups, cinds, t, clean, False, what)


@pytest.mark.parametrize("strategy", [1, 0])
def test_r3_paged_one_byte(monkeypatch, strategy):
    """A one-byte page budget: every binary dependent is a page of its own, so the work items of all but the first start
    at w0 != 0 (k_class_bin_eval; under strategy 0 k_heavy_eval / k_heavy_mark, whose bit base is (choff - w0) * 64).
    The pages' rows, concatenated, are the oracle's."""
    sh = H.shape("r3")
    g = context(monkeypatch, sh.heavy_min)
    g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    g.frequent_conditions(sh.min_support)
    g.build_capture_groups("s")
    ek, es, n_exp, h_exp = r3_expected(sh, strategy, True, "s")
    keys, sups, pages, n, h = [], [], 0, 0, 0
    for _ in g.pages(True, strategy, 1):
        parts = g.copy_result_compact()
        assert C.checksum_compact(parts, sh.num_terms)[:2] == (g.cind_count(), g.checksum()), (strategy, pages)
        n += g.cind_count()
        h = (h + g.checksum()) % (1 << 64)
        k, s_ = device_rows(g)
        keys.append(k)
        sups.append(s_)
        pages += 1
    assert pages > 129 and (n, h) == (n_exp, h_exp), (strategy, pages, n, n_exp)
    gk, gs_ = np.concatenate(keys), np.concatenate(sups)
    order = np.argsort(gk, kind="stable")
    np.testing.assert_array_equal(gk[order], ek)
    np.testing.assert_array_equal(gs_[order], es)


@pytest.mark.parametrize("name", ["r3", "r3s"])
def test_r3_heavy_bits_form(monkeypatch, name):
    """set_result_form(True): the classed binary dependents leave as survivor words over the class lists (k_heavy_pos);
    the checker's expansion and the rows are the oracle's.  r3 runs clean, r3s clean and raw (the Python restatement)."""
    sh = H.shape(name)
    monkeypatch.setenv("RDFIND_HEAVY_MIN", str(sh.heavy_min))
    with _lib.Context(0) as g:
        g.set_result_form(True)
        g.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
        for clean in ((True, False) if name == "r3s" else (True,)):
            what = (name, "heavy_bits", clean)
            g.run(sh.min_support, "s", clean, 1)
            _, _, n_exp, h_exp = r3_expected(sh, 1, clean, "s")
            parts = g.copy_result_compact()
            assert parts["n_heavy_chunks"] == r3_bin_chunks(sh, clean) > 0, what
            assert C.checksum_compact(parts, sh.num_terms)[:2] == (g.cind_count(), g.checksum()) == (n_exp, h_exp), what
            assert_shape_rows(g, sh, 1, clean, "s", what)
            assert (g.cind_count(), g.checksum()) == (n_exp, h_exp), what
