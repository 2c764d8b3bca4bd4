"""Result selection on the device (rdf_select_cinds, the selection view's accessors, rdf_find_terms and the driver's
--select-* flags) against the CPU reference (tests/select_ref.py) fed with the oracle's rows, always by exact equality
of sets, counts and bytes."""
import ctypes
import io
import os
import queue
import random
import time
from collections import Counter

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import c_oracle as C
from rdfind_amd import _lib, ntriples, program
from tests import cind_stats_ref, select_ref as ref
from tests.conftest import GOLDEN
from tests.parity import dataset
from tests.test_gpu import MODES, expected_set
from tests.test_gpu_cind_stats import _free_port, boundary_input, random_input
from tests.test_oracle import read_golden

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ANY = ref.ANY
ERR_ARG, ERR_STATE, ERR_LIMIT = -1, -4, -5


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def selected_set(g):
    """The selection view's rows in the oracle's comparison form; the view holds no row twice."""
    rows = g.selected_decoded()
    got = _lib.decoded_to_set(rows)
    assert len(got) == len(rows) == g.selected_count()
    return got


def reference(exp, q):
    return ref.select(exp, q.get("dep", ()), q.get("ref", ()), q.get("min_support", 0), q.get("max_support", ANY))


def check_query(g, exp, what=None, want=None, **q):
    """One query: count and set equal the reference's on the expected rows (`want`, when the caller already has them);
    returns the set."""
    want = reference(exp, q) if want is None else want
    n = g.select_cinds(**q)
    got = selected_set(g)
    assert n == len(got) and got == want, (what, q, len(got), len(want))
    return got


def raises_status(status, call):
    with pytest.raises(_lib.RdfError) as e:
        call()
    assert e.value.status == status, e.value
    return True


def test_empty_result(ctx):
    two = np.array([[0, 1, 2], [1, 1, 2]], np.uint32)
    ctx.set_triples(two[:, 0], two[:, 1], two[:, 2], 3)
    ctx.run(1000)  # a support above every count
    assert ctx.cind_count() == 0
    assert ctx.select_cinds() == 0 and ctx.selected_count() == 0 and len(ctx.selected_decoded()) == 0
    assert ctx.select_cinds(dep=[ref.exact(10, 1)], ref=[(ref.ALL_CODES, ANY, ANY)], min_support=1) == 0
    empty = np.zeros((0, 3), np.uint32)
    ctx.set_triples(empty[:, 0], empty[:, 1], empty[:, 2], 1)
    ctx.run(1)
    assert ctx.select_cinds() == 0 and len(ctx.selected_decoded()) == 0
    assert ctx.select_cinds(count_only=True) == 0


def test_single_cind(ctx):
    # s[p=0] = {a, b} within s[p=1] = {a, b, c}; every object is distinct, so no other condition reaches support 2
    arr = np.array([[10, 0, 2], [11, 0, 3], [10, 1, 4], [11, 1, 5], [12, 1, 6]], np.uint32)
    exp, _ = C.run_set(arr[:, 0], arr[:, 1], arr[:, 2], 13, 2, 1, True, "s")
    row = (10, 0, None, 10, 1, None, 2)
    assert exp == {row}
    ctx.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], 13)
    ctx.run(2, "s")
    S10, BIN = 1 << 0, (1 << 2) | (1 << 5) | (1 << 8)
    hits = [
        {},
        {"dep": [ref.exact(10, 0)]},                              # s[p=T]
        {"ref": [ref.exact(10, 1)]},
        {"dep": [ref.exact(10, 0)], "ref": [ref.exact(10, 1)]},
        {"dep": [(S10, ANY, ANY)]},                               # s[p=*]
        {"dep": [(ref.ALL_CODES, 0, ANY)]},                       # a bare term, first alternative
        {"ref": [(S10 | 1 << 7, 1, ANY), (1 << 2, 1, ANY), (1 << 8, ANY, 1)]},  # *[p=T]
        {"dep": [(BIN, ANY, 0), (ref.ALL_CODES, 0, ANY)]},        # a bare term, both alternatives
        {"dep": [ref.exact(12, 5), ref.exact(10, 0)]},            # any of several
        {"min_support": 2, "max_support": 2},
        {"min_support": 1},
        {"max_support": 2},
    ]
    misses = [
        {"dep": [ref.exact(10, 1)]},                              # the ref as dependent
        {"ref": [ref.exact(10, 0)]},
        {"dep": [ref.exact(12, 0)]},                              # the value under another code
        {"dep": [(1 << 2, 0, ANY)]},                              # s[p=T,o=*]: binary captures only
        {"dep": [(ref.ALL_CODES, ANY, 0)]},                       # a second value: no unary capture
        {"dep": [(0, ANY, ANY)]},                                 # no code admitted
        {"dep": [ref.exact(10, 0)], "ref": [ref.exact(10, 7)]},
        {"min_support": 3},
        {"max_support": 1},
    ]
    for q in hits:
        assert check_query(ctx, exp, **q) == {row}, q
        assert ctx.select_cinds(count_only=True, **q) == 1
    for q in misses:
        assert check_query(ctx, exp, **q) == set(), q
        assert ctx.select_cinds(count_only=True, **q) == 0


@pytest.mark.parametrize("clean", [False, True])
@pytest.mark.parametrize("r,d", [(63, 257), (64, 256), (65, 255), (255, 65), (256, 64), (257, 63)])
def test_run_edges(ctx, r, d, clean):
    """One run of r refs and d one-ref runs of the same ref, around the wave and block sizes."""
    sh = boundary_input(r, d)
    exp, _ = C.run_set(sh.s, sh.p, sh.o, sh.num_terms, 2, 1, clean, "s")
    assert len(exp) == r + d
    ctx.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    ctx.run(2, "s", clean, 1)
    dep, hub, first = ref.exact(10, 0), ref.exact(10, r + 1), ref.exact(10, 1)
    assert len(check_query(ctx, exp, dep=[dep])) == r
    assert len(check_query(ctx, exp, ref=[hub])) == d
    assert len(check_query(ctx, exp, dep=[dep], ref=[hub])) == 0
    assert len(check_query(ctx, exp, dep=[dep], ref=[first])) == 1
    assert len(check_query(ctx, exp, dep=[ref.exact(10, r + 2)], ref=[hub])) == 1
    assert len(check_query(ctx, exp)) == r + d
    assert len(check_query(ctx, exp, dep=[dep, ref.exact(10, r + 2), ref.exact(10, r + 1 + d)])) == r + 2


def compact_captures(g, parts):
    """compact capture id -> (code, v1, v2 or None), from the capture table of the compact hand-over."""
    L = parts["layout"]
    code, v1, v2 = _lib.decode_captures(parts["capture_ids"][: L["n_captures"]], g.num_terms, g.binary_keys())
    return [(int(c), int(a), None if int(b) == NONE else int(b)) for c, a, b in zip(code, v1, v2)]


def class_view(g, parts):
    """The class part of the compact hand-over as [(member capture, its support, [list captures])]."""
    L = parts["layout"]
    caps = compact_captures(g, parts)
    out = []
    for m in parts["members"][: L["n_members"]].tolist():
        lst, dep = m >> 32, m & NONE
        seg = parts["list_refs"][int(parts["list_off"][lst]):int(parts["list_off"][lst + 1])].tolist()
        out.append((caps[dep], int(parts["supports"][dep]), [caps[x] for x in seg]))
    return out


def class_effects(classes, q):
    """What a query does to the pending class part, from the compact hand-over alone: (rows selected from it, members
    selected on the dep side whose own capture is a selected entry of their list, selected members whose list has no
    selected entry)."""
    dep, rf = q.get("dep", ()), q.get("ref", ())
    lo, hi = q.get("min_support", 0), q.get("max_support", ANY)
    rows = selfs = empties = 0
    for cap, sup, lst in classes:
        if not (ref.matches_any(dep, *cap) and lo <= sup <= hi):
            continue
        kept = [x for x in lst if ref.matches_any(rf, *x)]
        rows += len(kept) - (cap in kept)
        selfs += cap in kept
        empties += not kept
    return rows, selfs, empties


def result_queries(rng, exp, classes):
    """Queries drawn from the result itself."""
    rows = sorted(exp, key=lambda r: tuple(-1 if x is None else x for x in r))
    qs = [("empty", {})]
    if not rows:
        return qs
    a, b = rng.choice(rows), rng.choice(rows)
    sups = sorted({r[6] for r in rows})
    qs += [
        ("dep", {"dep": [ref.exact(*a[0:3])]}),
        ("ref", {"ref": [ref.exact(*b[3:6])]}),
        ("both", {"dep": [ref.exact(*a[0:3])], "ref": [ref.exact(*a[3:6]), ref.exact(*b[3:6])]}),
        ("dep codes", {"dep": [(1 << ref.CODES.index(a[0]), ANY, ANY)], "ref": [(ref.ALL_CODES, b[4], ANY)]}),
        ("support", {"min_support": rng.choice(sups), "max_support": max(sups)}),
    ]
    with_self = [(cap, lst) for cap, _, lst in classes if cap in lst]
    if with_self:  # the self exclusion: a member as the dependent, its own capture among the refs asked for
        cap, lst = rng.choice(with_self)
        qs.append(("self", {"dep": [ref.exact(*cap)], "ref": [ref.exact(*cap), ref.exact(*rng.choice(lst))]}))
        qs.append(("self only", {"dep": [ref.exact(*cap)], "ref": [ref.exact(*cap)]}))
    if classes:  # a member as the dependent, a ref outside its list
        cap, _, lst = rng.choice(classes)
        outside = [r[3:6] for r in rows if r[3:6] not in lst]
        qs.append(("outside", {"dep": [ref.exact(*cap)], "ref": [ref.exact(*rng.choice(outside))] if outside else [(0, ANY, ANY)]}))
    return qs


_CASES = {}


def random_cases(count):
    """The first `count` random inputs of one seeded stream with the oracle's rows per mode, computed once and shared by
    the tests below (and by their parameters: the expected rows do not depend on the device's switches)."""
    if "rng" not in _CASES:
        _CASES["rng"], _CASES["list"] = random.Random(101), []
    while len(_CASES["list"]) < count:
        arr, nv, ms = random_input(_CASES["rng"])
        exp = {(strategy, clean): frozenset(expected_set(arr, nv, ms, strategy, clean)) for strategy, clean in MODES}
        _CASES["list"].append((arr, nv, ms, exp))
    return _CASES["list"][:count]


def sorted_rows(rows):
    return np.sort(rows, order=list(rows.dtype.names))


@pytest.mark.parametrize("heavy_min", [1, 2, 8])
def test_class_path(monkeypatch, heavy_min):
    """Random inputs of the shape of the statistics' class test: the mask classes carry most of the result.  The
    selections come first, take the class part unexpanded and leave it pending (the class emission timer stays zero);
    once a row accessor has expanded it the same queries give the same rows."""
    monkeypatch.setenv("RDFIND_HEAVY_MIN", str(heavy_min))
    g = _lib.Context(0)
    try:
        rng = random.Random(100 + heavy_min)
        n_class = n_from_class = n_self = n_empty = 0
        for arr, nv, ms, expected in random_cases(30):
            for strategy, clean in MODES:
                g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
                cs = g.run(ms, "spo", clean, strategy)
                exp = expected[(strategy, clean)]
                classes = class_view(g, g.copy_result_compact()) if cs["n_class_cinds"] else []
                queries = result_queries(rng, exp, classes)
                first = []
                for what, q in queries:  # before any row accessor
                    n = len(check_query(g, exp, (what, nv, ms, strategy, clean, heavy_min), **q))
                    first.append(sorted_rows(g.selected_decoded()))
                    assert g.select_cinds(count_only=True, **q) == n
                    rows, selfs, empties = class_effects(classes, q)
                    n_from_class += rows > 0
                    n_self += selfs > 0
                    n_empty += empties > 0
                if cs["n_class_cinds"]:
                    n_class += 1
                    assert g.kernel_times()["cemit"] == 0.0  # the class part is still pending
                assert _lib.decoded_to_set(g.decoded_cinds()) == exp, (nv, ms, strategy, clean, heavy_min)
                if cs["n_class_cinds"]:
                    assert g.kernel_times()["cemit"] > 0.0  # (the timer does see the expansion)
                for (what, q), before in zip(queries, first):  # the class rows are ordinary runs now
                    assert g.select_cinds(**q) == len(before), what
                    assert np.array_equal(sorted_rows(g.selected_decoded()), before), (what, nv, ms, strategy, clean)
        assert n_class > 0 and n_from_class > 0 and n_self > 0 and n_empty > 0, (n_class, n_from_class, n_self, n_empty)
    finally:
        g.close()


def test_heavy_bits_form(monkeypatch):
    """RDF_FORM_HEAVY_BITS: the deferred heavy-only refs are written before they are selected from; same sets as the
    expanded form and as the reference."""
    monkeypatch.setenv("RDFIND_HEAVY_MIN", "2")
    g, e = _lib.Context(0), _lib.Context(0)
    try:
        g.set_result_form(True)
        rng = random.Random(900 + 2)
        chunks = 0
        for _ in range(12):
            arr, nv, ms = random_input(rng)
            for c in (g, e):
                c.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
                c.run(ms)
            exp = expected_set(arr, nv, ms, 1, True)
            queries = result_queries(rng, exp, [])
            got = [check_query(g, exp, what, **q) for what, q in queries]  # first: the heavy refs are still bits
            chunks += g.copy_result_compact()["n_heavy_chunks"]
            for (what, q), want in zip(queries, got):
                check_query(e, exp, what, want=want, **q)
        assert chunks > 0
    finally:
        g.close()
        e.close()


@pytest.mark.parametrize("heavy_min", [64, 2])
def test_paged(monkeypatch, heavy_min):
    """A one-byte page budget (every binary dependent its own page): the pages' selections together equal the unpaged
    selection and the reference; the pages partition the dependents, so no row comes twice."""
    monkeypatch.setenv("RDFIND_HEAVY_MIN", str(heavy_min))
    g = _lib.Context(0)
    try:
        rng = random.Random(500 + heavy_min)
        most_pages = 0
        for arr, nv, ms, expected in random_cases(6):
            for strategy, clean in MODES:
                exp = expected[(strategy, clean)]
                queries = result_queries(rng, exp, [])[:4]
                g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
                g.frequent_conditions(ms)
                g.build_capture_groups("spo")
                g.discover_cinds_paged(clean, strategy, 1)
                parts = [[] for _ in queries]
                pages = 0
                while g.next_page() is not None:
                    pages += 1
                    for k, (_, q) in enumerate(queries):
                        n = g.select_cinds(**q)
                        parts[k].append(g.selected_decoded())
                        assert len(parts[k][-1]) == n == g.selected_count()
                most_pages = max(most_pages, pages)
                g.run(ms, "spo", clean, strategy)
                for k, (what, q) in enumerate(queries):
                    rows = np.concatenate(parts[k])
                    paged = _lib.decoded_to_set(rows)
                    assert len(paged) == len(rows) and paged == reference(exp, q), (what, nv, ms, strategy, clean, heavy_min, pages)
                    assert g.select_cinds(**q) == len(rows)
                    assert np.array_equal(sorted_rows(g.selected_decoded()), sorted_rows(rows)), what
        assert most_pages > 2
    finally:
        g.close()


def test_count_only(ctx):
    sh = boundary_input(65, 255)
    ctx.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    ctx.run(2, "s")
    hub = [ref.exact(10, 66)]
    assert ctx.select_cinds(ref=hub) == 255 and ctx.selected_count() == 255
    assert ctx.select_cinds(ref=hub, count_only=True) == 255  # the same number, and the earlier view is dropped
    for call in (ctx.selected_count, ctx.selected_decoded, lambda: ctx.selected_decoded(0, 1), ctx.format_selected):
        assert raises_status(ERR_STATE, call)
    assert ctx.select_cinds(ref=hub) == 255 and len(ctx.selected_decoded()) == 255
    assert ctx.last_select_ms > 0.0


@pytest.mark.parametrize("cfg,scale", [("c5", 0.01), ("c1", 0.05)])
def test_consistent_with_statistics(ctx, cfg, scale):
    """The in-degree of the most referenced captures is the count of the CINDs that reference them."""
    d = dataset(cfg, scale)
    ctx.set_triples(d.s, d.p, d.o, d.num_terms)
    cs = ctx.run(d.min_support)
    ctx.cind_histogram()
    top = ctx.top_refs(5)
    assert len(top) == 5
    code, v1, v2 = _lib.decode_captures(top["capture"], ctx.num_terms, ctx.binary_keys())
    for c, a, b, n in zip(code.tolist(), v1.tolist(), v2.tolist(), top["cinds"].tolist()):
        assert ctx.select_cinds(ref=[ref.exact(c, a, None if b == NONE else b)], count_only=True) == n > 0
    assert ctx.select_cinds(count_only=True) == ctx.cind_count() > 0
    c, a, b = int(code[0]), int(v1[0]), int(v2[0])
    assert ctx.select_cinds(ref=[ref.exact(c, a, None if b == NONE else b)]) == int(top["cinds"][0])
    rows = ctx.selected_decoded()
    assert len(rows) == int(top["cinds"][0])
    assert set(rows["ref_capture_type"].tolist()) == {c} and set(rows["ref_value1"].tolist()) == {a}
    assert cs["n_class_cinds"] == 0 or ctx.kernel_times()["cemit"] == 0.0


def test_formatting(ctx):
    sh = boundary_input(65, 255)
    ctx.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    ctx.run(2, "s")
    terms = [f"<http://example.org/t{i}>" if i % 3 else f'"literal {i}, ] = *"@en' for i in range(sh.num_terms)]
    ctx.set_dictionary(terms)
    n = ctx.select_cinds()
    assert n == 320
    for off in (0, 1, 63, 64, 65, n):
        for cnt in (0, 1, 63, 64, 65, n):
            rows = ctx.selected_decoded(off, cnt)
            assert len(rows) == max(min(cnt, n - off), 0)
            want = "".join(ln + "\n" for ln in program.format_rows(rows, terms.__getitem__)).encode()
            assert ctx.format_selected(off, cnt) == want, (off, cnt)
    whole = ctx.format_selected()
    assert whole.count(b"\n") == n
    # a selection proper, and the cap
    m = ctx.select_cinds(ref=[ref.exact(10, 66)])
    text = ctx.format_selected()
    assert m == 255 == text.count(b"\n") and text == \
        "".join(ln + "\n" for ln in program.format_rows(ctx.selected_decoded(), terms.__getitem__)).encode()
    need, got = ctypes.c_uint64(), ctypes.c_uint64()
    assert ctx.lib.rdf_format_selected_size(ctx.ptr, 0, m, ctypes.byref(need)) == 0 and need.value == len(text)
    buf = np.empty(len(text), np.uint8)
    assert ctx.lib.rdf_format_selected(ctx.ptr, 0, m, buf.ctypes.data, len(text) - 1, ctypes.byref(got)) == ERR_ARG
    assert got.value == len(text)  # *bytes is set
    assert ctx.lib.rdf_format_selected(ctx.ptr, 0, m, buf.ctypes.data, len(text), ctypes.byref(got)) == 0
    assert buf.tobytes() == text


NT_TEXT = (
    '<http://a> <http://p> "x" .\n'
    '<http://ab> <http://p> "x"@en .\n'
    '<http://a> <http://q> "grüß 世界" .\n'
    '_:b0 <http://q> "1"^^<http://www.w3.org/2001/XMLSchema#int> .\n'
    '<http://abc> <http://p> <http://zzz/last> .\n'
)


def test_find_terms(ctx, tmp_path):
    # the host dictionary: duplicates, the empty string, a term that is a prefix of another, multi-byte UTF-8
    terms = ["<a>", "<ab>", "", "<a>", "grüß 世界", "<abc>", "", "pre", "prefix", "<last>"]
    ctx.set_dictionary(terms)
    asked = ["<a>", "<ab>", "<abc>", "<abcd>", "<a", "a>", "", "grüß 世界", "grüß", "<last>", "<last> ", "<b>", "prefix", "pre",
             "pref", "p"]
    assert ctx.find_terms(asked).tolist() == [0, 1, 5, NONE, NONE, NONE, 2, 4, NONE, 9, NONE, NONE, 8, 7, NONE, NONE]
    assert ctx.find_terms([]).tolist() == []
    assert ctx.find_terms(["<last>"] * 512).tolist() == [9] * 512 and ctx.find_terms(["<b>", "<ab>"] * 300).tolist() == [NONE, 1] * 300
    heap = ctypes.create_string_buffer(b"x" * 513)
    offs = np.arange(514, dtype=np.uint64)
    ids = np.empty(513, np.uint32)
    assert ctx.lib.rdf_find_terms(ctx.ptr, heap, offs.ctypes.data, 513, ids.ctypes.data) == ERR_LIMIT
    # a query set larger than the staged bytes
    long_terms = ["<" + "y" * 40000 + ">", "<a>"]
    ctx.set_dictionary(terms + long_terms[:1])
    assert ctx.find_terms(long_terms + ["<" + "y" * 39999 + "z>"]).tolist() == [10, 0, NONE]
    # the device dictionary of a parse: the same ids as the host parser's
    path = tmp_path / "t.nt"
    path.write_text(NT_TEXT, encoding="utf-8")
    _, _, _, dic = ntriples.read_triples([str(path)])
    host_terms = list(dic.terms)
    with _lib.Context(0) as g:
        assert raises_status(ERR_STATE, lambda: g.find_terms(["<a>"]))  # no formatting dictionary
        n, v, _ = g.parse_ntriples(NT_TEXT.encode("utf-8"))
        assert (n, v) == (5, len(host_terms))
        g.set_dictionary_parsed()
        assert g.find_terms(host_terms).tolist() == list(range(v))
        assert g.find_terms(["<http://a", "<http://abcd>", "", '"x"@e', host_terms[-1]]).tolist() == [NONE, NONE, NONE, NONE, v - 1]
        g.set_dictionary(host_terms)
        assert g.find_terms(host_terms[::-1]).tolist() == list(range(v))[::-1]


def test_states_and_errors():
    arr, nv, ms = random_input(random.Random(7))
    with _lib.Context(0) as g:
        accessors = (g.selected_count, g.selected_decoded, lambda: g.format_selected(0, 1))
        assert raises_status(ERR_STATE, g.select_cinds)  # nothing resident
        g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
        g.frequent_conditions(ms)
        g.build_capture_groups("spo")
        assert raises_status(ERR_STATE, g.select_cinds)  # before a discovery
        assert all(raises_status(ERR_STATE, a) for a in accessors)
        g.discover_cinds()
        assert all(raises_status(ERR_STATE, a) for a in accessors)  # a result, no view yet
        n = g.select_cinds()
        assert n == g.cind_count() == g.selected_count() > 0
        # limits and arguments; a refused call leaves the earlier view alone or drops it, never a half-written one
        one = (ref.ALL_CODES, ANY, ANY)
        assert g.select_cinds(dep=[one] * 256, ref=[one] * 256) == n
        assert raises_status(ERR_LIMIT, lambda: g.select_cinds(dep=[one] * 257))
        assert raises_status(ERR_LIMIT, lambda: g.select_cinds(ref=[one] * 257))
        assert raises_status(ERR_ARG, lambda: g.select_cinds(dep=[(0x200, ANY, ANY)]))
        assert raises_status(ERR_ARG, lambda: g.select_cinds(ref=[(0x3FF, ANY, ANY)]))
        assert raises_status(ERR_ARG, lambda: g.select_cinds(min_support=3, max_support=2))
        q = _lib.CindQuery(None, 0, None, 0, 0, ANY, 2)  # an unknown flag
        cnt = ctypes.c_uint64()
        assert g.lib.rdf_select_cinds(g.ptr, ctypes.byref(q), ctypes.byref(cnt), None) == ERR_ARG
        assert g.select_cinds() == n and g.selected_count() == n
        # the view goes with the result it names
        drops = {
            "set_triples": lambda: g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv),
            "frequent_conditions": lambda: g.frequent_conditions(ms),
            "build_capture_groups": lambda: g.build_capture_groups("spo"),
            "discover_cinds": lambda: g.discover_cinds(),
            "run": lambda: g.run(ms),
            "discover_cinds_paged": lambda: (g.build_capture_groups("spo"), g.discover_cinds_paged(True, 1, 1)),
            "release_scratch": g.release_scratch,
        }
        for name, call in drops.items():
            g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
            g.run(ms)
            assert g.select_cinds() == n and len(g.selected_decoded()) == n
            call()
            assert all(raises_status(ERR_STATE, a) for a in accessors), name
        # ... and a page's view with the page
        g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
        g.frequent_conditions(ms)
        g.build_capture_groups("spo")
        g.discover_cinds_paged(True, 1, 1)
        assert raises_status(ERR_STATE, g.select_cinds)  # no current result before the first page
        total = pages = 0
        while g.next_page() is not None:
            assert all(raises_status(ERR_STATE, a) for a in accessors), pages
            total += g.select_cinds()
            assert g.selected_count() == g.cind_count()
            pages += 1
        assert total == n and pages > 1
        assert all(raises_status(ERR_STATE, a) for a in accessors)  # the end of the pages dropped the last view
        # row accessors and the statistics leave a view alone
        g.run(ms)
        some = g.select_cinds(min_support=ms + 1)
        before = g.selected_decoded()
        g.decoded_cinds()
        g.cind_histogram()
        assert g.selected_count() == some and (g.selected_decoded() == before).all()


def _sharded_worker(rank, world, port, case, q):
    """Two ranks over gloo, each with its own context on the one GPU (the statistics' state test): after the sharded run
    the selection and its accessors answer RDF_ERR_STATE."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rdfind_amd import distributed
    try:
        s, p, o, nv, ms = case
        with _lib.Context(0) as g:
            g.set_triples(s, p, o, nv)
            distributed.run_sharded(g, ms, "spo", True, 1)
            status = []
            for call in (g.select_cinds, lambda: g.select_cinds(count_only=True), g.selected_count, g.selected_decoded,
                         lambda: g.format_selected(0, 1)):
                try:
                    call()
                    status.append(0)
                except _lib.RdfError as e:
                    status.append(e.status)
            q.put((rank, (status, g.cind_count())))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, repr(e) + "\n" + traceback.format_exc()[-1500:]))
    finally:
        dist.destroy_process_group()


def test_sharded_run_is_refused():
    arr, nv, ms = random_input(random.Random(7))
    case = (arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy(), nv, ms)
    world = 2
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_sharded_worker, args=(r, world, port, case, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = {}
    deadline = time.monotonic() + 300
    try:
        while len(res) < world:
            try:
                r, item = q.get(timeout=1)
            except queue.Empty:  # a rank that died before it could report ends the wait at once
                dead = {i: pr.exitcode for i, pr in enumerate(procs) if pr.exitcode not in (None, 0)}
                assert not dead, f"ranks ended without a report (exit codes {dead})"
                assert time.monotonic() < deadline, "no report from the ranks"
                continue
            assert not isinstance(item, str), f"rank {r}: {item}"
            res[r] = item
    finally:
        for pr in procs:
            pr.join(timeout=5 if len(res) < world else 60)
            if pr.is_alive():
                pr.terminate()
    for r in range(world):
        status, n = res[r]
        assert status == [ERR_STATE] * 5, (r, status)
    assert sum(res[r][1] for r in range(world)) == len(expected_set(arr, nv, ms, 1, True)) > 0  # (the run had a result)


# ---------------------------------------------------------------------------
# the driver

_GOLDEN = {}


def golden(name):
    """(min support, golden lines, their (dep, ref, support) splits, parsed rows)."""
    if name not in _GOLDEN:
        ms, lines = read_golden(name, "s1_clean")
        split = []
        for ln in lines:
            dep, rest = ln.split(" < ")
            rf, sup = rest.rsplit(" (support=", 1)
            split.append((dep, rf, int(sup[:-1])))
        _GOLDEN[name] = (ms, lines, split, [cind_stats_ref.parse_line(ln) for ln in lines])
    return _GOLDEN[name]


def run_driver(argv):
    """(returned lines, printed lines) of one driver run."""
    out = io.StringIO()
    lines = program.RDFind(argv).run(out=out)
    return lines, out.getvalue().splitlines()


def driver_cases(name):
    """(flags, the golden lines they select) for one fixture."""
    ms, lines, split, rows = golden(name)
    top_ref = Counter(rf for _, rf, _ in split).most_common(1)[0][0]
    top_dep = Counter(dep for dep, _, _ in split).most_common(1)[0][0]
    sups = sorted({s for _, _, s in split})
    lo, hi = sups[len(sups) // 2], sups[-1] - 1 if len(sups) > 2 else sups[-1]
    cases = [
        (["--select-ref", top_ref], [ln for ln, (_, rf, _) in zip(lines, split) if rf == top_ref]),
        (["--select-dep", top_dep], [ln for ln, (dep, _, _) in zip(lines, split) if dep == top_dep]),
        (["--select-support", f"{lo}:{hi}"], [ln for ln, (_, _, s) in zip(lines, split) if lo <= s <= hi]),
        (["--select-support", str(lo), "--select-dep", top_dep, "--select-dep", "s[p=*]"],
         [ln for ln, (dep, _, s), r in zip(lines, split, rows) if s >= lo and (dep == top_dep or r[0] == 10)]),
        (["--select-ref", "<http://no.such/term>"], []),
    ]
    lits = Counter(v for r in rows for v in (r[4], r[5]) if v is not None and v.startswith('"'))
    if name != "lubm_small":
        assert lits, name
    if lits:  # a bare literal term: every referenced capture that names it
        lit = lits.most_common(1)[0][0]
        cases.append((["--select-ref", lit], [ln for ln, r in zip(lines, rows) if lit in (r[4], r[5])]))
    return ms, lines, top_ref, cases


@pytest.mark.parametrize("name", ["lubm_small", "skew_small", "zipf_small"])
def test_program_selection(tmp_path, name):
    ms, lines, top_ref, cases = driver_cases(name)
    if name == "lubm_small":
        assert top_ref.startswith("s[p=<http://") and top_ref.endswith("univ-bench.owl#name>]") and len(cases[0][1]) == 119
    inp = os.path.join(GOLDEN, f"{name}.nt.gz")
    base = ["--use-fis", "--clean-implied", "--support", str(ms)]
    assert any(0 < len(want) < len(lines) for _, want in cases)
    for k, (flags, want) in enumerate(cases):
        got, printed = run_driver(base + flags + [inp])
        assert sorted(got) == want, flags
        assert printed == [f"Selected {len(want)} CINDs.", f"Detected {len(lines)} CINDs."], flags
        out = tmp_path / f"sel{k}.txt"
        got, printed = run_driver(base + flags + ["--output", f"file://{out}", inp])
        assert sorted(out.read_text(encoding="utf-8").splitlines()) == want == sorted(got), flags
        assert printed == [f"Selected {len(want)} CINDs."], flags
        out = tmp_path / f"cnt{k}.txt"
        got, printed = run_driver(base + flags + ["--select-count", "--output", f"file://{out}", inp])
        assert printed == [f"Selected {len(want)} CINDs."] and out.read_bytes() == b"" and not got, flags
        got, printed = run_driver(base + flags + ["--page-bytes", "1", inp])
        assert sorted(got) == want and printed[0] == f"Selected {len(want)} CINDs.", flags
    # --cind-statistics still describes the whole result
    flags, want = cases[0]
    _, with_stats = run_driver(base + flags + ["--cind-statistics", "2", inp])
    _, plain_stats = run_driver(base + ["--cind-statistics", "2", inp])
    assert with_stats == plain_stats[:-1] + [f"Selected {len(want)} CINDs.", plain_stats[-1]]
    # without the flags nothing changes
    got, printed = run_driver(base + [inp])
    assert sorted(got) == lines and printed == [f"Detected {len(lines)} CINDs."]
    for flags in (["--select-ref", top_ref], ["--select-count"], ["--select-support", "2"]):
        with pytest.raises(NotImplementedError):
            program.RDFind(base + flags + ["-dop", "2", inp])
