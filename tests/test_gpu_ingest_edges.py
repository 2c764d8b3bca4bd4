"""The device N-Triples ingest at its byte edges: the constructed texts of tests/nt_shapes.py (tile and load edges of
the line-start passes, the tokenizer's LDS tile at 12288 / 12289 words for every alignment, the second trip of the
grid-stride loops, the grammar rows, the byte comparison's tail at every alignment, the heap append at every
heap0 & 3 and with empty terms) through rdf_parse_ntriples and the chunked parse, compared with the constructed
triples and terms, bytes included.  tests/test_nt_shapes_cpu.py proves that the texts hit the edges they claim."""
import ctypes

import numpy as np
import pytest

from rdfind_amd import _lib
from tests import nt_shapes as ns

pytestmark = pytest.mark.gpu

RDF_ERR_ARG = -1
RDF_ERR_STATE = -4
SMALL = ns.small_texts()


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def forced(monkeypatch):
    """A context that compares bytes on every occupied slot it probes and starts with a 16-slot term table."""
    monkeypatch.setenv("RDFIND_NT_FP_BITS", "0")
    monkeypatch.setenv("RDFIND_NT_DICT_SLOTS", str(ns.DICT_SLOTS))
    c = _lib.Context(0)
    yield c
    c.close()


def _raw_terms(c):
    """(offsets, lengths) of the device's term table (rdf_copy_terms)."""
    v = c.num_terms
    off, ln = np.empty(v, np.uint64), np.empty(v, np.uint32)
    got = ctypes.c_uint64()
    c._check(c.lib.rdf_copy_terms(c.ptr, off.ctypes.data, ln.ctypes.data, v, ctypes.byref(got)), "rdf_copy_terms")
    assert got.value == v
    return off, ln


def _terms(c):
    heap, offsets = c.parsed_terms()
    return [heap[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def _check(t, n, v, c, what):
    assert (n, v) == (len(t.s), len(t.terms)), (t.name, what)
    s, p, o = c.copy_triples(n + 1)
    for got, exp, pos in ((s, t.s, "s"), (p, t.p, "p"), (o, t.o, "o")):
        np.testing.assert_array_equal(got, exp, err_msg=f"{t.name} {what} {pos}")
    assert _terms(c) == t.terms, (t.name, what)


def _single(c, t):
    n, v, _ = c.parse_ntriples(t.data, tabs=t.tabs)
    _check(t, n, v, c, "single")


def _chunked(c, t, windows, what):
    c.parse_begin(tabs=t.tabs)
    for w in windows:
        c.parse_chunk(w)
    st = c.parse_end()
    _check(t, st["n_triples"], st["n_terms"], c, what)
    assert st["n_lines"] == t.n_lines == ns.window_line_count(windows), (t.name, what)
    assert st["heap_bytes"] == t.heap_bytes and st["n_chunks"] == len(windows), (t.name, what)
    return st


def _gather(c, t, what):
    """k_nt_dict_gather: the parse's dictionary as the formatting dictionary, every term read back."""
    c.set_dictionary_parsed()
    got = c.dictionary_terms(np.arange(len(t.terms), dtype=np.uint32)) if t.terms else []
    assert [x.encode() for x in got] == t.terms, (t.name, what)


def _modes(t):
    if t.cuts and t.family == "heap":  # the heap family is its explicit windows
        return [("windows", t.windows())]
    if t.cuts:
        return [("windows", t.windows()), ("three", ns.split_k(t.data, 3)), ("one", [t.data])]
    return [("per_line", ns.split_lines(t.data)), ("three", ns.split_k(t.data, 3)), ("one", [t.data])]


@pytest.mark.parametrize("name", ns.names("lines") + ns.names("blocks") + ns.names("grammar") + ns.names("dict")
                         + ns.names("heap"))
def test_text_in_every_mode(ctx, name):
    """One call and the chunked parses give the constructed triples and terms; lines, triples, terms and heap bytes of
    a chunked parse are exact; on dict and heap the gathered dictionary equals the terms after every mode."""
    t = SMALL[name]
    gather = t.family in ("dict", "heap")
    _single(ctx, t)
    if gather:
        _gather(ctx, t, "single")
    for what, windows in _modes(t):
        _chunked(ctx, t, windows, what)
        if gather:
            _gather(ctx, t, what)


def test_big(ctx):
    """More than 2048 tiles and more than 2048 * 256 lines: both grid-stride loops take a second trip, block 0 from
    global memory to LDS and block 1 the other way round."""
    t = ns.big()
    _single(ctx, t)


@pytest.mark.parametrize("name", ns.names("dict") + ns.names("heap"))
def test_unequal_comparison(forced, name):
    """Without fingerprint bits every occupied slot a probe meets is compared by its bytes (nt_equal in the window's
    own table, nt_equal2 against the heap), and the 16-slot table grows from the ninth term on."""
    t = SMALL[name]
    for what, windows in _modes(t):
        st = _chunked(forced, t, windows, "forced " + what)
        _gather(forced, t, "forced " + what)
        if len(t.terms) > 8:
            assert st["n_table_growths"] >= 1 and st["table_slots"] >= 2 * len(t.terms)


def test_last_byte_pairs_cover_every_alignment(forced):
    """dict_lastbyte_chain: X lies in the heap, X' (its last byte differs) comes in a later window and its probe passes
    X's slot.  The heap offsets are the device's (rdf_copy_terms after rdf_parse_end), the window offsets the bytes'."""
    t = ns.dict_lastbyte_chain()
    wins = t.windows()
    _chunked(forced, t, wins, "chain")
    off, ln = _raw_terms(forced)
    seen = set()
    for ix, iy, k, w, h, l in t.marks:
        x, y = t.terms[ix], t.terms[iy]
        assert x[:-1] == y[:-1] and x[-1] != y[-1] and int(ln[ix]) == int(ln[iy]) == len(x)
        assert wins[k].find(y) == w
        seen.add((wins[k].find(y) % 4, int(off[ix]) % 4, int(ln[ix]) % 4))
        assert (int(off[ix]) % 4, int(ln[ix]) % 4) == (h, l)
    assert seen == {(w, h, l) for w in range(4) for h in range(4) for l in range(4)}


def test_table_growth_at_the_ninth_term(forced):
    t = SMALL["heap_slots"]
    forced.parse_begin()
    counts = [forced.parse_chunk(w)[1] for w in t.windows()]
    st = forced.parse_end()
    assert counts == t.terms_at_cut == [8, 9, 9]
    assert (st["n_table_growths"], st["table_slots"]) == (1, 32)
    forced.parse_begin()
    forced.parse_chunk(t.windows()[0])
    st = forced.parse_end()
    assert (st["n_terms"], st["n_table_growths"], st["table_slots"]) == (8, 0, 16)


@pytest.mark.parametrize("name", ns.names("grammar", bad=True) + ["bad_two_blocks"])
def test_malformed_line_number(ctx, name):
    """The first malformed line is named, 1-based, with the comments and blank lines before it counted; of two bad
    lines in different tokenizer blocks the lower one."""
    t = SMALL[name]
    with pytest.raises(_lib.RdfError, match=rf"malformed N-Triples line {t.bad_line}$") as e:
        ctx.parse_ntriples(t.data, tabs=t.tabs)
    assert e.value.status == RDF_ERR_ARG
    for what, windows in (("per_line", ns.split_lines(t.data)), ("three", ns.split_k(t.data, 3))):
        ctx.parse_begin(tabs=t.tabs)
        with pytest.raises(_lib.RdfError, match=rf"malformed N-Triples line {t.bad_line}$") as e:
            for w in windows:
                ctx.parse_chunk(w)
        assert e.value.status == RDF_ERR_ARG, what
        with pytest.raises(_lib.RdfError) as e:
            ctx.parse_chunk(b"<a> <p> <b> .\n")
        assert e.value.status == RDF_ERR_STATE, what


def test_malformed_line_number_across_windows(ctx):
    """An empty window, an all-comment window and a non-final window without '\\n' all count towards the number."""
    t = SMALL["bad_chunked"]
    wins = t.windows()
    assert wins[1] == b"" and not wins[3].endswith(b"\n") and t.bad_line == 8
    ctx.parse_begin()
    for w in wins[:-1]:
        ctx.parse_chunk(w)
    with pytest.raises(_lib.RdfError, match=r"malformed N-Triples line 8$") as e:
        ctx.parse_chunk(wins[-1])
    assert e.value.status == RDF_ERR_ARG
    for call in (lambda: ctx.parse_chunk(wins[0]), ctx.parse_end):
        with pytest.raises(_lib.RdfError) as e:
            call()
        assert e.value.status == RDF_ERR_STATE
    # the same windows without the bad line parse, and count their lines
    ctx.parse_begin()
    for w in wins[:-1]:
        ctx.parse_chunk(w)
    st = ctx.parse_end()
    assert (st["n_lines"], st["n_triples"], st["n_chunks"]) == (6, 3, 4)
