"""Chunked N-Triples ingest (rdf_parse_begin / rdf_parse_chunk / rdf_parse_end): for any split of a text at line
boundaries the resident triples and the dictionary are bit-identical to one rdf_parse_ntriples over the whole text
and to the host parser; the table growth and the byte-comparison path are forced on small inputs."""
import gzip
import os
import re

import numpy as np
import pytest

from rdfind_amd import _lib, ntriples, program, synth
from tests.conftest import GOLDEN
from tests.test_oracle import read_golden

pytestmark = pytest.mark.gpu

RDF_ERR_STATE = -4


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# 10 lines: a comment, blank lines, CRLF, an escaped quote, a typed literal, a fourth term, no final newline
_SAMPLE = (
    "# a comment\n"
    "<http://ex.org/a> <http://ex.org/p> \"plain\" .\n"
    "\n"
    "  \t \n"
    "<http://ex.org/a> <http://ex.org/p> \"esc \\\" quote\"@en-US .\n"
    "_:b0 <http://ex.org/q> \"5\"^^<http://www.w3.org/2001/XMLSchema#int> .\r\n"
    "<http://ex.org/b>\t<http://ex.org/p>   \"x\"^^xsd:int .\n"
    "<http://ex.org/b> <http://ex.org/p> <http://ex.org/a> <http://ex.org/graph> .\n"
    "#<http://ex.org/c> <http://ex.org/p> <http://ex.org/a> .\n"
    "<http://ex.org/a> <http://ex.org/q> _:b0 ."
).encode()

# <a>, <p>: first seen in chunk 1, used again in chunks 2 and 3 (the 5th); <d>, <q>: new in chunk 2, twice there and
# again in the last chunk; an empty chunk and an all-comment chunk in the middle; the last chunk without a final newline
_REUSE_CHUNKS = [
    b"<a> <p> <b> .\n<c> <p> <a> .\n",
    b"<a> <q> <d> .\n<d> <q> <d> .\n",
    b"",
    b"# only comments\n\n   \n# here\n",
    b"<d> <p> <a> .\n<e> <q> <a> .\n<f> <p> <e> ",
]

_TABS = b"<a>\t<p>\t\"x y\"\t.\n# c\n<b>\t<p>\t<a>\n\n<a> x\t<q>\t\"z\"\r\n<b>\t<q>\t\"x y\"\n<a> x\t<p>\t<b>\n"


def _lines_of(data: bytes):
    """The lines of data, each with its '\\n' (the last one maybe without): only '\\n' ends a line."""
    return re.findall(rb"[^\n]*\n|[^\n]+$", data)


def _split(data: bytes, k: int):
    """data in k chunks of whole lines (cut at line starts)."""
    lines = _lines_of(data)
    step = -(-len(lines) // k)
    return [b"".join(lines[i:i + step]) for i in range(0, len(lines), step)]


def _long_lines() -> bytes:
    """About 600 lines with 300-2000 B literals (4096-byte windows hold a few each) and one line of 60 000 B, which
    becomes a window of its own and parses from global memory (it exceeds the tokenizer's LDS tile)."""
    rng = np.random.default_rng(11)
    lines = []
    for i in range(600):
        lit = "".join(chr(97 + c) for c in rng.integers(0, 26, int(rng.integers(300, 2000))))
        lines.append(f"<s{i % 53}> <p{i % 5}> \"{lit if i % 4 else 'same literal'}\"@en .")
        if i == 300:
            lines.append("<big> <p0> \"" + "z" * (60000 - 15) + "\" .")
    return ("\n".join(lines) + "\n").encode()


_CACHE = {}


def _c1_text() -> bytes:
    if "c1" not in _CACHE:
        _CACHE["c1"] = "".join(ln + "\n" for ln in synth.config("c1", 0.05).lines()).encode()
    return _CACHE["c1"]


def _lubm() -> bytes:
    return gzip.open(os.path.join(GOLDEN, "lubm_small.nt.gz"), "rb").read()


def _whole(chunks):
    """The text whose single parse a chunked parse must equal: a chunk without a final '\\n' ends its last line."""
    return b"".join(c if not c or c.endswith(b"\n") else c + b"\n" for c in chunks)


def _host(tmp_path, data: bytes, tabs=False):
    f = tmp_path / "host.nt"
    f.write_bytes(data)
    s, p, o, d = ntriples.read_triples([str(f)], tabs=tabs)
    return s, p, o, d.terms


def _single(c, data: bytes, tabs=False):
    n, v, _ = c.parse_ntriples(data, tabs=tabs)
    s, p, o = c.copy_triples(n)
    return s, p, o, ntriples.HeapDictionary(*c.parsed_terms()).terms


def _chunked(c, chunks, tabs=False):
    c.parse_begin(tabs=tabs)
    n = v = 0
    for ch in chunks:
        n2, v2 = c.parse_chunk(ch)
        assert n2 >= n and v2 >= v
        n, v = n2, v2
    st = c.parse_end()
    assert (st["n_triples"], st["n_terms"], st["n_chunks"]) == (n, v, len(chunks))
    s, p, o = c.copy_triples(n + 1)
    return s, p, o, ntriples.HeapDictionary(*c.parsed_terms()).terms, st


def _same(got, exp):
    assert len(got[0]) == len(exp[0])
    for a, b in zip(got[:3], exp[:3]):
        np.testing.assert_array_equal(a, b)
    assert got[3] == exp[3]


def _assert_parity(c, tmp_path, chunks, tabs=False):
    """chunked == single call == host parser: s, p, o, their order, n, V and every term's bytes.  Returns the stats."""
    chunks = list(chunks)
    data = _whole(chunks)
    host = _host(tmp_path, data, tabs)
    single = _single(c, data, tabs)
    _same(single, host)
    *got, st = _chunked(c, chunks, tabs)
    _same(got, single)
    assert st["n_lines"] == sum(len(_lines_of(ch)) for ch in chunks)
    assert st["heap_bytes"] == sum(len(t.encode()) for t in single[3])
    return st


@pytest.mark.parametrize("case", ["sample_per_line", "sample_3", "reuse", "tabs_2", "long_lines_4096", "lubm_3",
                                  "lubm_4096", "c1_5"])
def test_chunked_parse_matches_single_call(ctx, tmp_path, case):
    tabs = case == "tabs_2"
    if case == "sample_per_line":
        chunks = _lines_of(_SAMPLE)
        assert len(chunks) == 10
    elif case == "sample_3":
        chunks = _split(_SAMPLE, 3)
    elif case == "reuse":
        chunks = _REUSE_CHUNKS
    elif case == "tabs_2":
        chunks = _split(_TABS, 2)
    elif case == "long_lines_4096":
        f = tmp_path / "long.nt"
        f.write_bytes(_long_lines())
        chunks = list(ntriples.iter_windows([str(f)], 4096))
        assert sum(len(ch) > 49152 for ch in chunks) == 1 and len(chunks) > 100
    elif case == "lubm_3":
        chunks = _split(_lubm(), 3)
    elif case == "lubm_4096":
        chunks = list(ntriples.iter_windows([os.path.join(GOLDEN, "lubm_small.nt.gz")], 4096))
        assert len(chunks) > 100
    else:
        chunks = _split(_c1_text(), 5)
    if case in ("sample_3", "tabs_2", "lubm_3", "c1_5"):
        assert len(chunks) == int(case.rsplit("_", 1)[1])
    _assert_parity(ctx, tmp_path, chunks, tabs)


def _growth_chunks():
    """8 chunks, about 2000 distinct terms whose number doubles from chunk to chunk, and every chunk uses terms of all
    the earlier ones again."""
    sizes = [10, 10, 20, 40, 80, 160, 320, 1360]
    chunks, base = [], 0
    for k, m in enumerate(sizes):
        lines = [f"<s{j}> <p{k % 3}> <o{j % 7}> ." for j in range(base, base + m)]
        lines += [f"<s{j}> <q> <s{(j * 5) % (base + m)}> ." for j in range(0, base + m, 3)]
        chunks.append(("\n".join(lines) + "\n").encode())
        base += m
    return chunks


def test_forced_table_growth(tmp_path, monkeypatch):
    chunks = _growth_chunks()
    with _lib.Context(0) as c:
        st0 = _assert_parity(c, tmp_path, chunks)
    monkeypatch.setenv("RDFIND_NT_DICT_SLOTS", "16")
    with _lib.Context(0) as c:
        st = _assert_parity(c, tmp_path, chunks)
    assert 1900 <= st["n_terms"] <= 2100
    assert st["n_table_growths"] >= 5, st
    assert st["table_slots"] >= 2 * st["n_terms"], st
    assert st0["n_table_growths"] < 5 and st0["n_table_growths"] < st["n_table_growths"], st0
    assert (st0["n_triples"], st0["n_terms"], st0["heap_bytes"]) == (st["n_triples"], st["n_terms"], st["heap_bytes"])


def test_collision_path(tmp_path, monkeypatch):
    """No fingerprint bits: every probe that meets an occupied slot compares lengths and bytes, and the terms have
    equal lengths, so only the bytes tell them apart."""
    monkeypatch.setenv("RDFIND_NT_FP_BITS", "0")
    monkeypatch.setenv("RDFIND_NT_DICT_SLOTS", "16")
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 1000, size=(1500, 3))
    lines = [f"<a{a:03d}> <a{b % 10:03d}> <a{c:03d}> ." for a, b, c in ids.tolist()]
    chunks = _split(("\n".join(lines) + "\n").encode(), 6)
    with _lib.Context(0) as c:
        st = _assert_parity(c, tmp_path, chunks)
    assert st["n_terms"] > 900 and st["n_table_growths"] >= 1


def test_errors_and_state(tmp_path):
    good = [b"<a> <p> <b> .\n<b> <p> <c> .\n", b"# c\n\n<c> <p> <a> .\n<a> <q> <c> .\n"]
    with _lib.Context(0) as c:
        with pytest.raises(_lib.RdfError) as e:
            c.parse_chunk(b"<a> <p> <b> .\n")  # no open parse
        assert e.value.status == RDF_ERR_STATE
        c.parse_begin()
        c.parse_chunk(good[0])
        with pytest.raises(_lib.RdfError) as e:
            c.frequent_conditions(1)  # no input between begin and end
        assert e.value.status == RDF_ERR_STATE
        c.parse_chunk(good[1])
        with pytest.raises(_lib.RdfError, match="line 7") as e:
            c.parse_chunk(b"<a> <p> \"unterminated .\n<a> <p> <b> .\n")
        assert e.value.status == -1
        with pytest.raises(_lib.RdfError) as e:
            c.frequent_conditions(1)  # the parse was abandoned: no input
        assert e.value.status == RDF_ERR_STATE
        with pytest.raises(_lib.RdfError) as e:
            c.parse_chunk(good[0])
        assert e.value.status == RDF_ERR_STATE
        with pytest.raises(_lib.RdfError) as e:
            c.parse_end()
        assert e.value.status == RDF_ERR_STATE
        _assert_parity(c, tmp_path, good + [b"<d> <p> <a> .\n"])
        c.frequent_conditions(1)
        # a call that replaces the input abandons an open parse
        c.parse_begin()
        c.parse_chunk(good[0])
        z = np.zeros(3, np.uint32)
        c.set_triples(z, z, z, 1)
        with pytest.raises(_lib.RdfError) as e:
            c.parse_chunk(good[1])
        assert e.value.status == RDF_ERR_STATE
        c.frequent_conditions(1)  # the triples that were set are the input


def test_downstream_of_chunked_parse(ctx):
    """Discovery and the device-side formatting dictionary (rdf_set_dictionary_parsed, gathered from the term heap)
    after a chunked parse give the lines and the checksum of the same sequence after the single call.  The lines are
    compared sorted, as the golden tests compare them: the order of a run's result rows is not part of the result (the
    printed flags show whether two runs after the single call, and the chunked one, happen to agree in order too)."""
    data = _c1_text()

    def result():
        ctx.run(5)
        ctx.set_dictionary_parsed()
        count = ctx.cind_count()
        assert 0 < count <= 1 << 20
        return ctx.format_array(0, count).tobytes(), ctx.checksum()

    ctx.parse_ntriples(data)
    exp_text, exp_sum = result()
    ctx.parse_ntriples(data)
    again_text, again_sum = result()
    ctx.parse_windows(_split(data, 5))
    got_text, got_sum = result()
    print("row order: single == single again:", again_text == exp_text, "; chunked == single:", got_text == exp_text)
    assert exp_text and len(got_text) == len(exp_text)
    assert sorted(got_text.split(b"\n")) == sorted(exp_text.split(b"\n"))
    assert got_sum == exp_sum == again_sum


def test_program_ingest_window(tmp_path):
    """The driver parses in windows once the input exceeds --ingest-window, and in one call otherwise."""
    ms, expected = read_golden("lubm_small", "s1_clean")
    path = os.path.join(GOLDEN, "lubm_small.nt.gz")
    calls = []
    real = _lib.Context.parse_windows, _lib.Context.parse_ntriples

    def spy(name, fn):
        def wrapped(self, *a, **k):
            calls.append(name)
            return fn(self, *a, **k)
        return wrapped

    for window, path_taken in ((4096, "windows"), (1 << 24, "single")):
        out = tmp_path / f"cinds_{window}.txt"
        _lib.Context.parse_windows, _lib.Context.parse_ntriples = spy("windows", real[0]), spy("single", real[1])
        try:
            program.RDFind(["--use-fis", "--clean-implied", "--support", str(ms), "--ingest-window", str(window),
                            "--output", f"file://{out}", path]).run()
        finally:
            _lib.Context.parse_windows, _lib.Context.parse_ntriples = real
        assert sorted(out.read_text().splitlines()) == expected, window
        assert calls == [path_taken], window
        calls.clear()


def test_chunked_parse_memory():
    """The single call keeps the whole text in HBM; the chunked parse keeps the distinct terms only, and after
    rdf_parse_end nothing but the triples, the term table and the term heap (no window, no scratch, no hash table)."""
    rng = np.random.default_rng(3)
    terms = [f"<http://example.org/resource/{i:02d}>" for i in range(100)]
    ids = rng.integers(0, 100, size=(48000, 3))
    data = "".join(f"{terms[a]} {terms[b % 10]} {terms[c]} .\n" for a, b, c in ids.tolist()).encode()
    assert len(data) >= 4 << 20
    windows = _split(data, -(-len(data) // (60 << 10)))
    assert max(len(w) for w in windows) <= 64 << 10
    with _lib.Context(0) as c:
        base = c.device_bytes()
        n, v, _ = c.parse_ntriples(data)
        single = c.device_bytes() - base
    with _lib.Context(0) as c:
        assert c.device_bytes() == base
        c.parse_begin()
        for w in windows:
            c.parse_chunk(w)
        during = c.device_bytes() - base
        st = c.parse_end()
        chunked = c.device_bytes() - base
        assert (st["n_triples"], st["n_terms"]) == (n, v) and v <= 100
        print("single", single, "chunked", chunked, "open parse", during, "text", len(data), "stats", st)
        assert single - chunked >= len(data) // 2, (single, chunked, len(data))
        # what stays: 12 B per triple, 12 B per term, the heap and its padding, each buffer at least 256 B; the scan
        # workspace of the parse is the only other thing the context may hold
        kept = 3 * max(4 * n, 256) + max(8 * v, 256) + max(4 * v, 256) + max(st["heap_bytes"] + 16, 256)
        assert kept <= chunked < kept + (1 << 20), (chunked, kept)
        assert during > chunked  # the window, its scratch and the table were held and are gone
        c.run(10)
