"""The constructed N-Triples texts (tests/nt_shapes.py) against the host parser, and every edge they claim, decided
from their bytes by the geometry helpers.  No GPU: this pins the generator, the host parser and the claims that
tests/test_gpu_ingest_edges.py relies on."""
import numpy as np
import pytest

from rdfind_amd import ntriples
from tests import nt_shapes as ns

SMALL = ns.small_texts()
GOOD = [n for n, t in SMALL.items() if t.bad_line is None]
BAD = [n for n, t in SMALL.items() if t.bad_line is not None]


def _host(tmp_path, t):
    f = tmp_path / "t.nt"
    f.write_bytes(t.data)
    s, p, o, d = ntriples.read_triples([str(f)], tabs=t.tabs)
    return s, p, o, [x.encode() for x in d.terms]


def _check_host(tmp_path, t):
    s, p, o, terms = _host(tmp_path, t)
    assert terms == t.terms
    for got, exp in ((s, t.s), (p, t.p), (o, t.o)):
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, exp)


def _check_edges(t):
    assert t.edges or t.family == "heap"
    for e in t.edges:
        assert ns.edge_present(t, e), (t.name, e)


def test_constants_match_the_sources():
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rdfind_amd", "csrc")
    k = open(os.path.join(csrc, "kernels.inl")).read()
    assert "NT_CHUNK = RDF_BLOCK * 16;" in k and ns.NT_CHUNK == ns.BLOCK_LINES * ns.NT_LOAD
    assert f"NT_TILE = {ns.NT_TILE};" in k
    assert f"#define RDF_BLOCK {ns.BLOCK_LINES}" in open(os.path.join(csrc, "common.hpp")).read()
    assert f"#define RDF_KGRID {ns.KGRID}" in open(os.path.join(csrc, "rdfind_hip.hip")).read()


def test_families_are_complete():
    fam = {f: ns.names(f) for f in ("lines", "blocks", "grammar", "dict", "heap")}
    assert all(fam.values())
    sizes = {(len(SMALL[n].data), SMALL[n].data.endswith(b"\n")) for n in fam["lines"]}
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 8192):
        assert (n, True) in sizes and (n, False) in sizes
    assert (0, False) in sizes
    got = {e for n in fam["blocks"] for e in SMALL[n].edges if e.startswith("block=1:")}
    assert got == {f"block=1:{w}:{int(w == 12288)}:{r}" for r in range(4) for w in (12288, 12289)}
    assert len(ns.names("grammar", bad=True)) == 6


@pytest.mark.parametrize("name", GOOD)
def test_host_parser_gives_the_constructed_values(tmp_path, name):
    t = SMALL[name]
    _check_host(tmp_path, t)
    assert t.n_lines == ns.window_line_count([t.data])
    if t.cuts:
        assert b"".join(t.windows()) == t.data and t.n_lines == ns.window_line_count(t.windows())


@pytest.mark.parametrize("name", BAD)
def test_host_parser_rejects_the_malformed_texts(tmp_path, name):
    t = SMALL[name]
    with pytest.raises(ntriples.ParseError):
        _host(tmp_path, t)
    # the text up to the bad line is good, and the bad line is the one the builder named
    lines = ns.split_lines(b"".join(w if not w or w.endswith(b"\n") else w + b"\n" for w in t.windows())
                           if t.cuts else t.data)
    f = tmp_path / "head.nt"
    f.write_bytes(b"".join(lines[:t.bad_line - 1]))
    ntriples.read_triples([str(f)], tabs=t.tabs)
    f.write_bytes(lines[t.bad_line - 1])
    with pytest.raises(ntriples.ParseError):
        ntriples.read_triples([str(f)], tabs=t.tabs)


@pytest.mark.parametrize("name", list(SMALL))
def test_claimed_edges_are_present(name):
    _check_edges(SMALL[name])


def test_big(tmp_path):
    t = ns.big()
    _check_edges(t)
    assert ns.n_tiles(t.data) > ns.KGRID and len(ns.line_starts(t.data)) > ns.KGRID * ns.BLOCK_LINES
    assert len(t.data) > ns.KGRID * ns.NT_CHUNK and t.n_lines == ns.KGRID * 256 + 512 + 3
    bl = ns.blocks(t.data)
    assert len(bl) > ns.KGRID + 2  # blocks 0 and 1 take a second trip
    assert [bl[i][3] for i in (0, ns.KGRID, 1, ns.KGRID + 1)] == [False, True, True, False]
    _check_host(tmp_path, t)


def test_grammar_rows(tmp_path):
    """The rows by their bytes, one text each: what the host parser gives today."""
    rows = [(False, b'<s> <a b> "x"^^', [b"<s>", b"<a b>", b'"x"^^']),
            (False, b'"lit"xyz <o>', [b'"lit"', b"xyz", b"<o>"]),
            (False, b'"l"^x <o>', [b'"l"', b"^x", b"<o>"]),
            (False, b"<s><p><o>.", [b"<s>", b"<p>", b"<o>"]),
            (False, b'<s> <p> "a\\\\" .', [b"<s>", b"<p>", b'"a\\\\"']),
            (False, b"  # not a comment", [b"#", b"not", b"a"]),
            (False, b'<s> "x\x1cy" \x1c<o>', [b"<s>", b'"x\x1cy"', b"<o>"]),
            (False, '"été" "étè" <o>'.encode(), ['"été"'.encode(), '"étè"'.encode(), b"<o>"]),
            (True, b"a\t\tb", [b"a", b"", b"b"]),
            (True, b"\t\t\na\tb\tc", [b"a", b"b", b"c"]),
            (True, b"x\ty\t", [b"x", b"y", b""]),
            (True, b"a\tb\tc\r\n", [b"a", b"b", b"c"]),
            (True, b"a\tb\tc\r", [b"a", b"b", b"c\r"])]
    for tabs, raw, exp in rows:
        f = tmp_path / "row.nt"
        f.write_bytes(raw)
        s, p, o, d = ntriples.read_triples([str(f)], tabs=tabs)
        assert len(s) == 1, raw
        assert [d.terms[int(x[0])].encode() for x in (s, p, o)] == exp, raw


def test_dict_lengths_and_variants():
    t = ns.dict_pairs()
    lens = {len(x) for x in t.terms}
    assert set(ns.LENGTHS) <= lens and ns.LENGTHS == list(range(1, 14)) + [15, 17, 19, 21, 23, 25, 27, 29, 31, 33]
    # per length: a pair that differs in the first byte only, in each tail byte only, in the last byte only
    diffs = {}
    for i in range(len(t.s)):
        x, y = t.terms[t.s[i]], t.terms[t.p[i]]
        if len(x) == len(y) and x != y:
            d = [k for k in range(len(x)) if x[k] != y[k]]
            if len(d) == 1:
                diffs.setdefault(len(x), set()).add(d[0])
    for n in ns.LENGTHS:
        assert {0, n - 1} | set(range(4 * (n // 4), n)) <= diffs[n], n
    assert any(x[-1] >= 0x80 and x[:-1] + bytes([x[-1] ^ 1]) in t.terms for x in t.terms)
    assert b"abc" in t.terms and b"abcd" in t.terms and b"ab" in t.terms
    assert all(s % 4 == 0 for s in ns.line_starts(t.data)[:-3].tolist())


def test_dict_pairs_cover_every_alignment():
    """The pair lines replayed from the bytes as one window per line: both terms of a marked line occur on no earlier
    line (both are misses of the persistent table, so both enter the window's own table), that table has 16 slots,
    and the two share their home slot in it: the one inserted second meets the other and nt_equal compares them.
    Per length and differing byte (first, each tail byte, last) all 16 offset combinations occur."""
    t = ns.dict_pairs()
    marked = {a: (b, n, k) for a, b, n, k in t.marks}
    seen_terms, found, pos = set(), {}, 0
    for line in ns.split_lines(t.data):
        toks = line.split()
        a = pos + line.index(toks[0])
        if a in marked:
            b, n, k = marked.pop(a)
            x, y = t.data[a:a + n], t.data[b:b + n]
            assert (x, y) == (toks[0], toks[1]) and b == a + n + line[a - pos + n:].index(y)
            assert len(x) == len(y) == n and [q for q in range(n) if x[q] != y[q]] == [k]
            assert x not in seen_terms and y not in seen_terms and toks[2] not in seen_terms, (x, y)
            assert ns.local_slots(line) == 16 and (ns.nt_hash(x) ^ ns.nt_hash(y)) & 15 == 0
            found.setdefault((n, k), set()).add((a % 4, b % 4))
        seen_terms.update(toks[:3])
        pos += len(line)
    assert not marked
    for n in ns.LENGTHS:
        for k in {0, n - 1} | set(range(4 * (n // 4), n)):
            assert len(found[(n, k)]) == (16 if n > 1 else len(found[(1, 0)])), (n, k)
    assert len(found[(1, 0)]) >= 4
    for kind in (lambda n, k: k == 0, lambda n, k: k == n - 1, lambda n, k: k >= 4 * (n // 4)):
        combos = {(a, b, n % 4) for (n, k), v in found.items() if kind(n, k) and n > 1 for a, b in v}
        assert len(combos) == (64 if kind(4, 3) or kind(4, 0) else 48)  # a tail exists for n % 4 in 1, 2, 3
    assert any(t.data[a + n - 1] >= 0x80 for a, _, n, _ in t.marks)


def test_lastbyte_chain_covers_every_alignment():
    """(window offset & 3, heap offset & 3, length & 3) of a pair that differs in its last byte only, the first in the
    heap and the second in a later window, with the probe certain to pass the first one's slot: replayed here from
    the windows and the constructed terms."""
    t = ns.dict_lastbyte_chain()
    wins = t.windows()
    heap_off = np.concatenate([[0], np.cumsum([len(x) for x in t.terms])])
    sim, v, state = ns.TableSim(ns.DICT_SLOTS), 0, {}
    for k, v1 in enumerate(t.terms_at_cut):
        state[k] = sim.copy()  # the table the lookups of window k see
        sim.add_window([ns.nt_hash(x) for x in t.terms[v:v1]])
        v = v1
    assert sim.growths >= 3
    seen = set()
    for ix, iy, k, w, h, l in t.marks:
        x, y = t.terms[ix], t.terms[iy]
        assert len(x) == len(y) and x[:-1] == y[:-1] and x[-1] != y[-1]
        assert t.terms_at_cut[k - 1] == iy and t.terms_at_cut[k] == iy + 1 and ix == iy - 1  # each alone in its window
        assert wins[k].find(y) == w and heap_off[ix] % 4 == h and len(x) % 4 == l
        assert state[k].meets(ns.nt_hash(y), ns.nt_hash(x))
        seen.add((w, h, l))
    assert seen == {(w, h, l) for w in range(4) for h in range(4) for l in range(4)}


def test_heap_windows_cover_every_alignment():
    t = SMALL["heap_align"]
    lens = [len(x) for x in t.terms]
    seen, no_new, v = set(), 0, 0
    for v1 in t.terms_at_cut:
        if v1 == v:
            no_new += 1
        elif v:
            seen.add((sum(lens[:v]) % 4, sum(lens[v:v1])))
        v = v1
    assert {(h, n) for h in range(4) for n in range(1, 9)} <= seen and no_new >= 32
    for k, name in enumerate(("only", "first", "middle", "last")):
        t = SMALL[f"heap_empty_{name}"]
        a, b = t.terms_at_cut[0], t.terms_at_cut[1]
        new = t.terms[a:b]
        assert sum(len(x) for x in t.terms[:a]) % 4 == (k + 1) % 4
        assert len(new) == (1 if name == "only" else 3) and new[(0, 0, 1, 2)[k]] == b"" and new.count(b"") == 1
    sim, v = ns.TableSim(ns.DICT_SLOTS), 0
    t, growths = SMALL["heap_slots"], []
    for v1 in t.terms_at_cut:
        sim.add_window([ns.nt_hash(x) for x in t.terms[v:v1]])
        growths.append(sim.growths)
        v = v1
    assert growths == [0, 1, 1] and sim.slots == 32


def test_first_appearance_at_block_edges():
    t = SMALL["dict_first_appearance"]
    for name in (b"<new1>", b"<new2>"):
        i = t.terms.index(name)
        first = int(np.flatnonzero(t.o == i)[0])
        assert first % ns.BLOCK_LINES == ns.BLOCK_LINES - 1  # the object of a block's last line
        assert not (t.s[:first + 1] == i).any() and not (t.p[:first + 1] == i).any() and t.s[first + 1] == i
