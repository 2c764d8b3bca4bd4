"""The CPU reference of the result selection (tests/select_ref.py) on hand-derived cases, and the driver's pattern parser
(program.parse_capture_pattern, pure host code): round trips through codes.pretty_print, every meaning of the grammar,
its errors, and the golden CIND lines as fixtures."""
import gzip
import os

import pytest

from rdfind_amd import _lib, codes, program
from tests import cind_stats_ref, select_ref as ref
from tests.conftest import GOLDEN

ANY = ref.ANY
IDX = {c: i for i, c in enumerate(ref.CODES)}


def bit(*cs):
    return sum(1 << IDX[c] for c in cs)


# s[p=1] < s[p=2], s[p=1] < s[p=1,o=7], o[s=3,p=1] < o[p=1], p[o=7] < p[s=3], s[o=7] < s[p=2] (supports 2, 2, 5, 9, 9)
ROWS = {
    (10, 1, None, 10, 2, None, 2),
    (10, 1, None, 14, 1, 7, 2),
    (35, 3, 1, 34, 1, None, 5),
    (20, 7, None, 17, 3, None, 9),
    (12, 7, None, 10, 2, None, 9),
}


def test_reference_hand_cases():
    assert ref.select(ROWS) == ROWS  # the empty query
    assert ref.select(ROWS, dep=[ref.exact(10, 1)]) == {(10, 1, None, 10, 2, None, 2), (10, 1, None, 14, 1, 7, 2)}
    assert ref.select(ROWS, ref=[ref.exact(10, 2)]) == {(10, 1, None, 10, 2, None, 2), (12, 7, None, 10, 2, None, 9)}
    assert ref.select(ROWS, dep=[ref.exact(10, 1)], ref=[ref.exact(10, 2)]) == {(10, 1, None, 10, 2, None, 2)}
    assert ref.select(ROWS, lo=5) == {r for r in ROWS if r[6] >= 5}
    assert ref.select(ROWS, lo=3, hi=5) == {(35, 3, 1, 34, 1, None, 5)}
    assert ref.select(ROWS, lo=10) == set()
    # any of several patterns on a side
    assert ref.select(ROWS, dep=[ref.exact(12, 7), ref.exact(20, 7)]) == {r for r in ROWS if r[6] == 9}
    # a code only; a value in either slot; value2 set never matches a unary capture
    assert ref.select(ROWS, dep=[(bit(10), ANY, ANY)]) == {r for r in ROWS if r[0] == 10}
    assert ref.select(ROWS, ref=[(ref.ALL_CODES, 1, ANY), (bit(14, 21, 35), ANY, 1)]) == \
        {(10, 1, None, 14, 1, 7, 2), (35, 3, 1, 34, 1, None, 5)}
    assert ref.select(ROWS, dep=[(ref.ALL_CODES, ANY, 1)]) == {(35, 3, 1, 34, 1, None, 5)}
    assert ref.select(ROWS, dep=[(ref.ALL_CODES, ANY, 7)]) == set()  # 7 is a first value only, of unary captures
    assert ref.select(ROWS, dep=[(0, ANY, ANY)]) == set()  # no code admitted
    assert ref.select(ROWS, dep=[(ref.ALL_CODES, None, None)]) == ROWS  # None stands for ANY
    assert ref.exact(14, 1, 7) == (bit(14), 1, 7) and ref.exact(10, 1) == (bit(10), 1, ANY)
    assert ref.CODES == _lib.SEL_CODES == tuple(sorted(codes.ALL_CODES)) and ANY == _lib.RDF_SEL_ANY


NASTY = ['<http://example.org/a,b]c=d*e>', '"a, b] c=d * \\" e\\\\"', '"x=]"@en', '"1,5"^^<http://www.w3.org/2001/XMLSchema#decimal>',
         '"]"@en-US', '<*>', '"*"', '_:b0', '"tab\\tquote\\""^^<http://t/x,y]>']


def captures():
    for code in codes.ALL_CODES:
        for i, v1 in enumerate(NASTY):
            yield code, v1, (NASTY[(i + 3) % len(NASTY)] if codes.is_binary(code) else None)


def test_parser_round_trip():
    """Every string codes.pretty_print produces parses to one pattern that matches exactly that capture."""
    seen = set()
    for code, v1, v2 in captures():
        text = codes.pretty_print(code, v1, v2)
        spec = program.parse_capture_pattern(text)
        assert spec == [(1 << IDX[code], v1, v2)], text
        seen.add(code)
        pats = [(m, ANY if a is None else a, ANY if b is None else b) for m, a, b in spec]
        for c2, w1, w2 in captures():
            assert ref.matches_any(pats, c2, w1, w2) == ((c2, w1, w2) == (code, v1, v2)), (text, c2, w1, w2)
    assert seen == set(ref.CODES)


def test_pattern_meanings():
    T, U = "<http://t>", '"u"@en'
    P = program.parse_capture_pattern
    assert P(f"s[p={T}]") == [(bit(10), T, None)]  # exactly that unary capture
    assert P(f"s[p={T},o=*]") == [(bit(14), T, None)]  # the binary captures with p = T
    assert P(f"s[p=*,o={U}]") == [(bit(14), None, U)]
    assert P(f"o[s={T},p={U}]") == [(bit(35), T, U)]
    assert P("s[p=*]") == [(bit(10), None, None)]  # a code only
    assert P("p[s=*,o=*]") == [(bit(21), None, None)]
    assert P(f"*[s={T},o={U}]") == [(bit(21), T, U)]  # two conditions leave one projection
    # every capture that has the condition p = T: unary s[p] o[p]; binary s[p,o] (first slot) and o[s,p] (second)
    assert P(f"*[p={T}]") == [(bit(10, 34), T, None), (bit(14), T, None), (bit(35), None, T)]
    assert P(f"*[s={T}]") == [(bit(17, 33), T, None), (bit(21, 35), T, None)]
    assert P(f"*[o={T}]") == [(bit(12, 20), T, None), (bit(14, 21), None, T)]
    # a bare term: every capture that names it as a condition value
    assert P(T) == [(ref.ALL_CODES, T, None), (bit(14, 21, 35), None, T)]
    assert P(U) == [(ref.ALL_CODES, U, None), (bit(14, 21, 35), None, U)]
    assert P("_:b1") == [(ref.ALL_CODES, "_:b1", None), (bit(14, 21, 35), None, "_:b1")]
    # a bare token ends before the next , or ]
    assert P("s[p=_:b1,o=x]") == [(bit(14), "_:b1", "x")]


def test_pattern_expansion_against_the_reference():
    """The parsed alternatives, read as reference patterns, select what the grammar says."""
    t = {1: "<p1>", 2: "<p2>", 3: "<s3>", 7: '"seven"'}
    ROWS_T = {(dc, t[d1], None if d2 is None else t[d2], rc, t[r1], None if r2 is None else t[r2], s)
              for dc, d1, d2, rc, r1, r2, s in ROWS}

    def sel(text, **kw):
        pats = [(m, ANY if a is None else a, ANY if b is None else b) for m, a, b in program.parse_capture_pattern(text)]
        return ref.select(ROWS_T, **{k: pats for k in kw})
    assert len(sel("*[p=<p1>]", dep=1)) == 3 and len(sel("*[p=<p1>]", ref=1)) == 2
    assert sel('"seven"', ref=1) == {r for r in ROWS_T if r[3] == 14}
    assert len(sel('"seven"', dep=1)) == 2
    assert sel("s[p=<p1>]", dep=1) == {r for r in ROWS_T if r[0] == 10}
    assert sel("s[p=<p1>,o=*]", ref=1) == {r for r in ROWS_T if r[3] == 14}
    assert sel("s[p=<p1>,o=*]", dep=1) == set()


@pytest.mark.parametrize("text", [
    "s[o=<a>,p=<b>]",      # attribute order
    "s[p=<a>,p=<b>]",      # attributes not distinct
    "s[s=<a>]",            # attribute == projection
    "p[s=<a>,p=<b>]",
    "o[s=<a>,o=<b>]",
    "s[p=<a>",             # no closing bracket
    "s[p=<a>]x",           # trailing text
    "s[p=<a>,o=<b>,s=<c>]",
    "s[q=<a>]",
    "s[p=]",
    "s[p=<a]",
    's[p="a]',
    "s[]",
    "",
])
def test_pattern_errors(text):
    with pytest.raises(ValueError):
        program.parse_capture_pattern(text)


def test_support_range():
    assert program.parse_support_range(None) == (0, ANY)
    assert program.parse_support_range("5") == (5, ANY)
    assert program.parse_support_range("5:9") == (5, 9) and program.parse_support_range("7:7") == (7, 7)
    for bad in ("9:5", "-1", "a", "1:b", "1:2:3"):
        with pytest.raises(ValueError):
            program.parse_support_range(bad)


def test_resolve_patterns():
    ids = {"<a>": 4, "<gone>": codes.UINT32_NONE}
    P = program.parse_capture_pattern
    assert program.resolve_patterns([], ids) == []
    assert program.resolve_patterns([P("s[p=<a>]"), P("s[o=*]")], ids) == [(bit(10), 4, ANY), (bit(12), ANY, ANY)]
    # a term the dictionary lacks: its alternatives are dropped; a side that loses every pattern matches nothing
    assert program.resolve_patterns([P("s[p=<a>]"), P("<gone>")], ids) == [(bit(10), 4, ANY)]
    assert program.resolve_patterns([P("<gone>")], ids) == [(0, ANY, ANY)]
    assert ref.select(ROWS, dep=program.resolve_patterns([P("<gone>")], ids)) == set()
    with pytest.raises(ValueError):
        program.resolve_patterns([P("<a>")] * 129, ids)  # 258 alternatives on one side


@pytest.mark.parametrize("name", ["lubm_small", "skew_small", "zipf_small"])
def test_golden_lines_split_and_parse(name):
    """Every golden line has exactly one " < ", so a host split into (dep, ref, support) is unambiguous; both halves
    parse to the exact pattern of the capture the statistics reference's own line parser reads."""
    with gzip.open(os.path.join(GOLDEN, f"{name}.s1_clean.txt.gz"), "rt", encoding="utf-8") as f:
        f.readline()
        lines = [ln.rstrip("\n") for ln in f]
    assert len(lines) > 50
    for ln in lines:
        assert ln.count(" < ") == 1, ln
        dep, rest = ln.split(" < ")
        rf, sup = rest.rsplit(" (support=", 1)
        dc, d1, d2, rc, r1, r2, n = cind_stats_ref.parse_line(ln)
        assert int(sup[:-1]) == n
        assert program.parse_capture_pattern(dep) == [(1 << IDX[dc], d1, d2)], ln
        assert program.parse_capture_pattern(rf) == [(1 << IDX[rc], r1, r2)], ln
