"""Host side of ``python -m rdfind_amd.check``: the CIND-line parser inverts codes.format_cind, and the three output
formats."""
import itertools

import numpy as np
import pytest

from rdfind_amd import check as chk, codes

NONE = codes.UINT32_NONE

# terms that hold every separator of a CIND line
TERMS = [
    "<http://example.org/a>",
    "<http://example.org/a,b]c=d>",
    '"plain"',
    '"a < b"',
    '"]"',
    '","',
    '"s=1,p=2]"',
    '"x (support=3)"',
    '" < s[p=<u>] (support=9)"',
    '"say \\"hi\\" ] , < "',
    '"back\\\\"',
    '"bonjour"@fr',
    '"1"^^<http://www.w3.org/2001/XMLSchema#integer>',
    '"a]b"^^<http://example.org/t,u>',
    "_:b0",
    "ub:advisor",
]


def captures():
    """Every code with every term (pairs of neighbouring terms for the binary codes)."""
    out = []
    for code in codes.ALL_CODES:
        for k, t in enumerate(TERMS):
            out.append((code, t, TERMS[(k + 5) % len(TERMS)] if codes.is_binary(code) else None))
    return out


def test_parse_inverts_format_for_all_codes_and_terms():
    caps = captures()
    assert {c[0] for c in caps} == set(codes.ALL_CODES)
    for k, dep in enumerate(caps):
        ref = caps[(7 * k + 3) % len(caps)]
        line = codes.format_cind(*dep, *ref, k)
        assert chk.parse_cind_line(line, 1) == (dep, ref, k), line
        assert chk.parse_cind_line(line + "\n", 1) == (dep, ref, k)
        # without the support suffix
        bare = line[:line.rindex(" (support=")]
        assert chk.parse_cind_line(bare, 1) == (dep, ref, None), bare


def test_blank_and_comment_lines_are_skipped():
    assert chk.parse_cind_line("", 1) is None
    assert chk.parse_cind_line("   \n", 1) is None
    assert chk.parse_cind_line("# s[p=<a>] < s[p=<b>]\n", 1) is None
    lines = ["# header", "", "s[p=<a>] < o[p=<b>] (support=4)", "\n", "o[s=<a>,p=<b>] < o[s=<a>]"]
    assert chk.read_cinds(lines) == [((10, "<a>", None), (34, "<b>", None), 4), ((35, "<a>", "<b>"), (33, "<a>", None), None)]


@pytest.mark.parametrize("bad", [
    "garbage",
    "s[p=<a>]",
    "s[p=<a>] < ",
    "s[p=<a>] <= o[p=<b>]",
    "s[p=<a>] < o[p=<b>] trailing",
    "s[p=<a>] < o[p=<b>] (support=x)",
    "s[p=<a>] < o[p=<b>] (support=3",
    "s[p=<a>] < o[p=<b>] (support=)",
    "s[s=<a>] < o[p=<b>]",
    "s[o=<a>,p=<b>] < o[p=<b>]",
    "s[p=<a>,o=<b>,s=<c>] < o[p=<b>]",
    "x[p=<a>] < o[p=<b>]",
    "s[p=<a] < o[p=<b>]",
    's[p="open] < o[p=<b>]',
    "s[p=] < o[p=<b>]",
    " s[p=<a>] < o[p=<b>]",
])
def test_garbage_is_rejected_with_the_line_number(bad):
    with pytest.raises(ValueError, match="CIND line 7"):
        chk.parse_cind_line(bad, 7)
    with pytest.raises(ValueError, match="CIND line 3"):
        chk.read_cinds(["s[p=<a>] < o[p=<b>]", "# fine", bad])


def test_candidate_array_and_terms():
    cands = chk.read_cinds(["s[p=<a>] < o[p=<b>] (support=4)", "o[s=<a>,p=<zz>] < o[s=<b>]"])
    assert chk.candidate_terms(cands) == ["<a>", "<b>", "<zz>"]
    arr = chk.candidate_array(cands, {"<a>": 3, "<b>": 0, "<zz>": NONE})
    assert arr.dtype == np.uint32
    assert arr.tolist() == [[10, 3, NONE, 34, 0, NONE], [35, 3, 0xFFFFFFFE, 33, 0, NONE]]


def test_output_formats():
    dep, ref = (10, "<a>", None), (35, "<b>", '"c < d"')
    hold = chk.format_checked(dep, ref, (4, 9, 4, 0))
    assert hold == codes.format_cind(*dep, *ref, 4) == 's[p=<a>] < o[s=<b>,p="c < d"] (support=4)'
    assert chk.parse_cind_line(hold, 1) == (dep, ref, 4)  # the holding lines are again a CIND file
    assert chk.format_checked(dep, ref, (4, 9, 1, 2)) == 's[p=<a>] !< o[s=<b>,p="c < d"] (support=4, overlap=1, violations=3)'
    assert chk.format_checked(dep, ref, (4, 9, 1, 2), ["<x>", '"y z"']) == \
        's[p=<a>] !< o[s=<b>,p="c < d"] (support=4, overlap=1, violations=3) e.g. <x> "y z"'
    assert chk.format_checked(dep, ref, (0, 9, 0, 0)) == 's[p=<a>] ?< o[s=<b>,p="c < d"] (support=0)'


def test_report_lines():
    cands = [((10, "<a>", None), (10, "<b>", None), 4), ((12, "<a>", None), (10, "<b>", None), None),
             ((17, "<a>", None), (20, "<b>", None), 1), ((10, "<a>", None), (10, "<c>", None), 4)]
    rows = [(4, 5, 4, 0), (3, 5, 1, 2), (0, 2, 0, 0), (4, 1, 0, 1)]
    ex = np.array([[NONE, NONE], [7, 9], [NONE, NONE], [2, NONE]], np.uint32)
    asked = []

    def term(ids):
        asked.append(list(ids))
        return [f"<t{i}>" for i in ids]
    lines = chk.report_lines(cands, rows, ex, term)
    assert asked == [[7, 9, 2]]  # one dictionary call
    assert lines == ["s[p=<a>] < s[p=<b>] (support=4)",
                     "s[o=<a>] !< s[p=<b>] (support=3, overlap=1, violations=2) e.g. <t7> <t9>",
                     "p[s=<a>] ?< p[o=<b>] (support=0)",
                     "s[p=<a>] !< s[p=<c>] (support=4, overlap=0, violations=4) e.g. <t2>",
                     "Checked 4 CINDs: 1 hold, 2 violated, 1 empty."]
    assert chk.report_lines(cands, rows, None, None, violated_only=True) == [
        "s[o=<a>] !< s[p=<b>] (support=3, overlap=1, violations=2)",
        "s[p=<a>] !< s[p=<c>] (support=4, overlap=0, violations=4)",
        "Checked 4 CINDs: 1 hold, 2 violated, 1 empty."]
    assert chk.report_lines([], [], np.zeros((0, 3), np.uint32), term) == ["Checked 0 CINDs: 0 hold, 0 violated, 0 empty."]
    assert list(itertools.chain(*asked)) == [7, 9, 2]
