"""The CPU reference of the result statistics (tests/cind_stats_ref.py) and the driver's line formatting, without a GPU:
a hand example, the golden CIND files parsed back into rows (the four sums agree with the line count), and
``program.cind_statistics_lines`` on fixed rows."""
import numpy as np
import pytest

from rdfind_amd import codes, program
from tests import cind_stats_ref as ref
from tests.test_oracle import read_golden

# ten CINDs, written out: dependents a = s[p=1] (support 5), b = s[p=2] (5), c = o[p=1] (7), d = s[p=1,o=9] (2);
# referenced h = s[p=3] (by a, b, c, d), i = o[s=4] (by a, b), j = s[p=2,o=8] (by a, d), a (by b), b (by d)
A, B, C, D = (10, 1, None), (10, 2, None), (34, 1, None), (14, 1, 9)
H, I, J = (10, 3, None), (33, 4, None), (14, 2, 8)
HAND = [A + H + (5,), A + I + (5,), A + J + (5,), B + H + (5,), B + I + (5,), B + A + (5,), C + H + (7,), D + H + (2,),
        D + J + (2,), D + B + (2,)]
HAND_HIST = [
    (1, (10 << 8) | 10, 3), (1, (10 << 8) | 14, 1), (1, (10 << 8) | 33, 2), (1, (14 << 8) | 10, 2), (1, (14 << 8) | 14, 1),
    (1, (34 << 8) | 10, 1),
    (2, 2, 3), (2, 5, 6), (2, 7, 1),
    (3, 1, 1), (3, 3, 3),                   # c has one ref; a, b and d three each
    (4, 1, 2), (4, 2, 2), (4, 4, 1),        # a, b once; i, j twice; h four times
]
HAND_TOP = [(H, 4), (I, 2), (J, 2), (A, 1), (B, 1)]  # ties: unary before binary (i before j), then by type and value


def sums(hist):
    """(sum times of kind 1, of kind 2, sum value * times of kind 3, of kind 4)"""
    by = {k: [(v, t) for kk, v, t in hist if kk == k] for k in (1, 2, 3, 4)}
    return (sum(t for _, t in by[1]), sum(t for _, t in by[2]), sum(v * t for v, t in by[3]), sum(v * t for v, t in by[4]))


def test_hand_example():
    hist, top = ref.statistics(HAND)
    assert hist == HAND_HIST
    assert top == HAND_TOP
    assert sums(hist) == (10, 10, 10, 10)
    assert ref.statistics(reversed(HAND)) == (hist, top)  # a set: the order of the rows does not matter
    assert ref.statistics([]) == ([], [])


def test_numpy_form_agrees_with_the_plain_one():
    """statistics_np on capture ids numbered in capture order gives the same rows and the same top order."""
    caps = sorted({r[:3] for r in HAND} | {r[3:6] for r in HAND}, key=ref.capture_order)
    ident = {c: 100 + 7 * i for i, c in enumerate(caps)}
    dep = np.array([ident[r[:3]] for r in HAND], np.uint32)
    rf = np.array([ident[r[3:6]] for r in HAND], np.uint32)
    hist, top = ref.statistics_np(dep, rf, np.array([r[6] for r in HAND]), np.array([r[0] for r in HAND]),
                                  np.array([r[3] for r in HAND]))
    assert hist == HAND_HIST
    assert top == [(ident[c], n) for c, n in HAND_TOP]


def test_parse_line():
    assert ref.parse_line('o[s=<http://ex.org/e13>,p=<http://ex.org/p3>] < s[o="l2"] (support=3)') == \
        (35, "<http://ex.org/e13>", "<http://ex.org/p3>", 12, '"l2"', None, 3)
    assert ref.parse_line('p[s=<a>,o="x, y] < \\"z\\""@en] < s[p=<b>,o="1"^^<http://t>] (support=12)') == \
        (21, "<a>", '"x, y] < \\"z\\""@en', 14, "<b>", '"1"^^<http://t>', 12)
    assert ref.parse_line("s[p=_:b0] < p[o=<c>] (support=1)") == (10, "_:b0", None, 20, "<c>", None, 1)


@pytest.mark.parametrize("name", ["lubm_small", "zipf_small", "skew_small"])
@pytest.mark.parametrize("mode", ["s1_clean", "s0_clean", "s0_raw"])
def test_golden_sum_identities(name, mode):
    ms, lines = read_golden(name, mode)
    rows = [ref.parse_line(ln) for ln in lines]
    assert len(set(rows)) == len(lines) > 1000
    assert [codes.format_cind(*r) for r in rows] == lines  # the parsed rows print the lines again
    hist, top = ref.statistics(rows)
    assert sums(hist) == (len(lines),) * 4
    assert [k for k, _, _ in hist] == sorted(k for k, _, _ in hist)
    assert all(v >= ms for k, v, _ in hist if k == 2)  # a dependent's support is frequent
    assert sum(n for _, n in top) == len(lines) and [n for _, n in top] == sorted((n for _, n in top), reverse=True)
    assert len(top) == sum(t for k, _, t in hist if k == 4)
    assert {v >> 8 for k, v, _ in hist if k == 1} <= set(ref.UNARY + ref.BINARY)


def test_cind_statistics_lines():
    term = {1: "<http://ex.org/p1>", 2: "<http://ex.org/e2>", 9: '"nine"'}.__getitem__
    decode = {70: (10, 1, None), 71: (35, 2, 1), 72: (20, 9, None)}.__getitem__
    rows = [(1, (10 << 8) | 35, 12), (1, (21 << 8) | 12, 1), (2, 3, 40), (3, 5, 7), (4, 256, 1)]
    assert program.cind_statistics_lines(rows, [(70, 256), (71, 3), (72, 1)], decode, term) == [
        "CIND shape s[p] < o[s,p] encountered 12x",
        "CIND shape p[s,o] < s[o] encountered 1x",
        "CIND support 3 encountered 40x",
        "Dependents with 5 references encountered 7x",
        "Captures referenced 256 times encountered 1x",
        "Most referenced: s[p=<http://ex.org/p1>] by 256 CINDs",
        "Most referenced: o[s=<http://ex.org/e2>,p=<http://ex.org/p1>] by 3 CINDs",
        'Most referenced: p[o="nine"] by 1 CINDs',
    ]
    assert program.cind_statistics_lines([], [], decode, term) == []
    assert [program.shape_name(c) for c in ref.UNARY + ref.BINARY] == \
        ["s[p]", "s[o]", "p[s]", "p[o]", "o[s]", "o[p]", "s[p,o]", "p[s,o]", "o[s,p]"]
    with pytest.raises(ValueError):
        program.cind_statistics_lines([(5, 1, 1)], [], decode, term)


def test_flag_parsing():
    base = ["--use-fis", "x.nt"]
    assert program.RDFind(base).args.cind_statistics is None
    assert program.RDFind(base + ["--cind-statistics"]).args.cind_statistics == 10
    assert program.RDFind(["--use-fis", "--cind-statistics", "3", "x.nt"]).args.cind_statistics == 3
    with pytest.raises(NotImplementedError):
        program.RDFind(base + ["--cind-statistics", "-dop", "2"])
