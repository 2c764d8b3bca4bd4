"""The CPU reference of the dataset statistics (tests/histo_ref.py) pinned on a hand-derived example, and the host
parts of the feature: the driver's flag check, ``rdfind_amd.count triples`` and the count programs' argument parser."""
import io

import numpy as np
import pytest

from rdfind_amd import _lib, count, program
from tests import histo_ref

# terms a, b, p, q, x, y
A, B, P, Q, X, Y = range(6)
HAND = [(A, P, X), (B, P, X), (A, Q, Y)]
# s: a twice, b once; p: p twice, q once; o: x twice, y once; (p, x) twice, (q, y) once; every sp and so pair once
HAND_CONDITIONS = [(0, 1, 10), (0, 2, 4), (1, 1, 1), (1, 2, 1), (2, 1, 1), (2, 2, 1), (3, 1, 3), (4, 1, 1), (4, 2, 1),
                   (5, 1, 3), (6, 1, 1), (6, 2, 1)]


def test_hand_conditions():
    assert histo_ref.condition_histogram(HAND) == HAND_CONDITIONS
    assert histo_ref.condition_histogram([]) == []


def test_hand_join_no_fis():
    # b, q, y each join one triple in one position: 2 conditions; a, p, x two triples that share the always-emitted
    # unary's value or not: a {s[p=p,o=x], s[p=p], s[p=q,o=y], s[p=q]} = 4, likewise p and x
    assert histo_ref.join_histogram(HAND, 1, "spo", use_fis=False) == {2: 3, 4: 3}


def test_hand_join_fis():
    # ms = 2: frequent s=a, p=p, o=x, (p, x).  a: s[p=p,o=x] and s[p=p] (K3's form would add s[o=x]); b the same two;
    # p: p[s=a], p[o=x] (the pair (a, x) is not frequent); x: o[s=a], o[p=p]; q: p[s=a]; y: o[s=a]
    assert histo_ref.join_histogram(HAND, 2, "spo") == {1: 2, 2: 4}
    lines = histo_ref.join_lines(HAND, 2, "spo")
    assert len(lines[A]) == 2 and {c.v2 for c in lines[A]} == {None, X}
    assert histo_ref.join_histogram(HAND, 2, "o") == {1: 1, 2: 1}
    assert histo_ref.join_rows(HAND, 2, "o") == [(0, 1, 1), (0, 2, 1)]


def test_fis_at_support_one_is_no_fis():
    for proj in ("spo", "s", "po"):
        assert histo_ref.join_histogram(HAND, 1, proj) == histo_ref.join_histogram(HAND, 1, proj, use_fis=False)


def test_join_histogram_flag_refuses_dop(tmp_path):
    f = tmp_path / "x.nt"
    f.write_text("<a> <p> <x> .\n")
    with pytest.raises(NotImplementedError):
        program.RDFind(["--use-fis", "--create-join-histogram", "-dop", "2", str(f)])
    program.RDFind(["--use-fis", "--create-join-histogram", str(f)])  # one GPU: accepted
    rows = np.array([(0, 1, 2), (0, 4, 1)], dtype=_lib.HIST_DTYPE)
    assert program.join_histogram_lines(rows) == ["Join size 1 encountered 2x", "Join size 4 encountered 1x"]


TEXT = (b"# a comment\n<a> <p> <x> .\n\n<b> <p> \"l\" .\r\n#another\r\n   \n<a> <q> <y> .")


def _expected_lines(text):
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return sum(1 for ln in lines if not ln.startswith(b"#"))


@pytest.mark.parametrize("tail", [b"", b"\n", b"\n\n", b"\n#end", b"\n#end\n"])
def test_count_triples(tmp_path, tail):
    text = TEXT + tail
    # every way the stream may be cut into chunks gives the same count
    exp = _expected_lines(text)
    assert count.count_lines([text]) == exp
    for step in (1, 2, 3, 7):
        assert count.count_lines(text[i:i + step] for i in range(0, len(text), step)) == exp
    # through the program: the window stream ends a file without a final line break with one
    f = tmp_path / "t.nt"
    f.write_bytes(text)
    exp_file = _expected_lines(text if text.endswith(b"\n") else text + b"\n")
    for window in (1 << 30, 16):
        out = io.StringIO()
        assert count.run(["triples", "--ingest-window", str(window), str(f)], out) == 0
        assert out.getvalue() == f"Counted {exp_file}.\n"
    assert count.count_lines([]) == 0 and count.count_lines([b""]) == 0


def test_count_triples_hand():
    assert _expected_lines(TEXT) == 5  # three triples, one blank line, one line of blanks; two comments
    assert count.count_lines([TEXT + b"\n"]) == 5


def test_count_parser():
    ap = count.build_parser()
    a = ap.parse_args(["conditions", "--tabs", "--distinct-triples", "--prefixes", "p1,p2", "--prefixes", "p3",
                       "--ingest-window", "4096", "--device", "1", "a.nt", "b.nt"])
    assert (a.what, a.tabs, a.distinct_triples, a.prefixes, a.ingest_window, a.device, a.inputs) == \
        ("conditions", True, True, ["p1,p2", "p3"], 4096, 1, ["a.nt", "b.nt"])
    a = ap.parse_args(["values", "x.nt"])
    assert (a.what, a.tabs, a.distinct_triples, a.prefixes, a.ingest_window, a.device) == \
        ("values", False, False, None, 1 << 30, 0)
    for bad in (["lines", "x.nt"], ["triples"], []):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    rows = np.array([(0, 1, 10), (6, 2, 1)], dtype=_lib.HIST_DTYPE)
    assert count.condition_lines(rows) == ["0;1;10", "6;2;1"]
