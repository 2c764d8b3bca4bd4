"""The CPU reference of the CIND check (tests/check_ref.py): hand-written known answers, and every line of every
committed golden holds under it with overlap = dep_support = the printed support."""
import os

import pytest

from rdfind_amd import check as chk, ntriples
from tests import check_ref as R
from tests.conftest import GOLDEN
from tests.test_oracle import read_golden

N, A = R.NONE, R.ABSENT

# One input for all known answers (V = 8 terms).  (0, 5, 1) is there twice; (2, 5, 2) has s == o; the value 1 is an object
# in (0, 5, 1) and a subject in (1, 6, 3); 7 occurs nowhere.
#   s[p=5] = {0, 2, 4}   o[p=5] = {1, 2, 3}   s[p=6] = {1, 3}   o[p=6] = {0, 3}   s[o=3] = {1, 4}   s[p=5,o=1] = {0}
#   p[s=0] = {5}   p[o=3] = {5, 6}   p[s=0,o=1] = {5}   o[s=0] = {1}   o[s=0,p=5] = {1}
KAT_TRIPLES = [(0, 5, 1), (0, 5, 1), (2, 5, 2), (1, 6, 3), (3, 6, 0), (4, 5, 3)]
KAT_TERMS = 8
# (name, dep, ref, (dep_support, ref_support, overlap), every violating value ascending)
KATS = [
    ("binary dependent, its own unary component as ref", (14, 5, 1), (10, 5, N), (1, 3, 1), []),
    ("violated, one common value (the s == o triple's)", (10, 5, N), (34, 5, N), (3, 3, 1), [0, 4]),
    ("a subject here, an object there", (10, 6, N), (34, 5, N), (2, 3, 2), []),
    ("empty dependent", (10, 7, N), (10, 5, N), (0, 3, 0), []),
    ("empty ref", (10, 5, N), (10, 7, N), (3, 0, 0), [0, 2, 4]),
    ("absent term in the dependent", (10, A, N), (10, 5, N), (0, 3, 0), []),
    ("absent term in a binary ref", (10, 6, N), (14, 5, A), (2, 0, 0), [1, 3]),
    ("dep == ref", (10, 5, N), (10, 5, N), (3, 3, 3), []),
    ("binary in unary on the object", (35, 0, 5), (33, 0, N), (1, 1, 1), []),
    ("projection on the predicate", (20, 3, N), (17, 0, N), (2, 1, 1), [6]),
    ("a duplicate candidate", (10, 5, N), (34, 5, N), (3, 3, 1), [0, 4]),
    ("object values in subject values", (34, 6, N), (10, 5, N), (2, 3, 1), [3]),
    ("binary on the predicate", (21, 0, 1), (20, 3, N), (1, 2, 1), []),
    ("s[o] against s[p]", (12, 3, N), (10, 6, N), (2, 2, 1), [4]),
    ("both sides empty", (10, 7, N), (12, 7, N), (0, 0, 0), []),
]


def kat_expected(examples):
    """rows and example ids of KATS at `examples` example slots."""
    rows = [(sup[0], sup[1], sup[2], min(len(viol), examples)) for _, _, _, sup, viol in KATS]
    ex = [(viol[:examples] + [N] * examples)[:examples] for _, _, _, _, viol in KATS]
    return rows, ex


@pytest.mark.parametrize("examples", [0, 1, 2, 16])
def test_known_answers(examples):
    rows, ex = R.check(KAT_TRIPLES, [(d, r) for _, d, r, _, _ in KATS], examples)
    exp_rows, exp_ex = kat_expected(examples)
    for kat, row, e, er, ee in zip(KATS, rows, ex, exp_rows, exp_ex):
        assert (row, e) == (er, ee), kat[0]
    assert [R.classify(r) for r in rows] == ["holding", "violated", "holding", "empty", "violated", "empty", "violated",
                                             "holding", "holding", "violated", "violated", "violated", "holding",
                                             "violated", "empty"]


def test_index_equals_the_definition():
    """all_interpretations (one pass, what `check` uses) gives the sets of `interpretation` (the definition, one scan
    per capture) for every capture that has a value, and nothing else."""
    index = R.all_interpretations(KAT_TRIPLES)
    for capture, values in index.items():
        assert values and values == R.interpretation(KAT_TRIPLES, capture), capture
    for code in R.CODES:
        for v1 in range(KAT_TERMS):
            for v2 in (range(KAT_TERMS) if code in (14, 21, 35) else [None]):
                c = (code, v1, v2)
                assert R.interpretation(KAT_TRIPLES, c) == index.get(c, set()), c


_FIXTURE = {}


def fixture_ids(name):
    """(triples as id tuples, the dictionary, all_interpretations) of a golden fixture, read once."""
    if name not in _FIXTURE:
        s, p, o, dic = ntriples.read_triples([os.path.join(GOLDEN, f"{name}.nt.gz")])
        triples = list(zip(s.tolist(), p.tolist(), o.tolist()))
        _FIXTURE[name] = (triples, dic, R.all_interpretations(triples))
    return _FIXTURE[name]


def golden_candidates(name, mode, ids=None):
    """The golden's lines parsed: ([(dep, ref) with term ids], [printed support]); a term the ids lack is ABSENT."""
    triples, dic, _ = fixture_ids(name)
    ids = dic.ids if ids is None else ids

    def cap(c):
        return (c[0], ids.get(c[1], A), N if c[2] is None else ids.get(c[2], A))
    parsed = chk.read_cinds(read_golden(name, mode)[1])
    return [(cap(d), cap(r)) for d, r, _ in parsed], [sup for _, _, sup in parsed]


@pytest.mark.parametrize("mode", ["s1_clean", "s0_clean", "s0_raw"])
@pytest.mark.parametrize("name", ["lubm_small", "zipf_small", "skew_small"])
def test_every_golden_line_holds(name, mode):
    """The project's own outputs are exact known answers: under plain set semantics every printed CIND holds and its
    printed support is |I(dep)|."""
    _, _, index = fixture_ids(name)
    cands, printed = golden_candidates(name, mode)
    assert len(cands) == len(read_golden(name, mode)[1]) > 0
    rows, _ = R.check(None, cands, 0, index=index)
    for (dep, ref), row, sup in zip(cands, rows, printed):
        assert row[0] == row[2] == sup and row[0] > 0 and row[1] >= row[0], (dep, ref, row, sup)
