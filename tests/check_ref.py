"""CPU reference of the CIND check (rdf_check_cinds), for the tests.  Plain Python sets over id triples, no code shared
with the device path; it follows the definition in include/rdfind_hip.h literally.

A capture is ``(code, value1, value2)`` with ``value2`` None (or 0xFFFFFFFF) for a unary capture; a value may be
``ABSENT``, a term the dictionary lacks (such a capture is empty).  I(c) = the distinct values of c's projection
attribute over the triples that match c's condition.
"""
from __future__ import annotations

ABSENT = 0xFFFFFFFE
NONE = 0xFFFFFFFF
CODES = (10, 12, 14, 17, 20, 21, 33, 34, 35)
_POS = {1: 0, 2: 1, 4: 2}  # attribute bit -> position in a triple


def interpretation(triples, capture):
    """I(capture) as a set of term ids; triples: an iterable of (s, p, o)."""
    code, v1, v2 = capture
    if v2 == NONE:
        v2 = None
    cond, proj = code & 7, code >> 3
    attrs = [b for b in (1, 2, 4) if cond & b]  # ascending: value1 belongs to the lowest condition bit
    assert code in CODES and len(attrs) == (1 if v2 is None else 2), capture
    want = list(zip(attrs, (v1, v2)))
    return {t[_POS[proj]] for t in triples if all(t[_POS[a]] == v for a, v in want)}


def all_interpretations(triples):
    """{(code, value1, value2 or None): I(capture)} for every capture with a value: each triple adds its projection
    values to its nine captures (the same sets as `interpretation`, in one pass)."""
    out = {}
    for t in triples:
        for code in CODES:
            cond, proj = code & 7, code >> 3
            vals = [t[_POS[b]] for b in (1, 2, 4) if cond & b]
            out.setdefault((code, vals[0], vals[1] if len(vals) == 2 else None), set()).add(t[_POS[proj]])
    return out


def check(triples, cands, examples=0, index=None):
    """rows [(dep_support, ref_support, overlap, n_examples)] and the example ids [[...] * examples] (ascending, padded
    with NONE) of the candidates [(dep capture, ref capture)]; index: all_interpretations(triples), if at hand."""
    if index is None:
        index = all_interpretations([tuple(int(x) for x in t) for t in triples])
    nothing = frozenset()

    def I(c):
        return index.get((c[0], c[1], None if c[2] == NONE else c[2]), nothing)
    rows, ex = [], []
    for dep, ref in cands:
        d, r = I(tuple(dep)), I(tuple(ref))
        viol = sorted(d - r)[:examples]
        rows.append((len(d), len(r), len(d & r), len(viol)))
        ex.append(viol + [NONE] * (examples - len(viol)))
    return rows, ex


def classify(row):
    """"empty", "holding" or "violated"."""
    if row[0] == 0:
        return "empty"
    return "holding" if row[2] == row[0] else "violated"


def candidates_from_array(arr):
    """[(dep, ref)] of an (M, 6) array [dep_code, d1, d2, ref_code, r1, r2]."""
    return [((int(a[0]), int(a[1]), int(a[2])), (int(a[3]), int(a[4]), int(a[5]))) for a in arr]
