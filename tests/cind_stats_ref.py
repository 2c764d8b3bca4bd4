"""CPU reference of the result statistics (rdf_cind_histogram / rdf_cind_stats_* / rdf_copy_top_refs), for the tests.

Works from the result's rows alone and shares no code with the device path:

* ``statistics(rows)``: rows are ``(dep_code, d1, d2, ref_code, r1, r2, support)`` with ``d2`` / ``r2`` ``None`` for
  unary captures (the oracle's comparison form, ``_lib.decoded_to_set``); the condition values may be term ids or
  term strings.  Plain Python.
* ``statistics_np(dep, ref, support, dep_code, ref_code)``: the same from arrays of external capture ids, for results
  of millions of rows.  numpy.
* ``parse_line(line)``: a ``Cind.toString`` line back into such a row (term strings).

Both return ``(hist, top)``: ``hist`` the rows ``(kind, value, times)`` ascending by (kind, value) -- kind 1: value =
dep_code << 8 | ref_code, times = CINDs; 2: value = support, times = CINDs whose dependent has it; 3: value = r,
times = dependents with exactly r refs; 4: value = d, times = captures referenced by exactly d CINDs -- and ``top``
every referenced capture with its in-degree, descending by in-degree, ties in the order of the external capture ids:
unary before binary, then by capture type in the order of the id layout, then by the condition values.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

UNARY = (10, 12, 17, 20, 33, 34)   # s[p] s[o] p[s] p[o] o[s] o[p]: the unary types in capture-id order
BINARY = (14, 21, 35)              # s[p,o] p[s,o] o[s,p]
SHAPE, SUPPORT, REFS, INDEGREE = 1, 2, 3, 4


def capture_order(cap):
    """Sort key of a capture (code, v1, v2) equal to the order of the external capture ids t * V + v | 6 V + b (b
    indexes the binary conditions sorted by (type, v1, v2))."""
    code, v1, v2 = cap
    if v2 is None:
        return (0, UNARY.index(code), v1)
    return (1, BINARY.index(code), v1, v2)


def statistics(rows):
    shape, support, nref, indeg = Counter(), Counter(), Counter(), Counter()
    for dc, d1, d2, rc, r1, r2, sup in rows:
        shape[(dc << 8) | rc] += 1
        support[sup] += 1
        nref[(dc, d1, d2)] += 1
        indeg[(rc, r1, r2)] += 1
    hist = [(SHAPE, v, t) for v, t in sorted(shape.items())]
    hist += [(SUPPORT, v, t) for v, t in sorted(support.items())]
    hist += [(REFS, v, t) for v, t in sorted(Counter(nref.values()).items())]
    hist += [(INDEGREE, v, t) for v, t in sorted(Counter(indeg.values()).items())]
    top = sorted(indeg.items(), key=lambda kv: (-kv[1], capture_order(kv[0])))
    return hist, top


def statistics_np(dep, ref, support, dep_code, ref_code):
    """dep / ref: external capture ids per row, support: the dependent's support per row, dep_code / ref_code: the
    capture codes per row.  ``top`` holds (external capture id, in-degree)."""
    def counted(kind, values):
        v, t = np.unique(values, return_counts=True)
        return [(kind, int(a), int(b)) for a, b in zip(v, t)]
    hist = counted(SHAPE, (np.asarray(dep_code, np.int64) << 8) | np.asarray(ref_code, np.int64))
    hist += counted(SUPPORT, support)
    hist += counted(REFS, np.unique(dep, return_counts=True)[1])
    caps, deg = np.unique(ref, return_counts=True)
    hist += counted(INDEGREE, deg)
    order = np.lexsort((caps, -deg.astype(np.int64)))
    return hist, [(int(caps[i]), int(deg[i])) for i in order]


def _capture(text, pos):
    """One pretty-printed capture at text[pos:]: ((code, v1, v2), position behind it).  Terms are N-Triples terms:
    <iri>, "literal" with an optional @lang / ^^<type>, or a blank node label."""
    bit = {"s": 1, "p": 2, "o": 4}
    proj = bit[text[pos]]
    assert text[pos + 1] == "[", text
    pos += 2
    conds, values = [], []
    while True:
        conds.append(bit[text[pos]])
        assert text[pos + 1] == "=", text
        pos += 2
        start = pos
        if text[pos] == "<":
            pos = text.index(">", pos) + 1
        elif text[pos] == '"':
            pos += 1
            while text[pos] != '"':
                pos += 2 if text[pos] == "\\" else 1
            pos += 1
            if text.startswith("^^<", pos):
                pos = text.index(">", pos) + 1
            elif text[pos] == "@":
                while text[pos] not in ",]":
                    pos += 1
        else:
            while text[pos] not in ",]":
                pos += 1
        values.append(text[start:pos])
        if text[pos] == "]":
            break
        assert text[pos] == ",", text
        pos += 1
    code = sum(conds) | (proj << 3)
    assert (code in UNARY and len(values) == 1) or (code in BINARY and len(values) == 2 and conds[0] < conds[1]), text
    return (code, values[0], values[1] if len(values) == 2 else None), pos + 1


def parse_line(line):
    """``dep < ref (support=n)`` -> (dep_code, d1, d2, ref_code, r1, r2, n) with term strings."""
    dep, pos = _capture(line, 0)
    assert line.startswith(" < ", pos), line
    ref, pos = _capture(line, pos + 3)
    assert line.startswith(" (support=", pos) and line.endswith(")"), line
    return dep + ref + (int(line[pos + len(" (support="):-1]),)
