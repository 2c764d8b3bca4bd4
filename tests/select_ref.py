"""CPU reference of the result selection (rdf_select_cinds), for the tests.  Plain Python, no code shared with the
device path; it follows the definition in include/rdfind_hip.h literally.

Rows are ``(dep_code, d1, d2, ref_code, r1, r2, support)`` with ``d2`` / ``r2`` ``None`` for unary captures (the
oracle's comparison form, ``_lib.decoded_to_set``); the condition values may be term ids or term strings.  A pattern is
``(codes, value1, value2)``: ``codes`` a bit set over the capture codes 10 12 14 17 20 21 33 34 35 in ascending order,
``value1`` / ``value2`` a condition value or ``ANY`` (``None`` also stands for ANY).
"""
from __future__ import annotations

CODES = (10, 12, 14, 17, 20, 21, 33, 34, 35)
ANY = 0xFFFFFFFF
ALL_CODES = 0x1FF


def matches(pattern, code, v1, v2):
    """Whether capture (code, v1, v2 or None) matches the pattern."""
    codes, p1, p2 = pattern
    if not (codes >> CODES.index(code)) & 1:
        return False
    if p1 is not None and p1 != ANY and p1 != v1:
        return False
    if p2 is not None and p2 != ANY and (v2 is None or p2 != v2):
        return False
    return True


def matches_any(patterns, code, v1, v2):
    """A side of a query: no pattern at all admits every capture."""
    return not patterns or any(matches(p, code, v1, v2) for p in patterns)


def select(rows, dep=(), ref=(), lo=0, hi=ANY):
    """The rows whose dependent matches any of `dep`, whose referenced capture matches any of `ref` and whose support
    lies in [lo, hi], as a set."""
    return {r for r in rows
            if matches_any(dep, r[0], r[1], r[2]) and matches_any(ref, r[3], r[4], r[5]) and lo <= r[6] <= hi}


def exact(code, v1, v2=None):
    """The pattern that matches exactly the capture (code, v1, v2)."""
    return (1 << CODES.index(code), v1, ANY if v2 is None else v2)
