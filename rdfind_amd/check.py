"""``python -m rdfind_amd.check [flags] --cinds FILE input.nt ...``: which of the CINDs listed in FILE hold in the input,
and how badly the others are violated.

FILE holds one CIND per line as ``Cind.toString`` writes it, ``dep < ref`` with an optional `` (support=n)`` (the
output of a discovery run, of this program, or hand-written); blank lines and lines starting with ``#`` are skipped.
The input is ingested exactly as ``rdfind_amd.count`` does (device parse, windows of whole lines, one
``rdf_rewrite_terms`` for ``--prefixes`` / ``--asciify-triples``), the terms of FILE are looked up in the device
dictionary (``rdf_find_terms``; a term the input lacks makes its capture empty), and ``rdf_check_cinds`` checks all
candidates at once.  A capture denotes the distinct values of its projection over the triples that match its condition;
no support threshold, association rule or minimality rule plays a part.  One line per candidate, in input order:

  holding    ``dep < ref (support=S)``                                   (again a CIND file)
  violated   ``dep !< ref (support=S, overlap=O, violations=V)``         with ``--examples K``: `` e.g. t1 t2 ...``
  empty      ``dep ?< ref (support=0)``                                  the dependent has no value: vacuous

then ``Checked M CINDs: H hold, V violated, E empty.``  One GPU.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import codes, ntriples

NONE = codes.UINT32_NONE
_ATTR_BIT = {"s": codes.SUBJECT, "p": codes.PREDICATE, "o": codes.OBJECT}
_SUPPORT = " (support="


def build_parser():
    ap = argparse.ArgumentParser(prog="rdfind-check", description="check given CINDs against RDF inputs (MI355X)")
    ap.add_argument("inputs", nargs="+", help="input files to process")
    ap.add_argument("--cinds", required=True, metavar="FILE", help="the CINDs to check, one per line ('-': standard input)")
    ap.add_argument("--examples", type=int, default=0, metavar="K",
                    help="print up to K violating values (the smallest term ids) per violated CIND, at most 16")
    ap.add_argument("--violated-only", action="store_true", help="print the violated CINDs and the summary only")
    ap.add_argument("--tabs", action="store_true", help="if input file is tab-separated")
    ap.add_argument("--prefixes", action="append", default=None,
                    help="a list of nt-prefix files to apply on the input triple (repeatable or comma-separated)")
    ap.add_argument("--asciify-triples", action="store_true", help="asciify the input triples")
    ap.add_argument("--ingest-window", type=int, default=1 << 30, metavar="BYTES",
                    help="an input larger than this is parsed on the device in windows of whole lines of at most this "
                         "many bytes")
    ap.add_argument("--device", type=int, default=0)
    return ap


def _parse_capture(text, i):
    """The capture ``PROJ[ATTR=TERM]`` or ``PROJ[ATTR=TERM,ATTR=TERM]`` starting at text[i] (what codes.pretty_print
    writes): ((code, term1, term2 or None), the index after its ``]``).  The terms end where program._pattern_term_end
    says, so a literal may hold `` < ``, ``]``, ``,`` or ``(support=1)``."""
    from .program import _pattern_term_end
    if not (i + 1 < len(text) and text[i] in _ATTR_BIT and text[i + 1] == "["):
        raise ValueError(f"expected s[, p[ or o[ at offset {i}")
    proj = _ATTR_BIT[text[i]]
    i += 2
    conds = []
    while True:
        if not (i + 1 < len(text) and text[i] in _ATTR_BIT and text[i + 1] == "="):
            raise ValueError(f"expected s=, p= or o= at offset {i}")
        attr = _ATTR_BIT[text[i]]
        i += 2
        if i >= len(text):
            raise ValueError("the line ends after '='")
        j = _pattern_term_end(text, i)
        if j == i:
            raise ValueError(f"empty condition value at offset {i}")
        conds.append((attr, text[i:j]))
        i = j
        if i < len(text) and text[i] == "," and len(conds) < 2:
            i += 1
            continue
        if i < len(text) and text[i] == "]":
            break
        raise ValueError(f"expected ',' or ']' at offset {i}")
    if len(conds) == 2 and not conds[0][0] < conds[1][0]:
        raise ValueError("the conditions of a capture must be distinct and in s < p < o order")
    code = codes.create_code(conds[0][0], conds[1][0] if len(conds) == 2 else 0, proj)
    if not codes.is_valid_standard_capture(code):
        raise ValueError("the projection of a capture is one of its condition attributes")
    return (code, conds[0][1], conds[1][1] if len(conds) == 2 else None), i + 1


def parse_cind_line(line, lineno=0):
    """One line of a CIND file: ``(dep, ref, support)`` with captures ``(code, term1, term2 or None)`` and the printed
    support or None; None for a blank line or a ``#`` comment.  The inverse of codes.format_cind.  Anything else raises
    ValueError naming ``lineno``."""
    text = line.rstrip("\r\n")
    if not text.strip() or text.startswith("#"):
        return None
    try:
        dep, i = _parse_capture(text, 0)
        if text[i:i + 3] != " < ":
            raise ValueError(f"expected ' < ' at offset {i}")
        ref, i = _parse_capture(text, i + 3)
        rest = text[i:]
        support = None
        if rest:
            digits = rest[len(_SUPPORT):-1]
            if not (rest.startswith(_SUPPORT) and rest.endswith(")") and digits.isascii() and digits.isdigit()):
                raise ValueError(f"expected the end of the line or ' (support=n)' at offset {i}")
            support = int(digits)
    except ValueError as e:
        raise ValueError(f"CIND line {lineno}: {e}: {text!r}") from None
    return dep, ref, support


def read_cinds(lines):
    """The candidates of a CIND file's lines, [(dep, ref, support)], line numbers counted from 1."""
    out = []
    for no, line in enumerate(lines, 1):
        cand = parse_cind_line(line, no)
        if cand is not None:
            out.append(cand)
    return out


def candidate_terms(cands):
    """The distinct terms the candidates name, in order of first appearance."""
    seen = {}
    for dep, ref, _ in cands:
        for _, t1, t2 in (dep, ref):
            seen.setdefault(t1, None)
            if t2 is not None:
                seen.setdefault(t2, None)
    return list(seen)


def candidate_array(cands, ids):
    """The (M, 6) uint32 array Context.check_cinds takes; ids: term -> id, UINT32_NONE for a term the dictionary lacks."""
    from ._lib import RDF_CHK_ABSENT

    def tid(t):
        return RDF_CHK_ABSENT if ids[t] == NONE else ids[t]
    arr = np.empty((len(cands), 6), dtype=np.uint32)
    for k, (dep, ref, _) in enumerate(cands):
        arr[k] = (dep[0], tid(dep[1]), NONE if dep[2] is None else tid(dep[2]),
                  ref[0], tid(ref[1]), NONE if ref[2] is None else tid(ref[2]))
    return arr


def format_checked(dep, ref, row, examples=()):
    """One output line: dep / ref as (code, term1, term2 or None), row = (dep_support, ref_support, overlap, ...),
    examples = the violating terms to show."""
    d, r = codes.pretty_print(*dep), codes.pretty_print(*ref)
    support, overlap = int(row[0]), int(row[2])
    if support == 0:
        return f"{d} ?< {r} (support=0)"
    if overlap == support:
        return f"{d} < {r} (support={support})"
    line = f"{d} !< {r} (support={support}, overlap={overlap}, violations={support - overlap})"
    if len(examples):
        line += " e.g. " + " ".join(examples)
    return line


def report_lines(cands, rows, example_ids=None, term=None, violated_only=False):
    """The program's output for candidates [(dep, ref, support)] and their rows; example_ids: (M, K) term ids padded
    with UINT32_NONE, term: ids -> strings (called once, with every id to show)."""
    n_ex = [0] * len(cands)
    names = []
    if example_ids is not None and len(cands) and example_ids.shape[1]:
        shown = example_ids != NONE
        n_ex = shown.sum(axis=1).tolist()
        names = term(example_ids[shown]) if shown.any() else []
    out, at = [], 0
    hold = violated = empty = 0
    for k, (dep, ref, _) in enumerate(cands):
        row = rows[k]
        ex = names[at:at + n_ex[k]]
        at += n_ex[k]
        if row[0] == 0:
            empty += 1
        elif row[2] == row[0]:
            hold += 1
        else:
            violated += 1
        if not violated_only or (row[0] != 0 and row[2] != row[0]):
            out.append(format_checked(dep, ref, row, ex))
    out.append(f"Checked {len(cands)} CINDs: {hold} hold, {violated} violated, {empty} empty.")
    return out


def run(argv, out=None):
    a = build_parser().parse_args(argv)
    out = sys.stdout if out is None else out
    from . import _lib
    from .program import device_ingest
    if not 0 <= a.examples <= _lib.RDF_CHK_MAX_EXAMPLES:
        raise ValueError(f"--examples {a.examples}: expected 0 .. {_lib.RDF_CHK_MAX_EXAMPLES}")
    paths = ntriples.resolve_paths(a.inputs)
    if not paths:
        raise ValueError("no input files")
    if a.cinds == "-":
        cands = read_cinds(sys.stdin)
    else:
        with open(a.cinds, encoding="utf-8", newline="\n") as f:
            cands = read_cinds(f)
    with _lib.Context(a.device) as ctx:
        device_ingest(ctx, paths, a.tabs, a.ingest_window)
        if a.prefixes or a.asciify_triples:
            files = [x for arg in (a.prefixes or []) for x in arg.split(",") if x]
            ctx.rewrite_terms(ntriples.read_prefixes(files), asciify=a.asciify_triples)
        ctx.set_dictionary_parsed()
        terms = candidate_terms(cands)
        ids = dict(zip(terms, ctx.find_terms(terms).tolist()))
        rows, ex = ctx.check_cinds(candidate_array(cands, ids), a.examples)
        lines = report_lines(cands, rows.tolist(), ex, ctx.dictionary_terms, a.violated_only)
    for ln in lines:
        print(ln, file=out)
    return 0


def main(argv=None):
    return run(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    sys.exit(main())
