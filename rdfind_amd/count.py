"""``python -m rdfind_amd.count {conditions,values,triples} [flags] input.nt ...``: the reference's counting programs.

  conditions  CountConditions (ALG/programs/CountConditions.scala:192-212): ``{kind};{count};{times}`` lines = ``times``
              distinct conditions of ``kind`` (1 s, 2 p, 4 o, 3 sp, 5 so, 6 po; 0 all six) occur in exactly ``count``
              triples, sorted by (kind, count) (Flink's print order is unspecified).  ``--distinct-triples`` acts first.
  values      CountDistinctValues (ALG/programs/CountDistinctValues.scala:112-119): the distinct terms that start with
              ``"`` are the literals, the others the URLs.
  triples     CountTriples (ALG/programs/CountTriples.scala:57-65): the input lines that do not start with ``#``; blank
              lines count.  Host only: no GPU is touched.

``conditions`` and ``values`` ingest exactly as the main driver does (device parse, windows of whole lines, one
``rdf_rewrite_terms`` for ``--prefixes``) and count on the device (rdf_condition_histogram, rdf_count_literals).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import ntriples


def build_parser():
    ap = argparse.ArgumentParser(prog="rdfind-count", description="dataset statistics of RDF inputs (MI355X)")
    ap.add_argument("what", choices=("conditions", "values", "triples"), help="what to count")
    ap.add_argument("inputs", nargs="+", help="input files to process")
    ap.add_argument("--tabs", action="store_true", help="if input file is tab-separated")
    ap.add_argument("--prefixes", action="append", default=None,
                    help="a list of nt-prefix files to apply on the input triple (repeatable or comma-separated)")
    ap.add_argument("--distinct-triples", action="store_true", help="whether to ensure that triples are distinct")
    ap.add_argument("--ingest-window", type=int, default=1 << 30, metavar="BYTES",
                    help="an input larger than this is parsed on the device in windows of whole lines of at most this "
                         "many bytes")
    ap.add_argument("--device", type=int, default=0)
    return ap


def count_lines(chunks) -> int:
    """Lines of the byte stream ``chunks`` (split at ``\\n`` wherever the chunks end; nothing after a final ``\\n`` is a
    line, an unterminated last line is one) that do not start with ``#``.  Blank lines count."""
    total = 0
    open_line = False  # the last chunk ended inside a line
    for chunk in chunks:
        a = np.frombuffer(chunk, np.uint8)
        if not a.size:
            continue
        starts = np.flatnonzero(a == 10) + 1
        if not open_line:
            starts = np.concatenate([[0], starts])
        starts = starts[starts < a.size]
        total += int((a[starts] != 35).sum())
        open_line = a[-1] != 10
    return total


def condition_lines(rows):
    """``{kind};{count};{times}`` of rdf_hist_row rows (already sorted by kind, count)."""
    return [f"{k};{c};{t}" for k, c, t in rows.tolist()]


def run(argv, out=None):
    a = build_parser().parse_args(argv)
    out = sys.stdout if out is None else out
    paths = ntriples.resolve_paths(a.inputs)
    if not paths:
        raise ValueError("no input files")
    if a.what == "triples":
        print(f"Counted {count_lines(ntriples.iter_windows(paths, a.ingest_window))}.", file=out)
        return 0
    from . import _lib
    from .program import device_ingest
    with _lib.Context(a.device) as ctx:
        device_ingest(ctx, paths, a.tabs, a.ingest_window)
        if a.prefixes:
            files = [x for arg in a.prefixes for x in arg.split(",") if x]
            ctx.rewrite_terms(ntriples.read_prefixes(files))
        if a.what == "values":
            literals, terms = ctx.count_literals()
            print(f"Counted {terms - literals} URLs and {literals} literals.", file=out)
            return 0
        if a.distinct_triples:
            ctx.distinct_triples()
        for ln in condition_lines(ctx.condition_histogram()):
            print(ln, file=out)
    return 0


def main(argv=None):
    return run(sys.argv[1:] if argv is None else argv)


if __name__ == "__main__":
    sys.exit(main())
