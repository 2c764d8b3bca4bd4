"""CPU reference of the dataset statistics (rdf_condition_histogram, rdf_join_histogram): plain dictionaries over the
triples, and the oracle's frequent conditions, rules and join lines (oracle/rdfind_oracle.py)."""
from collections import Counter

from oracle import rdfind_oracle as R


def condition_histogram(triples):
    """CountConditions (ALG/programs/CountConditions.scala:192-212) as sorted rows (kind, count, times): ``times``
    distinct conditions of ``kind`` (1 s, 2 p, 4 o, 3 sp, 5 so, 6 po) occur in exactly ``count`` triples; kind 0 sums
    the six kinds.  Duplicate triples count."""
    occ = Counter()
    for s, p, o in triples:
        for key in ((1, s), (2, p), (4, o), (3, s, p), (5, s, o), (6, p, o)):
            occ[key] += 1
    hist = Counter()
    for key, c in occ.items():
        hist[(key[0], c)] += 1
        hist[(0, c)] += 1
    return sorted((k, c, t) for (k, c), t in hist.items())


def join_lines(triples, ms, projection="spo", use_fis=True, use_ars=False):
    """The oracle's join lines: with ``use_fis`` the frequent conditions at support ``ms`` (and, with ``use_ars``,
    without the rule-implied binary conditions); without it every value passes."""
    if not use_fis:
        return R.join_lines(triples, None, None, projection, False)
    uf = R.frequent_unary_conditions(triples, ms)
    bf = R.frequent_binary_conditions(triples, uf, ms)
    implied = R.ar_implied_conditions(R.association_rules(uf, bf)) if use_ars else frozenset()
    return R.join_lines(triples, uf, bf, projection, True, implied)


def join_histogram(triples, ms, projection="spo", use_fis=True, use_ars=False):
    """RDFind.scala:449-452: {join line size: number of join lines}."""
    return dict(Counter(len(line) for line in join_lines(triples, ms, projection, use_fis, use_ars).values()))


def join_rows(triples, ms, projection="spo", use_fis=True, use_ars=False):
    """join_histogram as the library's sorted rows (0, size, times)."""
    return sorted((0, k, t) for k, t in join_histogram(triples, ms, projection, use_fis, use_ars).items())
