"""The dataset statistics on the device (rdfind_amd/csrc/histo.inl): rdf_condition_histogram, rdf_join_histogram and
rdf_count_literals against the CPU reference (tests/histo_ref.py, pinned by tests/test_histo_ref.py), with exact
equality everywhere, and the drivers that print them (--create-join-histogram, rdfind_amd.count).

The three calls take one path at every size, so there are no forced paths to prove.  RDF_BLOCK is 256 and a wave 64:
the shapes below put runs of equal keys across several blocks and end runs exactly at those boundaries.

The driver tests run at --support 10, and also at the support of a fixture's ``*_clean`` golden where that is another
one (zipf_small 3, skew_small 2), because only at the golden's support can the CIND lines be compared with it."""
import gzip
import io
import os
import random

import numpy as np
import pytest

from rdfind_amd import _lib, count, ntriples, program
from tests import histo_ref
from tests.conftest import GOLDEN
from tests.test_histo_ref import HAND, HAND_CONDITIONS
from tests.test_oracle import golden_triples, read_golden

pytestmark = pytest.mark.gpu

RDF_ERR_STATE = -4
FIXTURES = ("lubm_small", "zipf_small", "skew_small")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def rows(a):
    return [tuple(r) for r in a.tolist()]


def load(g, triples, num_terms):
    arr = np.array(triples, dtype=np.uint32).reshape(-1, 3)
    g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], num_terms)


def check_all(g, triples, num_terms, supports=(1, 2), projections=("spo",), ars=(False,)):
    """Condition histogram, no-FIS join histogram and the FIS one at every given support, rules on / off."""
    load(g, triples, num_terms)
    assert rows(g.condition_histogram()) == histo_ref.condition_histogram(triples)
    for proj in projections:
        exp = histo_ref.join_rows(triples, 1, proj, use_fis=False)
        assert rows(g.join_histogram(proj, use_fis=False)) == exp, (len(triples), proj)
        assert g.join_lines == sum(t for _, _, t in exp)
        for ms in supports:
            for use_ars in ars:
                g.frequent_conditions(ms)
                if use_ars:
                    g.association_rules()
                exp = histo_ref.join_rows(triples, ms, proj, True, use_ars)
                assert rows(g.join_histogram(proj)) == exp, (len(triples), proj, ms, use_ars)
                assert g.join_lines == sum(t for _, _, t in exp)


def test_hand_example(ctx):
    load(ctx, HAND, 6)
    assert rows(ctx.condition_histogram()) == HAND_CONDITIONS
    assert rows(ctx.join_histogram("spo", use_fis=False)) == [(0, 2, 3), (0, 4, 3)]
    assert ctx.join_lines == 6
    ctx.frequent_conditions(2)
    assert rows(ctx.join_histogram("spo")) == [(0, 1, 2), (0, 2, 4)]
    assert ctx.join_lines == 6
    assert rows(ctx.join_histogram("o")) == [(0, 1, 1), (0, 2, 1)]
    assert ctx.join_lines == 2
    ctx.frequent_conditions(1)
    assert rows(ctx.join_histogram("spo")) == [(0, 2, 3), (0, 4, 3)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_edge_sizes(ctx, n):
    distinct = [(3 * i, 3 * i + 1, 3 * i + 2) for i in range(n)]
    check_all(ctx, distinct, 3 * n)
    if n == 0:
        assert ctx.join_lines == 0 and len(ctx.copy_histogram()) == 0
    same = [(0, 0, 0)] * n
    check_all(ctx, same, 1, supports=(1, n + 1))
    if n:  # one condition of every kind, n times; one join value with the three projections' two captures each
        assert rows(ctx.condition_histogram()) == [(0, n, 6)] + [(k, n, 1) for k in range(1, 7)]
        assert rows(ctx.join_histogram("spo", use_fis=False)) == [(0, 6, 1)]


def test_run_over_several_blocks(ctx):
    n = 3 * 256 + 1
    tr = [(10 + i, 0, 10 + n + i) for i in range(n)]
    check_all(ctx, tr, 10 + 2 * n, supports=(1, 2, n), projections=("spo", "p"))


def test_frequency_above_2_16(ctx):
    n = 70001
    tr = [(2 + i, 0, 1) for i in range(n)]
    load(ctx, tr, n + 2)
    assert rows(ctx.condition_histogram()) == histo_ref.condition_histogram(tr)
    got = rows(ctx.join_histogram("spo", use_fis=False))
    assert got == histo_ref.join_rows(tr, 1, "spo", use_fis=False)
    assert (0, 2 * n, 2) in got  # the predicate's and the object's lines: n binary captures and n unary ones each
    ctx.frequent_conditions(2)
    assert rows(ctx.join_histogram("spo")) == histo_ref.join_rows(tr, 2, "spo")


def test_runs_end_at_wave_and_block_boundaries(ctx):
    """The sorted unary keys start with the subjects: value 0 fills sorted indices [0, 64), value 1 [64, 256); the
    sorted binary keys start with the (p, o) pairs, which do the same; the join records of the subject projection
    (two per triple) put join value 0 at [0, 128) and value 1 at [128, 512)."""
    rest = 44
    s = [0] * 64 + [1] * 192 + [10 + i for i in range(rest)]
    o = [2] * 64 + [3] * 192 + [100 + i for i in range(rest)]
    tr = [(s[i], 5, o[i]) for i in range(len(s))]
    check_all(ctx, tr, 200, supports=(1, 2, 65), projections=("spo", "s", "o"))
    # level 2: 64 conditions that occur once and 192 that occur twice give runs that end at 64 and 256 there too
    tr = [(i, 300, 400 + i) for i in range(64)] + [(500 + i // 2, 301, 700 + i // 2) for i in range(384)]
    check_all(ctx, tr, 1000, supports=(1, 2))


def test_sparse_high_ids():
    """num_terms = 2^30 - 1 with ids at both ends of the range: the keys keep every bit, and nothing is sized by the
    number of terms (a |V|-sized u32 array alone would take 4 GiB)."""
    top = (1 << 30) - 2
    ids = [0, 1, top - 1, top]
    rng = random.Random(7)
    tr = [(rng.choice(ids), rng.choice(ids), rng.choice(ids)) for _ in range(300)]
    with _lib.Context(0) as g:
        load(g, tr, top + 1)
        assert rows(g.condition_histogram()) == histo_ref.condition_histogram(tr)
        for proj in ("spo", "s", "po"):
            assert rows(g.join_histogram(proj, use_fis=False)) == histo_ref.join_rows(tr, 1, proj, use_fis=False)
        assert g.device_bytes() < 64 << 20


def test_random_parity(ctx):
    n_rows = 0
    for seed in range(20):
        rng = random.Random(1000 + seed)
        n = rng.choice((rng.randrange(1, 300), rng.randrange(300, 3001)))
        nv = rng.randrange(5, 201)
        npred = rng.randrange(1, max(nv // 3, 2))
        tr = [(rng.randrange(nv), rng.randrange(npred), rng.randrange(nv)) for _ in range(n)]
        tr += [rng.choice(tr) for _ in range(n // 10)]  # duplicate triples
        ms = (1, 2, 5)[seed % 3]
        proj = ("spo", "s", "po")[(seed // 3) % 3]
        check_all(ctx, tr, nv, supports=(ms,), projections=(proj,), ars=(False, True))
        n_rows += ctx.hist_rows
    assert n_rows > 100


def test_state_is_untouched():
    rng = random.Random(5)
    tr = [(rng.randrange(40), rng.randrange(6), rng.randrange(40)) for _ in range(1500)]
    with _lib.Context(0) as g:
        load(g, tr, 40)
        with pytest.raises(_lib.RdfError) as e:
            g.copy_histogram()  # no histogram yet
        assert e.value.status == RDF_ERR_STATE
        with pytest.raises(_lib.RdfError) as e:
            g.join_histogram("spo")  # the default mode before rdf_frequent_conditions
        assert e.value.status == RDF_ERR_STATE
        g.run(2)
        checksum, cinds, stats = g.checksum(), g.copy_cinds().tolist(), g.last_stats()
        assert cinds
        assert rows(g.condition_histogram()) == histo_ref.condition_histogram(tr)
        assert rows(g.join_histogram("spo")) == histo_ref.join_rows(tr, 2, "spo")
        assert rows(g.join_histogram("sp", use_fis=False)) == histo_ref.join_rows(tr, 1, "sp", use_fis=False)
        assert g.checksum() == checksum and g.copy_cinds().tolist() == cinds and g.last_stats() == stats
        g.discover_cinds(True, 1)  # the groups are still those of the run
        assert g.checksum() == checksum and sorted(g.copy_cinds().tolist()) == sorted(cinds)
        # between the stages, with the rules
        g.frequent_conditions(2)
        g.association_rules()
        assert rows(g.join_histogram("spo")) == histo_ref.join_rows(tr, 2, "spo", True, True)
        g.build_capture_groups("spo")
        assert rows(g.join_histogram("spo")) == histo_ref.join_rows(tr, 2, "spo", True, True)
        g.discover_cinds(True, 1)
        with_rules = g.checksum()
        assert rows(g.condition_histogram()) == histo_ref.condition_histogram(tr)
        assert g.checksum() == with_rules


LITERAL_TEXT = (b'<http://a/x> <http://p/1> "plain" .\n'
                b'<http://b/x> <http://p/1> "tagged"@en .\n'
                b'_:b1 <http://p/2> "5"^^<http://www.w3.org/2001/XMLSchema#int> .\n'
                b'<http://a/x> <http://p/2> _:b1 .\n'
                b'# a comment\n'
                b'<http://b/x> <http://p/3> "plain" .\n'
                b'<http://a/y> <http://p/3> "" .\n')
MERGING = [("m", "http://a/"), ("m", "http://b/")]  # <http://a/x> and <http://b/x> both become m:x


def _host_counts(tmp_path, text, prefixes=()):
    path = tmp_path / "ref.nt"
    path.write_bytes(text)
    s, p, o, dic = ntriples.read_triples([str(path)])
    if prefixes:
        s, p, o, dic = ntriples.shorten_dictionary(s, p, o, dic, list(prefixes))
    return sum(t.startswith('"') for t in dic.terms), dic.size


def test_count_literals(ctx, tmp_path):
    exp = _host_counts(tmp_path, LITERAL_TEXT)
    assert exp == (4, 11)
    ctx.parse_ntriples(LITERAL_TEXT)
    assert ctx.count_literals() == exp
    lines = LITERAL_TEXT.splitlines(keepends=True)
    ctx.parse_windows([b"".join(lines[:3]), b"".join(lines[3:])])
    assert ctx.count_literals() == exp
    for single in (True, False):
        if single:
            ctx.parse_ntriples(LITERAL_TEXT)
        else:
            ctx.parse_windows([b"".join(lines[:3]), b"".join(lines[3:])])
        st = ctx.rewrite_terms(MERGING)
        assert st["n_terms_after"] == st["n_terms_before"] - 1
        assert ctx.count_literals() == _host_counts(tmp_path, LITERAL_TEXT, MERGING) == (4, 10)
    load(ctx, HAND, 6)
    with pytest.raises(_lib.RdfError) as e:
        ctx.count_literals()
    assert e.value.status == RDF_ERR_STATE


# ---- drivers on the golden fixtures ----

_REF = {}


def fixture_triples(name):
    """The fixture's triples as term ids of the host parser (the reference is computed once per fixture and kept)."""
    if name not in _REF:
        s, p, o, dic = ntriples.read_triples([os.path.join(GOLDEN, f"{name}.nt.gz")])
        _REF[name] = (list(zip(s.tolist(), p.tolist(), o.tolist())), dic)
    return _REF[name]


def expected_join_lines(name, ms, use_fis=True, use_ars=False):
    key = (name, ms, use_fis, use_ars)
    if key not in _REF:
        _REF[key] = program.join_histogram_lines(
            np.array(histo_ref.join_rows(fixture_triples(name)[0], ms, "spo", use_fis, use_ars), dtype=_lib.HIST_DTYPE))
    return _REF[key]


def run_main(argv, capsys):
    capsys.readouterr()
    assert program.main(argv) == 0
    return capsys.readouterr().out.splitlines()


def supports(name):
    return sorted({10, read_golden(name, "s1_clean")[0]})


@pytest.mark.parametrize("name", FIXTURES)
def test_program_join_histogram_fis(tmp_path, capsys, name):
    inp = os.path.join(GOLDEN, f"{name}.nt.gz")
    for ms in supports(name):
        out = tmp_path / f"cinds{ms}.txt"
        base = ["--use-fis", "--clean-implied", "--support", str(ms), "--create-join-histogram"]
        printed = run_main(base + ["--output", f"file://{out}", inp], capsys)
        exp = expected_join_lines(name, ms)
        assert 30 < len(exp) and printed == exp
        gms, golden = read_golden(name, "s1_clean")
        if ms == gms:
            assert sorted(out.read_text().splitlines()) == golden
        # without --output: the histogram, then the count
        printed = run_main(base + [inp], capsys)
        assert printed[:-1] == exp and printed[-1].startswith("Detected ") and printed[-1].endswith(" CINDs.")
        if ms == gms:
            assert printed[-1] == f"Detected {len(golden)} CINDs."
        # --do-only-join prints it and nothing else; --find-only-fcs returns before it
        assert run_main(base + ["--do-only-join", inp], capsys) == exp
        assert run_main(base + ["--find-only-fcs", "1", inp], capsys) == []


@pytest.mark.parametrize("name", FIXTURES)
def test_program_join_histogram_ars(tmp_path, capsys, name):
    inp = os.path.join(GOLDEN, f"{name}.nt.gz")
    for ms in supports(name):
        out, plain = tmp_path / f"cinds{ms}.txt", tmp_path / f"plain{ms}.txt"
        base = ["--use-fis", "--use-ars", "--clean-implied", "--support", str(ms)]
        printed = run_main(base + ["--create-join-histogram", "--output", f"file://{out}", inp], capsys)
        assert printed == expected_join_lines(name, ms, True, True)
        assert run_main(base + ["--output", f"file://{plain}", inp], capsys) == []
        assert sorted(out.read_text().splitlines()) == sorted(plain.read_text().splitlines())  # the flag changes no CIND


@pytest.mark.parametrize("name", FIXTURES)
def test_program_join_histogram_strategy0_no_fis(tmp_path, capsys, name):
    inp = os.path.join(GOLDEN, f"{name}.nt.gz")
    gms, golden = read_golden(name, "s0_clean")
    for ms in sorted({10, gms}):
        out = tmp_path / f"cinds{ms}.txt"
        printed = run_main(["--traversal-strategy", "0", "--clean-implied", "--support", str(ms), "--create-join-histogram",
                            "--output", f"file://{out}", inp], capsys)
        assert printed == expected_join_lines(name, 1, use_fis=False)  # every value passes, whatever the support
        if ms == gms:
            assert sorted(out.read_text().splitlines()) == golden


def test_program_histogram_once_with_pages(tmp_path, capsys, monkeypatch):
    """The discovery that runs out of memory starts over in pages; the histogram is not printed again."""
    monkeypatch.setenv("RDFIND_TEST_OOM_DISCOVERY", "1")
    inp = os.path.join(GOLDEN, "lubm_small.nt.gz")
    out = tmp_path / "cinds.txt"
    printed = run_main(["--use-fis", "--clean-implied", "--support", "10", "--create-join-histogram", "--output",
                        f"file://{out}", inp], capsys)
    assert printed == expected_join_lines("lubm_small", 10)
    assert sorted(out.read_text().splitlines()) == read_golden("lubm_small", "s1_clean")[1]


@pytest.mark.parametrize("name", FIXTURES)
def test_count_programs(tmp_path, name):
    inp = os.path.join(GOLDEN, f"{name}.nt.gz")
    tr, dic = fixture_triples(name)
    assert len(tr) == {"lubm_small": 7830, "zipf_small": 4000, "skew_small": 1417}[name]

    def run(argv):
        out = io.StringIO()
        assert count.run(argv, out) == 0
        return out.getvalue().splitlines()
    exp = [f"{k};{c};{t}" for k, c, t in histo_ref.condition_histogram(tr)]
    assert run(["conditions", inp]) == exp
    assert run(["conditions", "--ingest-window", "65536", inp]) == exp  # several windows
    assert run(["conditions", "--distinct-triples", inp]) == \
        [f"{k};{c};{t}" for k, c, t in histo_ref.condition_histogram(sorted(set(tr)))]
    lit = sum(t.startswith('"') for t in dic.terms)
    assert run(["values", inp]) == [f"Counted {dic.size - lit} URLs and {lit} literals."]
    text = gzip.open(inp, "rb").read()
    n_lines = sum(1 for ln in text.split(b"\n")[:-1 if text.endswith(b"\n") else None] if not ln.startswith(b"#"))
    assert run(["triples", inp]) == [f"Counted {n_lines}."]
    assert n_lines >= len(tr)


def test_count_values_with_prefixes(tmp_path):
    nt, pf = tmp_path / "t.nt", tmp_path / "p.nt"
    nt.write_bytes(LITERAL_TEXT)
    pf.write_text("@prefix m: <http://a/> .\n@prefix m: <http://b/> .\n")
    prefixes = ntriples.read_prefixes([str(pf)])
    lit, terms = _host_counts(tmp_path, LITERAL_TEXT, prefixes)
    out = io.StringIO()
    assert count.run(["values", "--prefixes", str(pf), str(nt)], out) == 0
    assert out.getvalue() == f"Counted {terms - lit} URLs and {lit} literals.\n"
    assert (lit, terms) == (4, 10)
