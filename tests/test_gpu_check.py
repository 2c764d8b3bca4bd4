"""rdf_check_cinds on the GPU against the plain-set reference (tests/check_ref.py): rows and examples must be equal
exactly.  Random candidates over all nine codes, the hand-written known answers, the work-item chunk boundaries, both
table paths, batches, errors and state, and ``python -m rdfind_amd.check`` on the golden fixtures."""
import gzip
import io
import os
import random

import numpy as np
import pytest

from rdfind_amd import _lib, check as chk, ntriples
from tests import check_ref as R
from tests.conftest import GOLDEN
from tests.test_check_ref import KAT_TERMS, KAT_TRIPLES, KATS, kat_expected
from tests.test_oracle import read_golden

pytestmark = pytest.mark.gpu

N, A = R.NONE, R.ABSENT
ERR_ARG, ERR_OOM, ERR_STATE, ERR_LIMIT = -1, -3, -4, -5


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def raises_status(status, call):
    with pytest.raises(_lib.RdfError) as e:
        call()
    assert e.value.status == status, e.value
    return e.value


def cand_array(cands):
    return np.array([list(d) + list(r) for d, r in cands], dtype=np.uint32).reshape(-1, 6)


def set_triples(g, triples, nv):
    arr = np.array(triples, dtype=np.uint32).reshape(-1, 3)
    g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)


def device_check(g, cands, examples):
    rows, ex = g.check_cinds(cand_array(cands), examples)
    assert ex.shape == (len(cands), examples)
    return [tuple(r) for r in rows.tolist()], ex.tolist()


def assert_parity(g, triples, cands, examples, index=None):
    """The device's rows, examples and class counts equal the reference's; returns the rows."""
    rows, ex = device_check(g, cands, examples)
    exp_rows, exp_ex = R.check(triples, cands, examples, index=index)
    bad = [(k, cands[k], rows[k], exp_rows[k]) for k in range(len(cands)) if rows[k] != exp_rows[k]]
    assert not bad, bad[:5]
    bad = [(k, cands[k], ex[k], exp_ex[k]) for k in range(len(cands)) if ex[k] != exp_ex[k]]
    assert not bad, bad[:5]
    st = g.last_check
    classes = [R.classify(r) for r in exp_rows]
    assert (st["n_holding"], st["n_violated"], st["n_empty"]) == tuple(classes.count(c) for c in ("holding", "violated", "empty"))
    assert st["n_candidates"] == len(cands)
    return rows


def random_input(rng):
    n = rng.randrange(20, 400)
    nv = rng.randrange(4, 40)
    triples = [(rng.randrange(nv), rng.randrange(nv // 4 + 1), rng.randrange(nv)) for _ in range(n)]
    return triples, nv


def random_capture(rng, nv, triples):
    """A capture over all nine codes: mostly with values some triple has together, sometimes any id, sometimes absent."""
    code = rng.choice(R.CODES)
    attrs = [b for b in (1, 2, 4) if code & 7 & b]
    t = rng.choice(triples)
    vals = [t[{1: 0, 2: 1, 4: 2}[a]] for a in attrs]
    for k in range(len(vals)):
        x = rng.random()
        if x < 0.25:
            vals[k] = rng.randrange(nv)
        elif x < 0.32:
            vals[k] = A
    return (code, vals[0], vals[1] if len(vals) == 2 else N)


def random_candidates(rng, nv, triples):
    caps = [random_capture(rng, nv, triples) for _ in range(rng.randrange(2, 30))]
    cands = [(rng.choice(caps), rng.choice(caps)) for _ in range(rng.randrange(1, 60))]
    cands += [(c, c) for c in rng.sample(caps, min(3, len(caps)))]  # dep == ref
    cands += [rng.choice(cands) for _ in range(3)]                   # duplicates
    rng.shuffle(cands)
    return cands


@pytest.mark.parametrize("block", range(4))
def test_random_parity(ctx, block):
    """240 seeds of small random inputs; the example slots go round 0, 1, 16."""
    seen = set()
    for seed in range(block * 60, block * 60 + 60):
        rng = random.Random(9000 + seed)
        triples, nv = random_input(rng)
        set_triples(ctx, triples, nv)
        cands = random_candidates(rng, nv, triples)
        rows = assert_parity(ctx, triples, cands, (0, 1, 16)[seed % 3])
        seen |= {R.classify(r) for r in rows}
        if ctx.last_check["n_captures"]:  # (no capture at all: nothing to look for, no batch)
            assert ctx.last_check["n_batches"] == 1 and ctx.last_check["table_in_lds"] == 1
    assert seen == {"holding", "violated", "empty"}


@pytest.mark.parametrize("examples", [0, 1, 2, 16])
def test_known_answers(ctx, examples):
    set_triples(ctx, KAT_TRIPLES, KAT_TERMS)
    rows, ex = device_check(ctx, [(d, r) for _, d, r, _, _ in KATS], examples)
    exp_rows, exp_ex = kat_expected(examples)
    for kat, row, e, er, ee in zip(KATS, rows, ex, exp_rows, exp_ex):
        assert (row, e) == (er, ee), kat[0]


def test_other_stages_and_duplicates(ctx):
    """After rdf_distinct_triples the resident triples are the distinct ones: the same sets, the same rows."""
    set_triples(ctx, KAT_TRIPLES, KAT_TERMS)
    before = device_check(ctx, [(d, r) for _, d, r, _, _ in KATS], 2)
    assert ctx.distinct_triples()[0] == len(set(KAT_TRIPLES))
    raises_status(ERR_STATE, lambda: ctx.check_rows(0, 1))  # the rows went with the old triples
    assert device_check(ctx, [(d, r) for _, d, r, _, _ in KATS], 2) == before == kat_expected(2)


# ---- chunk boundaries ----

def chunk_cases(c):
    """[(name, dependent values, ref values)] around the work-item size c."""
    rng = random.Random(77)
    cases = []
    for n in (c - 1, c, c + 1, 3 * c + 1):
        d = sorted(rng.sample(range(8 * c), n))
        last0 = ((n - 1) // c) * c  # first index of the last chunk
        cases += [(f"{n} values, ref lacks the first", d, d[1:]),
                  (f"{n} values, ref lacks the last of a chunk", d, d[:min(c, n) - 1] + d[min(c, n):]),
                  (f"{n} values, ref lacks only values of the last chunk", d, d[:last0] + d[last0 + 1::2]),
                  (f"{n} values, ref equal", d, list(d))]
    d = sorted(rng.sample(range(8 * c), 3 * c + 1))
    cases.append(("violations straddle two chunks", d, d[:c - 2] + d[c + 2:]))
    cases.append(("violations straddle three chunks", d, d[:c - 1] + d[2 * c + 1:]))
    small = list(range(0, 8 * c, 8 * c // 50))[:50]
    cases.append(("ref 100x longer, every dependent value in it", small, list(range(8 * c))))
    cases.append(("ref 100x longer, some missing", small, [v for v in range(8 * c) if v % 40]))
    cases.append(("dependent 100x longer", list(range(5000)), list(range(0, 5000, 100))))
    cases.append(("ref disjoint, above", list(range(0, 2 * c)), list(range(2 * c, 3 * c))))
    cases.append(("ref disjoint, below", list(range(2 * c, 3 * c + 5)), list(range(0, 2 * c))))
    cases.append(("strictly interleaved", list(range(0, 4 * c, 2)), list(range(1, 4 * c, 2))))
    return cases


def test_chunk_boundaries(ctx):
    set_triples(ctx, KAT_TRIPLES, KAT_TERMS)
    ctx.check_cinds(np.zeros((0, 6), np.uint32))
    assert ctx.last_check["chunk_values"] == 0  # (n = 0: zeroed stats)
    device_check(ctx, [((10, 5, N), (10, 5, N))], 0)
    c = ctx.last_check["chunk_values"]
    assert c >= 64
    cases = chunk_cases(c)
    # case k: the dependent s[p=P + 2k], the ref s[p=P + 2k + 1]; values are subjects, predicates sit above them
    P = 8 * c
    nv = P + 2 * len(cases)
    triples, cands = [], []
    for k, (_, dep, ref) in enumerate(cases):
        triples += [(v, P + 2 * k, v) for v in dep] + [(v, P + 2 * k + 1, 0) for v in ref]
        cands.append(((10, P + 2 * k, N), (10, P + 2 * k + 1, N)))
    set_triples(ctx, triples, nv)
    index = R.all_interpretations(triples)
    for examples in (16, 3, 1, 0):
        rows = assert_parity(ctx, triples, cands, examples, index=index)
    for (name, dep, ref), row in zip(cases, rows):
        assert row[:3] == (len(dep), len(ref), len(set(dep) & set(ref))), name
    st = ctx.last_check
    assert st["n_work_items"] == sum((len(dep) + c - 1) // c for _, dep, _ in cases)
    assert st["n_values"] == sum(len(dep) + len(ref) for _, dep, ref in cases) and st["n_records"] == len(triples)
    # the same lists as object values of binary captures: o[s=.., p=..] cannot be built this way, so the projection on
    # the object with a unary condition
    cands_o = [((34, P + 2 * k, N), (10, P + 2 * k + 1, N)) for k in range(len(cases))]
    assert_parity(ctx, triples, cands_o, 16, index=index)


# ---- table paths ----

def table_query(rng):
    triples, nv = random_input(rng)
    return triples, nv, random_candidates(rng, nv, triples)


def test_table_paths(monkeypatch, ctx):
    triples, nv, cands = table_query(random.Random(31))
    results = {}
    for slots in ("0", None):
        if slots is None:
            monkeypatch.delenv("RDFIND_CHECK_LDS_SLOTS", raising=False)
        else:
            monkeypatch.setenv("RDFIND_CHECK_LDS_SLOTS", slots)
        with _lib.Context(0) as g:
            set_triples(g, triples, nv)
            results[slots] = (assert_parity(g, triples, cands, 16), g.last_check)
    assert results["0"][0] == results[None][0]
    assert results["0"][1]["table_in_lds"] == 0 and results["0"][1]["lds_slots"] == 0
    assert results[None][1]["table_in_lds"] == 1
    slots = results[None][1]["lds_slots"]
    assert slots >= 1024 and slots & (slots - 1) == 0
    # a cap below the default: a power of two at most the cap
    monkeypatch.setenv("RDFIND_CHECK_LDS_SLOTS", "100")
    with _lib.Context(0) as g:
        set_triples(g, triples, nv)
        assert assert_parity(g, triples, cands, 16) == results[None][0]
        assert g.last_check["lds_slots"] == 64
        assert g.last_check["table_in_lds"] == (1 if 4 * g.last_check["n_conditions"] <= 64 else 0)
    monkeypatch.delenv("RDFIND_CHECK_LDS_SLOTS")
    # one condition more than a quarter of the slots: the table no longer fits, on its own
    rng = random.Random(32)
    nv = slots // 4 + 40
    triples = [(rng.randrange(nv), rng.randrange(nv), rng.randrange(nv)) for _ in range(3000)]
    set_triples(ctx, triples, nv)
    for nconds, in_lds in ((slots // 4, 1), (slots // 4 + 1, 0)):
        cands = [((10, p, N), (34, p, N)) for p in range(nconds)]
        assert_parity(ctx, triples, cands, 2)
        assert ctx.last_check["n_conditions"] == nconds and ctx.last_check["table_in_lds"] == in_lds, nconds
        assert ctx.last_check["n_captures"] == 2 * nconds


# ---- batches ----

def own_need(triples, cand):
    """Records candidate `cand` needs on its own: the triples matching its dep and (if another capture) its ref."""
    def matching(c):
        if A in c[1:]:
            return 0
        attrs = [b for b in (1, 2, 4) if c[0] & 7 & b]
        want = list(zip(attrs, c[1:]))
        return sum(all(t[{1: 0, 2: 1, 4: 2}[a]] == v for a, v in want) for t in triples)
    dep, ref = cand
    return matching(dep) + (matching(ref) if ref != dep else 0)


def test_batches(monkeypatch):
    rng = random.Random(41)
    nv = 40  # ten predicates: no capture matches more than a small part of the triples
    triples = [(rng.randrange(nv), rng.randrange(10), rng.randrange(nv)) for _ in range(400)]
    cands = random_candidates(rng, nv, triples) + random_candidates(rng, nv, triples)
    shared = (10, triples[0][1], N)  # one capture on a side of candidates all along the list
    cands = [(shared, c[1]) if k % 7 == 0 else (c[0], shared) if k % 7 == 3 else c for k, c in enumerate(cands)]
    need = max(own_need(triples, c) for c in cands)
    assert need > 0
    monkeypatch.delenv("RDFIND_CHECK_RECORDS", raising=False)
    with _lib.Context(0) as g:
        set_triples(g, triples, nv)
        one = assert_parity(g, triples, cands, 16)
        one_stats = g.last_check
    assert one_stats["n_batches"] == 1 and one_stats["n_records"] > 3 * need
    monkeypatch.setenv("RDFIND_CHECK_RECORDS", str(need))
    with _lib.Context(0) as g:
        set_triples(g, triples, nv)
        assert assert_parity(g, triples, cands, 16) == one
        st = g.last_check
        assert st["n_batches"] >= 3 and st["n_records"] >= one_stats["n_records"]  # (a shared capture is rebuilt)
        assert [r[:3] for r in assert_parity(g, triples, cands, 0)] == [r[:3] for r in one]
    # a budget below one candidate's own need
    monkeypatch.setenv("RDFIND_CHECK_RECORDS", str(need - 1))
    with _lib.Context(0) as g:
        set_triples(g, triples, nv)
        e = raises_status(ERR_OOM, lambda: g.check_cinds(cand_array(cands), 0))
        assert "bytes" in str(e) and f"needs {need} records" in str(e)
        raises_status(ERR_STATE, lambda: g.check_rows(0, 1))


# ---- errors and state ----

def test_errors(ctx):
    set_triples(ctx, KAT_TRIPLES, KAT_TERMS)
    good = ((10, 5, N), (34, 5, N))
    for bad, word in (((11, 5, N), "code"), ((0, 5, N), "code"), ((10, 5, 1), "unary"), ((10, 5, A), "unary"),
                      ((14, 5, N), "binary"), ((10, KAT_TERMS, N), "term id"), ((10, N, N), "term id"),
                      ((14, 5, KAT_TERMS), "term id"), ((14, 0x40000000, 1), "term id")):
        for cands in ([good, (bad, good[0])], [good, good, (good[1], bad)]):
            e = raises_status(ERR_ARG, lambda: ctx.check_cinds(cand_array(cands), 0))
            assert word in str(e) and f"candidate {len(cands) - 1} " in str(e), (bad, str(e))
    raises_status(ERR_ARG, lambda: ctx.check_cinds(cand_array([good]), 17))
    lib, one = ctx.lib, cand_array([good])
    assert lib.rdf_check_cinds(ctx.ptr, None, 3, 0, None) == ERR_ARG
    assert lib.rdf_check_cinds(ctx.ptr, one.ctypes.data, 1 << 31, 0, None) == ERR_LIMIT
    # a failed call leaves no rows
    raises_status(ERR_STATE, lambda: ctx.check_rows(0, 1))
    # n = 0: valid, zero rows, zeroed stats
    rows, ex = ctx.check_cinds(np.zeros((0, 6), np.uint32), 5)
    assert len(rows) == 0 and ex.shape == (0, 5) and not any(ctx.last_check.values())
    assert len(ctx.check_rows(0, 10)) == 0
    # the copy calls clip
    ctx.check_cinds(cand_array([good, good, good]), 2)
    assert len(ctx.check_rows(1, 10)) == 2 and len(ctx.check_rows(3, 1)) == 0 and ctx.check_examples(2, 5, 2).shape == (1, 2)


def test_state():
    good = cand_array([((10, 5, N), (34, 5, N))])
    with _lib.Context(0) as g:
        raises_status(ERR_STATE, lambda: g.check_cinds(good, 0))  # no triples
        raises_status(ERR_STATE, lambda: g.check_rows(0, 1))      # the copy calls before any check
        raises_status(ERR_STATE, lambda: g.check_examples(0, 1, 1))
        set_triples(g, KAT_TRIPLES, KAT_TERMS)
        raises_status(ERR_STATE, lambda: g.check_rows(0, 1))
        # whatever changes the resident triples drops the rows; a new check or the pipeline's stages do not
        drops = {"set_triples": lambda: set_triples(g, KAT_TRIPLES, KAT_TERMS), "distinct_triples": g.distinct_triples,
                 "release_scratch": g.release_scratch}
        for name, call in drops.items():
            g.check_cinds(good, 1)
            assert len(g.check_rows(0, 1)) == 1
            call()
            raises_status(ERR_STATE, lambda: g.check_rows(0, 1))
            raises_status(ERR_STATE, lambda: g.check_examples(0, 1, 1))
        g.check_cinds(good, 1)
        g.run(1)
        assert g.check_rows(0, 1).tolist() == [(3, 3, 1, 1)] and g.check_examples(0, 1, 1).tolist() == [[0]]
        # a sharded run's state: a rank holds a slice
        g.shard_begin(0, 2, 1)
        e = raises_status(ERR_STATE, lambda: g.check_cinds(good, 0))
        assert "sharded" in str(e)


def test_check_leaves_the_pipeline_alone(ctx):
    rng = random.Random(55)
    triples, nv = random_input(rng)
    cands = random_candidates(rng, nv, triples)
    set_triples(ctx, triples, nv)
    ctx.run(2)
    n, checksum = ctx.cind_count(), ctx.checksum()
    assert n > 0
    sel = ctx.select_cinds(min_support=3)
    view = ctx.selected_decoded()
    decoded = ctx.copy_cinds_decoded()
    assert_parity(ctx, triples, cands, 16)
    assert ctx.cind_count() == n and ctx.checksum() == checksum
    assert ctx.selected_count() == sel and (ctx.selected_decoded() == view).all()
    assert (ctx.copy_cinds_decoded() == decoded).all()
    # the result's own rows are candidates that hold, with the dependent's support
    cands = [((r[0], r[1], r[2]), (r[3], r[4], r[5])) for r in decoded.tolist()]
    rows = assert_parity(ctx, triples, cands, 1)
    assert [r[0] for r in rows] == [r[6] for r in decoded.tolist()] and all(r[0] == r[2] for r in rows)
    # after each earlier stage too
    set_triples(ctx, triples, nv)
    ctx.frequent_conditions(2)
    first = assert_parity(ctx, triples, cands, 1)
    ctx.build_capture_groups("spo")
    assert assert_parity(ctx, triples, cands, 1) == first == rows
    ctx.discover_cinds()
    assert ctx.cind_count() == n and ctx.checksum() == checksum


# ---- the program ----

def run_check(argv):
    out = io.StringIO()
    assert chk.run(argv, out=out) == 0
    return out.getvalue().splitlines()


@pytest.mark.parametrize("mode", ["s1_clean", "s0_clean", "s0_raw"])
@pytest.mark.parametrize("name", ["lubm_small", "zipf_small", "skew_small"])
def test_program_round_trip(tmp_path, name, mode):
    """The golden's lines checked against their own input come back byte for byte, all holding."""
    lines = read_golden(name, mode)[1]
    cinds = tmp_path / "cinds.txt"
    cinds.write_text("# a golden\n\n" + "".join(ln + "\n" for ln in lines), encoding="utf-8")
    got = run_check(["--cinds", str(cinds), os.path.join(GOLDEN, f"{name}.nt.gz")])
    assert got[:-1] == lines
    assert got[-1] == f"Checked {len(lines)} CINDs: {len(lines)} hold, 0 violated, 0 empty."


def truncated_fixture(tmp_path, name):
    """The fixture without the last tenth of its triples: (path, triples as id tuples, the dictionary)."""
    with gzip.open(os.path.join(GOLDEN, f"{name}.nt.gz"), "rt", encoding="utf-8", newline="\n") as f:
        text = [ln for ln in f if ln.strip() and not ln.startswith("#")]
    keep = text[:len(text) - len(text) // 10]
    path = tmp_path / f"{name}_cut.nt"
    path.write_text("".join(keep), encoding="utf-8", newline="\n")
    s, p, o, dic = ntriples.read_triples([str(path)])
    return str(path), list(zip(s.tolist(), p.tolist(), o.tolist())), dic


def expected_report(cands_terms, triples, dic, examples, violated_only=False):
    """The program's lines by the reference: terms -> host ids (the device's, ids follow first appearance)."""
    def cap(c):
        return (c[0], dic.ids.get(c[1], A), N if c[2] is None else dic.ids.get(c[2], A))
    rows, ex = R.check(triples, [(cap(d), cap(r)) for d, r, _ in cands_terms], examples)
    lines = chk.report_lines(cands_terms, rows, np.array(ex, np.uint32).reshape(len(rows), examples),
                             lambda ids: [dic.term(int(i)) for i in ids], violated_only)
    return rows, lines


@pytest.mark.parametrize("name,mode,flags", [("lubm_small", "s1_clean", ["--examples", "3"]),
                                             ("zipf_small", "s0_raw", ["--violated-only"]),
                                             ("skew_small", "s0_clean", [])])
def test_program_on_a_truncated_input(tmp_path, name, mode, flags):
    lines = read_golden(name, mode)[1]
    cinds = tmp_path / "cinds.txt"
    cinds.write_text("".join(ln + "\n" for ln in lines), encoding="utf-8")
    path, triples, dic = truncated_fixture(tmp_path, name)
    cands = chk.read_cinds(lines)
    rows, expected = expected_report(cands, triples, dic, 3 if "--examples" in flags else 0, "--violated-only" in flags)
    assert any(R.classify(r) == "violated" for r in rows), "the reference finds no violated line"
    got = run_check(flags + ["--cinds", str(cinds), path])
    assert got == expected
    if "--examples" in flags:
        assert any(" e.g. " in ln for ln in got)
    if "--violated-only" in flags:
        assert all(" !< " in ln for ln in got[:-1]) and len(got) > 1


def test_program_prefixes(tmp_path):
    """--prefixes with two URLs under one prefix: <http://a.org/x> and <http://b.org/x> become the one term p:x."""
    nt = tmp_path / "in.nt"
    nt.write_text("".join(f"{s} {p} {o} .\n" for s, p, o in [
        ("<http://a.org/x>", "<http://a.org/knows>", "<http://a.org/y>"),
        ("<http://b.org/x>", "<http://b.org/likes>", "<http://a.org/z>"),
        ("<http://a.org/y>", "<http://b.org/knows>", "<http://b.org/z>"),
        ("<http://b.org/y>", "<http://a.org/likes>", '"a < b ] , (support=1)"'),
        ("<http://c.org/w>", "<http://a.org/likes>", "<http://a.org/y>"),
    ]), encoding="utf-8")
    pf = tmp_path / "p.nt"
    pf.write_text("@prefix p: <http://a.org/> .\n@prefix p: <http://b.org/> .\n", encoding="utf-8")
    lines = ["s[p=p:knows] < s[p=p:likes] (support=2)",
             "s[p=p:likes] < s[p=p:knows]",
             "o[p=p:knows] < o[p=p:likes] (support=2)",
             's[o="a < b ] , (support=1)"] < s[p=p:likes,o="a < b ] , (support=1)"] (support=1)',
             "s[p=<http://a.org/knows>] < s[p=p:likes]",
             "p[s=p:x] < p[s=p:y]"]
    cinds = tmp_path / "cinds.txt"
    cinds.write_text("".join(ln + "\n" for ln in lines), encoding="utf-8")
    s, p, o, dic = ntriples.read_triples([str(nt)])
    s, p, o, short = ntriples.shorten_dictionary(s, p, o, dic, ntriples.read_prefixes([str(pf)]))
    assert short.size < dic.size and "p:x" in short.ids
    triples = list(zip(s.tolist(), p.tolist(), o.tolist()))
    rows, expected = expected_report(chk.read_cinds(lines), triples, short, 2)
    assert sorted(R.classify(r) for r in rows) == ["empty", "holding", "holding", "holding", "holding", "violated"]
    assert run_check(["--prefixes", str(pf), "--examples", "2", "--cinds", str(cinds), str(nt)]) == expected
    assert expected[1] == "s[p=p:likes] !< s[p=p:knows] (support=3, overlap=2, violations=1) e.g. <http://c.org/w>"
