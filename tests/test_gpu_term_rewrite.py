"""rdf_rewrite_terms: --prefixes and --asciify-triples on the device dictionary.  The reference everywhere is the host
parse of the same text followed by ``ntriples.shorten_dictionary`` (or its asciify form): s, p, o, num_terms and every
term's bytes are compared for equality."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from rdfind_amd import _lib, ntriples, program
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

RDF_BLOCK = 256  # rdfind_amd/csrc/common.hpp
RDF_ERR_ARG, RDF_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _text(triples):
    return "".join(f"{a} {b} {c} .\n" for a, b, c in triples).encode("utf-8")


def host_reference(tmp_path, text, prefixes, asciify=False):
    """(s, p, o, [term bytes]) of the host parse of `text` followed by shorten_dictionary."""
    path = tmp_path / "ref.nt"
    path.write_bytes(text)
    s, p, o, dic = ntriples.read_triples([str(path)])
    s, p, o, dic = ntriples.shorten_dictionary(s, p, o, dic, prefixes, asciify_terms=asciify)
    return s, p, o, [t.encode("utf-8") for t in dic.terms]


def device_state(ctx, n):
    """(s, p, o, [term bytes]) resident in the context."""
    s, p, o = ctx.copy_triples(n)
    heap, off = ctx.parsed_terms()
    return s, p, o, [heap[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def device_parse(ctx, text, windows=0):
    if not windows:
        return ctx.parse_ntriples(text)[0]
    lines = text.splitlines(keepends=True)
    step = max((len(lines) + windows - 1) // windows, 1)
    parts = [b"".join(lines[i:i + step]) for i in range(0, len(lines), step)]
    assert len(parts) >= min(windows, len(lines))
    return ctx.parse_windows(parts)[0]


def check_rewrite(ctx, tmp_path, text, prefixes, asciify=False, windows=0):
    """Parse + rewrite on the device against the host reference; returns (stats, reference)."""
    ref = host_reference(tmp_path, text, prefixes, asciify)
    n = device_parse(ctx, text, windows)
    st = ctx.rewrite_terms(prefixes, asciify=asciify)
    assert_state(ctx, n, ref, st)
    return st, ref


def assert_state(ctx, n, ref, st=None):
    s, p, o, terms = device_state(ctx, n)
    assert ctx.num_terms == len(ref[3])
    assert terms == ref[3]
    np.testing.assert_array_equal(s, ref[0])
    np.testing.assert_array_equal(p, ref[1])
    np.testing.assert_array_equal(o, ref[2])
    if st is not None:
        assert st["n_terms_after"] == len(ref[3])
        assert st["heap_bytes"] == sum(len(t) for t in ref[3])


# ---- 1. random tables x random terms -------------------------------------------------------------------------------

CANDIDATES = [("ex", "http://ex.org/"), ("exa", "http://ex.org/a/"), ("exab", "http://ex.org/a/b"),
              ("m", "http://a/"), ("m", "http://b/"), ("far", "http://nowhere.example.org/never/")]
POOL = ([f"<http://ex.org/a/b/c{i}>" for i in range(6)] + [f"<http://ex.org/a/x{i}>" for i in range(6)]
        + [f"<http://ex.org/y{i}>" for i in range(6)]
        + ["<http://ex.org/a/>", "<http://ex.org/a/b>", "<http://ex.org/>",  # key + '>': an empty tail
           "<h>",  # shorter than every key
           "<urn:zzz:1>", "<urn:zzz:2>",  # IRIs no key matches
           '"lit1"', '"lit two"@en', '"5"^^<http://ex.org/int>', "_:b1", "_:b2",
           "<http://a/x>", "<http://b/x>",  # two keys with one value: they merge
           "ex:y1", "exa:x2", "m:x"])  # bare tokens that meet a shortened IRI


def _events(terms, prefixes):
    """Which of the cases the issue lists occur for these distinct terms under this table (the host decides)."""
    keys = ["<" + u for _, u in prefixes]
    table = ntriples.PrefixTable(prefixes)
    ev = set()
    short = {}
    for t in terms:
        nk = sum(t.startswith(k) for k in keys) if t.endswith(">") else 0
        if nk >= 2:
            ev.add("nested")
        if t.endswith(">") and t[:-1] in keys:
            ev.add("empty_tail")
        if keys and all(len(t) < len(k) for k in keys):
            ev.add("shorter_than_keys")
        if t.startswith("<") and t.endswith(">") and keys and table.shorten(t) == t:
            ev.add("iri_no_key")
        if t.startswith('"') and not t.endswith(">"):
            ev.add("plain_literal")
        if t.startswith('"') and t.endswith(">"):
            ev.add("typed_literal")
        if t.startswith("_:"):
            ev.add("blank")
        short.setdefault(table.shorten(t), []).append(t)
    for group in short.values():
        if len(group) > 1:
            if sum(g.startswith("<") for g in group) >= 2:
                ev.add("same_value_merge")
            if any(not g.startswith("<") for g in group) and any(g.startswith("<") for g in group):
                ev.add("bare_token_merge")
    return ev


def test_random_tables_and_terms(ctx, tmp_path):
    seen, merged = set(), 0
    for seed in range(40):
        rng = random.Random(seed)
        prefixes = [c for c in CANDIDATES if rng.random() < 0.7]
        rng.shuffle(prefixes)
        tr = [(rng.choice(POOL), rng.choice(POOL[:18]), rng.choice(POOL)) for _ in range(rng.randint(20, 300))]
        text = _text(tr)
        for windows in (0, 3 + seed % 3):
            st, ref = check_rewrite(ctx, tmp_path, text, prefixes, windows=windows)
        seen |= _events({x for t in tr for x in t}, prefixes)
        merged += st["n_terms_after"] < st["n_terms_before"]
    assert seen >= {"nested", "empty_tail", "shorter_than_keys", "iri_no_key", "plain_literal", "typed_literal", "blank",
                    "same_value_merge", "bare_token_merge"}, seen
    assert merged >= 1


# ---- 2. boundaries -------------------------------------------------------------------------------------------------

PFX = [("ex", "http://ex.org/"), ("exa", "http://ex.org/a/")]


def test_empty_input_and_one_triple(ctx, tmp_path):
    st, _ = check_rewrite(ctx, tmp_path, b"", PFX)
    assert st["n_terms_before"] == st["n_terms_after"] == 0 and st["heap_bytes"] == 0
    st, ref = check_rewrite(ctx, tmp_path, b"<http://ex.org/a/s> <http://ex.org/p> \"o\" .\n", PFX)
    assert ref[3] == [b"exa:s", b"ex:p", b'"o"'] and st["n_changed"] == 2
    check_rewrite(ctx, tmp_path, b"<http://ex.org/a/s> <http://ex.org/p> \"o\" .\n", PFX, windows=1)


@pytest.mark.parametrize("n_keys,form", [(0, None), (1, "lds"), (2500, "global")])
def test_key_counts_and_lookup_form(ctx, tmp_path, n_keys, form):
    """No key (the flag alone acts), one key, and more keys than the LDS-staged lookup holds."""
    prefixes = ([("ex", "http://ex.org/")] if n_keys else []) + [(f"n{i}", f"http://other{i}.example.org/ns/")
                                                                 for i in range(n_keys - 1)]
    if n_keys > 1:
        prefixes[7:7] = [("exa", "http://ex.org/a/")]  # a nested key somewhere in the middle of the table
        prefixes = prefixes[:n_keys]
    assert len(prefixes) == n_keys
    rng = random.Random(n_keys)
    tr = [(rng.choice(POOL), rng.choice(POOL[:18]), rng.choice(POOL)) for _ in range(200)]
    tr.append(("<http://other5.example.org/ns/z>", "<http://other1999.example.org/ns/>", "<http://other2600.example.org/ns/q>"))
    st, _ = check_rewrite(ctx, tmp_path, _text(tr), prefixes)
    assert ctx.rewrite_form() == form
    assert (st["n_changed"] > 0) == (n_keys > 0)


def test_key_lengths(ctx, tmp_path):
    """Keys of 1, 3, 4, 5, 15, 16 and 17 bytes, nested in one another, against terms that end around each of them."""
    body = "abcdefghijklmnopqrstuvwxyz"
    lengths = [1, 3, 4, 5, 15, 16, 17]
    prefixes = [(f"k{n}", body[:n - 1]) for n in lengths]  # the key is '<' + url
    assert [len("<" + u) for _, u in prefixes] == lengths
    terms = []
    for m in range(0, 20):
        terms += [f"<{body[:m]}>", f"<{body[:m]}_t>", f"k{m}:{body[:m]}"]  # empty tail, a tail, a bare token
    tr = [(terms[i], terms[(7 * i + 3) % len(terms)], terms[(11 * i + 5) % len(terms)]) for i in range(len(terms))]
    check_rewrite(ctx, tmp_path, _text(tr), prefixes)
    check_rewrite(ctx, tmp_path, _text(tr), prefixes, windows=4)


@pytest.mark.parametrize("asciify", [False, True])
def test_term_lengths(ctx, tmp_path, asciify):
    """Terms of 63 .. 257 bytes and one of 70,000 (the wave-cooperative write), as IRIs a key matches, IRIs none
    matches and literals; under asciify with multi-byte characters across the 64-byte steps."""
    terms = []
    for n in (63, 64, 65, 255, 256, 257, 70000):
        fill = "x" * n
        terms += ["<http://ex.org/a/" + fill[:n - 18] + ">", "<urn:q:" + fill[:n - 8] + ">", '"' + fill[:n - 2] + '"']
        assert [len(t) for t in terms[-3:]] == [n, n, n]
        if asciify:
            unit = "aé中\U0001f600b"  # 1 + 2 + 3 + 4 + 1 = 11 bytes: every phase against the 64-byte steps
            rep = unit * ((n - 18) // 11)
            terms += ["<http://ex.org/a/" + rep + ">", '"' + rep + '"']
    tr = [(terms[i], "<http://ex.org/p>", terms[(i + 1) % len(terms)]) for i in range(len(terms))]
    st, ref = check_rewrite(ctx, tmp_path, _text(tr), PFX, asciify=asciify)
    assert max(len(t) for t in ref[3]) >= 69000
    check_rewrite(ctx, tmp_path, _text(tr), PFX, asciify=asciify, windows=3)


def test_many_terms_and_all_to_one(ctx, tmp_path):
    n = 3 * RDF_BLOCK + 1  # n - 1 subjects and the predicate
    tr = [(f"<http://ex.org/a/s{i}>", "<http://ex.org/p>", f"<http://ex.org/a/s{(i * 5) % (n - 1)}>") for i in range(n - 1)]
    st, _ = check_rewrite(ctx, tmp_path, _text(tr), PFX)
    assert st["n_terms_before"] == n and st["n_terms_after"] == n
    both = [("m", "http://a/"), ("m", "http://b/")]
    tr = [("<http://a/x>", "<http://b/x>", "m:x"), ("m:x", "<http://a/x>", "<http://b/x>")] * 20
    st, ref = check_rewrite(ctx, tmp_path, _text(tr), both)
    assert st["n_terms_before"] == 3 and st["n_terms_after"] == 1 and ref[3] == [b"m:x"]
    assert st["heap_bytes"] == 3


# ---- 3. asciify ----------------------------------------------------------------------------------------------------

def test_asciify_on_device(ctx, tmp_path):
    from tests.test_term_rewrite_cpu import ASCIIFY_KNOWN
    chars = [c for c, _ in ASCIIFY_KNOWN[:6]]  # é € 中 Ċ U+0080 U+1F600: 2-, 3- and 4-byte UTF-8
    tr = []
    for i, ch in enumerate(chars):
        tr.append((f"<http://ex.org/a/{ch}{i}>", f"<http://ex.org/p{ch}>", f'"lit {ch}{ch} end"@en'))
        tr.append((f"_:b{ch}", "<http://ex.org/p>", f'"{ch}"^^<http://ex.org/t{ch}>'))
    tr.append(("<http://ex.org/café>", "<http://ex.org/p>", "<http://ex.org/cafi\x01>"))  # equal once asciified
    text = _text(tr)
    st, ref = check_rewrite(ctx, tmp_path, text, [], asciify=True)
    assert st["n_terms_after"] < st["n_terms_before"]
    assert b"<http://ex.org/a/i\x010>" in ref[3] and b"<http://ex.org/p-\x1c\x01>" in ref[3]
    assert all(max(t) < 0x80 for t in ref[3])
    check_rewrite(ctx, tmp_path, text, [], asciify=True, windows=3)
    # asciify and prefixes in one call = the host = two calls in sequence
    st, ref = check_rewrite(ctx, tmp_path, text, PFX, asciify=True)
    n = device_parse(ctx, text)
    ctx.rewrite_terms([], asciify=True)
    ctx.rewrite_terms(PFX)
    assert_state(ctx, n, ref)


# ---- 4. errors and state -------------------------------------------------------------------------------------------

def _shorten_bytes(t, prefixes):
    keys = sorted(((("<" + u).encode(), (p + ":").encode()) for p, u in prefixes), key=lambda kv: -len(kv[0]))
    if t.endswith(b">"):
        for k, v in keys:
            if t.startswith(k):
                return v + t[len(k):-1]
    return t


@pytest.mark.parametrize("windows", [0, 3])
def test_errors_leave_the_parse_untouched(ctx, tmp_path, windows):
    rng = random.Random(5)
    tr = [(rng.choice(POOL), rng.choice(POOL[:18]), rng.choice(POOL)) for _ in range(100)]
    tr += [("<http://ex.org/a/b>", "<http://ex.org/y2>", "ex:y1")]
    text = _text(tr) + b'<http://ex.org/y1> <http://ex.org/p> "bad \xff byte" .\n'
    n = device_parse(ctx, text, windows)
    before = device_state(ctx, n)
    v0 = ctx.num_terms
    whole = before[3].index(b"<http://ex.org/a/b>")
    bad = before[3].index(b'"bad \xff byte"')
    cases = [(dict(prefixes=PFX + [("w", "http://ex.org/a/b>")]), f"term {whole}\\b"),
             (dict(prefixes=PFX + [("other", "http://ex.org/")]), "Key already exists"),
             (dict(prefixes=PFX, asciify=True), f"term {bad} is not valid UTF-8")]
    for kwargs, message in cases:
        with pytest.raises(_lib.RdfError, match=message) as e:
            ctx.rewrite_terms(**kwargs)
        assert e.value.status == RDF_ERR_ARG
        assert ctx.num_terms == v0
        after = device_state(ctx, n)
        assert after[3] == before[3]
        for x, y in zip(after[:3], before[:3]):
            np.testing.assert_array_equal(x, y)
    st = ctx.rewrite_terms(PFX)  # a valid rewrite then succeeds (the host parser cannot read the invalid byte)
    exp = {}
    remap = [exp.setdefault(_shorten_bytes(t, PFX), len(exp)) for t in before[3]]
    s, p, o, terms = device_state(ctx, n)
    assert terms == list(exp) and st["n_terms_after"] == len(exp) < v0
    for got, old in zip((s, p, o), before[:3]):
        np.testing.assert_array_equal(got, np.array(remap, np.uint32)[old])
    # a second rewrite with an empty table and no flag changes nothing
    st2 = ctx.rewrite_terms()
    assert st2["n_terms_after"] == st2["n_terms_before"] == len(exp) and st2["n_changed"] == 0
    again = device_state(ctx, n)
    assert again[3] == terms
    for x, y in zip(again[:3], (s, p, o)):
        np.testing.assert_array_equal(x, y)


def test_state_errors(ctx, tmp_path):
    ids = np.arange(6, dtype=np.uint32)
    ctx.set_triples(ids, ids, ids, 6)
    with pytest.raises(_lib.RdfError) as e:
        ctx.rewrite_terms(PFX)
    assert e.value.status == RDF_ERR_STATE
    text = _text([("<http://ex.org/a/s>", "<http://ex.org/p>", '"o"')] * 3)
    ref = host_reference(tmp_path, text, PFX)
    ctx.parse_begin()
    cut = text.index(b"\n") + 1
    ctx.parse_chunk(text[:cut])
    with pytest.raises(_lib.RdfError) as e:
        ctx.rewrite_terms(PFX)
    assert e.value.status == RDF_ERR_STATE
    ctx.parse_chunk(text[cut:])  # the open parse goes on
    n = ctx.parse_end()["n_triples"]
    st = ctx.rewrite_terms(PFX)
    assert_state(ctx, n, ref, st)


# ---- 5. through the program ----------------------------------------------------------------------------------------

LUBM_PREFIXES = ("@prefix onto: <http://swat.cse.lehigh.edu/onto/> .\n"
                 "@prefix ub: <http://swat.cse.lehigh.edu/onto/univ-bench.owl#> .\n"  # nested in the one above
                 "@prefix rdf: <http://www.w3.org/1999/02/22-rdf-syntax-ns#> .\n"
                 "# a comment\n"
                 "@prefix d0: <http://www.Department0.University0.edu/> .\n")


def _run_program(tmp_path, tag, flags, inputs, rules=False):
    out = tmp_path / f"{tag}.txt"
    argv = list(flags) + ["--output", f"file://{out}"] + inputs
    if rules:
        argv += ["--ar-output", f"file://{tmp_path / (tag + '.rules')}"]
    prog = program.RDFind(argv)
    prog.run()
    lines = sorted(out.read_bytes().split(b"\n"))
    return prog, lines, ((tmp_path / (tag + ".rules")).read_bytes() if rules else None)


@pytest.mark.parametrize("flags", [["--use-fis", "--clean-implied"], ["--traversal-strategy", "0"],
                                   ["--use-fis", "--clean-implied", "--distinct-triples"],
                                   ["--use-fis", "--use-ars", "--ar-output"],
                                   ["--use-fis", "--clean-implied", "--ingest-window", "4096"]],
                         ids=["s2l_clean", "strategy0", "distinct", "ars", "windowed"])
def test_program_device_rewrite_equals_host_parser(tmp_path, monkeypatch, flags):
    from tests.test_oracle import read_golden
    ms, _ = read_golden("lubm_small", "s0_raw" if "0" in flags else "s1_clean")
    (tmp_path / "pre.nt").write_text(LUBM_PREFIXES)
    rules = "--ar-output" in flags
    flags = [f for f in flags if f != "--ar-output"] + ["--support", str(ms), "--prefixes", str(tmp_path / "pre.nt")]
    inputs = [os.path.join(GOLDEN, "lubm_small.nt.gz")]
    _, host_lines, host_rules = _run_program(tmp_path, "host", flags + ["--host-parser"], inputs, rules)
    assert len(host_lines) > 10 and any(b"ub:" in ln for ln in host_lines)

    def refuse(*a, **k):
        raise AssertionError("the device path went through the host")
    monkeypatch.setattr(ntriples, "shorten_dictionary", refuse)
    monkeypatch.setattr(_lib.Context, "copy_triples", refuse)
    prog, dev_lines, dev_rules = _run_program(tmp_path, "dev", flags, inputs, rules)
    assert prog.stats["rewrite"]["n_changed"] > 0
    assert dev_lines == host_lines
    assert dev_rules == host_rules
    if rules:
        assert host_rules


def test_program_asciify_triples(tmp_path):
    rng = random.Random(3)
    ents = [f"<http://ex.org/a/é{i}>" for i in range(6)] + [f"<http://ex.org/€{i}>" for i in range(6)] + ["<http://ex.org/中>"]
    preds = ["<http://ex.org/p>", "<http://ex.org/qé>"]
    objs = ents + ['"été"', '"plain"', "ex:,A1"]  # (no character whose asciified form holds a line break)
    tr = [(rng.choice(ents), rng.choice(preds), rng.choice(objs)) for _ in range(300)]
    (tmp_path / "in.nt").write_bytes(_text(tr))
    (tmp_path / "pre.nt").write_text("@prefix ex: <http://ex.org/> .\n@prefix exa: <http://ex.org/a/> .\n")
    flags = ["--use-fis", "--clean-implied", "--support", "2", "--asciify-triples", "--prefixes", str(tmp_path / "pre.nt")]
    _, host_lines, _ = _run_program(tmp_path, "host", flags + ["--host-parser"], [str(tmp_path / "in.nt")])
    prog, dev_lines, _ = _run_program(tmp_path, "dev", flags, [str(tmp_path / "in.nt")])
    assert len(host_lines) > 5 and any(b"exa:i\x01" in ln for ln in host_lines)
    assert dev_lines == host_lines
    assert prog.stats["rewrite"]["n_changed"] > 0


# ---- 6. -dop 2 -----------------------------------------------------------------------------------------------------

def test_program_dop2_prefixes_equals_one_gpu(tmp_path):
    """-dop 2 --prefixes: two ranks (gloo, on the one GPU), each rewriting its own device dictionary; the merged output
    equals the one-GPU output."""
    from tests.test_oracle import read_golden
    ms, _ = read_golden("lubm_small", "s1_clean")
    (tmp_path / "pre.nt").write_text(LUBM_PREFIXES)
    flags = ["--use-fis", "--clean-implied", "--support", str(ms), "--prefixes", str(tmp_path / "pre.nt")]
    inputs = [os.path.join(GOLDEN, "lubm_small.nt.gz")]
    _, one, _ = _run_program(tmp_path, "one", flags, inputs)
    out = tmp_path / "two.txt"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "rdfind_amd", "-dop", "2", *flags, "--output", f"file://{out}", "--debug-level",
                        "1", *inputs], cwd=root, env=dict(os.environ, RDFIND_DIST_BACKEND="gloo"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(out.read_bytes().split(b"\n")) == one
    assert r.stderr.count("terms rewritten") == 2, r.stderr[-2000:]
    assert not list(tmp_path.glob("two.txt.part*"))
