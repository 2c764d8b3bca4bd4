"""--asciify-triples and --prefixes on the host side (rdfind_amd/ntriples.py), no GPU: ``asciify`` against answers
derived by hand from AsciifyTriples.scala:17-37, the generalised ``shorten_dictionary`` against the per-triple
restatement, and the driver's ``--asciify-triples --host-parser``."""
import numpy as np
import pytest

from oracle import rdfind_oracle as R
from rdfind_amd import ntriples

# AsciifyTriples.asciify per UTF-16 code unit c: do { append(c & 0x7F); c >>= 7 } while (c != 0)
ASCIIFY_KNOWN = [
    # U+00E9 = 0b1_1101001: 0xE9 & 0x7F = 0x69 'i', then 0xE9 >> 7 = 1 -> "\x01"
    ("é", "i\x01"),
    # U+20AC = 0b1000001_0101100: & 0x7F = 0x2C ',', >> 7 = 0x41 'A', >> 7 = 0
    ("€", ",A"),
    # U+4E2D = 0b1_0011100_0101101: 0x2D '-', then 0x4E2D >> 7 = 0x9C -> 0x1C, then 0x9C >> 7 = 1
    ("中", "-\x1c\x01"),
    # U+010A = 0b10_0001010: 0x0A '\n', then 0x10A >> 7 = 2
    ("Ċ", "\n\x02"),
    # U+0080 = 0b1_0000000: 0x00, then 1
    ("\u0080", "\x00\x01"),
    # U+1F600 is the surrogates D83D DE00, three bytes each:
    # 0xD83D = 0b11_0110000_0111101: 0x3D '=', 0x30 '0', 0x03;  0xDE00 = 0b11_0111100_0000000: 0x00, 0x3C '<', 0x03
    ("\U0001f600", "=0\x03\x00<\x03"),
    # a pure-ASCII string is returned unchanged
    ("<http://ex.org/a b>\t\"x\"", "<http://ex.org/a b>\t\"x\""),
    # ASCII after a non-ASCII character passes through unchanged
    ("<café/x>", "<cafi\x01/x>"),
]


@pytest.mark.parametrize("term,expected", ASCIIFY_KNOWN)
def test_asciify_known_answers(term, expected):
    got = ntriples.asciify(term)
    assert got == expected
    assert got.isascii()


def _per_triple(triples, prefixes, asciify):
    """The reference's order (RDFind.scala:239-267): asciify each triple's terms, then shorten them, then encode."""
    f = (lambda t: R.shorten_term(ntriples.asciify(t), prefixes)) if asciify else (lambda t: R.shorten_term(t, prefixes))
    d = ntriples.Dictionary()
    ids = [[d.encode(f(x)) for x in t] for t in triples]
    return np.array(ids, dtype=np.uint32).reshape(-1, 3), d


NONASCII_TRIPLES = [
    ("<http://ex.org/café>", "<http://ex.org/p>", "\"中文\"@zh"),
    ("<http://ex.org/cafi\x01>", "<http://ex.org/p>", "<http://ex.org/a/€>"),
    ("<http://ü.org/x>", "<http://ex.org/q>", "exa:,A"),
    ("<http://ex.org/café>", "<http://ex.org/q>", "\"plain\""),
    ("_:b\U0001f600", "<http://ex.org/p>", "\"5\"^^<http://ex.org/inté>"),
    ("<http://ex.org/a/€>", "<http://ex.org/p>", "ex:cafi\x01"),
]
PREFIXES = [("ex", "http://ex.org/"), ("exa", "http://ex.org/a/")]


@pytest.mark.parametrize("asciify", [False, True])
def test_shorten_dictionary_with_asciify_matches_per_triple(asciify):
    d = ntriples.Dictionary()
    ids = np.array([[d.encode(x) for x in t] for t in NONASCII_TRIPLES], dtype=np.uint32)
    s, p, o, short = ntriples.shorten_dictionary(ids[:, 0], ids[:, 1], ids[:, 2], d, PREFIXES, asciify_terms=asciify)
    exp, ed = _per_triple(NONASCII_TRIPLES, PREFIXES, asciify)
    assert short.terms == ed.terms
    np.testing.assert_array_equal(np.stack([s, p, o], axis=1), exp)
    if asciify:  # the asciified café meets the literal spelling of its asciified form, and both shorten alike
        assert short.size < d.size
        assert "ex:cafi\x01" in short.terms and "exa:,A" in short.terms


def test_shorten_dictionary_signature_unchanged():
    d = ntriples.Dictionary()
    ids = np.array([[d.encode(x) for x in t] for t in NONASCII_TRIPLES], dtype=np.uint32)
    s, p, o, short = ntriples.shorten_dictionary(ids[:, 0], ids[:, 1], ids[:, 2], d, PREFIXES)
    exp, ed = _per_triple(NONASCII_TRIPLES, PREFIXES, False)
    assert short.terms == ed.terms


class _NoGpuContext:
    """Stands in for _lib.Context in the --only-read host path: records what the driver hands to the device."""
    last = None

    def __init__(self, device=0):
        type(self).last = self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def set_triples(self, s, p, o, num_terms):
        self.s, self.p, self.o, self.num_terms = np.array(s), np.array(p), np.array(o), num_terms


def test_driver_accepts_asciify_triples_host_parser(tmp_path, monkeypatch):
    from rdfind_amd import _lib, program

    assert "--asciify-triples" not in program._UNSUPPORTED
    src = tmp_path / "in.nt"
    src.write_text("".join(f"{a} {b} {c} .\n" for a, b, c in NONASCII_TRIPLES), encoding="utf-8")
    (tmp_path / "pre.nt").write_text("@prefix ex: <http://ex.org/> .\n@prefix exa: <http://ex.org/a/> .\n")
    monkeypatch.setattr(_lib, "Context", _NoGpuContext)
    monkeypatch.setenv("RDFIND_NUMA_BIND", "0")
    prog = program.RDFind(["--use-fis", "--asciify-triples", "--host-parser", "--only-read", "--prefixes",
                           str(tmp_path / "pre.nt"), str(src)])
    assert prog.args.asciify_triples is True
    assert prog.run() == []
    got = _NoGpuContext.last
    exp, ed = _per_triple(NONASCII_TRIPLES, PREFIXES, True)
    assert got.num_terms == ed.size  # the dictionary ...
    np.testing.assert_array_equal(np.stack([got.s, got.p, got.o], axis=1), exp)
    # ... and with it the frequency of every term at every position equal the per-triple restatement's
    for col in range(3):
        np.testing.assert_array_equal(np.bincount(np.stack([got.s, got.p, got.o], axis=1)[:, col], minlength=ed.size),
                                      np.bincount(exp[:, col], minlength=ed.size))
