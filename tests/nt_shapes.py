"""N-Triples texts by construction, for the ingest's byte edges (test infrastructure; plain Python and numpy, no GPU).

A text is built line by line from the triples it is to mean.  The expected ``s, p, o`` and the expected terms come from
the triples handed to the :class:`Builder` (ids in order of first appearance, line-major then s, p, o), never from
tokenizing ``data``: the host parser (rdfind_amd/ntriples.py) and the device ingest (kernels.inl, "N-Triples ingest")
are both compared with them.

The geometry helpers restate, from ``data`` alone, what the device code computes before it parses a byte: the line
starts (k_nt_line_starts), the span and the LDS decision of every 256-line tokenizer block (k_nt_tokenize), where the
newlines fall in a thread's 16-byte load and in a 4096-byte tile (nt_newline_mask), the term hash (nt_hash) and which
slots of the chunked parse's open-addressing tables are occupied (k_nt_publish, k_nt_dict_insert).  Every named text
lists the edges it claims to hit; :func:`edge_present` decides each claim from ``data`` with these helpers.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

NT_LOAD = 16          # kernels.inl nt_newline_mask: one 16-byte load per thread
NT_CHUNK = 4096       # kernels.inl NT_CHUNK = RDF_BLOCK * 16: bytes per tile of the line-start passes
NT_TILE = 49152       # kernels.inl NT_TILE: LDS bytes of one tokenizer block (NT_TILE / 4 = 12288 words)
BLOCK_LINES = 256     # common.hpp RDF_BLOCK: consecutive lines per tokenizer block (k_nt_tokenize)
KGRID = 2048          # rdfind_hip.hip RDF_KGRID: the cap of every grid-stride launch
DICT_SLOTS = 16       # the RDFIND_NT_DICT_SLOTS value the forced runs use (rdf_parse_begin: the table's first size)

LENGTHS = list(range(1, 14)) + list(range(15, 34, 2))  # every length 1..13, then 4k +- 1 up to 33


# ---------------------------------------------------------------------------------------------------------------
# builder

@dataclass
class Text:
    name: str
    family: str
    data: bytes
    tabs: bool
    s: np.ndarray
    p: np.ndarray
    o: np.ndarray
    terms: list            # bytes, in id order
    n_lines: int           # lines appended (a final '\n' opens no further line)
    bad_line: int | None   # 1-based number of the first malformed line
    edges: list            # claims, see edge_present
    cuts: list | None = None          # explicit window ends (byte offsets), the last one len(data)
    terms_at_cut: list = field(default_factory=list)  # distinct terms after each explicit window
    marks: list = field(default_factory=list)         # generator records (see the generators)

    def windows(self):
        """The explicit windows (heap family and the chained texts): data cut at ``cuts``; a window may be empty."""
        lo, out = 0, []
        for c in self.cuts:
            out.append(self.data[lo:c])
            lo = c
        return out

    @property
    def heap_bytes(self):
        return sum(len(t) for t in self.terms)


class Builder:
    def __init__(self, tabs: bool = False):
        self.tabs = tabs
        self.parts, self.nbytes = [], 0
        self.ids, self.terms = {}, []
        self.s, self.p, self.o = [], [], []
        self.n_lines, self.bad_line = 0, None
        self.cuts, self.terms_at_cut = [], []
        self.offsets = []  # per triple: the byte offsets of its three terms in data
        self._open = False  # the last line has no terminator: only a cut or the end may follow

    def _emit(self, raw: bytes, end: bytes):
        assert not self._open, "a line without '\\n' can only be followed by a cut"
        assert b"\n" not in raw and end in (b"\n", b"\r\n", b"")
        self.parts.append(raw + end)
        self.nbytes += len(raw) + len(end)
        self.n_lines += 1
        self._open = end == b""

    def _id(self, t: bytes) -> int:
        i = self.ids.get(t)
        if i is None:
            i = self.ids[t] = len(self.terms)
            self.terms.append(t)
        return i

    def triple(self, s: bytes, p: bytes, o: bytes, lead=b"", sep1=None, sep2=None, tail=None, end=b"\n"):
        """One line ``lead s sep1 p sep2 o tail end`` that means the triple (s, p, o)."""
        sep = b"\t" if self.tabs else b" "
        sep1 = sep if sep1 is None else sep1
        sep2 = sep if sep2 is None else sep2
        tail = (b"" if self.tabs else b" .") if tail is None else tail
        a = self.nbytes + len(lead)
        b = a + len(s) + len(sep1)
        c = b + len(p) + len(sep2)
        self._emit(lead + s + sep1 + p + sep2 + o + tail, end)
        self.offsets.append((a, b, c))
        self.s.append(self._id(s))
        self.p.append(self._id(p))
        self.o.append(self._id(o))
        return self

    def skip(self, raw=b"", end=b"\n"):
        """A comment, a blank line or (raw empty, end '\\r\\n') a terminator alone."""
        self._emit(raw, end)
        return self

    def bad(self, raw: bytes, end=b"\n"):
        if self.bad_line is None:
            self.bad_line = self.n_lines + 1
        self._emit(raw, end)
        return self

    def cut(self):
        """Ends a window of the explicit window sequence here."""
        self.cuts.append(self.nbytes)
        self.terms_at_cut.append(len(self.terms))
        self._open = False
        return self

    def build(self, name: str, family: str, edges=(), marks=()) -> Text:
        if self.cuts and self.cuts[-1] != self.nbytes:
            self.cut()
        u32 = lambda x: np.array(x, dtype=np.uint32)
        return Text(name, family, b"".join(self.parts), self.tabs, u32(self.s), u32(self.p), u32(self.o),
                    list(self.terms), self.n_lines, self.bad_line, list(edges), list(self.cuts) or None,
                    list(self.terms_at_cut), list(marks))


# ---------------------------------------------------------------------------------------------------------------
# geometry: what the device computes from the bytes alone

def newline_offsets(data: bytes) -> np.ndarray:
    return np.flatnonzero(np.frombuffer(data, np.uint8) == 10).astype(np.int64)


def line_starts(data: bytes) -> np.ndarray:
    """k_nt_line_starts: line 0 starts at 0, line j + 1 after the j-th newline (newlines + 1 entries: after a final
    newline the device sees one more, empty line)."""
    return np.concatenate([np.zeros(1, np.int64), newline_offsets(data) + 1])


def n_tiles(data: bytes) -> int:
    return max(-(-len(data) // NT_CHUNK), 1)


def blocks(data: bytes):
    """k_nt_tokenize, per block of 256 lines: (b0, b1, words, in_lds)."""
    ls = line_starts(data)
    nlines, out = len(ls), []
    for l0 in range(0, nlines, BLOCK_LINES):
        l1 = min(l0 + BLOCK_LINES, nlines)
        b0 = int(ls[l0])
        b1 = int(ls[l1]) if l1 < nlines else len(data)
        w0 = b0 & ~3
        nw = (b1 - w0 + 3) // 4
        out.append((b0, b1, nw, nw <= NT_TILE // 4))
    return out


def split_lines(data: bytes):
    """One window per line (each with its '\\n', the last one maybe without)."""
    ls = line_starts(data).tolist() + [len(data)]
    return [data[a:b] for a, b in zip(ls[:-1], ls[1:]) if b > a]


def split_k(data: bytes, k: int):
    """At most k windows of whole lines."""
    lines = split_lines(data)
    step = max(-(-len(lines) // k), 1)
    return [b"".join(lines[i:i + step]) for i in range(0, len(lines), step)]


def window_line_count(windows) -> int:
    """rdf_parse_chunk's line count: per window its newlines, plus one for a last line without one."""
    return sum(w.count(b"\n") + (1 if w and not w.endswith(b"\n") else 0) for w in windows)


_M64 = (1 << 64) - 1


def mix64(x: int) -> int:
    """common.hpp mix64."""
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x


def nt_hash(t: bytes) -> int:
    """kernels.inl nt_hash: 8 little-endian bytes per step, then the rest."""
    n = len(t)
    h = 0x243F6A8885A308D3 ^ n
    i = 0
    while i + 8 <= n:
        h = mix64(h ^ int.from_bytes(t[i:i + 8], "little"))
        i += 8
    return mix64(h ^ int.from_bytes(t[i:], "little") ^ 0x9E3779B97F4A7C15)


def next_pow2(x: int) -> int:
    p = 1
    while p < x:
        p *= 2
    return p


def local_slots(window: bytes) -> int:
    """The window-local table of parse_chunk_body: next_pow2(2 * 3 * (newlines + 1)) slots."""
    return next_pow2(2 * 3 * (window.count(b"\n") + 1))


class TableSim:
    """Which slots of the chunked parse's persistent table are occupied (k_nt_publish: linear probing from
    hash & mask; the occupied set does not depend on the insertion order), and the table's growth
    (parse_chunk_body: rebuilt at next_pow2(2 * terms) slots once 2 * terms exceeds them)."""

    def __init__(self, slots: int = DICT_SLOTS):
        self.slots = next_pow2(max(slots, 2))
        self.hashes = []
        self.occ = [False] * self.slots
        self.growths = 0

    def copy(self):
        c = TableSim(self.slots)
        c.hashes, c.occ, c.growths = list(self.hashes), list(self.occ), self.growths
        return c

    def _put(self, h):
        i = h & (self.slots - 1)
        while self.occ[i]:
            i = (i + 1) & (self.slots - 1)
        self.occ[i] = True

    def add_window(self, new_hashes):
        new_hashes = list(new_hashes)
        if not new_hashes:
            return
        self.hashes += new_hashes
        if 2 * len(self.hashes) > self.slots:
            self.slots = next_pow2(2 * len(self.hashes))
            self.growths += 1
            self.occ = [False] * self.slots
            for h in self.hashes:
                self._put(h)
        else:
            for h in new_hashes:
                self._put(h)

    def meets(self, h_probe: int, h_target: int) -> bool:
        """True when a miss that probes from h_probe (k_nt_lookup: on to the first empty slot) is certain to pass the
        slot of the resident term with hash h_target: it reaches that term's home slot over occupied slots, and the
        term lies in the same occupied run at or after its home."""
        m = self.slots - 1
        i, t = h_probe & m, h_target & m
        for _ in range(self.slots):
            if not self.occ[i]:
                return False
            if i == t:
                return True
            i = (i + 1) & m
        return False


# ---------------------------------------------------------------------------------------------------------------
# the claims

def edge_present(t: Text, edge: str) -> bool:
    """Decides one claim of ``t.edges`` from ``t.data`` (and, for the term counts, from the constructed terms)."""
    d = t.data
    key, _, val = edge.partition("=")
    nl = newline_offsets(d)
    if key == "nbytes":
        return len(d) == int(val)
    if key == "final_nl":
        return d.endswith(b"\n")
    if key == "no_final_nl":
        return len(d) > 0 and not d.endswith(b"\n")
    if key == "nl_at":
        return d[int(val):int(val) + 1] == b"\n"
    if key == "nl_mod16":  # every residue of a thread's 16-byte load
        return set((nl % NT_LOAD).tolist()) == set(range(NT_LOAD))
    if key == "nl_mod4096":
        return int(val) in set((nl % NT_CHUNK).tolist())
    if key == "only_newlines":
        return len(d) > 0 and d.count(b"\n") == len(d)
    if key == "tiles_min":
        return n_tiles(d) >= int(val)
    if key == "newlines":
        return len(nl) == int(val)
    if key == "lines_min":
        return len(nl) + 1 >= int(val)
    if key == "block":  # block=<index>:<words or *>:<lds 0/1>:<b0 & 3 or *>
        i, words, lds, r = val.split(":")
        b0, b1, nw, in_lds = blocks(d)[int(i)]
        return ((words == "*" or nw == int(words)) and in_lds == bool(int(lds)) and (r == "*" or (b0 & 3) == int(r)))
    if key == "last_block_partial":
        n = len(nl) + 1
        return n % BLOCK_LINES != 0 and n > BLOCK_LINES
    if key == "last_line_cr":
        return d.endswith(b"\r")
    if key == "cr_at_span_end":  # an LDS block whose span is the whole tile and ends in "\r\n"
        return any(in_lds and b1 - (b0 & ~3) == NT_TILE and d[b1 - 2:b1] == b"\r\n" for b0, b1, _, in_lds in blocks(d))
    if key == "has":
        return val.encode("latin-1").decode("unicode_escape").encode("latin-1") in d
    if key == "terms_min":
        return len(t.terms) >= int(val)
    if key == "term_occurs_min":
        occ = np.bincount(np.concatenate([t.s, t.p, t.o]))
        return int(occ.max()) >= int(val)
    if key == "term_len":  # a term of exactly that length
        return any(len(x) == int(val) for x in t.terms)
    if key == "term_len_min":
        return any(len(x) >= int(val) for x in t.terms)
    if key == "terms_at_cut":
        return t.terms_at_cut == [int(x) for x in val.split(",")]
    if key == "empty_window":
        return any(len(w) == 0 for w in t.windows())
    if key == "window_no_nl":  # a window before the last one that does not end in '\n'
        return any(w and not w.endswith(b"\n") for w in t.windows()[:-1])
    if key == "bad_line":
        return t.bad_line == int(val)
    raise KeyError(edge)


def _has(raw: bytes) -> str:
    return "has=" + raw.decode("latin-1").encode("unicode_escape").decode("latin-1")


# ---------------------------------------------------------------------------------------------------------------
# lines: the line-start passes

def _plain(b: Builder, i: int):
    b.triple(b"<s%d>" % i, b"<p%d>" % (i % 3), b"<o%d>" % (i % 11))


def _fill_to(b: Builder, target: int, final_nl: bool = True):
    """Appends whole triples up to byte `target` exactly; the last one ends in '\\n' (at target - 1) or in nothing."""
    i = b.n_lines
    while target - b.nbytes > 120:
        _plain(b, i)
        i += 1
    body = target - b.nbytes - (1 if final_nl else 0)
    assert body >= 5, body
    b.triple(b"x", b"y", b"z" * (body - 4), tail=b"", end=b"\n" if final_nl else b"")


def _sized(n: int, final_nl: bool) -> Text:
    b = Builder()
    edges = [f"nbytes={n}", "final_nl" if final_nl else "no_final_nl"]
    body = n - (1 if final_nl else 0)
    if body < 5:  # too short for a triple: a blank line or a comment
        b.skip(b"#" * body, b"\n" if final_nl else b"")
    else:
        _fill_to(b, n, final_nl)
    if final_nl and n > NT_LOAD:
        edges.append(f"nl_at={n - 1}")
    return b.build(f"lines_{n}_{'nl' if final_nl else 'open'}", "lines", edges)


def _lines_family():
    out = [Builder().build("lines_0", "lines", ["nbytes=0"])]
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 8192):
        out += [_sized(n, True), _sized(n, False)]
    b = Builder()  # 17-byte lines: the newline moves on by one byte of the 16-byte load per line
    for i in range(40):
        b.triple(b"s%02d" % i, b"b", b"o%09d" % (i % 9), tail=b"")
    out.append(b.build("lines_mod16", "lines", ["nl_mod16=all"]))
    b = Builder()  # a newline in the last byte of tile 0 and one in the first byte of tile 1
    _fill_to(b, NT_CHUNK)
    b.skip(b"")
    for i in range(5):
        _plain(b, 1000 + i)
    out.append(b.build("lines_4095_4096", "lines", ["nl_at=4095", "nl_at=4096", "nl_mod4096=4095", "nl_mod4096=0"]))
    b = Builder()
    for _ in range(NT_CHUNK + 1):
        b.skip(b"")
    out.append(b.build("lines_only_newlines", "lines", [f"nbytes={NT_CHUNK + 1}", "only_newlines", "tiles_min=2"]))
    b = Builder()
    b.triple(b"<s>", b"<p>", b'"' + b"z" * 9000 + b'"', end=b"")
    out.append(b.build("lines_one_line_3_tiles", "lines", ["newlines=0", "tiles_min=3", "no_final_nl"]))
    return out


# ---------------------------------------------------------------------------------------------------------------
# blocks: the tokenizer's LDS tile

def _block_text(r: int, words: int, tabs: bool = False) -> Text:
    """Block 0 ends at a byte with (offset & 3) == r; block 1 spans exactly `words` aligned words from there: with
    12288 its span [b0 & ~3, b1) is the whole tile, with 12289 it is one byte more.  Its last line ends in "\\r\\n": a
    span always ends in its last line's '\\n', so the '\\r' is the tile's last byte but one (it cannot be the last).
    Block 2 is partly filled; its last line has no newline, and for odd r (and in the tabs form) it ends in '\\r'."""
    b = Builder(tabs)
    for i in range(BLOCK_LINES - 1):
        b.triple(b"<a%d>" % i, b"<p>", b"<b%d>" % (i % 7))
    pad = (r - (b.nbytes + (11 if tabs else 13))) % 4  # the line below has 11 (13 with " .") + pad bytes
    b.triple(b"<a>", b"<p>", b"<" + b"w" * pad + b">")
    assert b.nbytes & 3 == r and b.n_lines == BLOCK_LINES
    b0 = b.nbytes
    span = (NT_TILE if words == NT_TILE // 4 else NT_TILE + 1) - r
    for i in range(BLOCK_LINES - 2):
        b.triple(b"<c%d>" % i, b"<p>", b"<d%d>" % (i % 5))
    last = len(b"<c> <p> <e>") + (0 if tabs else 2) + 2  # the block's last line with its "\r\n"
    fill = b0 + span - last - b.nbytes - 1  # the filler line's bytes without its '\n'
    lit = fill - len(b"<f> <p> ") - (0 if tabs else 2)
    b.triple(b"<f>", b"<p>", b'"' + b"y" * (lit - 2) + b'"')
    b.triple(b"<c>", b"<p>", b"<e>", end=b"\r\n")
    assert b.nbytes == b0 + span and b.n_lines == 2 * BLOCK_LINES
    for i in range(9):
        b.triple(b"<g%d>" % i, b"<p>", b"<a%d>" % i)
    cr = tabs or r % 2 == 1
    b.triple(b"<g>", b"<p>", b"<last>" + (b"\r" if cr and tabs else b""), tail=None if tabs or not cr else b" .\r", end=b"")
    lds = int(words == NT_TILE // 4)
    edges = [f"block=1:{words}:{lds}:{r}", "last_block_partial", "no_final_nl", "block=0:*:1:0", "block=2:*:1:*"]
    if cr:
        edges.append("last_line_cr")
    if lds:
        edges.append("cr_at_span_end")
    return b.build(f"blocks_{'tabs_' if tabs else ''}r{r}_{words}", "blocks", edges)


def _blocks_family():
    out = [_block_text(r, w) for r in range(4) for w in (NT_TILE // 4, NT_TILE // 4 + 1)]
    out.append(_block_text(0, NT_TILE // 4, tabs=True))  # the object of the last line is "<last>\r"
    return out


# ---------------------------------------------------------------------------------------------------------------
# big: the second trip of both grid-stride loops

BIG_LINES = KGRID * BLOCK_LINES + 2 * BLOCK_LINES + 3
BIG_LONG_LINE = KGRID * BLOCK_LINES + BLOCK_LINES + 56  # in block KGRID + 1, the second trip of block 1


@lru_cache(maxsize=1)
def big() -> Text:
    """20-byte lines, so more than KGRID tiles and more than KGRID blocks.  Line 0 holds a literal longer than the LDS
    tile (block 0: global memory first, LDS on its second trip), line BIG_LONG_LINE another (block 1: the reverse).
    3989 subjects that recur as objects, and one predicate on every line."""
    b = Builder()
    sub = [b"<s%04d>" % i for i in range(3989)]
    long0, long1 = b'"' + b"L" * 50000 + b'"', b'"' + b"M" * 50000 + b'"'
    for i in range(BIG_LINES):
        o = long0 if i == 0 else long1 if i == BIG_LONG_LINE else sub[(i * 7 + 1) % 3989]
        b.triple(sub[i % 3989], b"<h>", o, tail=b"")
    return b.build("big", "big", [f"tiles_min={KGRID + 1}", f"lines_min={KGRID * BLOCK_LINES + 1}", "block=0:*:0:0",
                                  f"block={KGRID}:*:1:*", "block=1:*:1:*", f"block={KGRID + 1}:*:0:*",
                                  "terms_min=3900", "term_occurs_min=300001"])


# ---------------------------------------------------------------------------------------------------------------
# grammar

def _grammar_family():
    out = []
    b = Builder()
    b.triple(b"<a b>", b"<p>", b"<o>")
    b.triple(b"<s>", b"<p>", b'"x"^^', tail=b"")
    b.triple(b"<s>", b'"lit"', b"xyz", sep2=b"", tail=b" <o> .")
    b.triple(b"<s>", b'"l"', b"^x", sep2=b"", tail=b" <o> .")
    b.triple(b"<s>", b"<p>", b"<o>", sep1=b"", sep2=b"", tail=b".")
    b.triple(b"<s>", b"<p>", b'"a\\\\"')
    b.triple(b"#", b"not", b"a", lead=b"  ", tail=b" comment")
    b.triple(b"<s>", b'"x\x1cy"', b"<o>", sep2=b" \x1c")
    b.triple(b"<s>", b"<p>", '"été"'.encode())
    b.triple(b"<s>", b"<p>", '"étè"'.encode())
    b.triple(b"<s>", b"<p>", b'"esc \\" q"@en')
    b.triple(b"<s>", b"<p>", b'"5"^^<http://t>')
    b.triple(b"<s>", b"<p>", b'"5"^^x:int')
    for k, sp in enumerate((b"\x1c", b"\x1d", b"\x1e", b"\x1f", b"\v", b"\f", b"\r", b"\t")):  # every separator of nt_space
        b.triple(b"<w%d>" % k, b"<p>", b"<o>", lead=sp, sep1=sp, sep2=sp + sp, tail=sp + b".")
    b.skip(b"# a comment").skip(b" \t\x1c\x1f").skip(b"", b"\r\n")
    b.triple(b"<s>", b"<p>", b"<o>", end=b"\r\n")
    b.triple(b"<s>", b"<p>", b"<z>", tail=b"", end=b"")
    rows = [b"<a b>", b'"x"^^\n', b'"lit"xyz', b'"l"^x', b"<s><p><o>.", b'"a\\\\"', b"  # not a comment",
            b'"x\x1cy" \x1c<o>', '"étè"'.encode()]
    out.append(b.build("grammar_rows", "grammar", [_has(r) for r in rows] + ["no_final_nl"]))

    b = Builder(tabs=True)
    b.triple(b"a", b"", b"b")
    b.skip(b"\t\t")
    b.triple(b"x", b"y", b"")
    b.triple(b"a", b"b", b"c", end=b"\r\n")
    b.triple(b"a", b"b", b"c", tail=b"\td e")
    b.triple(b" a ", b"<b c>", b'"q')
    b.skip(b"# c")
    b.triple(b"a", b"b", b"c\r", end=b"")
    rows = [b"a\t\tb\n", b"\n\t\t\n", b"x\ty\t\n", b"a\tb\tc\r\n"]
    out.append(b.build("grammar_tabs", "grammar", [_has(r) for r in rows] + ["last_line_cr", "term_len=0"]))

    bad = {"lit_escape_end": b'<s> <p> "a\\"', "iri": b"<s> <p> <unterminated", "datatype": b'<s> <p> "x"^^<unterminated',
           "two_terms": b"<s> <p>", "one_term": b"<s>  "}
    for k, (name, raw) in enumerate(bad.items()):
        b = Builder()
        b.skip(b"# c").triple(b"<s>", b"<p>", b"<o>").skip(b"")
        for i in range(k):
            _plain(b, i)
        b.bad(raw)
        b.triple(b"<s>", b"<p>", b"<o>")
        out.append(b.build(f"grammar_bad_{name}", "grammar", [_has(raw + b"\n"), f"bad_line={4 + k}"]))
    b = Builder(tabs=True)
    b.triple(b"a", b"b", b"c").bad(b"a\tb").triple(b"a", b"b", b"c")
    out.append(b.build("grammar_bad_tabs_two_fields", "grammar", [_has(b"\na\tb\n"), "bad_line=2"]))
    return out


# ---------------------------------------------------------------------------------------------------------------
# dict: the byte comparison and first appearance

_ALPHA = b"abcdefghijklmnopqrstuvwxyz0123456789"
_LAST = [c for c in range(0x21, 0x7f) if c not in b'<>"#\\']  # candidates for a differing last byte


_TERM = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"


def _same_home(x: bytes, y: bytes, slots: int) -> bool:
    return (nt_hash(x) ^ nt_hash(y)) & (slots - 1) == 0


def _pair_line(b: Builder, x: bytes, y: bytes, pa: int, pb: int, j: int):
    """``x y <oJ>`` with x at (offset & 3) == pa and y at pb; the line's length is a multiple of 4, and so is every
    line start of the text: offsets in a window of whole lines equal offsets in the text mod 4."""
    gap = 1 + (pb - (pa + len(x) + 1)) % 4
    o = b"<o%d>" % j
    n = pa + len(x) + gap + len(y) + 1 + len(o) + 1
    b.triple(x, y, o, lead=b" " * pa, sep1=b" " * gap, tail=b" " * (-n % 4))
    assert b.nbytes % 4 == 0


class _Fresh:
    """Pairs of terms that no earlier line of the text has: x and y differ in byte k only and share their home slot in
    a table of `slots` slots."""

    def __init__(self, slots: int = 16):
        self.slots, self.used, self.count = slots, set(), 0
        one = {}
        for c in _LAST:  # one-byte terms: paired up within their home slots
            one.setdefault(nt_hash(bytes([c])) & (slots - 1), []).append(bytes([c]))
        self.ones = [(v[i], v[i + 1]) for v in one.values() for i in range(0, len(v) - 1, 2)]

    def _next(self, n: int) -> bytes:
        while True:
            self.count += 1
            i, head = self.count, b""
            for _ in range(min(n, 4)):
                head += bytes([_TERM[i % 62]])
                i //= 62
            x = head + bytes(_ALPHA[(3 * q + n) % 36] for q in range(n - len(head)))
            if i == 0 and x not in self.used:
                return x

    def pair(self, n: int, k: int, tail=None):
        """(x, y); with `tail` both end in tail[0] / tail[1] instead (k must be the last byte then)."""
        if n == 1:
            x, y = self.ones.pop()
            self.used |= {x, y}
            return x, y
        while True:
            x = self._next(n)
            if tail:
                x = x[:n - len(tail[0])] + tail[0]
            cands = [x[:n - len(tail[1])] + tail[1]] if tail else [x[:k] + bytes([c]) + x[k + 1:] for c in _TERM]
            for y in cands:
                if y != x and y not in self.used and x not in self.used and _same_home(x, y, self.slots):
                    self.used |= {x, y}
                    return x, y


@lru_cache(maxsize=1)
def dict_pairs() -> Text:
    """Per length n of LENGTHS and per byte k among the first byte, each byte of the tail (4 * (n // 4) .. n - 1) and
    the last byte: 16 lines ``x y <o>``, one per combination of (offset of x & 3, offset of y & 3), where x and y
    differ in byte k only.  Every pair is fresh: neither term occurs on an earlier line, so in a window of that line
    alone both are misses of the persistent table and go into the window's own table (6 occurrences: 16 slots).  They
    share their home slot there, so whichever is inserted second meets the other in k_nt_dict_insert, and without
    fingerprint bits nt_equal compares the two.  This holds for one window per line only: a larger window has a larger
    table, where the two meet by chance.  A length of 1 has as many lines as one-byte terms pair up (at least 4).
    Then pairs that end in e acute / e grave (a last byte >= 0x80), fresh and with a shared home slot as well.
    marks: (offset of x, offset of y, n, k) of every such line."""
    b = Builder()
    fresh = _Fresh(16)
    marks, j = [], 0

    def line(x, y, pa, pb, n, k):
        nonlocal j
        _pair_line(b, x, y, pa, pb, j)
        marks.append((b.offsets[-1][0], b.offsets[-1][1], n, k))
        j += 1

    for n in LENGTHS:
        for k in sorted({0, n - 1} | set(range(4 * (n // 4), n))):
            for pa in range(4):
                for pb in range(4):
                    if n == 1 and not fresh.ones:
                        continue
                    line(*fresh.pair(n, k), pa, pb, n, k)
    acute, grave = "é".encode(), "è".encode()
    for n in (4, 5, 6, 7):
        for pa in range(4):
            line(*fresh.pair(n, n - 1, (acute, grave)), pa, (pa + n) % 4, n, n - 1)
    b.triple(b"abc", b"abcd", b"ab")  # proper prefixes
    b.triple(b"<a>", b"<a>", b"<a>")
    return b.build("dict_pairs", "dict", ["term_len=1", "term_len=33", _has(b"<a> <a> <a>")], marks)


def dict_first_appearance() -> Text:
    """A term whose first occurrence is the object of the last line of a 256-line block and that is the subject of the
    first line of the next block (thread 0), then of every line of that block; twice."""
    b = Builder()
    for i in range(BLOCK_LINES - 1):
        b.triple(b"<f%d>" % i, b"<p>", b"<g%d>" % (i % 3))
    b.triple(b"<f>", b"<p>", b"<new1>")
    for i in range(BLOCK_LINES - 1):
        b.triple(b"<new1>", b"<p>", b"<g%d>" % (i % 5))
    b.triple(b"<new1>", b"<p>", b"<new2>")
    for i in range(200):
        b.triple(b"<new2>", b"<q>", b"<new1>" if i % 2 else b"<new2>")
    return b.build("dict_first_appearance", "dict", ["lines_min=700", _has(b"<new1> .\n<new1> "), _has(b"<new2> .\n<new2> ")])


def _b36(i: int, n: int) -> bytes:
    out = b""
    while i:
        out = bytes([_ALPHA[i % 36]]) + out
        i //= 36
    return out.rjust(n, b"x")


@lru_cache(maxsize=1)
def dict_lastbyte_chain() -> Text:
    """An explicit window sequence for nt_equal2 (window text against the term heap) in k_nt_lookup, meant for
    RDFIND_NT_FP_BITS=0 and RDFIND_NT_DICT_SLOTS=16.  For every (w, h, l) in 0..3 cubed: a window that brings X as its
    only new term, at heap offset & 3 == h, length & 3 == l; then a window with X' at window offset & 3 == w, where X'
    differs from X in its last byte only and is chosen so that its probe is certain to pass X's slot
    (TableSim.meets).  marks: (id of X, id of X', index of the window of X', w, h, l)."""
    b = Builder()
    sim = TableSim(DICT_SLOTS)
    b.triple(b"<p>", b"<p>", b"<o>", tail=b"").cut()
    sim.add_window([nt_hash(b"<p>"), nt_hash(b"<o>")])
    heap, marks, count = 6, [], 0
    by_res = {r: [n for n in LENGTHS if n >= 4 and n % 4 == r] for r in range(4)}
    for h in range(4):
        for l in range(4):
            for w in range(4):
                d = (h - heap) % 4
                if d:  # a filler term moves the heap's end to h
                    count += 1
                    f = b"F" + _b36(count, d + 3)
                    b.triple(f, b"<p>", b"<o>", tail=b"").cut()
                    sim.add_window([nt_hash(f)])
                    heap += len(f)
                n = by_res[l][(4 * h + w) % len(by_res[l])]
                while True:
                    count += 1
                    x = _b36(count, n - 1) + b"a"
                    after = sim.copy()
                    after.add_window([nt_hash(x)])
                    y = next((x[:-1] + bytes([c]) for c in _LAST
                              if c != x[-1] and after.meets(nt_hash(x[:-1] + bytes([c])), nt_hash(x))), None)
                    if y is not None:
                        break
                assert heap % 4 == h
                b.triple(x, b"<p>", b"<o>", tail=b"").cut()
                b.triple(y, b"<p>", b"<o>", lead=b" " * w, tail=b"")
                marks.append((b.ids[x], b.ids[y], len(b.cuts), w, h, l))
                b.cut()
                sim = after
                sim.add_window([nt_hash(y)])
                heap += 2 * n
    t = b.build("dict_lastbyte_chain", "dict", ["term_len=4", "term_len=33"], marks)
    assert t.heap_bytes == heap
    return t


def _dict_family():
    return [dict_pairs(), dict_first_appearance(), dict_lastbyte_chain()]


# ---------------------------------------------------------------------------------------------------------------
# heap: k_nt_append_bytes (explicit windows)

class _Uniq:
    """Distinct letter-only terms of a given length."""

    def __init__(self):
        self.count = {}

    def __call__(self, n: int) -> bytes:
        i = self.count[n] = self.count.get(n, 0) + 1
        out = b""
        for _ in range(n):
            out = bytes([b"ABCDEFGHJKLMNPQRSTUVWXYZabcdefghjk"[i % 34]]) + out
            i //= 34
        assert i == 0
        return out


def _heap_family():
    out = []
    b, u = Builder(), _Uniq()
    b.triple(b"<s>", b"<p>", b"<o>", tail=b"").cut()
    heap = 9
    for h in range(4):
        for t in range(1, 9):
            d = (h - heap) % 4
            if d:
                b.triple(u(d), b"<p>", b"<o>", tail=b"").cut()
                heap += d
            if t < 4:
                x = u(t)
                b.triple(x, b"<p>", b"<o>", tail=b"").cut()
            else:
                x, y = u(t // 2), u(t - t // 2)
                b.triple(x, b"<p>", y, tail=b"").cut()
            heap += t
            b.triple(b"<s>", b"<p>", x, tail=b"").cut()  # a window with no new term
    t = b.build("heap_align", "heap", [])
    assert t.heap_bytes == heap
    out.append(t)

    # the empty term (tabs) as the only, the first, a middle and the last new term of a window; heap0 & 3 = 1, 2, 3, 0
    forms = {"only": (b"a", b"", b"b"), "first": (b"", b"n1", b"n2"), "middle": (b"n1", b"", b"n2"),
             "last": (b"n1", b"n2", b"")}
    for k, (name, (s, p, o)) in enumerate(forms.items()):
        b = Builder(tabs=True)
        b.triple(b"a", b"b", b"c" * ((k + 1 - 2) % 4 or 4)).cut()
        b.triple(s, p, o).cut()
        b.triple(o, s, p).triple(b"z", b"", b"a").cut()
        t = b.build(f"heap_empty_{name}", "heap", ["term_len=0"])
        assert (t.terms_at_cut[0], len(b"".join(t.terms[:3])) % 4) == (3, (k + 1) % 4)
        out.append(t)

    b = Builder()
    big_lit = b'"' + bytes(_ALPHA[(i * i) % 36] for i in range(5000)) + b'"'
    b.triple(b"<s>", b"<p>", b"<o>").cut()
    b.triple(b"<s>", b"<p>", big_lit).cut()
    b.triple(big_lit, b"<p>", b"<t>").cut()
    out.append(b.build("heap_long", "heap", [f"term_len_min={NT_CHUNK + 1}"]))

    b = Builder()  # 16 slots hold 8 terms at load 1/2: exactly 8 after window 0, the ninth makes the table grow
    b.triple(b"a", b"b", b"c", tail=b"").triple(b"d", b"e", b"f", tail=b"").triple(b"g", b"h", b"a", tail=b"").cut()
    b.triple(b"a", b"b", b"i", tail=b"").cut()
    b.triple(b"i", b"h", b"g", tail=b"").cut()
    out.append(b.build("heap_slots", "heap", ["terms_at_cut=8,9,9"]))
    return out


# ---------------------------------------------------------------------------------------------------------------
# malformed lines: numbering

def bad_two_blocks() -> Text:
    """Two bad lines in different tokenizer blocks, behind comments and blank lines that count."""
    b = Builder()
    b.skip(b"# head").skip(b"")
    for i in range(700):
        if i == 300 or i == 650:
            b.bad(b"<s%d> <p>" % i)
        elif i % 50 == 7:
            b.skip(b"# c%d" % i)
        else:
            _plain(b, i)
    return b.build("bad_two_blocks", "bad", ["bad_line=303", "lines_min=700", _has(b"<s650> <p>\n")])


def bad_chunked() -> Text:
    """The bad line behind an empty window, an all-comment window and a window without a final newline."""
    b = Builder()
    b.triple(b"<a>", b"<p>", b"<b>").triple(b"<b>", b"<p>", b"<c>").cut()
    b.cut()
    b.skip(b"# only").skip(b"").skip(b"   ").cut()
    b.triple(b"<c>", b"<p>", b"<a>", end=b"").cut()
    b.triple(b"<a>", b"<q>", b"<c>").bad(b'<a> <q> "open').triple(b"<a>", b"<q>", b"<b>").cut()
    return b.build("bad_chunked", "bad", ["bad_line=8", "empty_window", "window_no_nl"])


# ---------------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=1)
def small_texts() -> dict:
    """Every named text but big(), by name."""
    ts = (_lines_family() + _blocks_family() + _grammar_family() + _dict_family() + _heap_family()
          + [bad_two_blocks(), bad_chunked()])
    out = {t.name: t for t in ts}
    assert len(out) == len(ts)
    return out


def names(family: str, bad: bool = False):
    return [n for n, t in small_texts().items() if t.family == family and (t.bad_line is not None) == bad]
