"""The scan and radix primitives of rdfind_amd/csrc/primitives.hip, called directly (rdf_test_*, csrc/test_abi.h) and
compared element for element with the NumPy references of tests/prim_ref.py.  Every call also reports whether the
canaries around its device buffers survived; every case asserts that too.

The sizes are the smallest that cross each boundary of the code.  They are derived from the constants below, which
mirror primitives.hip: a retune there is a one-line change here."""
import zlib

import numpy as np
import pytest

from rdfind_amd import _lib
from tests import prim_ref

pytestmark = pytest.mark.gpu

# primitives.hip
SCAN_TILE = 256 * 16            # SCAN_TILE = RDF_BLOCK * SCAN_ITEMS
SCAN_SMALL_TILES = 4            # up to here one block scans everything (k_scan_small)
SCAN_FOLD_TILES = 1024          # up to here the apply kernel folds the tile sums; above: k_scan_single + apply
SCAN_BATCH_MAX = 4              # primitives.hpp
RS_TILE = 256 * 16              # RS_TILE = RDF_BLOCK * RS_ITEMS
RS_ROWSCAN_STEP = 1024 * 16     # tiles per loop step of k_radix_rowscan (RS_SCAN_THREADS * RS_SCAN_ITEMS)
RS_MAX_BITS = 9                 # widest digit of a sort (primitives.hpp)

M64 = prim_ref.M64
KINDS = {"u32_u32": _lib.SCAN_U32_U32, "u32_u64": _lib.SCAN_U32_U64, "u64_u64": _lib.SCAN_U64_U64}

SCAN_SIZES = [0, 1, 3, 4, 5, 15, 16, 17, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1,
              SCAN_SMALL_TILES * SCAN_TILE,            # the last single-block size
              SCAN_SMALL_TILES * SCAN_TILE + 1,        # the first folded size
              5 * SCAN_TILE + 2,
              SCAN_FOLD_TILES * SCAN_TILE,             # the last folded size
              SCAN_FOLD_TILES * SCAN_TILE + 1,         # the first k_scan_single size
              (SCAN_FOLD_TILES + 1) * SCAN_TILE + SCAN_TILE + 1]

RADIX_SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, RS_TILE - 1, RS_TILE, RS_TILE + 1, 2 * RS_TILE - 1, 2 * RS_TILE,
               3 * RS_TILE + 1, 5 * RS_TILE - 1,       # 1..5 tiles: every remainder of the padded histogram stride
               40 * RS_TILE + 7]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def rng_for(*key):
    """A generator seeded by the case's name and numbers (the same data in every run)."""
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


# ------------------------------------------------------------------------------------------------
# scans

def scan_values(kind, n, rng):
    """The kind's everyday values: full-range u32 for u32 -> u64 (lane sums pass 2^32), below 2^20 for u64 -> u64,
    small for u32 -> u32 (no wrap)."""
    if kind == _lib.SCAN_U32_U64:
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == _lib.SCAN_U64_U64:
        return rng.integers(0, 1 << 20, n, dtype=np.uint64)
    return rng.integers(0, 16, n, dtype=np.uint64).astype(np.uint32)


def check_scan(ctx, kind, vals, in_skew=0, out_skew=0, in_place=False, want_total=True):
    want, want_sum = prim_ref.exclusive_scan(vals, _lib.SCAN_DTYPES[kind][1])
    got, total, ok = ctx.test_scan(kind, vals, in_skew, out_skew, in_place, want_total)
    what = (kind, len(vals), in_skew, out_skew, in_place, want_total)
    assert ok, ("canaries", what)
    assert got.dtype == want.dtype
    np.testing.assert_array_equal(got, want, err_msg=str(what))
    if want_total:
        assert total == want_sum, what


def scan_variants(kind):
    """(in_skew, out_skew, in_place) combinations of a kind: aligned and skew-1 pointers for the u32 inputs (a skewed
    pointer on either side takes the non-vector kernels), in place where the element types allow it."""
    if kind == _lib.SCAN_U32_U32:
        return [(0, 0, False), (1, 0, False), (0, 1, False), (0, 0, True), (1, 1, True)]
    if kind == _lib.SCAN_U32_U64:
        return [(0, 0, False), (1, 0, False), (0, 1, False)]
    return [(0, 0, False), (0, 0, True), (1, 1, True)]


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("kind", sorted(KINDS), ids=str)
def test_scan_sizes_alignment_in_place_total(ctx, kind, n):
    k = KINDS[kind]
    vals = scan_values(k, n, rng_for("scan", kind, n))
    for in_skew, out_skew, in_place in scan_variants(k):
        for want_total in (True, False):
            check_scan(ctx, k, vals, in_skew, out_skew, in_place, want_total)


@pytest.mark.parametrize("kind", sorted(KINDS), ids=str)
def test_scan_value_patterns(ctx, kind):
    k = KINDS[kind]
    ti = _lib.SCAN_DTYPES[k][0]
    for n in SCAN_SIZES:
        first, last, ends = np.zeros(n, ti), np.zeros(n, ti), np.zeros(n, ti)
        first[:1] = 1
        last[n - 1:] = 1
        ends[SCAN_TILE - 1::SCAN_TILE] = 1  # each tile's last element
        for vals in (np.zeros(n, ti), first, last, ends):
            check_scan(ctx, k, vals)
            if k != _lib.SCAN_U32_U64:
                check_scan(ctx, k, vals, in_place=True)
        check_scan(ctx, k, ends, 1, 0)
        if k != _lib.SCAN_U32_U64:
            check_scan(ctx, k, ends, 1, 1, True)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_u32_wraps_modulo_2_32(ctx, n):
    # sums far past 2^32: the u32 -> u32 scan wraps (unsigned arithmetic), the reference is reduced modulo 2^32
    vals = rng_for("wrap", n).integers(1 << 31, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    check_scan(ctx, _lib.SCAN_U32_U32, vals)
    check_scan(ctx, _lib.SCAN_U32_U32, vals, 1, 1, True)


def check_batch(ctx, rows, skew_mask=0):
    out, ok = ctx.test_scan_batch(rows, skew_mask)
    assert ok, ("canaries", rows.shape, skew_mask)
    for j in range(rows.shape[0]):
        want, total = prim_ref.exclusive_scan(rows[j], np.uint64)
        np.testing.assert_array_equal(out[j, :-1], want, err_msg=str((rows.shape, skew_mask, j)))
        assert int(out[j, -1]) == total, (rows.shape, skew_mask, j)


BATCH_SIZES = [0, 1, SCAN_TILE + 1, SCAN_SMALL_TILES * SCAN_TILE,   # the single-block range: one scan per array
               SCAN_SMALL_TILES * SCAN_TILE + 1, 5 * SCAN_TILE + 2, 37 * SCAN_TILE + 4095,  # the batch kernels
               SCAN_FOLD_TILES * SCAN_TILE,                          # ... their last size
               SCAN_FOLD_TILES * SCAN_TILE + 1]                      # above: the fallback, one scan per array


@pytest.mark.parametrize("n", BATCH_SIZES)
def test_scan_batch(ctx, n):
    rng = rng_for("batch", n)
    for k in range(1, SCAN_BATCH_MAX + 1):
        rows = rng.integers(0, 1 << 32, (k, n), dtype=np.uint64).astype(np.uint32)
        check_batch(ctx, rows)
        check_batch(ctx, rows, 1 << (k - 1))        # one input skewed: the non-vector batch kernels
        check_batch(ctx, rows, 1 << 4)              # one output skewed


@pytest.mark.parametrize("k", [0, SCAN_BATCH_MAX + 1])
def test_scan_batch_refuses_bad_counts(ctx, k):
    rows = np.ones((max(k, 1), 5 * SCAN_TILE + 2), np.uint32)
    with pytest.raises(_lib.RdfError) as e:
        ctx.test_scan_batch(rows, 0, k=k)
    assert e.value.status not in (None, 0)
    assert ctx.test_canaries_ok  # (and the outputs still hold the fill pattern: checked by the entry point)
    check_batch(ctx, rows[:1])  # the context goes on working


# ------------------------------------------------------------------------------------------------
# radix sort / partition

def place_bits(field, idx, lo, hi, width):
    """Keys with ``field`` in bits [lo, hi) and as much of the element index ``idx`` as fits in the bits outside it
    (low part below lo, the rest from hi up): a stable result lists equal fields in ascending index order, so a rank
    error that keeps the multiset but not the order shows."""
    key = field.astype(np.uint64) << np.uint64(lo)
    if lo:
        key |= idx & np.uint64((1 << lo) - 1)
    if hi < width:
        key |= ((idx >> np.uint64(lo)) << np.uint64(hi)) & np.uint64((1 << width) - 1)
    return key


def key_shapes(n, lo, hi, width, rng):
    """name -> keys of ``width`` bits whose bits [lo, hi) are the sorted field."""
    fb = max(hi - lo, 0)
    full = np.uint64((1 << width) - 1)
    idx = np.arange(n, dtype=np.uint64)
    rnd = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False) & full
    fmax = (1 << fb) - 1
    some = rng.integers(0, min(fmax, 4) + 1, n, dtype=np.uint64)
    two = np.where(rng.integers(0, 2, n) == 1, np.uint64(fmax), np.uint64(fmax >> 1))
    asc = idx & np.uint64(fmax)
    shapes = {
        "random": rnd,
        "equal": np.full(n, rnd[0] if n else 0, np.uint64),          # one digit owns the whole tile
        "two_valued": place_bits(two, idx, lo, hi, width) if fb else rnd,
        "ascending": place_bits(asc, idx, lo, hi, width) if fb else idx & full,
        "descending": place_bits(np.uint64(fmax) - asc, idx, lo, hi, width) if fb else (full - idx) & full,
        "stability": place_bits(some, idx, lo, hi, width) if fb else rnd,
    }
    return shapes


def check_radix(ctx, op, keys, want, lo=0, hi=64, hmask=M64, what=()):
    got, ok = ctx.test_radix(op, keys, lo, hi, hmask)
    assert ok, ("canaries", op, len(keys), lo, hi, what)
    assert got.shape == want.shape, (op, len(keys), lo, hi, what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=str((op, len(keys), lo, hi, what)))


SORT_WINDOWS = [(0, 1), (0, 8), (0, 9), (0, 10),   # (0, 10): two passes of 5 bits
                (0, 17),                           # 9 then 8 bits
                (0, 43), (0, 64), (32, 33), (32, 45), (58, 64), (63, 64),
                (0, 0), (9, 9), (20, 4)]           # hi <= lo: the identity


@pytest.mark.parametrize("n", RADIX_SIZES)
def test_radix_sort_u64_bits(ctx, n):
    for lo, hi in SORT_WINDOWS:
        for name, keys in key_shapes(n, lo, hi, 64, rng_for("sort", n, lo, hi)).items():
            check_radix(ctx, _lib.RADIX_SORT_BITS, keys, prim_ref.sort_bits(keys, lo, hi), lo, hi, what=name)


def test_radix_sort_pass_counts(ctx):
    for bits in sorted({hi - lo for lo, hi in SORT_WINDOWS if hi > lo}):
        assert ctx.lib.rdf_test_radix_passes(bits) == -(-bits // RS_MAX_BITS), bits
    assert ctx.lib.rdf_test_radix_passes(0) == 0


@pytest.mark.parametrize("n", RADIX_SIZES)
def test_radix_partition_u32(ctx, n):
    for lo, hi in [(0, 8), (14, 29), (15, 32), (31, 32), (8, 8)]:
        for name, keys in key_shapes(n, lo, hi, 32, rng_for("u32", n, lo, hi)).items():
            keys = keys.astype(np.uint32)
            check_radix(ctx, _lib.RADIX_PART_U32, keys, prim_ref.sort_bits(keys, lo, hi), lo, hi, what=name)


@pytest.mark.parametrize("n", RADIX_SIZES)
def test_radix_partition_hashed(ctx, n):
    # (RDFIND_PART_DIGIT stays at its default: it is read once per process)
    for bits in (1, 9, 10, 20, 30):
        for hmask in (M64, M64 & ~0xFFFF):
            rng = rng_for("hashed", n, bits, hmask & 0xFFFFFF)
            shapes = key_shapes(n, 0, 64, 64, rng)
            idx = np.arange(n, dtype=np.uint64)
            # few distinct hashed parts, the element index in the 16 bits the second mask leaves out of the hash
            shapes["stability"] = (rng.integers(0, 5, n, dtype=np.uint64) << np.uint64(16)) | (idx & np.uint64(0xFFFF))
            shapes["two_valued"] = np.where(idx % np.uint64(3) == 0, np.uint64(0x1234_0000), np.uint64(M64))
            for name, keys in shapes.items():
                check_radix(ctx, _lib.RADIX_PART_HASHED, keys, prim_ref.partition_hashed(keys, bits, hmask), 0, bits, hmask,
                            what=(name, hex(hmask)))


def padded(keys, pattern):
    """``keys`` with the padding key ~0 written by ``pattern``."""
    k = keys.copy()
    n = k.shape[0]
    if pattern == "all":
        k[:] = prim_ref.PAD
    elif pattern == "alternate":
        k[1::2] = prim_ref.PAD
    elif pattern == "last_tile" and n:
        k[(n - 1) // RS_TILE * RS_TILE:] = prim_ref.PAD
    return k


@pytest.mark.parametrize("n", RADIX_SIZES)
def test_radix_sort_u64_drop(ctx, n):
    for bits in (1, 8, 9, 10, 17, 43, 64):
        rng = rng_for("drop", n, bits)
        low_ones = np.uint64((1 << bits) - 1)  # bits < 64: the sorted bits all ones, but not the padding key: kept
        for name, keys in key_shapes(n, 0, bits, 64, rng).items():
            if name == "equal" and n and keys[0] == prim_ref.PAD:
                keys = keys - np.uint64(1)
            for pattern in ("none", "all", "alternate", "last_tile"):
                k = padded(keys, pattern)
                if n and bits < 64 and pattern != "all":
                    at = np.unique(rng.integers(0, n, 3))
                    k[at] = low_ones                            # exactly (1 << bits) - 1
                    k[(at + 1) % n] = low_ones | np.uint64(1 << 63)  # ... and with a bit above the sorted ones
                want = prim_ref.sort_drop(k, bits)
                check_radix(ctx, _lib.RADIX_SORT_DROP, k, want, 0, bits, what=(name, pattern))


def test_radix_partition_u32_crosses_the_rowscan_step(ctx):
    """One more tile than k_radix_rowscan covers in one step of its loop (256 MiB of keys, a single 8-bit pass): the
    only test of that loop's second step outside the full-size goldens."""
    n = RS_ROWSCAN_STEP * RS_TILE + 1
    keys = rng_for("rowscan").integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    got, ok = ctx.test_radix(_lib.RADIX_PART_U32, keys, 0, 8)
    assert ok
    want = prim_ref.sort_bits(keys, 0, 8)
    assert got.shape == want.shape
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------
# the entry points leave the pipeline alone

def test_primitive_calls_leave_a_run_intact():
    rng = rng_for("run")
    with _lib.Context(0) as ctx:
        _run_around_primitive_calls(ctx, rng)


def _run_around_primitive_calls(ctx, rng):
    check_scan(ctx, _lib.SCAN_U32_U32, scan_values(_lib.SCAN_U32_U32, SCAN_TILE + 1, rng))
    with pytest.raises(_lib.RdfError):
        ctx.test_paths()  # no completed run: the primitive call did not move the stage
    s, p, o = (rng.integers(0, 12, 300).astype(np.uint32) for _ in range(3))
    ctx.set_triples(s, p, o, 12)
    ctx.run(2)
    before = (ctx.cind_count(), ctx.checksum(), ctx.test_paths())
    check_scan(ctx, _lib.SCAN_U32_U64, scan_values(_lib.SCAN_U32_U64, 5 * SCAN_TILE + 2, rng))
    keys = rng.integers(0, 1 << 63, 3 * RS_TILE + 1, dtype=np.uint64)
    check_radix(ctx, _lib.RADIX_SORT_BITS, keys, prim_ref.sort_bits(keys, 0, 43), 0, 43)
    assert (ctx.cind_count(), ctx.checksum(), ctx.test_paths()) == before
    ctx.run(2)
    assert (ctx.cind_count(), ctx.checksum(), ctx.test_paths()) == before
