"""The record sort's first pass over a producer's segments (radix_seg_first_pass + radix_sort_u64_rest in
rdfind_amd/csrc/primitives.hip), called directly through rdf_test_radix_segments: the keys lie in disjoint segments of a
larger array, the call builds the segments' histogram of the first digit on the host, and the result must be
numpy.sort of the segments' keys.  Every call reports whether the canaries around its device buffers survived.

RS_TILE mirrors primitives.hip: a segment longer than it is walked in several sub-tiles, whose digit positions carry
over in LDS."""
import zlib

import numpy as np
import pytest

from rdfind_amd import _lib

pytestmark = pytest.mark.gpu

RS_TILE = 256 * 16
RDF_ERR_ARG, RDF_ERR_LIMIT = -1, -5  # include/rdfind_hip.h
GAP_FILL = np.uint64(0x5A5A5A5A5A5A5A5A)  # the keys between the segments (never part of the result)

# name -> segment lengths
SHAPES = {
    "edges": [0, 1, RS_TILE - 1, RS_TILE, RS_TILE + 1, 3 * RS_TILE + 5],
    "one": [2 * RS_TILE + 3],
    "three": [700, 0, RS_TILE + 9],
    "five": [5, RS_TILE, 0, 63, 2 * RS_TILE + 1],  # a column count that is no multiple of the histogram's row padding
    "all_empty": [0, 0, 0],
}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def rng_for(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def layout(lengths, rng, strided):
    """(src, bases or None, stride, the segments' keys in order): segments at b * stride, or at bases with random gaps."""
    if strided:
        stride = max(lengths) + 7
        bases = [b * stride for b in range(len(lengths))]
        total = stride * len(lengths)
    else:
        stride, bases, at = 0, [], 3
        for n in lengths:
            bases.append(at)
            at += n + int(rng.integers(1, 40))
        total = at
    src = np.full(total, GAP_FILL, np.uint64)
    return src, (None if strided else np.array(bases, np.uint64)), stride, bases


def fill(src, bases, lengths, bits, rng, same_digit_bits=0):
    keys = []
    for b, n in zip(bases, lengths):
        k = rng.integers(0, 1 << bits, n, dtype=np.uint64)
        if same_digit_bits:  # every key with the same first digit
            k = (k >> np.uint64(same_digit_bits) << np.uint64(same_digit_bits)) | np.uint64(0x155 & ((1 << same_digit_bits) - 1))
        src[b:b + n] = k
        keys.append(k)
    return np.concatenate(keys) if keys else np.zeros(0, np.uint64)


@pytest.mark.parametrize("strided", [False, True], ids=["bases", "stride"])
@pytest.mark.parametrize("bits", [17, 43])
@pytest.mark.parametrize("w0", [8, 9])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_segment_sort_matches_numpy(ctx, shape, w0, bits, strided):
    lengths = SHAPES[shape]
    rng = rng_for(shape, w0, bits, int(strided))
    src, bases, stride, at = layout(lengths, rng, strided)
    keys = fill(src, at, lengths, bits, rng)
    got, ok = ctx.test_radix_segments(src, lengths, bases, stride, w0, bits)
    assert ok, ("canaries", shape, w0, bits, strided)
    np.testing.assert_array_equal(got, np.sort(keys))


@pytest.mark.parametrize("w0", [8, 9])
def test_one_first_digit(ctx, w0):
    """Every key in the same bin of the first pass: one digit's run takes the whole output."""
    lengths = SHAPES["edges"]
    rng = rng_for("same", w0)
    src, bases, stride, at = layout(lengths, rng, False)
    keys = fill(src, at, lengths, 43, rng, same_digit_bits=w0)
    assert len(set((keys & np.uint64((1 << w0) - 1)).tolist())) == 1
    got, ok = ctx.test_radix_segments(src, lengths, bases, stride, w0, 43)
    assert ok
    np.testing.assert_array_equal(got, np.sort(keys))


def test_default_width_is_the_sorts_own(ctx):
    """w0 = 0: the width the whole sort gives its first pass (43 bits: 9 of 9+9+9+8+8)."""
    lengths = SHAPES["three"]
    rng = rng_for("default")
    src, bases, stride, at = layout(lengths, rng, False)
    keys = fill(src, at, lengths, 43, rng)
    assert _lib.load().rdf_test_radix_passes(43) == 5
    got, ok = ctx.test_radix_segments(src, lengths, bases, stride, 0, 43)
    assert ok
    np.testing.assert_array_equal(got, np.sort(keys))


@pytest.mark.parametrize("w0", [8, 9])
def test_overstated_histogram_is_an_error(ctx, w0):
    """A histogram that claims one key more of one digit than its segment holds: RDF_ERR_LIMIT, intact canaries (the
    scatter's writes are bounded, and a segment that does not match its column is reported)."""
    lengths = SHAPES["edges"]
    rng = rng_for("bump", w0)
    src, bases, stride, at = layout(lengths, rng, False)
    fill(src, at, lengths, 43, rng)
    for seg, digit in ((3, 5), (0, (1 << w0) - 1), (5, 0)):
        with pytest.raises(_lib.RdfError) as e:
            ctx.test_radix_segments(src, lengths, bases, stride, w0, 43, bump=(seg, digit, 1))
        assert e.value.status == RDF_ERR_LIMIT, str(e.value)
        assert ctx.test_canaries_ok
    # ... and the context still sorts
    keys = fill(src, at, lengths, 43, rng)
    got, ok = ctx.test_radix_segments(src, lengths, bases, stride, w0, 43)
    assert ok
    np.testing.assert_array_equal(got, np.sort(keys))


def test_bad_layouts_are_refused(ctx):
    src = np.zeros(100, np.uint64)
    for lengths, bases in (([60, 60], [0, 50]), ([10], [95]), ([101], [0])):
        with pytest.raises(_lib.RdfError) as e:
            ctx.test_radix_segments(src, lengths, np.array(bases, np.uint64), 0, 8, 17)
        assert e.value.status == RDF_ERR_ARG
