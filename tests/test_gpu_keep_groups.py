"""The record-tile kernels of the group build (rdfind_amd/csrc/kernels.inl: k_fresh_bounds, k_keep_scatter, k_group_flags,
k_group_build / k_group_build_at), called directly through rdf_test_keep_records and rdf_test_group_build on sorted
records made here, and compared exactly with numpy (np.unique, cumsum).  The kernels rank fresh records and group heads
inside tiles of T consecutive records and carry one count per tile between them, so the shapes put runs, capture
boundaries and group heads on, across and next to the tile edges.  Every call reports whether the canaries around its
device buffers survived."""
import zlib

import numpy as np
import pytest

from rdfind_amd import _lib

pytestmark = pytest.mark.gpu

JB = 20  # join bits of the keep tests' records
PATTERN = np.uint32(0xA5A5A5A5)  # RDF_TEST_CANARY_BYTE: what gmap holds at join values without records


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T(ctx):
    t = ctx.test_record_tile()
    assert t >= 256 and t % 256 == 0
    return t


def rng_for(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def records(spec, rng=None, joinbits=JB):
    """Sorted records of spec = [(capture, distinct joins, copies)]: the capture's joins are 3 * arange + capture % 3 and
    each record is there `copies` times (copies 0: 1..3 times, drawn)."""
    out = []
    for cap, distinct, copies in spec:
        j = 3 * np.arange(distinct, dtype=np.uint64) + np.uint64(cap % 3)
        rep = rng.integers(1, 4, distinct) if copies == 0 else np.full(distinct, copies)
        out.append(np.repeat((np.uint64(cap) << np.uint64(joinbits)) | j, rep))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def keep_ref(keys, joinbits, ncap, ms):
    uk = np.unique(keys)
    caps = (uk >> np.uint64(joinbits)).astype(np.int64)
    support = np.bincount(caps, minlength=ncap).astype(np.uint32)
    freq = support >= ms
    fidx = np.cumsum(freq) - freq
    kept = uk[freq[caps]]
    c = fidx[(kept >> np.uint64(joinbits)).astype(np.int64)].astype(np.uint64)
    j = kept & np.uint64((1 << joinbits) - 1)
    doff = np.concatenate([[0], np.cumsum(support[freq], dtype=np.uint64)]).astype(np.uint64)
    return support, (c << np.uint64(32)) | j, (j << np.uint64(32)) | c, doff


def check_keep(ctx, keys, ncap, ms, joinbits=JB):
    assert (np.diff(keys.astype(np.int64)) >= 0).all()
    sup, dk, fk, doff, ok = ctx.test_keep_records(keys, joinbits, ncap, ms)
    assert ok, "a canary around a device buffer was overwritten"
    rsup, rdk, rfk, rdoff = keep_ref(keys, joinbits, ncap, ms)
    assert np.array_equal(sup, rsup)
    assert np.array_equal(doff, rdoff)
    assert dk.shape[0] == rdk.shape[0] == int(rdoff[-1])  # Jf
    assert np.array_equal(dk, rdk)
    assert np.array_equal(fk, rfk)
    return rsup, rdk


def random_records(rng, n, ncap):
    """n sorted records with repeats: few joins per capture, captures drawn with a skew."""
    caps = np.minimum(rng.integers(0, ncap, n), rng.integers(0, ncap, n)).astype(np.uint64)
    joins = rng.integers(0, 6, n).astype(np.uint64)
    return np.sort((caps << np.uint64(JB)) | joins)


@pytest.mark.parametrize("which", ["0", "1", "T-1", "T", "T+1", "3T+5"])
def test_keep_sizes(ctx, T, which):
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[which]
    keys = random_records(rng_for("keep_sizes", n), n, 300)
    for ms in (1, 3):
        check_keep(ctx, keys, 300, ms)


def test_keep_capture_over_three_tiles(ctx, T):
    # capture 5 holds the whole of tiles 1-3 and parts of tiles 0 and 4: no head inside three tiles in a row
    keys = records([(1, 10, 2), (5, 4 * T, 1), (7, 20, 3)])
    sup, _ = check_keep(ctx, keys, 9, 2)
    assert sup[5] == 4 * T
    keys = records([(1, 10, 2), (5, 2 * T, 0), (7, 20, 3)], rng_for("three_tiles"))  # ... with repeated records
    assert keys.shape[0] > 3 * T + 40
    check_keep(ctx, keys, 9, 2)
    check_keep(ctx, keys, 9, 2 * T + 1)  # the large capture infrequent: everything after it moves up by its records


def test_keep_equal_run_across_tile_edge(ctx, T):
    # records T-3 .. T+3 are one key: the second tile's first record is not fresh
    head = records([(2, T - 3, 1)])
    run = np.full(7, (3 << JB) | 9, np.uint64)
    tail = records([(3, 40, 2), (4, 5, 1)])[1:]
    keys = np.concatenate([head, run, tail[tail > run[0]]])
    assert keys[T - 1] == keys[T] == run[0] and keys[T - 4] != run[0]
    check_keep(ctx, keys, 6, 1)
    check_keep(ctx, keys, 6, 6)
    # ... and a run of one key over a whole tile and both its edges
    keys = np.concatenate([records([(2, T - 2, 1)]), np.full(T + 5, (3 << JB) | 1, np.uint64), records([(4, 9, 1)])])
    check_keep(ctx, keys, 6, 1)


def test_keep_capture_boundary_on_tile_edge(ctx, T):
    keys = records([(0, T, 1), (1, T // 2, 2), (2, 7, 1)])  # capture 1 starts at T, capture 2 at 2T
    assert keys[T - 1] >> np.uint64(JB) == 0 and keys[T] >> np.uint64(JB) == 1 and keys[2 * T] >> np.uint64(JB) == 2
    sup, _ = check_keep(ctx, keys, 3, 8)
    assert list(sup) == [T, T // 2, 7]
    check_keep(ctx, keys, 3, T)
    keys = records([(0, T, 1), (1, T, 1)])  # the last capture ends with the last tile
    check_keep(ctx, keys, 2, 1)


def test_keep_all_records_equal(ctx, T):
    keys = np.full(2 * T + 7, (4 << JB) | 77, np.uint64)
    sup, dk = check_keep(ctx, keys, 6, 1)
    assert sup[4] == 1 and sup.sum() == 1 and dk.shape[0] == 1
    check_keep(ctx, keys, 6, 2)


def test_keep_every_capture_infrequent(ctx, T):
    keys = records([(c, 1 + c % 5, 0) for c in range(0, 900, 2)], rng_for("infrequent"))
    assert keys.shape[0] > T
    _, dk = check_keep(ctx, keys, 900, 6)
    assert dk.shape[0] == 0


def test_keep_alternating_frequent_infrequent(ctx, T):
    # supports 5, 4, 5, 4, ...: min support 5 is one capture's support and one more than its neighbour's
    keys = records([(c, 5 - (c & 1), 0) for c in range(700)], rng_for("alternating"))
    assert keys.shape[0] > 2 * T
    sup, dk = check_keep(ctx, keys, 700, 5)
    assert dk.shape[0] == 5 * 350
    check_keep(ctx, keys, 700, 4)
    check_keep(ctx, keys, 700, 1)  # min support 1: every distinct record is kept


def test_keep_absent_captures(ctx, T):
    # more than 64 absent capture ids before the first capture, between two, and from the last one to ncap - 1
    spec = [(100, 30, 0), (101, 2, 1), (400, T, 0), (401, 3, 2), (1000, 12, 1)]
    keys = records(spec, rng_for("gaps"))
    assert keys.shape[0] > T
    sup, _ = check_keep(ctx, keys, 1500, 3)
    assert sup[:100].sum() == 0 and sup[102:400].sum() == 0 and sup[1001:].sum() == 0
    check_keep(ctx, keys, 1500, 1)
    check_keep(ctx, keys, 1001, 3)  # the last record belongs to capture ncap - 1
    check_keep(ctx, keys[: -12], 402, 4)  # ... and that capture is infrequent


def test_keep_wide_joins(ctx, T):
    # 32 join bits: dk / fk carry the whole join value
    rng = rng_for("wide")
    n = T + 100
    caps = np.sort(rng.integers(0, 40, n)).astype(np.uint64)
    keys = np.sort((caps << np.uint64(32)) | rng.integers(0xFFFFFF00, 1 << 32, n).astype(np.uint64))
    check_keep(ctx, keys, 40, 2, joinbits=32)


# ---- groups -----------------------------------------------------------------------------------------------------

def group_ref(fk, V, rbase, gbase):
    joins = (fk >> np.uint64(32)).astype(np.int64)
    uj, first = np.unique(joins, return_index=True)
    goff = np.concatenate([first + rbase, [rbase + fk.shape[0]]]).astype(np.uint64)
    gmap = np.full(V, PATTERN, np.uint32)
    gmap[uj] = gbase + np.arange(uj.shape[0], dtype=np.uint32)
    return goff, (fk & np.uint64(0xFFFFFFFF)).astype(np.uint32), gmap


def check_groups(ctx, joins, V=None, rbase=0, gbase=0):
    joins = np.asarray(joins, np.uint64)
    V = int(joins.max()) + 1 if V is None else V
    # the captures of a group ascend in the pipeline; any values do here
    fk = (joins << np.uint64(32)) | (np.arange(joins.shape[0], dtype=np.uint64) * np.uint64(7) % np.uint64(1000003))
    goff, gcap, gmap, ok = ctx.test_group_build(fk, V, rbase, gbase)
    assert ok, "a canary around a device buffer was overwritten, or something before rbase / gbase was written"
    rgoff, rgcap, rgmap = group_ref(fk, V, rbase, gbase)
    assert np.array_equal(goff, rgoff)
    assert np.array_equal(gcap, rgcap)
    assert np.array_equal(gmap, rgmap)
    return goff.shape[0] - 1


def sized(sizes, first=0, step=1):
    """join values first, first + step, ... with the given group sizes"""
    return np.repeat(first + step * np.arange(len(sizes), dtype=np.uint64), sizes)


@pytest.mark.parametrize("which", ["0", "1", "T-1", "T", "T+1", "3T+5"])
def test_group_sizes(ctx, T, which):
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[which]
    joins = np.sort(rng_for("group_sizes", n).integers(0, max(n // 3, 1), n)).astype(np.uint64)
    check_groups(ctx, joins, V=max(n // 3, 1) + 5)
    if n:
        check_groups(ctx, joins, V=max(n // 3, 1) + 5, rbase=1000, gbase=77)  # a join range's groups (k_group_build_at)


def test_group_every_record_its_own(ctx, T):
    assert check_groups(ctx, np.arange(2 * T + 3, dtype=np.uint64)) == 2 * T + 3


def test_group_over_three_tiles(ctx, T):
    assert check_groups(ctx, sized([9, 4 * T, 30], first=2)) == 3  # tiles 1-3 hold no head
    assert check_groups(ctx, sized([3 * T + 11])) == 1


def test_group_head_at_tile_start_and_end_at_tile_end(ctx, T):
    check_groups(ctx, sized([T, 3, T - 3, 5]))       # heads at T and at 2T
    check_groups(ctx, sized([10, 2 * T - 10, 7]))    # a group over a tile edge that ends with tile 1
    check_groups(ctx, sized([T - 1, 1, 1, T - 1]))   # one-record groups on both sides of the edge
    check_groups(ctx, sized([5, 2 * T - 5]))         # the last group ends with the last tile


def test_group_joins_with_gaps(ctx, T):
    rng = rng_for("join_gaps")
    values = np.sort(rng.choice(200000, 900, replace=False)).astype(np.uint64)
    joins = np.repeat(values, rng.integers(1, 9, 900))
    assert joins.shape[0] > T
    check_groups(ctx, joins, V=200000)
    check_groups(ctx, joins, V=200000, rbase=12345, gbase=4000)
