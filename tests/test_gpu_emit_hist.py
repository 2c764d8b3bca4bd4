"""K3 hands the record sort its first digit histogram (RDFIND_EMIT_HIST, default on): the emission blocks count the low
join bits of their kept records, and the sort's first pass scatters straight from the blocks' regions.  With the switch
off the regions are compacted and the sort counts its first digit itself.  Both forms must build the same groups and
find the same CINDs, and rdf_test_paths must say which one ran.

RDFIND_EMIT_GRID caps the emission grid, so that a small input's blocks emit regions of several sort sub-tiles."""
import random

import numpy as np
import pytest

from rdfind_amd import _lib
from tests.test_gpu import expected_set, gpu_set

pytestmark = pytest.mark.gpu

MODES = [(1, True), (0, True), (0, False)]


@pytest.fixture(scope="module")
def pairs():
    """(grid cap or None) -> (context with the histogram from K3, context without); the switches are read at creation."""
    mp = pytest.MonkeyPatch()
    made = {}

    def get(grid=None):
        if grid not in made:
            if grid is not None:
                mp.setenv("RDFIND_EMIT_GRID", str(grid))
            mp.setenv("RDFIND_EMIT_HIST", "1")
            on = _lib.Context(0)
            mp.setenv("RDFIND_EMIT_HIST", "0")
            off = _lib.Context(0)
            mp.undo()
            made[grid] = (on, off)
        return made[grid]

    yield get
    for on, off in made.values():
        on.close()
        off.close()
    mp.undo()


def random_triples(seed, n, nv, npred):
    rng = random.Random(seed)
    return np.array([(rng.randrange(nv), rng.randrange(npred), rng.randrange(nv)) for _ in range(n)], dtype=np.uint32)


def run_both(on, off, arr, nv, ms, strategy, clean, what, records=None):
    """Both forms on one input: the same records, groups and CINDs; the path report names the form.  Returns the
    histogram form's decoded CIND set."""
    got = gpu_set(on, arr, nv, ms, strategy, clean)
    gpu_set(off, arr, nv, ms, strategy, clean)
    ton, toff = on.test_paths(), off.test_paths()
    n = arr.shape[0]
    assert ton["k3_form"] == toff["k3_form"] == ("onepass" if n else None), what
    assert ton["k3_hist"] == (n > 0) and not toff["k3_hist"], what
    for key in ("n_records", "n_sorted_records", "n_groups", "n_frequent_records", "n_captures"):
        assert on.groups[key] == off.groups[key], (what, key)
    if records is not None:
        assert (on.groups["n_records"] > 0) == records, what
    assert (on.cind_count(), on.checksum()) == (off.cind_count(), off.checksum()), what
    return got


def test_small_random_inputs_both_forms_and_oracle(pairs):
    """One emission block (n < 256) and a few blocks whose triples per block are no multiple of the block size; every
    mode, strategy 0 included, against the oracle."""
    on, off = pairs()
    rng = random.Random(5200)
    sizes = [1, 7, 255, 256, 257, 600, 1999]  # 600: 3 blocks of 200 triples; 1999: 8 blocks of 250
    for n in sizes:
        nv = rng.randrange(4, 80)
        ms = rng.randrange(1, 4)
        arr = random_triples(5200 + n, n, nv, nv // 3 + 1)
        for strategy, clean in MODES:
            what = (n, nv, ms, strategy, clean)
            got = run_both(on, off, arr, nv, ms, strategy, clean, what)
            assert got == expected_set(arr, nv, ms, strategy, clean), what


def test_no_frequent_condition(pairs):
    """No condition reaches the support: K3 emits no record, every segment is empty."""
    on, off = pairs()
    nv = 3000
    arr = np.stack([np.arange(1000, dtype=np.uint32), 1000 + np.arange(1000, dtype=np.uint32),
                    2000 + np.arange(1000, dtype=np.uint32)], 1)
    got = run_both(on, off, arr, nv, 2, 1, True, "no frequent condition", records=False)
    assert got == set()


def test_regions_of_several_sub_tiles(pairs):
    """20k triples from 4 emission blocks (RDFIND_EMIT_GRID=4): each block's region holds several 4096-record sub-tiles
    of the sort's first pass, whose digit positions carry over; few predicates put most records into a few bins."""
    on, off = pairs(4)
    arr = random_triples(77, 20000, 1500, 12)
    for strategy, clean in ((1, True), (0, True)):
        run_both(on, off, arr, 1500, 3, strategy, clean, ("grid4", strategy, clean), records=True)
    assert on.groups["n_sorted_records"] > 4 * 4096  # (more than one sub-tile per region)
    # ... and the default grid on the same input (79 blocks of 254 triples) builds the same groups
    d_on, d_off = pairs()
    run_both(d_on, d_off, arr, 1500, 3, 0, True, "grid default", records=True)
    # (the sorted records' number follows the grid: repeats are dropped per iteration of 256 triples of one block; the
    # distinct records, the groups and the result do not)
    for key in ("n_records", "n_frequent_records", "n_groups", "n_captures"):
        assert d_on.groups[key] == on.groups[key], key
    assert (d_on.cind_count(), d_on.checksum()) == (on.cind_count(), on.checksum())


def test_grid_cap_small_inputs_vs_oracle(pairs):
    """The capped grid on inputs small enough for the oracle: blocks of several iterations each."""
    on, off = pairs(4)
    for n in (5, 1030, 3001):
        arr = random_triples(900 + n, n, 40, 9)
        for strategy, clean in MODES:
            what = ("grid4", n, strategy, clean)
            assert run_both(on, off, arr, 40, 2, strategy, clean, what) == expected_set(arr, 40, 2, strategy, clean), what


# ---------------------------------------------------------------------------------------------------------------------
# sharded runs: a rank's K3 selects its join shard (the lazy form of the emission kernel) and takes the same path

def _shard_worker(rank, world, port, cases, q, env):
    import os

    os.environ.update(env)  # library switches (read when a context is created)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rdfind_amd import _lib as lib, distributed

    try:
        out = []
        with lib.Context(0) as ctx:
            for s, p, o, nv, ms, strategy, clean in cases:
                ctx.set_triples(s, p, o, nv)
                gs, _ = distributed.run_sharded(ctx, ms, "spo", clean, strategy)
                t = ctx.test_paths()
                out.append({"n": ctx.cind_count(), "checksum": ctx.checksum(), "k3_hist": t["k3_hist"],
                            "k3_form": t["k3_form"], "sorted": gs["n_sorted_records"], "records": gs["n_records"]})
        q.put((rank, out))
    except Exception as e:  # report instead of hanging the parent
        import traceback

        q.put((rank, repr(e) + "\n" + traceback.format_exc()[-1500:]))
    finally:
        dist.destroy_process_group()


def _run_world2(cases, env):
    import torch.multiprocessing as tmp

    from tests.test_gpu_sharded import _free_port

    mpc = tmp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_shard_worker, args=(r, 2, port, cases, q, env)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            r, item = q.get(timeout=300)
            assert not isinstance(item, str), f"rank {r}: {item}"
            res[r] = item
    finally:
        for p in procs:
            p.join(timeout=5 if len(res) < 2 else 60)
            if p.is_alive():
                p.terminate()
    return res


def test_world2_sharded_both_forms_match_single_gpu():
    """Two gloo ranks, each emitting its join shard: with the histogram from K3 and without it the ranks' CINDs add up to
    the single-GPU result, every rank reports the form its switch asks for, and both forms emit the same records."""
    cases = []
    for k, (n, nv) in enumerate(((300, 30), (1999, 60), (6000, 400))):
        arr = random_triples(7300 + n, n, nv, nv // 3 + 1)
        strategy, clean = MODES[k % len(MODES)]
        cases.append((arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy(), nv, 2, strategy, clean))
    single = []
    with _lib.Context(0) as g:
        for s, p, o, nv, ms, strategy, clean in cases:
            g.set_triples(s, p, o, nv)
            g.run(ms, "spo", clean, strategy)
            single.append((g.cind_count(), g.checksum()))
    res = {hist: _run_world2(cases, {"RDFIND_EMIT_HIST": hist}) for hist in ("1", "0")}
    for k, (n_single, h_single) in enumerate(single):
        for hist in ("1", "0"):
            parts = [res[hist][r][k] for r in range(2)]
            assert sum(p["n"] for p in parts) == n_single, (k, hist)
            assert sum(p["checksum"] for p in parts) % (1 << 64) == h_single, (k, hist)
            for p in parts:  # (a rank receives triples of every case: the emission ran)
                assert p["k3_form"] == "onepass" and p["k3_hist"] == (hist == "1"), (k, hist, p)
        for r in range(2):  # (the emitted records; the sorted ones follow the order in which the routing kernel's LDS
            # cursors placed the received triples, which differs from run to run: repeats are dropped per 256 triples)
            assert res["1"][r][k]["records"] == res["0"][r][k]["records"], (k, r)
