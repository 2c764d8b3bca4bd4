"""Result statistics on the device (rdf_cind_stats_begin / _add / _end, rdf_cind_histogram, rdf_copy_top_refs and the
driver's --cind-statistics) against the CPU reference (tests/cind_stats_ref.py), always by exact equality.  The
reference is fed the oracle's rows, or (synthetic configs) the device's rows after the oracle has pinned them."""
import os
import queue
import random
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import c_oracle as C
from rdfind_amd import _lib, ntriples, program
from tests import cind_stats_ref as ref
from tests.conftest import GOLDEN
from tests.parity import assert_shape_rows, assert_stream_matches, dataset, shape_rows
from tests.test_gpu import MODES, expected_set
from tests.test_oracle import read_golden

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ERR_STATE = -4


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def hist_list(rows):
    return [tuple(int(x) for x in r) for r in rows.tolist()]


def top_ids(g):
    """Every referenced capture of the last statistics as (external capture id, cinds)."""
    t = g.top_refs(g.result_layout()["n_captures"] + 1)
    return [(int(c), int(n)) for c, n in t.tolist()]


def top_decoded(g):
    """... as ((code, v1, v2 or None), cinds), the reference's form."""
    t = top_ids(g)
    code, v1, v2 = _lib.decode_captures(np.array([c for c, _ in t], np.uint32), g.num_terms, g.binary_keys())
    return [((int(c), int(a), None if int(b) == NONE else int(b)), n)
            for c, a, b, (_, n) in zip(code, v1, v2, t)]


def device_stats(g):
    """(rows, top) of rdf_cind_histogram on the current result."""
    return hist_list(g.cind_histogram()), top_decoded(g)


def random_input(rng):
    n = rng.randrange(20, 400)
    nv = rng.randrange(4, 40)
    ms = rng.randrange(1, 4)
    arr = np.array([(rng.randrange(nv), rng.randrange(nv // 4 + 1), rng.randrange(nv)) for _ in range(n)], dtype=np.uint32)
    return arr, nv, ms


def test_empty_result(ctx):
    two = np.array([[0, 1, 2], [1, 1, 2]], np.uint32)
    ctx.set_triples(two[:, 0], two[:, 1], two[:, 2], 3)
    ctx.run(1000)  # a support above every count
    assert ctx.cind_count() == 0
    assert device_stats(ctx) == ([], [])
    assert ctx.hist_rows == 0 and len(ctx.top_refs(10)) == 0
    empty = np.zeros((0, 3), np.uint32)
    ctx.set_triples(empty[:, 0], empty[:, 1], empty[:, 2], 1)
    ctx.run(1)
    assert device_stats(ctx) == ([], [])


def test_single_cind(ctx):
    # s[p=0] = {a, b} within s[p=1] = {a, b, c}; every object is distinct, so no other condition reaches support 2
    arr = np.array([[10, 0, 2], [11, 0, 3], [10, 1, 4], [11, 1, 5], [12, 1, 6]], np.uint32)
    exp, _ = C.run_set(arr[:, 0], arr[:, 1], arr[:, 2], 13, 2, 1, True, "s")
    assert exp == {(10, 0, None, 10, 1, None, 2)}
    ctx.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], 13)
    ctx.run(2, "s")
    assert device_stats(ctx) == ref.statistics(exp) == \
        ([(1, (10 << 8) | 10, 1), (2, 2, 1), (3, 1, 1), (4, 1, 1)], [((10, 1, None), 1)])
    assert ctx.top_refs(0).shape[0] == 0


def boundary_input(r, d):
    """Projection s, support 2.  Subjects: a dependent s[p=0] = {0, 1} contained in exactly r others s[p=1 + i] =
    {0, 1, u_i}, and a hub s[p=r + 1] = {c_1 .. c_2d} containing exactly d others s[p=r + 2 + j] = {c_2j+1, c_2j+2}.
    Every object is distinct, so only predicates and subjects are frequent and every capture is a s[p=.]."""
    sp = [(0, 0), (1, 0)]
    nxt = 2
    for i in range(r):
        sp += [(0, 1 + i), (1, 1 + i), (nxt, 1 + i)]
        nxt += 1
    hub = r + 1
    for j in range(d):
        a, b = nxt, nxt + 1
        nxt += 2
        sp += [(a, hub), (b, hub), (a, hub + 1 + j), (b, hub + 1 + j)]
    npred = hub + 1 + d
    base = max(nxt, npred)
    s = np.array([x for x, _ in sp], np.uint32)
    p = np.array([y for _, y in sp], np.uint32)
    o = np.arange(base, base + len(sp), dtype=np.uint32)
    return SimpleNamespace(name=f"cind_stats_boundary_{r}_{d}", s=s, p=p, o=o, num_terms=int(base + len(sp)), min_support=2)


@pytest.mark.parametrize("clean", [False, True])
@pytest.mark.parametrize("r,d", [(63, 257), (64, 256), (65, 255), (255, 65), (256, 64), (257, 63)])
def test_run_boundaries(ctx, r, d, clean):
    sh = boundary_input(r, d)
    ctx.set_triples(sh.s, sh.p, sh.o, sh.num_terms)
    ctx.run(2, "s", clean, 1)
    hist, top = hist_list(ctx.cind_histogram()), top_ids(ctx)
    assert_shape_rows(ctx, sh, 1, clean, "s")  # the oracle decides the truth
    ek, es = shape_rows(sh, 1, clean, "s")
    dep, rf = (ek >> np.uint64(32)).astype(np.uint32), (ek & np.uint64(NONE)).astype(np.uint32)
    none = np.zeros(0, np.uint64)
    exp = ref.statistics_np(dep, rf, es, _lib.decode_captures(dep, sh.num_terms, none)[0],
                            _lib.decode_captures(rf, sh.num_terms, none)[0])
    assert (hist, top) == exp
    refs = {v: t for k, v, t in hist if k == 3}
    indeg = {v: t for k, v, t in hist if k == 4}
    assert refs.get(r, 0) >= 1 and indeg.get(d, 0) >= 1, (sorted(refs), sorted(indeg))  # the boundaries were met
    assert top[0][1] == d and len(ek) == r + d


def self_members(parts):
    """(members with, members without) a self entry in their class list, from the compact hand-over."""
    L = parts["layout"]
    with_self = without = 0
    for m in parts["members"][: L["n_members"]].tolist():
        lst, depid = m >> 32, m & NONE
        seg = parts["list_refs"][int(parts["list_off"][lst]):int(parts["list_off"][lst + 1])]
        if depid in seg:
            with_self += 1
        else:
            without += 1
    return with_self, without


@pytest.mark.parametrize("heavy_min", [1, 2, 8])
def test_class_path(monkeypatch, heavy_min):
    """The random inputs of test_heavy_paths_parity: the mask classes carry most of the result.  The statistics come
    first, count the class part unexpanded and leave it pending (the class emission timer stays zero until a row
    accessor runs); afterwards the rows still equal the oracle's and the statistics of the expanded rows are the same."""
    monkeypatch.setenv("RDFIND_HEAVY_MIN", str(heavy_min))
    g = _lib.Context(0)
    try:
        rng = random.Random(100 + heavy_min)
        n_class = n_self = n_noself = n_emitted = 0
        for _ in range(30):
            arr, nv, ms = random_input(rng)
            for strategy, clean in MODES:
                g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
                cs = g.run(ms, "spo", clean, strategy)
                first = device_stats(g)  # before any row accessor
                if cs["n_class_cinds"]:
                    n_class += 1
                    assert g.kernel_times()["cemit"] == 0.0  # the class part is still pending
                    w, wo = self_members(g.copy_result_compact())
                    n_self += w
                    n_noself += wo
                exp = expected_set(arr, nv, ms, strategy, clean)
                assert _lib.decoded_to_set(g.decoded_cinds()) == exp, (nv, ms, strategy, clean, heavy_min)
                if cs["n_class_cinds"]:
                    n_emitted += g.kernel_times()["cemit"] > 0.0  # (the timer does see the expansion)
                assert first == ref.statistics(exp), (nv, ms, strategy, clean, heavy_min)
                assert device_stats(g) == first  # the class rows materialised: counted as explicit rows now
        assert n_class > 0 and n_self > 0 and n_noself > 0 and n_emitted > 0, (n_class, n_self, n_noself, n_emitted)
    finally:
        g.close()


def test_heavy_bits_form(monkeypatch):
    """RDF_FORM_HEAVY_BITS: the deferred heavy-only refs are written before they are counted; same rows as the
    expanded form and as the reference."""
    monkeypatch.setenv("RDFIND_HEAVY_MIN", "2")
    g, e = _lib.Context(0), _lib.Context(0)
    try:
        g.set_result_form(True)
        rng = random.Random(900 + 2)
        chunks = 0
        for _ in range(12):
            arr, nv, ms = random_input(rng)
            for c in (g, e):
                c.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
                c.run(ms)
            got = device_stats(g)  # first: the heavy refs are still bits
            chunks += g.copy_result_compact()["n_heavy_chunks"]
            assert got == device_stats(e) == ref.statistics(expected_set(arr, nv, ms, 1, True)), (nv, ms)
        assert chunks > 0
    finally:
        g.close()
        e.close()


@pytest.mark.parametrize("heavy_min", [64, 2])
def test_paged(monkeypatch, heavy_min):
    """A one-byte page budget (every binary dependent its own page): begin, add per page, end equals the unpaged
    rdf_cind_histogram and the reference; rdf_next_page does not abandon the accumulation."""
    monkeypatch.setenv("RDFIND_HEAVY_MIN", str(heavy_min))
    g = _lib.Context(0)
    try:
        rng = random.Random(500 + heavy_min)
        most_pages = 0
        for _ in range(16):
            arr, nv, ms = random_input(rng)
            for strategy, clean in MODES:
                g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
                g.frequent_conditions(ms)
                g.build_capture_groups("spo")
                g.discover_cinds_paged(clean, strategy, 1)
                g.cind_stats_begin()
                pages = total = 0
                while g.next_page() is not None:
                    g.cind_stats_add()
                    total += g.cind_count()
                    pages += 1
                paged = hist_list(g.cind_stats_end()), top_decoded(g)
                most_pages = max(most_pages, pages)
                exp = expected_set(arr, nv, ms, strategy, clean)
                assert total == len(exp)
                assert paged == ref.statistics(exp), (nv, ms, strategy, clean, heavy_min, pages)
                g.run(ms, "spo", clean, strategy)
                assert device_stats(g) == paged
        assert most_pages > 2
    finally:
        g.close()


@pytest.mark.parametrize("cfg,scale", [("c5", 0.01), ("c1", 0.05)])
def test_synthetic_configs(ctx, cfg, scale):
    d = dataset(cfg, scale)
    ctx.set_triples(d.s, d.p, d.o, d.num_terms)
    cs = ctx.run(d.min_support)
    hist, top = hist_list(ctx.cind_histogram()), top_ids(ctx)
    assert cs["n_class_cinds"] == 0 or ctx.kernel_times()["cemit"] == 0.0
    assert_stream_matches(ctx, cfg, scale)  # count and checksum pin the rows to the oracle
    rows = ctx.copy_cinds()
    bk = ctx.binary_keys()
    exp = ref.statistics_np(rows["dep"], rows["ref"], rows["support"], _lib.decode_captures(rows["dep"], d.num_terms, bk)[0],
                            _lib.decode_captures(rows["ref"], d.num_terms, bk)[0])
    assert hist == exp[0]
    assert top == exp[1]
    assert sum(t for k, _, t in hist if k == 1) == ctx.cind_count() > 0
    assert top == [(int(c), int(n)) for c, n in ctx.top_refs(len(top)).tolist()] and len(ctx.top_refs(3)) == 3


def raises_state(call):
    with pytest.raises(_lib.RdfError) as e:
        call()
    assert e.value.status == ERR_STATE, e.value
    return True


def test_state_errors():
    arr, nv, ms = random_input(random.Random(7))
    with _lib.Context(0) as g:
        for call in (g.cind_stats_begin, g.cind_stats_add, g.cind_stats_end, g.cind_histogram, lambda: g.top_refs(1)):
            assert raises_state(call)  # nothing resident
        g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
        g.frequent_conditions(ms)
        g.build_capture_groups("spo")
        assert raises_state(g.cind_stats_begin) and raises_state(g.cind_histogram)  # before a discovery
        g.discover_cinds()
        assert raises_state(g.cind_stats_add) and raises_state(g.cind_stats_end)  # without begin
        assert raises_state(lambda: g.top_refs(1))  # without a completed end
        once = hist_list(g.cind_histogram())
        assert once and raises_state(g.cind_stats_add) and raises_state(g.cind_stats_end)  # end closed it
        # the same result added twice counts twice
        g.cind_stats_begin()
        g.cind_stats_add()
        g.cind_stats_add()
        twice = hist_list(g.cind_stats_end())
        assert [r for r in twice if r[0] <= 2] == [(k, v, 2 * t) for k, v, t in once if k <= 2]
        assert sum(v * t for k, v, t in twice if k == 3) == 2 * sum(v * t for k, v, t in once if k == 3)
        # whatever rebuilds the capture table abandons an open accumulation (and forgets the top list)
        rebuild = {
            "set_triples": lambda: g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv),
            "frequent_conditions": lambda: g.frequent_conditions(ms),
            "build_capture_groups": lambda: g.build_capture_groups("spo"),
            "discover_cinds": lambda: g.discover_cinds(),
            "discover_cinds_paged": lambda: (g.build_capture_groups("spo"), g.discover_cinds_paged(True, 1, 1)),
            "release_scratch": g.release_scratch,
        }
        for name, call in rebuild.items():
            g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
            g.run(ms)
            assert hist_list(g.cind_histogram()) == once and len(g.top_refs(1)) == 1
            g.cind_stats_begin()
            g.cind_stats_add()
            call()
            assert raises_state(g.cind_stats_add) and raises_state(g.cind_stats_end), name
            assert raises_state(lambda: g.top_refs(1)), name
        # a prepared paged run takes begin, but has no current result to add before its first page
        g.set_triples(arr[:, 0], arr[:, 1], arr[:, 2], nv)
        g.frequent_conditions(ms)
        g.build_capture_groups("spo")
        g.discover_cinds_paged(True, 1, 1)
        g.cind_stats_begin()
        assert raises_state(g.cind_stats_add)
        while g.next_page() is not None:
            g.cind_stats_add()
        assert hist_list(g.cind_stats_end()) == once
        # the rows are the context's histogram rows: the next histogram call replaces them
        g.condition_histogram()
        assert hist_list(g.copy_histogram())[0][0] == 0


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _sharded_worker(rank, world, port, case, q):
    """Two ranks over gloo, each with its own context on the one GPU (the style of tests/test_gpu_sharded.py): after the
    sharded run every statistics call answers RDF_ERR_STATE."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rdfind_amd import distributed
    try:
        s, p, o, nv, ms = case
        with _lib.Context(0) as g:
            g.set_triples(s, p, o, nv)
            distributed.run_sharded(g, ms, "spo", True, 1)
            status = []
            for call in (g.cind_stats_begin, g.cind_stats_add, g.cind_stats_end, g.cind_histogram, lambda: g.top_refs(1)):
                try:
                    call()
                    status.append(0)
                except _lib.RdfError as e:
                    status.append(e.status)
            q.put((rank, (status, g.cind_count())))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, repr(e) + "\n" + traceback.format_exc()[-1500:]))
    finally:
        dist.destroy_process_group()


def test_sharded_run_is_refused():
    arr, nv, ms = random_input(random.Random(7))
    case = (arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy(), nv, ms)
    world = 2
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_sharded_worker, args=(r, world, port, case, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = {}
    deadline = time.monotonic() + 300
    try:
        while len(res) < world:
            try:
                r, item = q.get(timeout=1)
            except queue.Empty:  # a rank that died before it could report ends the wait at once
                dead = {i: pr.exitcode for i, pr in enumerate(procs) if pr.exitcode not in (None, 0)}
                assert not dead, f"ranks ended without a report (exit codes {dead})"
                assert time.monotonic() < deadline, "no report from the ranks"
                continue
            assert not isinstance(item, str), f"rank {r}: {item}"
            res[r] = item
    finally:
        for pr in procs:
            pr.join(timeout=5 if len(res) < world else 60)
            if pr.is_alive():
                pr.terminate()
    for r in range(world):
        status, n = res[r]
        assert status == [ERR_STATE] * 5, (r, status)
    assert sum(res[r][1] for r in range(world)) == len(expected_set(arr, nv, ms, 1, True)) > 0  # (the run had a result)


_GOLDEN_STATS = {}


def golden_stat_lines(name, k):
    """cind_statistics_lines of the reference fed with the parsed golden CIND lines (terms as the ids of the fixture's
    dictionary, which order the ties of the top list), and the golden lines themselves."""
    if name not in _GOLDEN_STATS:
        ms, lines = read_golden(name, "s1_clean")
        _, _, _, dic = ntriples.read_triples([os.path.join(GOLDEN, f"{name}.nt.gz")])
        ident = {t: i for i, t in enumerate(dic.terms)}
        rows = []
        for ln in lines:
            dc, d1, d2, rc, r1, r2, sup = ref.parse_line(ln)
            rows.append((dc, ident[d1], None if d2 is None else ident[d2], rc, ident[r1], None if r2 is None else ident[r2],
                         sup))
        _GOLDEN_STATS[name] = (ms, lines, ref.statistics(rows), dic)
    ms, lines, (hist, top), dic = _GOLDEN_STATS[name]
    return ms, lines, program.cind_statistics_lines(hist, top[:k], lambda cap: cap, dic.term)


def run_main(argv, capsys):
    capsys.readouterr()
    assert program.main(argv) == 0
    return capsys.readouterr().out.splitlines()


@pytest.mark.parametrize("paged", [False, True], ids=["unpaged", "page-bytes-1"])
@pytest.mark.parametrize("name", ["lubm_small", "skew_small"])
def test_program_cind_statistics(tmp_path, capsys, name, paged):
    ms, golden, exp = golden_stat_lines(name, 3)
    assert len(exp) > 10 and sum(ln.startswith("Most referenced: ") for ln in exp) == 3
    inp = os.path.join(GOLDEN, f"{name}.nt.gz")
    base = ["--use-fis", "--clean-implied", "--support", str(ms), "--cind-statistics", "3"]
    base += ["--page-bytes", "1"] if paged else []
    out = tmp_path / "cinds.txt"
    assert run_main(base + ["--output", f"file://{out}", inp], capsys) == exp
    assert sorted(out.read_text().splitlines()) == golden  # the CIND output is unchanged
    assert run_main(base + [inp], capsys) == exp + [f"Detected {len(golden)} CINDs."]
    assert run_main(["--use-fis", "--clean-implied", "--support", str(ms), inp], capsys) == [f"Detected {len(golden)} CINDs."]  # without the flag: no such lines
