"""K3 emits a frequent binary key's two unary records once, from a key item behind the triples, and the triples that
hold the key leave them out (RDFIND_EMIT_KEYS, default on).  Every form of the emission (one pass with and without the
first-digit histogram, count + write, join ranges kept and re-emitted, a rank's shard) must produce the same records
under the rule, and the same result and statistics as without it.  tests/emit_keys_ref.py restates the emission and
gives the exact numbers; tests/test_emit_keys_cpu.py checks the restatement and the shapes against both oracles."""
import types

import numpy as np
import pytest

from oracle import c_oracle as C, rdfind_oracle as R
from rdfind_amd import _lib
from tests import emit_keys_ref as K
from tests.test_gpu import MODES, expected_set, gpu_set

pytestmark = pytest.mark.gpu

# the emission's forms: switches on top of RDFIND_EMIT_KEYS
FORMS = {
    "hist": {"RDFIND_EMIT_HIST": "1"},
    "compact": {"RDFIND_EMIT_HIST": "0"},
    "twopass": {"RDFIND_EMIT_ONEPASS": "0"},
    "ranges_kept": {"RDFIND_GROUP_RANGE": "1", "RDFIND_RANGE_KEEP": "1"},
    "ranges_again": {"RDFIND_GROUP_RANGE": "1", "RDFIND_RANGE_KEEP": "0"},
    # (a range per join value costs the larger shapes a second per run: theirs hold up to 200 records)
    "ranges200_kept": {"RDFIND_GROUP_RANGE": "200", "RDFIND_RANGE_KEEP": "1"},
    "ranges200_again": {"RDFIND_GROUP_RANGE": "200", "RDFIND_RANGE_KEEP": "0"},
}
ONE_BUILD = ("hist", "compact", "twopass")  # the forms RDFIND_EMIT_GRID applies to
ALL_FORMS = ONE_BUILD + ("ranges_kept", "ranges_again")
WIDE_FORMS = ONE_BUILD + ("ranges200_kept", "ranges200_again")


def forms_of(name):
    return WIDE_FORMS if name.startswith("more_keys") else ALL_FORMS

STATS = ("n_records", "n_frequent_records", "n_groups", "n_captures")


@pytest.fixture(scope="module")
def contexts():
    """(form, keys switch, grid cap or None) -> context; the switches are read when a context is created."""
    mp = pytest.MonkeyPatch()
    made = {}

    def get(form, keys, grid=None):
        k = (form, keys, grid)
        if k not in made:
            for name, v in FORMS[form].items():
                mp.setenv(name, v)
            mp.setenv("RDFIND_EMIT_KEYS", str(keys))
            if grid is not None:
                mp.setenv("RDFIND_EMIT_GRID", str(grid))
            made[k] = _lib.Context(0)
            mp.undo()
        return made[k]

    yield get
    for c in made.values():
        c.close()
    mp.undo()


def expected(arr, nv, ms, strategy, clean, proj):
    """The oracle's CIND set under a projection (tests/test_gpu.py expected_set is its "spo" case)."""
    if proj == "spo":
        return expected_set(arr, nv, ms, strategy, clean)
    if strategy == 1 and not clean:  # the exact-candidate S2L raw output has only the Python restatement
        tr = [tuple(x) for x in arr.tolist()]
        uf = R.frequent_unary_conditions(tr, ms)
        v = R.all_at_once(R.join_lines(tr, uf, R.frequent_binary_conditions(tr, uf, ms), proj), ms, False,
                          literal_implies=False)
        return R.cind_set(R.s2l_exact_raw(v))
    return C.run_set(arr[:, 0], arr[:, 1], arr[:, 2], nv, ms, strategy, clean, proj)[0]


def run_forms(contexts, arr, nv, ms, strategy, clean, proj, what, forms=ALL_FORMS, grid=None):
    """Every form with the rule and without it on one input; returns {(form, keys): (groups, paths)}."""
    exp = None
    out = {}
    for keys in (1, 0):
        for form in forms:
            g = contexts(form, keys, grid)
            got = gpu_set(g, arr, nv, ms, strategy, clean, proj)
            if exp is None:
                exp = expected(arr, nv, ms, strategy, clean, proj)
            assert got == exp, (what, form, keys)
            out[form, keys] = (dict(g.groups), g.test_paths(), (g.cind_count(), g.checksum()))
    ref = out[forms[0], 1]
    for (form, keys), (gs, paths, res) in out.items():
        assert res == ref[2], (what, form, keys)
        for key in STATS:
            assert gs[key] == ref[0][key], (what, form, keys, key)
        # the records into the sort: the same in every form at one switch value, and never more with the rule
        assert gs["n_sorted_records"] == out[forms[0], keys][0]["n_sorted_records"], (what, form, keys)
        assert out[form, 1][0]["n_sorted_records"] <= out[form, 0][0]["n_sorted_records"], (what, form)
        if not keys:
            assert paths["k3_key_items"] == 0 and paths["k3_suppressed"] == 0, (what, form)
    return out


def check_model(out, arr, ms, proj, what, forms, grid=None):
    """The restatement's exact numbers: the emitted and the sorted records, the key items, the records left to them."""
    for keys in (1, 0):
        m = K.model(arr, ms, proj, keys_on=bool(keys), grid_cap=grid)
        for form in forms:
            gs, paths, _ = out[form, keys]
            assert gs["n_records"] == m["n_records"], (what, form, keys)
            assert gs["n_sorted_records"] == m["sorted"], (what, form, keys)
            assert (paths["k3_key_items"], paths["k3_suppressed"]) == (m["key_items"], m["suppressed"]), (what, form, keys)


@pytest.mark.parametrize("grid", [None, 1, 4])
def test_exact_count(contexts, grid):
    """1024 triples (s_i, P, X): without the rule o[p=P]@X and p[o=X]@P reach the sort once per (block, iteration), with
    it exactly once."""
    arr, nv, ms = K.shape_exact()
    n = arr.shape[0]
    forms = WIDE_FORMS if grid is None else ONE_BUILD  # (a range per join value: a thousand ranges)
    for strategy, clean in MODES:
        out = run_forms(contexts, arr, nv, ms, strategy, clean, "spo", ("exact", grid, strategy, clean), forms, grid)
        for form in forms:
            on, off = out[form, 1], out[form, 0]
            assert on[0]["n_sorted_records"] == 3 * n + 2, (form, grid)
            assert off[0]["n_sorted_records"] == 3 * n + 2 * len(K.windows(n, grid)), (form, grid)
            assert (on[1]["k3_key_items"], on[1]["k3_suppressed"]) == (1, 2 * n), (form, grid)
            assert on[0]["n_records"] == off[0]["n_records"] == 5 * n, (form, grid)
        check_model(out, arr, ms, "spo", ("exact", grid, strategy, clean), forms, grid)


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_shapes_all_forms_and_modes(contexts, name):
    """All three key kinds in one input, B = 0, n = 0 and B > n, in the four modes and every form."""
    arr, nv, ms = K.SHAPES[name]()
    for strategy, clean in MODES:
        out = run_forms(contexts, arr, nv, ms, strategy, clean, "spo", (name, strategy, clean), forms_of(name))
        # (the range forms' blocks are the one-pass build's at these sizes, so the iteration windows agree)
        check_model(out, arr, ms, "spo", (name, strategy, clean), forms_of(name))
    if name == "kinds":
        paths = out["ranges_kept", 1]
        assert paths[1]["k3_key_items"] == 3 and paths[0]["n_join_ranges"] > 6  # (a range per join value)
    if name.startswith("more_keys"):
        assert out["ranges200_kept", 1][0]["n_join_ranges"] > 1


@pytest.mark.parametrize("name", ["kinds", "no_keys", "empty", "more_keys_100", "more_keys_300"])
def test_projection_subsets(contexts, name):
    """A key item writes only the records whose projection bit is set."""
    arr, nv, ms = K.SHAPES[name]()
    for proj in K.PROJECTIONS[:-1]:
        for strategy, clean in MODES:
            out = run_forms(contexts, arr, nv, ms, strategy, clean, proj, (name, proj, strategy, clean), forms_of(name))
            check_model(out, arr, ms, proj, (name, proj), forms_of(name))


@pytest.mark.parametrize("grid", [1, 4])
def test_key_items_across_iterations(contexts, grid):
    """B > n in one block and in four (RDFIND_EMIT_GRID): the key items cross the blocks' 256-item iterations, and one
    iteration holds the last triples and the first key items."""
    for name in ("more_keys_100", "more_keys_300"):
        arr, nv, ms = K.SHAPES[name]()
        for proj in ("spo", "p", "so"):
            for strategy, clean in MODES:
                what = (name, grid, proj, strategy, clean)
                out = run_forms(contexts, arr, nv, ms, strategy, clean, proj, what, ONE_BUILD, grid)
                check_model(out, arr, ms, proj, what, ONE_BUILD, grid)


def test_association_rules_remove_keys(contexts):
    """--use-ars: a key that a rule implies leaves the lookup table, so it has no key item and its two records come from
    the triples again; the key items are the table's keys."""
    CODE = {R.S: 0, R.P: 1, R.O: 2}
    from tests.test_gpu_ars import expected, gpu_run

    # (s = 0, p = 1): every triple of subject 0 has predicate 1, so s = 0 -> p = 1 is a rule; (p = 20, o = 21) has none
    t = [(0, 1, 2 + j) for j in range(4)] + [(22 + j, 20, 21) for j in range(4)] + [(30, 20, 31), (32, 33, 21), (34, 1, 35)]
    arr, nv, ms = np.array(t, np.uint32), 36, 3
    tr = [tuple(x) for x in arr.tolist()]
    uf = R.frequent_unary_conditions(tr, ms)
    bf = R.frequent_binary_conditions(tr, uf, ms)
    ruled = set()
    for ta, tc, va, vc, _ in R.association_rules(uf, bf):
        a, b = CODE[ta], CODE[tc]
        ruled.add((a, b, va, vc) if a < b else (b, a, vc, va))
    _, fb = K.frequent(arr, ms)
    table = fb - ruled
    assert ruled and table and ruled < fb
    for strategy, clean in MODES:
        exp = expected(tr, ms, strategy, clean)
        res = {}
        for keys in (1, 0):
            for form in ALL_FORMS:
                g = contexts(form, keys)
                got, _ = gpu_run(g, arr, nv, ms, strategy, clean)
                assert got == exp, (form, keys, strategy, clean)
                m = K.model(arr, ms, keys_on=bool(keys), table_keys=table)
                paths = g.test_paths()
                assert (paths["k3_key_items"], paths["k3_suppressed"]) == (m["key_items"], m["suppressed"]), (form, keys)
                assert g.groups["n_sorted_records"] == m["sorted"], (form, keys)
                res[form, keys] = tuple(g.groups[k] for k in STATS) + (g.cind_count(), g.checksum())
            assert paths["k3_key_items"] == (len(table) if keys else 0)
        assert len(set(res.values())) == 1, res


# ---------------------------------------------------------------------------------------------------------------------
# a sharded run: a rank's emission selects its join shard (the lazy form), the key items under the same selection

def _rank_worker(rank, world, port, shape, modes, env, q):
    import os

    os.environ.update(env)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rdfind_amd import _lib as lib, distributed
    from tests.parity import device_rows

    s, p, o, nv, ms = shape
    try:
        out = []
        with lib.Context(0) as ctx:
            ctx.set_triples(s[rank::world], p[rank::world], o[rank::world], nv)
            for strategy, clean in modes:
                gs, _ = distributed.run_sharded(ctx, ms, "spo", clean, strategy, local_slice=True)
                item = {"n": ctx.cind_count(), "checksum": ctx.checksum(), "records": int(gs["n_records"]),
                        "sorted": int(gs["n_sorted_records"]), "paths": ctx.test_paths()}
                item["keys"], item["sup"] = device_rows(ctx)
                item["expanded"] = (ctx.cind_count(), ctx.checksum())
                out.append(item)
        q.put((rank, out))
    except Exception as e:  # report instead of hanging the parent
        import traceback

        q.put((rank, repr(e) + "\n" + traceback.format_exc()[-1500:]))
    finally:
        dist.destroy_process_group()


def test_sharded_rows_exact():
    """Two ranks on one GPU, each with a slice of the three-kinds shape: the parts' rows are the oracle's, with the rule
    and without it, and the ranks emit the same logical records either way."""
    import torch.multiprocessing as tmp

    from tests.test_gpu_sharded import _free_port
    from tests.test_gpu_sharded_shapes import check_rows

    arr, nv, ms = K.shape_kinds()
    sh = types.SimpleNamespace(name="emit_keys_kinds", s=arr[:, 0].copy(), p=arr[:, 1].copy(), o=arr[:, 2].copy(),
                               num_terms=nv, min_support=ms)
    modes = [(1, True), (0, False)]
    res = {}
    for keys in ("1", "0"):
        mpc = tmp.get_context("spawn")
        q = mpc.Queue()
        port = _free_port()
        procs = [mpc.Process(target=_rank_worker, args=(r, 2, port, (sh.s, sh.p, sh.o, nv, ms), modes,
                                                        {"RDFIND_EMIT_KEYS": keys}, q)) for r in range(2)]
        for pr in procs:
            pr.start()
        got = {}
        try:
            for _ in procs:
                r, item = q.get(timeout=180)
                assert not isinstance(item, str), f"rank {r}: {item}"
                got[r] = item
        finally:
            for pr in procs:
                pr.join(timeout=60 if len(got) == 2 else 5)
                if pr.is_alive():
                    pr.terminate()
        res[keys] = got
        for k, (strategy, clean) in enumerate(modes):
            check_rows(2, [got[r][k] for r in range(2)], sh, strategy, clean, "spo", ("emit keys", keys, strategy, clean))
    for k in range(len(modes)):
        for r in range(2):
            on, off = res["1"][r][k], res["0"][r][k]
            assert on["records"] == off["records"] and on["sorted"] <= off["sorted"], (k, r)
            assert off["paths"]["k3_key_items"] == 0 and off["paths"]["k3_suppressed"] == 0
        assert sum(res["1"][r][k]["paths"]["k3_suppressed"] for r in range(2)) == K.model(arr, ms)["suppressed"]
