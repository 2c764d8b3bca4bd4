"""Shared checkers for the GPU parity tests (test infrastructure: imports the oracle).

* ``dataset(cfg, scale)``: one synthetic BASELINE-shaped input per (config, scale) per pytest session, kept in a
  size-bounded cache (the 10^9-triple c4 input is 12 GB and is drawn once, not once per test);
* ``oracle_stream(...)``: the streamed C oracle's (count, checksum, per-kind counts) per (config, scale, mode), cached
  for the session, so the hook-variant tests (heavy columns, dense bitmaps, pages, join ranges) that re-run one
  config compare against one oracle run;
* ``assert_rows_equal(ctx, d, ...)``: exact row-by-row parity of the current result with the materializing oracle, as
  sorted packed (dep, ref) keys + supports (vectorized; a Python set of 10^7 tuples took ~40 s per check);
* ``dataset_npz(cfg, scale)``: the same input saved once as .npy files, for child processes that must start fresh
  (switches read when the context is created) without regenerating it;
* ``shape_rows(sh, ...)`` / ``assert_shape_rows(ctx, sh, ...)``: the oracle's sorted packed rows of a near-miss shape
  (tests/light_shapes.py, either form) or a heavy / class shape (tests/heavy_shapes.py) per (shape, form, mode,
  projection), cached for the session, and the row-exact comparison with them;
* ``expected_checksum(keys, supports)``: the library's order-independent result checksum of expected rows;
* ``ars_expected(sh, ...)``: the rules and the CIND set of a shape with association rules on (Python oracle), cached.
"""
from __future__ import annotations

import os
import tempfile
from collections import OrderedDict

import numpy as np

from oracle import c_oracle as C
from rdfind_amd import synth

_CACHE_BYTES = int(os.environ.get("RDFIND_TEST_CACHE_BYTES", str(40 << 30)))
_DATA: "OrderedDict[tuple, synth.Dataset]" = OrderedDict()
_STREAM: dict = {}
_NPZ: dict = {}
_NPZ_DIR = None


def _nbytes(d) -> int:
    return d.s.nbytes + d.p.nbytes + d.o.nbytes


def dataset(cfg: str, scale: float):
    """The seeded synthetic input (synth.config), shared by every test of the session; least recently used inputs are
    dropped once the cache exceeds RDFIND_TEST_CACHE_BYTES (default 40 GiB of host memory)."""
    key = (cfg, float(scale))
    if key in _DATA:
        _DATA.move_to_end(key)
        return _DATA[key]
    d = synth.config(cfg, scale)
    need = _nbytes(d)
    while _DATA and sum(_nbytes(x) for x in _DATA.values()) + need > _CACHE_BYTES:
        _DATA.popitem(last=False)
    _DATA[key] = d
    return d


def oracle_stream(cfg: str, scale: float, strategy: int = 1, clean: bool = True, projection: str = "spo") -> dict:
    """Streamed C oracle on the dataset: dict(n_cinds, checksum, n_kind, n_raw, stats); cached per session."""
    key = (cfg, float(scale), strategy, bool(clean), projection)
    if key not in _STREAM:
        d = dataset(cfg, scale)
        _STREAM[key] = C.stream(d.s, d.p, d.o, d.num_terms, d.min_support, strategy, clean, projection)
    return _STREAM[key]


def assert_stream_matches(ctx, cfg: str, scale: float, strategy: int = 1, clean: bool = True, what=None):
    """The context's current result has the oracle's count and order-independent checksum (rdf_cind_checksum =
    orc_stream's mix over (dep, ref, support) rows)."""
    exp = oracle_stream(cfg, scale, strategy, clean)
    got = (ctx.cind_count(), ctx.checksum())
    assert got == (exp["n_cinds"], exp["checksum"]), (cfg, scale, strategy, clean, what, got, exp["n_cinds"])
    return exp


def packed(rows):
    """(sorted dep<<32|ref keys, supports in that order) of a dep/ref/support row array."""
    key = (rows["dep"].astype(np.uint64) << np.uint64(32)) | rows["ref"].astype(np.uint64)
    order = np.argsort(key, kind="stable")
    return key[order], np.asarray(rows["support"])[order]


def assert_rows_equal(ctx, d, strategy: int = 1, clean: bool = True, projection: str = "spo"):
    """Every row of the context's current result equals the materializing C oracle's (external capture ids: binary
    ids index the sorted frequent binary keys on both sides).  Returns the oracle's stage statistics."""
    rows, _, st = C.run(d.s, d.p, d.o, d.num_terms, d.min_support, strategy, clean, projection)
    got = ctx.copy_cinds()
    assert got.shape[0] == rows.shape[0], (got.shape[0], rows.shape[0])
    ek, es = packed(rows)
    gk, gs = packed(got)
    np.testing.assert_array_equal(gk, ek)
    np.testing.assert_array_equal(gs, es)
    return st


def dataset_npz(cfg: str, scale: float) -> str:
    """Directory holding s.npy, p.npy, o.npy and meta.npy (num_terms, min_support) of the dataset, written once per
    session under the system temp dir (removed at interpreter exit)."""
    global _NPZ_DIR
    key = (cfg, float(scale))
    if key in _NPZ:
        return _NPZ[key]
    if _NPZ_DIR is None:
        _NPZ_DIR = tempfile.TemporaryDirectory(prefix="rdfind_tests_")
    path = os.path.join(_NPZ_DIR.name, f"{cfg}_{scale}")
    os.makedirs(path, exist_ok=True)
    d = dataset(cfg, scale)
    for name in ("s", "p", "o"):
        np.save(os.path.join(path, name + ".npy"), getattr(d, name))
    np.save(os.path.join(path, "meta.npy"), np.array([d.num_terms, d.min_support], np.uint64))
    _NPZ[key] = path
    return path


def load_npz(path: str):
    """(s, p, o, num_terms, min_support) of a dataset_npz directory, memory-mapped."""
    s, p, o = (np.load(os.path.join(path, n + ".npy"), mmap_mode="r") for n in ("s", "p", "o"))
    nv, ms = (int(x) for x in np.load(os.path.join(path, "meta.npy")))
    return s, p, o, nv, ms


_SHAPE_ROWS: dict = {}


def shape_rows(sh, strategy: int = 1, clean: bool = True, projection: str = "s"):
    """(sorted dep << 32 | ref keys, supports in that order) of the oracle on a light_shapes.Shape; cached per session.
    Mode (1, False), the exact-candidate S2L raw output, has only the Python restatement as its oracle (as in
    tests/test_gpu.py expected_set); its rows are turned into capture ids with the C oracle's binary-key table (both
    index the sorted frequent binary keys)."""
    key = (sh.name, bool(getattr(sh, "shared_objects", False)), strategy, bool(clean), projection)
    if key in _SHAPE_ROWS:
        return _SHAPE_ROWS[key]
    if strategy == 1 and not clean and getattr(sh, "algebra_raw_s2l", False):
        assert sh.name in ("emit16k", "emit32k")  # no other shape may leave the oracles
        # a heavy_shapes.HShape too large for the Python restatement: its own set algebra, which tests/test_heavy_shapes_cpu.py
        # proves equal to both oracles in all four modes on the same generator at a small size
        _SHAPE_ROWS[key] = sh.rows()
        return _SHAPE_ROWS[key]
    if strategy == 1 and not clean:
        from oracle import rdfind_oracle as R
        from rdfind_amd import codes
        tr = list(zip(sh.s.tolist(), sh.p.tolist(), sh.o.tolist()))
        uf = R.frequent_unary_conditions(tr, sh.min_support)
        v = R.all_at_once(R.join_lines(tr, uf, R.frequent_binary_conditions(tr, uf, sh.min_support), projection),
                          sh.min_support, False, literal_implies=False)
        cinds = R.cind_set(R.s2l_exact_raw(v))
        _, bkeys, _ = C.run(sh.s, sh.p, sh.o, sh.num_terms, sh.min_support, 0, False, projection)
        V = sh.num_terms

        def cap(code, v1, v2):
            if v2 is None:
                return codes.UNARY_TYPE_INDEX[code] * V + v1
            k = (codes.BINARY_TYPE_INDEX[code] << 62) | (v1 << 31) | v2
            j = int(np.searchsorted(bkeys, np.uint64(k)))
            assert j < len(bkeys) and int(bkeys[j]) == k
            return 6 * V + j

        rows = np.zeros(len(cinds), dtype=[("dep", "<u4"), ("ref", "<u4"), ("support", "<u4")])
        for i, (dt, d1, d2, rt, r1, r2, sup) in enumerate(cinds):
            rows[i] = (cap(dt, d1, d2), cap(rt, r1, r2), sup)
    else:
        rows, _, _ = C.run(sh.s, sh.p, sh.o, sh.num_terms, sh.min_support, strategy, clean, projection)
    _SHAPE_ROWS[key] = packed(rows)
    return _SHAPE_ROWS[key]


def shared_captures(sh):
    """External capture ids (projection s) of the three captures every set k of a shared-object light shape has:
    int64 [n_sets, 3] = s[p=P_k], s[o=O_k], s[p=P_k,o=O_k] (the binary id indexes the C oracle's sorted frequent binary
    keys, as on the device)."""
    from rdfind_amd import codes
    _, bkeys, _ = C.run(sh.s, sh.p, sh.o, sh.num_terms, sh.min_support, 0, False, "s")
    V = sh.num_terms
    out = np.zeros((len(sh.sets), 3), np.int64)
    for k in range(len(sh.sets)):
        key = (codes.BINARY_TYPE_INDEX[14] << 62) | (sh.pred(k) << 31) | sh.obj(k)
        j = int(np.searchsorted(bkeys, np.uint64(key)))
        assert j < len(bkeys) and int(bkeys[j]) == key, (sh.name, k)
        out[k] = (codes.UNARY_TYPE_INDEX[10] * V + sh.pred(k), codes.UNARY_TYPE_INDEX[12] * V + sh.obj(k), 6 * V + j)
    return out


def device_rows(ctx):
    """(sorted dep << 32 | ref keys, supports) of the context's current result from its id-records
    (rdf_copy_result_raw: refs, run table, capture ids, supports), decoded here.  Every ref and dependent id is checked
    against the capture table first, so a wrong id fails an assertion; rdf_copy_cinds indexes the library's host table
    with it unchecked."""
    n_refs, n_runs, n_cap = ctx.result_sizes()
    refs, runoff, rundep = np.empty(max(n_refs, 1), np.uint32), np.empty(n_runs + 1, np.uint64), np.empty(max(n_runs, 1), np.uint32)
    ids, sup = np.empty(max(n_cap, 1), np.uint32), np.empty(max(n_cap, 1), np.uint32)
    ctx.copy_result_raw(refs, runoff, rundep, ids, sup)
    refs, rundep = refs[:n_refs], rundep[:n_runs]
    assert int(runoff[0]) == 0 and int(runoff[n_runs]) == n_refs and (np.diff(runoff.astype(np.int64)) >= 0).all()
    bad = np.nonzero(refs >= n_cap)[0]
    assert bad.size == 0 and (rundep < n_cap).all(), ("ref id outside the capture table", bad[:4].tolist(),
                                                     refs[bad[:4]].tolist(), n_cap)
    dep = np.repeat(rundep, np.diff(runoff.astype(np.int64)))
    key = (ids[dep].astype(np.uint64) << np.uint64(32)) | ids[refs].astype(np.uint64)
    order = np.argsort(key, kind="stable")
    return key[order], sup[dep][order]


def assert_shape_rows(ctx, sh, strategy: int = 1, clean: bool = True, projection: str = "s", what=None):
    """Every row of the context's current result equals the oracle's rows of the shape.  A heavy / class shape and a
    shared-object light shape are decoded by device_rows, whose ids are checked before use."""
    ek, es = shape_rows(sh, strategy, clean, projection)
    checked = hasattr(sh, "heavy_min") or getattr(sh, "shared_objects", False)
    gk, gs = device_rows(ctx) if checked else packed(ctx.copy_cinds())
    assert gk.shape[0] == ek.shape[0], (sh.name, strategy, clean, projection, what, gk.shape[0], ek.shape[0],
                                        _first_diff(gk, ek))
    bad = np.nonzero(gk != ek)[0]
    assert bad.size == 0, (sh.name, strategy, clean, projection, what, _first_diff(gk, ek))
    np.testing.assert_array_equal(gs, es)


_ARS: dict = {}


def ars_expected(sh, strategy: int, clean: bool):
    """(sorted rules, CIND set) of a shape with --use-ars under projection spo: the Python oracle as
    tests/test_gpu_ars.py states it (rules as (antecedent code, consequent code, values, count)); cached per session."""
    key = (sh.name, strategy, bool(clean))
    if key not in _ARS:
        from oracle import rdfind_oracle as R
        from tests.test_gpu_ars import CODE, expected
        tr = list(zip(sh.s.tolist(), sh.p.tolist(), sh.o.tolist()))
        if ("rules", sh.name) not in _ARS:
            uf = R.frequent_unary_conditions(tr, sh.min_support)
            bf = R.frequent_binary_conditions(tr, uf, sh.min_support)
            _ARS[("rules", sh.name)] = sorted((CODE[ta], CODE[tc], va, vc, n) for ta, tc, va, vc, n in R.association_rules(uf, bf))
        _ARS[key] = (_ARS[("rules", sh.name)], expected(tr, sh.min_support, strategy, clean))
    return _ARS[key]


_M64 = (1 << 64) - 1


def expected_checksum(keys, supports) -> int:
    """rdf_cind_checksum of the rows (sorted or not): the sum mod 2^64 of mix64(((dep << 32) | ref) + support * phi)
    over external capture ids (tests/test_gpu_full.py states it; mix64 = the murmur3 finaliser of common.hpp)."""
    x = keys.astype(np.uint64) + supports.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # wraps mod 2^64
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    return int(np.add.reduce(x, dtype=np.uint64)) & _M64 if x.size else 0


def _first_diff(gk, ek):
    """A few (dep, ref) pairs only the device has, and a few only the oracle has."""
    pair = lambda k: [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in k[:4]]
    return {"device_only": pair(np.setdiff1d(gk, ek)), "oracle_only": pair(np.setdiff1d(ek, gk))}
