"""The NumPy references of tests/prim_ref.py against plain Python (no GPU), and the test-only symbols of the library."""
import os
import random
import re

import numpy as np

from rdfind_amd import _lib
from tests import prim_ref, shard_sim
from tests.conftest import ROOT

M64 = prim_ref.M64


def test_mix64_matches_scalar():
    rng = random.Random(7)
    vals = [0, 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1, 1 << 32, (1 << 32) - 1, 1 << 33, 0xFF51AFD7ED558CCD]
    vals += [rng.getrandbits(64) for _ in range(4000)] + [rng.getrandbits(20) for _ in range(500)]
    got = prim_ref.mix64(np.array(vals, dtype=np.uint64))
    assert got.dtype == np.uint64
    assert got.tolist() == [shard_sim.mix64(v) for v in vals]


def test_exclusive_scan_reference():
    rng = random.Random(3)
    for n in (0, 1, 2, 7, 100):
        vals = [rng.getrandbits(32) for _ in range(n)]
        want = [sum(vals[:i]) for i in range(n)]
        out, total = prim_ref.exclusive_scan(np.array(vals, np.uint32), np.uint64)
        assert out.dtype == np.uint64 and out.tolist() == want and total == sum(vals)
        out, total = prim_ref.exclusive_scan(np.array(vals, np.uint32), np.uint32)
        assert out.dtype == np.uint32 and out.tolist() == [w % (1 << 32) for w in want]
        assert total == sum(vals) % (1 << 32)
        vals64 = [rng.getrandbits(40) for _ in range(n)]
        out, total = prim_ref.exclusive_scan(np.array(vals64, np.uint64), np.uint64)
        assert out.tolist() == [sum(vals64[:i]) for i in range(n)] and total == sum(vals64)


def _py_stable(keys, field):
    return [k for _, k in sorted(enumerate(keys), key=lambda ik: (field(ik[1]), ik[0]))]


def test_stable_sort_reference():
    rng = random.Random(11)
    for n in (0, 1, 2, 50, 300):
        keys = [rng.getrandbits(64) for _ in range(n)]
        if n > 10:
            keys[3] = keys[7] = M64
            keys[5] = (1 << 9) - 1
        a = np.array(keys, dtype=np.uint64)
        for lo, hi in ((0, 1), (0, 9), (0, 64), (32, 45), (58, 64), (63, 64), (5, 5), (9, 3)):
            def field(k, lo=lo, hi=hi):
                return (k >> lo) & ((1 << (hi - lo)) - 1) if hi > lo else 0
            assert prim_ref.sort_bits(a, lo, hi).tolist() == _py_stable(keys, field), (n, lo, hi)
        for bits in (3, 9, 20, 64):
            kept = [k for k in keys if k != M64]
            got = prim_ref.sort_drop(a, bits)
            assert got.tolist() == _py_stable(kept, lambda k, b=bits: k & ((1 << b) - 1)), (n, bits)
        for bits, hmask in ((1, M64), (10, M64), (30, M64 & ~0xFFFF)):
            def hfield(k, b=bits, m=hmask):
                return shard_sim.mix64(k & m) >> (64 - b)
            assert prim_ref.partition_hashed(a, bits, hmask).tolist() == _py_stable(keys, hfield), (n, bits)
        k32 = [rng.getrandbits(32) for _ in range(n)]
        got = prim_ref.sort_bits(np.array(k32, dtype=np.uint32), 15, 32)
        assert got.dtype == np.uint32 and got.tolist() == _py_stable(k32, lambda k: k >> 15)


def test_stable_sort_keeps_order_of_equal_fields():
    # the element index in the bits outside the field: a stable result lists them ascending within each field value
    idx = np.arange(200, dtype=np.uint64)
    keys = ((idx % np.uint64(3)) << np.uint64(8)) | (idx << np.uint64(16))
    got = prim_ref.sort_bits(keys, 8, 10)
    for f in range(3):
        run = got[((got >> np.uint64(8)) & np.uint64(3)) == f] >> np.uint64(16)
        assert (np.diff(run.astype(np.int64)) > 0).all()


def test_library_exports_test_symbols():
    """The rdf_test_* entry points resolve, are declared in csrc/test_abi.h and stay out of the product header."""
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "rdfind_amd", "csrc", "test_abi.h")).read()
    declared = sorted(set(re.findall(r"^(?:rdf_status|int)\s+(rdf_test_[a-z_0-9]+)\s*\(", hdr, re.M)))
    assert declared == sorted(_lib.TEST_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(_lib.TEST_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    assert "rdf_test_" not in open(os.path.join(ROOT, "include", "rdfind_hip.h")).read()
    # the ctypes mirror of rdf_test_path_report has the header's fields, in order
    body = hdr[hdr.index("typedef struct rdf_test_path_report {"):hdr.index("} rdf_test_path_report;")]
    fields = []
    for typ, names in re.findall(r"^\s*(uint32_t|uint64_t)\s+([a-z0-9_, ]+);", body, re.M):
        fields += [(n.strip(), typ) for n in names.split(",")]
    ctype = {"uint32_t": _lib.ctypes.c_uint32, "uint64_t": _lib.ctypes.c_uint64}
    assert [(n, ctype[t]) for n, t in fields] == list(_lib.PathReport._fields_)
