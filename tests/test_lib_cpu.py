"""The C-ABI library loads and exports every symbol include/rdfind_hip.h declares (no compute calls
without a GPU), and the product path fails loudly instead of falling back to the CPU."""
import os
import re

import pytest

from rdfind_amd import _lib
from tests.conftest import ROOT


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "rdfind_hip.h")).read()
    return sorted(set(re.findall(r"^(?:rdf_status|void\s*\*|void|const char\s*\*)\s*(rdf_[a-z_0-9]+)\s*\(", src, re.M)))


def test_library_exports_header_symbols():
    lib = _lib.load()
    names = declared_symbols()
    assert names, "no declarations found"
    for name in names:
        assert hasattr(lib, name), name
    assert set(names) == set(_lib.EXPORTED_SYMBOLS)
    assert lib.rdf_version().startswith(b"rdfind_amd")


def test_context_tables_are_the_only_lists():
    """Every device buffer of rdf_ctx is declared in the RDF_CTX_BUFFERS table (none in the struct itself, none in a
    hand-written list), and the environment is read by the one table-driven reader of switches.hpp only."""
    csrc = os.path.join(ROOT, "rdfind_amd", "csrc")
    src = open(os.path.join(csrc, "rdfind_hip.hip")).read()
    table = src[src.index("#define RDF_CTX_BUFFERS(B)"):src.index("enum BufClass")]
    names = re.findall(r"\bB\((\w+), (\w+)\)", table)
    assert len(names) > 200 and len({n for _, n in names}) == len(names)
    assert {c for c, _ in names} == {"INPUT", "PARSE", "SPARE_FC", "SPARE_GROUPS", "SPARE_X", "RUN"}
    ctx = src[src.index("struct rdf_ctx : CtxBuffers {"):]
    ctx = ctx[:ctx.index("\n};\n")]
    assert len(ctx.splitlines()) > 100, "rdf_ctx not found whole"
    assert [ln for ln in ctx.splitlines() if re.match(r"\s*DevBuf\b", ln)] == []
    # the only DevBuf declaration outside the table's expansion (and Workspace) would be a field of rdf_ctx
    assert re.findall(r"^ +DevBuf [a-z_0-9, ]+;", src, re.M) == []
    assert "static_assert(sizeof(CtxBuffers) ==" in src
    for gone in ("ctx_buffers", "kBufNames"):
        assert gone not in src, gone
    getenv_lines = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".hpp", ".inl", ".h")):
            for ln in open(os.path.join(csrc, name)).read().splitlines():
                if "getenv(" in ln:
                    getenv_lines.append((name, ln.strip()))
    assert getenv_lines == [("switches.hpp", "if (const char* v = getenv(name)) s.field = (parse);")]
    # ... and that reader runs in two places: read_switches (per context) and proc_switches (per process)
    sw = open(os.path.join(csrc, "switches.hpp")).read()
    assert len(re.findall(r"\(RDF_SW_READ\)", src + sw)) == 2
    assert src.count("read_switches()") == 2  # its definition and rdf_ctx_create


def test_no_silent_cpu_fallback():
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("GPU present")
    with pytest.raises(_lib.RdfError):
        _lib.Context(0)


def test_missing_library_raises(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/librdfind_hip.so")
    with pytest.raises(_lib.RdfError):
        _lib.load()
