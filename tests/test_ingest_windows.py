"""ntriples.iter_windows: the input stream of read_bytes cut into windows of whole lines for the chunked device
parse, and the driver's --ingest-window option (no GPU needed)."""
import gzip

import pytest

from rdfind_amd import ntriples, program


def _lines(n, seed=0):
    return "".join(f"<s{(i * 7 + seed) % 13}> <p{i % 3}> \"{'v' * ((i * 11 + seed) % 90)}\" .\n" for i in range(n)).encode()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("windows")
    plain = d / "plain.nt"
    plain.write_bytes(_lines(200))
    gz = d / "packed.nt.gz"
    with gzip.open(gz, "wb") as f:
        f.write(_lines(150, 3) + b"# last line without a line break")
    open_end = d / "open_end.nt"
    open_end.write_bytes(_lines(20, 5)[:-1])  # no final newline
    second = d / "second.nt"
    second.write_bytes(b"\n\r\n" + _lines(30, 9))
    empty = d / "empty.nt"
    empty.write_bytes(b"")
    long_line = d / "long.nt"
    long_line.write_bytes(b"<a> <p> <b> .\n<a> <p> \"" + b"z" * 9987 + b"\" .\n<c> <p> <d> .\n")
    return {
        "plain": [str(plain)],
        "gz": [f"file://{gz}"],
        "two_files": [str(open_end), str(second)],
        "empty": [str(empty)],
        "empty_between": [str(plain), str(empty), str(open_end)],
        "long_line": [str(long_line)],
    }


@pytest.mark.parametrize("window", [1, 64, 4096, 1 << 30])
@pytest.mark.parametrize("case", ["plain", "gz", "two_files", "empty", "empty_between", "long_line"])
def test_windows_partition_the_stream(inputs, case, window):
    paths = inputs[case]
    whole = ntriples.read_bytes(paths)
    items = list(ntriples.iter_windows(paths, window))
    assert b"".join(items) == whole
    for k, item in enumerate(items):
        assert isinstance(item, bytes) and item and item.endswith(b"\n")
        single_line = item.count(b"\n") == 1
        assert len(item) <= window or single_line, (k, len(item))
        if k + 1 < len(items):  # the next line would not have fitted
            nxt = items[k + 1]
            assert len(item) + nxt.index(b"\n") + 1 > window, k
    if case == "empty":
        assert items == []
    if window >= len(whole) and whole:
        assert items == [whole]
    if case == "long_line" and window in (64, 4096):
        assert max(len(i) for i in items) == 10000 and sum(len(i) > window for i in items) == 1


def test_windows_stream_a_large_step(monkeypatch, inputs):
    """Windows that span several read steps, and read steps that hold several windows."""
    monkeypatch.setattr(ntriples, "_GZ_STEP", 97)
    for case in ("plain", "gz", "two_files", "long_line"):
        whole = ntriples.read_bytes(inputs[case])
        for window in (50, 500, 20000):
            items = list(ntriples.iter_windows(inputs[case], window))
            assert b"".join(items) == whole
            assert all(len(i) <= window or i.count(b"\n") == 1 for i in items)
            assert all(len(a) + b.index(b"\n") + 1 > window for a, b in zip(items, items[1:]))


def test_ingest_window_option():
    ap = program.build_parser()
    assert ap.parse_args(["in.nt"]).ingest_window == 1 << 30
    assert ap.parse_args(["--ingest-window", "4096", "in.nt"]).ingest_window == 4096
    assert program.RDFind(["--use-fis", "--ingest-window", "65536", "in.nt"]).args.ingest_window == 65536
