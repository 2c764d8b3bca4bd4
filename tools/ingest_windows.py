"""Dev tool: chunked N-Triples ingest (rdf_parse_begin / _chunk / _end) against the single call (rdf_parse_ntriples)
on a synthetic config written as N-Triples text.  Both parses must agree in n, V and a checksum of s, p, o; the
table gives the device time and text throughput of each, the chunked parse's stats, and what the context holds
afterwards (rdf_device_bytes).  Device ms exclude the upload (as rdf_parse_ntriples reports them); wall ms include it.

    python tools/ingest_windows.py --config c2 [--scale 1.0] --window 16777216 268435456 [--repeats 5]
"""
import argparse
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from rdfind_amd import _lib, synth


def text_of(cfg, scale) -> bytes:
    d = synth.config(cfg, scale)
    term = d.terms.term
    strs = np.array([term(i) + " " for i in range(d.num_terms)], dtype=object)
    return "".join(map("".join, zip(strs[d.s], strs[d.p], strs[d.o], [".\n"] * d.n))).encode()


def windows_of(data: bytes, w: int):
    """data cut as ntriples.iter_windows cuts a file: the longest runs of whole lines of at most w bytes."""
    out, pos = [], 0
    while pos < len(data):
        cut = len(data) if len(data) - pos <= w else data.rfind(b"\n", pos, pos + w) + 1
        if cut <= pos:
            cut = data.find(b"\n", pos + w) + 1 or len(data)
        out.append(data[pos:cut])
        pos = cut
    return out


def checksum(ctx, n):
    h = hashlib.blake2b(digest_size=8)
    for a in ctx.copy_triples(n):
        h.update(a.tobytes())
    return h.hexdigest()


def measure(run, repeats):
    """One warm-up run (allocations, first launches), then the median of `repeats` runs: (device ms, wall ms, last)."""
    run()
    dev, wall, last = [], [], None
    for _ in range(repeats):
        t = time.perf_counter()
        last = run()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(last[2])
    return float(np.median(dev)), float(np.median(wall)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--window", type=int, nargs="+", required=True, help="window sizes in bytes")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    data = text_of(a.config, a.scale)
    gb = len(data) / 1e9
    print(f"{a.config} at {a.scale}: text {gb:.3f} GB, {data.count(10)} lines", flush=True)
    rows = []
    with _lib.Context(0) as ctx:
        base = ctx.device_bytes()
        dev, wall, (n, v, _) = measure(lambda: ctx.parse_ntriples(data), a.repeats)
        ref = (n, v, checksum(ctx, n))
        rows.append(("single call", "-", dev, wall, ctx.device_bytes() - base, "-", "-", "-"))
    for w in a.window:
        wins = windows_of(data, w)
        with _lib.Context(0) as ctx:
            stats = {}

            def run():
                ctx.parse_begin()
                for x in wins:
                    ctx.parse_chunk(x)
                stats.update(ctx.parse_end())
                return stats["n_triples"], stats["n_terms"], stats["ms"]

            dev, wall, (n, v, _) = measure(run, a.repeats)
            got = (n, v, checksum(ctx, n))
            assert got == ref, (got, ref)
            rows.append((f"windows of {w}", len(wins), dev, wall, ctx.device_bytes() - base, stats["heap_bytes"],
                         stats["table_slots"], stats["n_table_growths"]))
    print(f"n = {ref[0]}, V = {ref[1]}, checksum {ref[2]} (equal for every row)")
    print("| parse | windows | device ms | GB/s of text | wall ms | held after (MiB) | heap bytes | table slots | growths |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name, k, dev, wall, held, heap, slots, gr in rows:
        print(f"| {name} | {k} | {dev:.2f} | {gb / dev * 1e3:.1f} | {wall:.1f} | {held / 2**20:.1f} | {heap} | {slots} | {gr} |")


if __name__ == "__main__":
    main()
