"""Dev tool: --prefixes on the c2 triples written as N-Triples text, on the device (rdf_rewrite_terms after the device
parse) against the host route it replaces (parsed_terms + copy_triples + shorten_dictionary + set_triples after the
same parse).  The table holds the generator's namespaces and 1,000 keys that match nothing.
python tools/rewrite_bench.py [scale]         both legs, each a child process with its own time limit; a failed leg
                                              stops the run
python tools/rewrite_bench.py [scale] --leg device|host   one leg (the text is cached in bench_out/)"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from rdfind_amd import _lib, ntriples, synth

LEG_LIMIT_S = {"device": 300, "host": 600}
PREFIXES = ([("ub", "http://swat.cse.lehigh.edu/onto/univ-bench.owl#"), ("onto", "http://swat.cse.lehigh.edu/onto/"),
             ("rdf", "http://www.w3.org/1999/02/22-rdf-syntax-ns#"), ("www", "http://www.")]
            + [(f"n{i}", f"http://nomatch{i}.example.org/{'ns/' * (i % 7)}") for i in range(1000)])


def text_path(scale):
    return os.path.join(ROOT, "bench_out", f"rewrite_c2_{scale}.nt")


def build_text(scale):
    path = text_path(scale)
    if os.path.exists(path):
        return
    t = time.perf_counter()
    d = synth.config("c2", scale)
    tt = d.terms.term
    strs = np.array([tt(i) + " " for i in range(d.num_terms)], dtype=object)
    data = "".join(map("".join, zip(strs[d.s], strs[d.p], strs[d.o], [".\n"] * d.n))).encode()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    print(f"text {len(data) / 1e9:.2f} GB, {d.n} lines (built in {time.perf_counter() - t:.1f}s)", flush=True)


def leg(scale, which):
    with open(text_path(scale), "rb") as f:
        data = f.read()
    with _lib.Context(0) as ctx:
        if which == "device":
            times, parse_ms = [], []
            for _ in range(4):
                n, v, pms = ctx.parse_ntriples(data)
                st = ctx.rewrite_terms(PREFIXES)
                times.append(st["ms"])
                parse_ms.append(pms)
            ms = float(np.median(times[1:]))
            print(f"REWRITE device: {st['n_terms_before']} terms -> {st['n_terms_after']}, {st['n_changed']} changed, "
                  f"{len(PREFIXES)} keys ({ctx.rewrite_form()}), heap {st['heap_bytes'] / 1e6:.1f} MB: {ms:.3f} ms "
                  f"(median of {len(times) - 1}; the parse before it: {float(np.median(parse_ms[1:])):.2f} ms)", flush=True)
        else:
            n, v, _ = ctx.parse_ntriples(data)
            t = time.perf_counter()
            dic = ntriples.HeapDictionary(*ctx.parsed_terms())
            s, p, o = ctx.copy_triples(n)
            t1 = time.perf_counter()
            s, p, o, dic = ntriples.shorten_dictionary(s, p, o, dic, PREFIXES)
            t2 = time.perf_counter()
            ctx.set_triples(s, p, o, dic.size)
            t3 = time.perf_counter()
            print(f"REWRITE host route: {v} terms -> {dic.size}: {(t3 - t) * 1e3:.0f} ms (download {(t1 - t) * 1e3:.0f}, "
                  f"shorten_dictionary {(t2 - t1) * 1e3:.0f}, set_triples {(t3 - t2) * 1e3:.0f})", flush=True)


def main():
    args = [a for a in sys.argv[1:]]
    which = None
    if "--leg" in args:
        i = args.index("--leg")
        which = args[i + 1]
        del args[i:i + 2]
    scale = float(args[0]) if args else 1.0
    if which:
        return leg(scale, which)
    build_text(scale)
    for which in ("device", "host"):  # chained: a leg that fails or runs out of time ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(scale), "--leg", which], timeout=LEG_LIMIT_S[which])
        if r.returncode:
            sys.exit(f"leg {which} failed ({r.returncode})")
    os.remove(text_path(scale))


if __name__ == "__main__":
    main()
