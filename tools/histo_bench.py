"""Dev tool: the dataset statistics on c2, on the device (rdf_condition_histogram, rdf_join_histogram in both modes)
against the host route each replaces (numpy.unique(..., return_counts=True) over the same keys, after downloading the
triples), and the join histogram's device time next to the same run's rdf_build_capture_groups stage (both emit and
sort records of the same order).
python tools/histo_bench.py [scale]                      both legs, each a child process with its own time limit; a
                                                         failed leg stops the run
python tools/histo_bench.py [scale] --leg device|host    one leg"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from rdfind_amd import _lib, synth

LEG_LIMIT_S = {"device": 300, "host": 600}
REPS = 5  # the first one warms up (allocations), the median of the others is reported


def device_leg(ctx, d):
    def timed(call):
        ms = []
        for _ in range(REPS):
            call()
            ms.append(ctx.hist_ms)
        return float(np.median(ms[1:]))
    cond = timed(ctx.condition_histogram)
    rows_c = ctx.hist_rows
    nofis = timed(lambda: ctx.join_histogram("spo", use_fis=False))
    lines_n, rows_n = ctx.join_lines, ctx.hist_rows
    groups = []
    for _ in range(REPS):
        ctx.frequent_conditions(d.min_support)
        ctx.build_capture_groups("spo")
        ctx.sync()
        groups.append(ctx.stage_times()[1])
    groups_ms = float(np.median(groups[1:]))
    fis = timed(lambda: ctx.join_histogram("spo"))
    lines_f, rows_f = ctx.join_lines, ctx.hist_rows
    print(f"HISTO device: n {d.n}, {d.num_terms} terms, support {d.min_support}", flush=True)
    print(f"HISTO device: rdf_condition_histogram {cond:.3f} ms ({rows_c} rows)", flush=True)
    print(f"HISTO device: rdf_join_histogram no FIS {nofis:.3f} ms ({lines_n} lines, {rows_n} sizes)", flush=True)
    print(f"HISTO device: rdf_join_histogram FIS {fis:.3f} ms ({lines_f} lines, {rows_f} sizes); "
          f"rdf_build_capture_groups {groups_ms:.3f} ms; ratio {fis / groups_ms:.2f} (no FIS {nofis / groups_ms:.2f})",
          flush=True)


def host_conditions(s, p, o, V):
    """The condition histogram's rows without kind 0, with numpy.unique over the keys the device sorts."""
    V2 = V * V
    rows = []
    for keys, kinds, span in ((np.concatenate([s, V + p, np.uint64(2) * V + o]), (1, 2, 4), V),
                              (np.concatenate([p * V + o, V2 + s * V + o, np.uint64(2) * V2 + s * V + p]), (6, 5, 3), V2)):
        uniq, cnt = np.unique(keys, return_counts=True)
        part = uniq // span
        for i, kind in enumerate(kinds):
            c, t = np.unique(cnt[part == i], return_counts=True)
            rows += [(kind, int(a), int(b)) for a, b in zip(c, t)]
    return sorted(rows)


def host_join_sizes(s, p, o, V):
    """The no-FIS join histogram {size: lines}: per projection the distinct binary captures and the distinct
    always-emitted unary captures of every join value."""
    total = np.zeros(int(V), np.int64)
    for join, a, b in ((o, s, p), (p, s, o), (s, p, o)):
        _, pair_id = np.unique(a * V + b, return_inverse=True)
        for cond in (pair_id.astype(np.uint64), a):
            pairs = np.unique((join << np.uint64(32)) | cond)
            total += np.bincount((pairs >> np.uint64(32)).astype(np.int64), minlength=int(V))
    sz, times = np.unique(total[total > 0], return_counts=True)
    return dict(zip(sz.tolist(), times.tolist()))


def host_leg(ctx, d):
    """The same counts with numpy on the triples copied back from the device."""
    t0 = time.perf_counter()
    s, p, o = (x.astype(np.uint64) for x in ctx.copy_triples(d.n))
    t1 = time.perf_counter()
    V = np.uint64(max(d.num_terms, 1))
    rows = host_conditions(s, p, o, V)
    t2 = time.perf_counter()
    sizes = host_join_sizes(s, p, o, V)
    t3 = time.perf_counter()
    print(f"HISTO host route: download {(t1 - t0) * 1e3:.0f} ms, conditions (numpy.unique) {(t2 - t1) * 1e3:.0f} ms "
          f"({len(rows)} rows without kind 0), no-FIS join sizes {(t3 - t2) * 1e3:.0f} ms ({sum(sizes.values())} lines, "
          f"{len(sizes)} sizes); a command's 16 CPUs, of which numpy.unique uses one", flush=True)


def leg(scale, which):
    d = synth.config("c2", scale)
    with _lib.Context(0) as ctx:
        ctx.set_triples(d.s, d.p, d.o, d.num_terms)
        (device_leg if which == "device" else host_leg)(ctx, d)


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
    for which in ("device", "host"):  # chained: a leg that fails or runs out of time ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(scale), "--leg", which], timeout=LEG_LIMIT_S[which])
        if r.returncode:
            sys.exit(f"leg {which} failed ({r.returncode})")


if __name__ == "__main__":
    main()
