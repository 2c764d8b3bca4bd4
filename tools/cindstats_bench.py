"""Dev tool: the result statistics on the device (rdf_cind_histogram) next to the discovery they describe.  Per
config: one run, then the statistics of its result REPS times with the class part still pending; prints the device time
split into the explicit pass (one atomic add per explicit ref into the in-degree array), the class pass (O(members +
list refs) per class) and the end (sorts and run lengths over the captures), beside rdf_stage_times()[2] (the
discovery stage) of the same run.
python tools/cindstats_bench.py                      c2 at scale 1 and c5 at 0.3 (the largest c5 that runs unpaged),
                                                     each a child process with its own time limit; a failed leg stops
                                                     the run
python tools/cindstats_bench.py --leg c5 0.3         one leg"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from rdfind_amd import _lib, synth

LEGS = (("c2", 1.0), ("c5", 0.3))
LEG_LIMIT_S = 400
REPS = 5  # the first one warms up (allocations), the median of the others is reported


def leg(cfg, scale):
    d = synth.config(cfg, scale)
    with _lib.Context(0) as ctx:
        ctx.set_triples(d.s, d.p, d.o, d.num_terms)
        cs = ctx.run(d.min_support)
        ctx.sync()
        discover_ms = ctx.stage_times()[2]
        L = ctx.result_layout()
        parts, total, rows = [], [], None
        for _ in range(REPS):
            rows = ctx.cind_histogram()
            parts.append(ctx.cind_stats_times())
            total.append(ctx.hist_ms)
        assert ctx.kernel_times()["cemit"] == 0.0  # the class part stayed pending
        top = ctx.top_refs(1)
        kinds = np.bincount(rows["kind"], minlength=5)[1:]
        explicit, cls, end = (float(np.median([p[i] for p in parts[1:]])) for i in range(3))
        ms = float(np.median(total[1:]))
        print(f"CINDSTATS {cfg} at {scale}: n {d.n}, support {d.min_support}, {L['n_captures']} captures, "
              f"{cs['n_cinds']} CINDs = {L['n_refs']} explicit refs + {cs['n_class_cinds']} of {L['n_members']} class members "
              f"over {L['n_lists']} lists of {L['n_list_refs']} refs", flush=True)
        print(f"CINDSTATS {cfg} at {scale}: rdf_cind_histogram {ms:.3f} ms = explicit {explicit:.3f} + class {cls:.3f} + "
              f"end {end:.3f}; discovery stage {discover_ms:.3f} ms; ratio {ms / discover_ms:.3f} "
              f"(explicit pass {explicit / discover_ms:.3f}); {L['n_refs'] / max(explicit, 1e-9) / 1e6:.1f} G explicit refs/s; "
              f"rows by kind {kinds.tolist()}, top in-degree {int(top['cinds'][0]) if len(top) else 0}", flush=True)


def main():
    args = sys.argv[1:]
    if "--leg" in args:
        i = args.index("--leg")
        return leg(args[i + 1], float(args[i + 2]))
    for cfg, scale in LEGS:  # chained: a leg that fails or runs out of time ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", cfg, str(scale)], timeout=LEG_LIMIT_S)
        if r.returncode:
            sys.exit(f"leg {cfg} at {scale} failed ({r.returncode})")


if __name__ == "__main__":
    main()
