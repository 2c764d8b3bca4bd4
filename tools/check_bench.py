"""Dev tool: the CIND check (rdf_check_cinds) on c2 at scale 1, with the result of a discovery as candidates, next to the
discovery that produced them.
  (d) the discovery itself (rdf_run), REPS runs after a warm-up one: host clock around the call and its sync, and the
      summed device time of its three stages;
  (a) every explicit row of the result as a candidate (the class part, members x shared lists, is 10^9 rows and more:
      beyond the 2^31 candidates of one call, and 24 B each);
  (b) a 1,000-row sample of it, evenly spaced;
  (c) a 250-row sample, whose condition table fits the LDS form;
  (b0) / (c0) the same samples in a context created with RDFIND_CHECK_LDS_SLOTS=0 (the table probed in global memory).
Each check: REPS calls after a warm-up one; the device time between HIP events (rdf_check_stats.ms_*) and the host clock
around the call, which ends in a stream wait.  Per stage the share of the 8 TB/s HBM peak by its algorithmic bytes
(DESIGN.md section 4): match 12 N per pass (a count pass and a write pass per batch) + 8 B per record written, sort
16 B per record and pass, intersection 4 B per dependent value.
python tools/check_bench.py [cfg scale]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from rdfind_amd import _lib, synth

REPS = 5
PEAK = 8e12  # bytes / s


def med(xs):
    return float(np.median(xs))


def bits_for(maxval):
    return max(int(maxval).bit_length(), 1)


def candidates(rows):
    return np.stack([rows[k] for k in ("dep_capture_type", "dep_value1", "dep_value2", "ref_capture_type", "ref_value1",
                                       "ref_value2")], axis=1).astype(np.uint32)


def leg(ctx, name, cands, n, num_terms, supports):
    tot, host, parts = [], [], []
    for _ in range(REPS + 1):
        t = time.perf_counter()
        rows, _ = ctx.check_cinds(cands, 0)
        host.append((time.perf_counter() - t) * 1e3)
        st = ctx.last_check
        tot.append(st["ms_total"])
        parts.append((st["ms_match"], st["ms_sort"], st["ms_intersect"]))
    assert st["n_holding"] == len(cands) and (rows["dep_support"] == supports).all(), "a row of the result does not hold"
    m, s, i = (med([p[k] for p in parts[1:]]) for k in range(3))
    passes = ctx.lib.rdf_test_radix_passes(bits_for(st["n_captures"] - 1) + bits_for(num_terms - 1))
    b_match = 12 * n * 2 * st["n_batches"] + 8 * st["n_records"]
    b_sort = 16 * st["n_records"] * passes
    b_isect = 4 * int(rows["dep_support"].astype(np.uint64).sum())
    share = lambda b, ms: b / (ms * 1e-3) / PEAK if ms > 0 else 0.0
    print(f"CHECK ({name}) {len(cands)} candidates: {st['n_captures']} captures, {st['n_conditions']} conditions, table in LDS "
          f"{st['table_in_lds']} (cap {st['lds_slots']} slots), {st['n_batches']} batch, {st['n_records']} records, "
          f"{st['n_values']} distinct values, {st['n_work_items']} work items of {st['chunk_values']}", flush=True)
    print(f"CHECK ({name}) device total {med(tot[1:]):.3f} ms (min {min(tot[1:]):.3f}, max {max(tot[1:]):.3f}), host "
          f"{med(host[1:]):.3f} ms; match {m:.3f} ms = {share(b_match, m):.3f} of HBM peak ({b_match} B), sort + unique {s:.3f} ms "
          f"= {share(b_sort, s):.3f} ({b_sort} B, {passes} passes), intersect {i:.3f} ms = {share(b_isect, i):.3f} ({b_isect} B)",
          flush=True)
    return med(tot[1:]), (m, s, i)


def main():
    cfg, scale = (sys.argv[1], float(sys.argv[2])) if len(sys.argv) > 2 else ("c2", 1.0)
    d = synth.config(cfg, scale)
    os.environ.pop("RDFIND_CHECK_LDS_SLOTS", None)
    with _lib.Context(0) as ctx:
        ctx.set_triples(d.s, d.p, d.o, d.num_terms)
        dev, host = [], []
        for _ in range(REPS + 1):
            ctx.sync()
            t = time.perf_counter()
            cs = ctx.run(d.min_support)
            ctx.sync()
            host.append((time.perf_counter() - t) * 1e3)
            dev.append(sum(ctx.stage_times()))
        L = ctx.result_layout()
        d_dev, d_host = med(dev[1:]), med(host[1:])
        print(f"CHECK {cfg} at {scale}: n {d.n}, {d.num_terms} terms, support {d.min_support}, {cs['n_cinds']} CINDs = "
              f"{L['n_refs']} explicit refs in {L['n_runs']} runs + {cs['n_class_cinds']} class rows", flush=True)
        print(f"CHECK (d) discovery: device {d_dev:.3f} ms (min {min(dev[1:]):.3f}, max {max(dev[1:]):.3f}), host {d_host:.3f} ms",
              flush=True)
        rows = ctx.copy_cinds_decoded(0, L["n_refs"])
        cands, sup = candidates(rows), rows["support"]
        pick = {k: np.linspace(0, len(cands) - 1, k).astype(np.int64) for k in (1000, 250)}
        a_ms, a_parts = leg(ctx, "a: all explicit rows", cands, d.n, d.num_terms, sup)
        b_ms, _ = leg(ctx, "b: 1,000-row sample", cands[pick[1000]], d.n, d.num_terms, sup[pick[1000]])
        c_ms, _ = leg(ctx, "c: 250-row sample", cands[pick[250]], d.n, d.num_terms, sup[pick[250]])
    os.environ["RDFIND_CHECK_LDS_SLOTS"] = "0"
    with _lib.Context(0) as ctx:
        ctx.set_triples(d.s, d.p, d.o, d.num_terms)
        b0_ms, _ = leg(ctx, "b0: 1,000-row sample, table in global memory", cands[pick[1000]], d.n, d.num_terms, sup[pick[1000]])
        c0_ms, _ = leg(ctx, "c0: 250-row sample, table in global memory", cands[pick[250]], d.n, d.num_terms, sup[pick[250]])
    os.environ.pop("RDFIND_CHECK_LDS_SLOTS")
    stage = ("match", "sort + unique", "intersect")[int(np.argmax(a_parts))]
    print(f"CHECK (a) / (d) device {a_ms / d_dev:.2f}x: checking the {len(cands)} explicit rows costs "
          f"{'more' if a_ms > d_dev else 'less'} than discovering the result; its largest stage is {stage}", flush=True)
    print(f"CHECK (b0) / (b) {b0_ms / b_ms:.2f}x, (c0) / (c) {c0_ms / c_ms:.2f}x (global table over the default)", flush=True)


if __name__ == "__main__":
    main()
