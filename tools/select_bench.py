"""Dev tool: the result selection (rdf_select_cinds) on the c2 result at scale 1, whose class part stays pending, next to
the cheapest way the row accessors alone reach the same rows.  After one run and its statistics, for the most
referenced capture T:
  (a) the count-only selection of the CINDs with ref = T;
  (b) the same selection with its view, and the view formatted whole (rdf_format_selected, device to host included);
  (c) rdf_copy_cinds_range(0, 1, ...), which does nothing but force the class part's expansion (materialize): every row
      accessor and the formatter start with it.  It understates that route, which still has to scan all rows after it.
(a) and (b): REPS calls after a warm-up one, the device time between HIP events (rdf_select_cinds' *ms) and the host
clock around the calls, which end in a stream wait.  (c) can run once per discovery, so the discovery is repeated REPS
times after a warm-up round; its device time is the class emission timer, its host time the clock around the call.
HBM held (rdf_device_bytes) is printed before and after each step.
python tools/select_bench.py [cfg scale]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from rdfind_amd import _lib, synth

REPS = 5
CODES = _lib.SEL_CODES


def med(xs):
    return float(np.median(xs))


def main():
    cfg, scale = (sys.argv[1], float(sys.argv[2])) if len(sys.argv) > 2 else ("c2", 1.0)
    d = synth.config(cfg, scale)
    terms = ["<http://www.Department%d.University%d.edu/Term%d>" % (i % 15, i % 7, i) for i in range(d.num_terms)]
    with _lib.Context(0) as ctx:
        ctx.set_triples(d.s, d.p, d.o, d.num_terms)
        cs = ctx.run(d.min_support)
        ctx.set_dictionary(terms)
        ctx.cind_histogram()
        top = ctx.top_refs(1)
        L = ctx.result_layout()
        code, v1, v2 = (int(x[0]) for x in _lib.decode_captures(top["capture"], ctx.num_terms, ctx.binary_keys()))
        pat = [(1 << CODES.index(code), v1, v2)]
        want = int(top["cinds"][0])
        print(f"SELECT {cfg} at {scale}: n {d.n}, support {d.min_support}, {L['n_captures']} captures, {cs['n_cinds']} CINDs = "
              f"{L['n_refs']} explicit refs in {L['n_runs']} runs + {cs['n_class_cinds']} of {L['n_members']} class members "
              f"over {L['n_lists']} lists of {L['n_list_refs']} refs; most referenced capture: code {code}, {want} CINDs",
              flush=True)
        held0 = ctx.device_bytes()
        print(f"SELECT HBM held before: {held0} bytes", flush=True)
        # (a) count only
        dev, host = [], []
        for _ in range(REPS + 1):
            t = time.perf_counter()
            n = ctx.select_cinds(ref=pat, count_only=True)
            host.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.last_select_ms)
            assert n == want
        held_a = ctx.device_bytes()
        a_dev, a_host = med(dev[1:]), med(host[1:])
        print(f"SELECT (a) count only: {n} rows; device {a_dev:.3f} ms (min {min(dev[1:]):.3f}, max {max(dev[1:]):.3f}), host "
              f"{a_host:.3f} ms; HBM held after: {held_a} bytes (+{held_a - held0})", flush=True)
        # (b) the view and its formatting
        dev, host, fmt = [], [], []
        nbytes = held_view = 0
        for k in range(REPS + 1):
            t = time.perf_counter()
            n = ctx.select_cinds(ref=pat)
            host.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.last_select_ms)
            if k == 0:
                held_view = ctx.device_bytes()  # the view and the selection's scratch, before the formatter's buffers
            t = time.perf_counter()
            nbytes = len(ctx.format_selected_array())
            fmt.append((time.perf_counter() - t) * 1e3)
            assert n == want
        held_b = ctx.device_bytes()
        b_dev, b_host, b_fmt = med(dev[1:]), med(host[1:]), med(fmt[1:])
        view = max(n, 1) * 4 + (L["n_runs"] + L["n_members"] + 1) * 12
        print(f"SELECT (b) view: {n} rows; device {b_dev:.3f} ms (min {min(dev[1:]):.3f}, max {max(dev[1:]):.3f}), host "
              f"{b_host:.3f} ms; formatting {nbytes} bytes: host {b_fmt:.3f} ms (device to host included); HBM held after the "
              f"view: {held_view} bytes (+{held_view - held0}), after its formatting (capture strings, line offsets, the text): "
              f"{held_b} bytes (+{held_b - held0}); the view is at most {view} bytes, captures + runs + list refs + members "
              f"= {L['n_captures'] + L['n_runs'] + L['n_list_refs'] + L['n_members']}", flush=True)
        assert ctx.kernel_times()["cemit"] == 0.0  # the class part stayed pending through (a) and (b)
        print("SELECT class part still pending after (a) and (b): cemit timer 0.0", flush=True)
        # (c) the expansion every row accessor starts with
        dev, host = [], []
        for k in range(REPS + 1):
            if k:
                ctx.run(d.min_support)
            ctx.sync()
            t = time.perf_counter()
            ctx.copy_cinds_range(0, 1)
            host.append((time.perf_counter() - t) * 1e3)
            dev.append(ctx.kernel_times()["cemit"])
        held_c = ctx.device_bytes()
        c_dev, c_host = med(dev[1:]), med(host[1:])
        print(f"SELECT (c) rdf_copy_cinds_range(0, 1): device (class emission) {c_dev:.3f} ms (min {min(dev[1:]):.3f}, max "
              f"{max(dev[1:]):.3f}), host {c_host:.3f} ms; HBM held after: {held_c} bytes (+{held_c - held0})", flush=True)
        print(f"SELECT (c) / (a) device {c_dev / max(a_dev, 1e-9):.1f}x, (c) / (b) device {c_dev / max(b_dev, 1e-9):.1f}x, "
              f"(c) / ((b) + formatting) host {c_host / max(b_host + b_fmt, 1e-9):.1f}x", flush=True)


if __name__ == "__main__":
    main()
