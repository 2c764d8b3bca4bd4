"""numpy restatement of the key-value form of the one-pass group build (rdfind_amd/csrc/rdfind_hip.hip g_compact_groups
under RDFIND_GROUP_KV) and of its pair sort (primitives.hip radix_sort_pairs_u32), for tests/test_group_kv_cpu.py and
tests/test_gpu_group_kv.py.

The build takes the K3 records ``capture << joinbits | join`` sorted by (capture, join), with repeats.  A capture's
support is its number of distinct join values; the captures with support >= ms are frequent and numbered in ascending
order (compact ids).  The distinct records of frequent captures are kept, Jf of them, in (capture, join) order; stably
sorted by join value they are the capture groups: one group per join value that occurs, numbered in ascending join
order, each group's captures ascending."""
import numpy as np

PATTERN = np.uint32(0xA5A5A5A5)  # what rdf_test_group_kv leaves in gmap at join values without kept records


def pair_sort(keys, vals, lo, hi):
    """(keys, vals) stably sorted by key bits [lo, hi)."""
    keys = np.asarray(keys, np.uint32)
    vals = np.asarray(vals, np.uint32)
    field = (keys.astype(np.uint64) >> np.uint64(lo)) & np.uint64((1 << max(hi - lo, 0)) - 1)
    order = np.argsort(field, kind="stable")
    return keys[order], vals[order]


def kept_records(records, joinbits, ncap, ms):
    """support[ncap], and the kept records as (compact capture, join) in (capture, join) order."""
    uk = np.unique(np.asarray(records, np.uint64))
    cap = (uk >> np.uint64(joinbits)).astype(np.int64)
    join = (uk & np.uint64((1 << joinbits) - 1)).astype(np.uint32)
    support = np.bincount(cap, minlength=ncap).astype(np.uint32)
    freq = support >= ms
    fidx = (np.cumsum(freq) - freq).astype(np.uint32)
    keep = freq[cap]
    return support, fidx[cap[keep]], join[keep]


def group_kv(records, joinbits, ncap, ms, num_values):
    """The whole build: a dict of support, doff, dgrp, G, goff, gcap, gmap and Jf."""
    support, kc, kj = kept_records(records, joinbits, ncap, ms)
    jf = kj.shape[0]
    doff = np.concatenate([[0], np.cumsum(support[support >= ms], dtype=np.uint64)]).astype(np.uint64)
    sj, gcap = pair_sort(kj, kc, 0, joinbits)
    head = np.ones(jf, bool)
    head[1:] = sj[1:] != sj[:-1]
    first = np.flatnonzero(head)
    g = first.shape[0]
    goff = np.concatenate([first, [jf]]).astype(np.uint64)
    gmap = np.full(num_values, PATTERN, np.uint32)
    gmap[sj[first]] = np.arange(g, dtype=np.uint32)
    return {"support": support, "doff": doff, "dgrp": gmap[kj], "G": g, "goff": goff, "gcap": gcap, "gmap": gmap, "Jf": jf}
