/* Test-only entry points of librdfind_hip.so (rdf_test_*): the scan and radix primitives of primitives.hip on
 * caller-given data, a report of the paths the last run took, the frequent-condition stage's shape and unary set, and
 * the split timing of the result statistics.  Not part of the product ABI (include/rdfind_hip.h): bound by
 * rdfind_amd/_lib.py for tests/test_gpu_primitives.py, tests/test_gpu_fc.py and the forced-path tests.
 *
 * Every call runs on the context's stream with the context's workspace, touches no pipeline state (the stage and
 * the last result stay; rdf_test_fc_trace sets a flag the next rdf_frequent_conditions reads) and fails with an
 * rdf_status and rdf_last_error like the product calls.
 *
 * Canaries: each call allocates its device buffers itself, with RDF_TEST_CANARY elements of the byte pattern
 * RDF_TEST_CANARY_BYTE directly before and directly after every range a primitive may write.  *canaries_ok = 1 when
 * all of them (and, for the scans, the input the primitive must not change) are intact after the call; it is
 * written whenever the buffers could be allocated, also when the primitive itself returned an error. */
#ifndef RDFIND_TEST_ABI_H
#define RDFIND_TEST_ABI_H

#include "../../include/rdfind_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RDF_TEST_CANARY 64
#define RDF_TEST_CANARY_BYTE 0xA5

/* rdf_test_scan kinds: input -> output element types */
enum { RDF_TEST_SCAN_U32_U32 = 0, RDF_TEST_SCAN_U32_U64 = 1, RDF_TEST_SCAN_U64_U64 = 2 };

/* Exclusive scan of in_host[0, n) into out_host[0, n); *total_out = the sum (read from the device only when
 * want_total, else the primitive gets a null total pointer and *total_out is left alone).
 * in_skew / out_skew: element offsets (0..3) of the device arrays from a 16-byte aligned address (0: the vector
 * kernels may run, otherwise not).  in_place: out == in on the device (equal element types only; out_skew must equal
 * in_skew) and the total goes to out[n], the way the pipeline's callers do it; otherwise the total has a buffer of
 * its own. */
rdf_status rdf_test_scan(rdf_ctx* ctx, int kind, const void* in_host, uint64_t n, uint32_t in_skew, uint32_t out_skew,
                         int in_place, int want_total, void* out_host, uint64_t* total_out, uint32_t* canaries_ok);

/* exclusive_scan_u32_u64_batch of k arrays of n elements: in_host = k rows of n uint32, out_host = k rows of n + 1
 * uint64 (the last one the row's total).  skew_mask: bit j skews input j by one element, bit 4 + j output j.
 * k outside 1..4 is passed through (the primitive must refuse it); at most 8. */
#define RDF_TEST_BATCH_CAP 8
rdf_status rdf_test_scan_batch(rdf_ctx* ctx, int k, const uint32_t* in_host, uint64_t n, uint32_t skew_mask,
                               uint64_t* out_host, uint32_t* canaries_ok);

/* rdf_test_radix ops */
enum {
    RDF_TEST_RADIX_SORT_BITS = 0,   /* radix_sort_u64_bits(lo, hi), uint64 keys */
    RDF_TEST_RADIX_SORT_DROP = 1,   /* radix_sort_u64_drop(bits = hi), uint64 keys; lo ignored */
    RDF_TEST_RADIX_PART_HASHED = 2, /* radix_partition_hashed(bits = hi, hmask), uint64 keys; lo ignored */
    RDF_TEST_RADIX_PART_U32 = 3     /* radix_partition_u32(lo, hi), uint32 keys */
};

/* out_host[0, *n_out) = the buffer `keys` names after the primitive's swaps; *n_out = n, for SORT_DROP the kept keys.
 * out_host holds n keys. */
rdf_status rdf_test_radix(rdf_ctx* ctx, int op, const void* keys_host, uint64_t n, int lo, int hi, uint64_t hmask,
                          void* out_host, uint64_t* n_out, uint32_t* canaries_ok);

/* radix_sort_passes(bits) */
int rdf_test_radix_passes(int bits);

/* The sort of keys that lie in segments (radix_seg_first_pass + radix_sort_u64_rest): segment b is seg_cnt[b] keys of
 * src_host[0, src_n) from seg_base[b] on (seg_base null: from b * stride on); the keys between the segments are not
 * part of the sort.  The call builds the segments' histogram of the low w0 bits on the host (w0 = 0: the width
 * radix_first_width(bits) gives), adds hist_bump to the count of digit hist_bump_digit of segment hist_bump_seg (0: the
 * true histogram; otherwise the primitive must report the disagreement: RDF_ERR_LIMIT), runs the first pass over the
 * segments and the remaining passes on bits [w0, bits).  out_host holds the segments' keys (sum of seg_cnt); *n_out =
 * their number.  Segments that overlap or leave src_host are refused (RDF_ERR_ARG). */
rdf_status rdf_test_radix_segments(rdf_ctx* ctx, const uint64_t* src_host, uint64_t src_n, const uint64_t* seg_base,
                                   uint64_t stride, const uint64_t* seg_cnt, uint32_t n_seg, int w0, int bits,
                                   int32_t hist_bump, uint32_t hist_bump_seg, uint32_t hist_bump_digit,
                                   uint64_t* out_host, uint64_t* n_out, uint32_t* canaries_ok);

/* The record-tile kernels of the group build (kernels.inl: k_fresh_bounds, k_keep_scatter, k_group_flags,
 * k_group_build) on caller data, every device array between canaries; no pipeline state is read or written.
 *
 * rdf_test_record_tile: records per tile (the kernels' edges lie at its multiples). */
int rdf_test_record_tile(void);

/* The support and keep passes over n sorted records keys_host[i] = capture << joinbits | join (capture < ncap, join <
 * 2^joinbits, 1 <= joinbits <= 32; unsorted keys are refused, RDF_ERR_ARG): support_out[0, ncap) = distinct join values
 * per capture; the captures with support >= ms are frequent, *C_out of them, numbered in ascending order; *Jf_out =
 * the distinct records of frequent captures, dk_out[0, Jf) = compact capture << 32 | join in (capture, join) order,
 * fk_out[0, Jf) = join << 32 | compact capture at the same positions; doff_out[0, C] = each compact capture's first
 * position in dk (doff_out[C] = Jf).  dk_out and fk_out hold n entries, doff_out ncap + 1. */
rdf_status rdf_test_keep_records(rdf_ctx* ctx, const uint64_t* keys_host, uint64_t n, int joinbits, uint64_t ncap,
                                 uint32_t ms, uint32_t* support_out, uint64_t* Jf_out, uint32_t* C_out, uint64_t* dk_out,
                                 uint64_t* fk_out, uint64_t* doff_out, uint32_t* canaries_ok);

/* The group passes over n records fk_host[i] = join << 32 | capture sorted by join value (join < V; refused otherwise):
 * *G_out = distinct join values; goff_out[0, G] = rbase + each group's first record (goff_out[G] = rbase + n);
 * gcap_out[0, n) = the records' captures; gmap_out[0, V): gbase + the group of every join value that occurs, the fill
 * pattern (RDF_TEST_CANARY_BYTE) elsewhere.  rbase / gbase: the offsets of a join range's records and groups in the
 * whole arrays (k_group_build_at; both 0: k_group_build); nothing before them may be written.  goff_out holds n + 1
 * entries. */
rdf_status rdf_test_group_build(rdf_ctx* ctx, const uint64_t* fk_host, uint64_t n, uint32_t V, uint64_t rbase,
                                uint32_t gbase, uint64_t* G_out, uint64_t* goff_out, uint32_t* gcap_out, uint32_t* gmap_out,
                                uint32_t* canaries_ok);

/* radix_sort_pairs_u32 on caller data: the n pairs (keys_host[i], vals_host[i]) stably sorted by key bits [lo, hi) into
 * keys_out / vals_out (n entries each).  The six device arrays lie between canaries; *canaries_ok also says that the input
 * keys and values still hold what was uploaded and that a sort of a single pass left the scratch arrays alone. */
rdf_status rdf_test_radix_pairs(rdf_ctx* ctx, const uint32_t* keys_host, const uint32_t* vals_host, uint64_t n, int lo,
                                int hi, uint32_t* keys_out, uint32_t* vals_out, uint32_t* canaries_ok);

/* The key-value form of the one-pass group build (g_compact_groups under RDFIND_GROUP_KV: k_fresh_bounds,
 * k_keep_scatter_kv, radix_sort_pairs_u32, k_group_flags_kv, k_group_build_kv, k_dgrp_kv) over n sorted records keys_host[i]
 * = capture << joinbits | join as rdf_test_keep_records takes them, join < V <= 2^joinbits.  support_out[0, ncap), *C_out,
 * *Jf_out and doff_out[0, C] as there; dgrp_out[0, Jf) = the group of every kept record in (capture, join) order; *G_out,
 * goff_out[0, G] (goff_out[G] = Jf), gcap_out[0, Jf) and gmap_out[0, V) as rdf_test_group_build gives them with rbase =
 * gbase = 0.  dgrp_out and gcap_out hold n entries, goff_out n + 1, doff_out ncap + 1.  The sorted joins live in the dgrp
 * array until k_dgrp_kv overwrites them, as in the pipeline. */
rdf_status rdf_test_group_kv(rdf_ctx* ctx, const uint64_t* keys_host, uint64_t n, int joinbits, uint64_t ncap, uint32_t ms,
                             uint32_t V, uint32_t* support_out, uint64_t* Jf_out, uint32_t* C_out, uint64_t* doff_out,
                             uint32_t* dgrp_out, uint64_t* G_out, uint64_t* goff_out, uint32_t* gcap_out,
                             uint32_t* gmap_out, uint32_t* canaries_ok);

/* Paths of the last completed run (RDF_ERR_STATE without one).  0 in a form field: that stage made no choice
 * (K2 and K3 of an input without triples). */
enum { RDF_TEST_K1_PARTITIONED = 1, RDF_TEST_K1_RADIX = 2, RDF_TEST_K1_ATOMIC = 3 };
enum { RDF_TEST_K2_PLAIN = 1, RDF_TEST_K2_SPLIT = 2, RDF_TEST_K2_RADIX = 3, RDF_TEST_K2_ATOMIC = 4 };
enum { RDF_TEST_K3_ONEPASS = 1, RDF_TEST_K3_TWOPASS = 2 }; /* TWOPASS: some emission ran as count + write */
enum { RDF_TEST_GROUPS_U64 = 1, RDF_TEST_GROUPS_KV = 2 }; /* KV: u32 joins and captures, the key-value group sort */

typedef struct rdf_test_path_report {
    uint32_t k1_form, k2_form, k3_form;
    uint32_t dense_on;             /* the light pass read member bitmaps */
    uint32_t light_stage;          /* the LDS-staging light kernel */
    uint32_t light_hiocc;          /* the high-occupancy plain light kernel */
    uint64_t n_dense;              /* light groups with a bitmap row */
    uint64_t n_dense_eligible;     /* ... of those large enough for one (the byte budget may hold fewer) */
    uint64_t n_dedup_members;      /* light dependents that took their class representative's refs */
    /* The light launches of the last discovery: sums over its pages, dependent ranges and (two light passes) both
     * passes; the npx fields are those of the last launch of that kernel. */
    uint64_t n_light_items;        /* k_light work items (dependent x chunk of 64 candidates x segment of groups) */
    uint64_t n_packed_octets;      /* k_light_packed output octets */
    uint64_t n_mseg_chunks;        /* chunks of multi-segment dependents (k_light_mseg_emit) */
    uint64_t n_multi_items;        /* k_light items of dependents with several chunks (unpaged single-GPU runs; else 0) */
    uint64_t n_light_survivors;    /* two light passes: pass A's tagged survivors, the input of pass B */
    uint32_t light_npx;            /* extra pivots k_light checked */
    uint32_t packed_npx;           /* ... and k_light_packed */
    uint32_t light_ordered;        /* k_light got an issue order (k_light_order) */
    uint32_t light_side;           /* k_light_packed ran on the side stream beside k_light */
    uint32_t light_two_pass;       /* the two light passes */
    uint32_t sig_on;               /* the run computed light-group signatures */
    uint32_t piv2_on;              /* ... and second pivots */
    uint32_t k3_hist;              /* K3 counted the record sort's first digit: the sort's first pass read K3's regions */
    /* The mask classes of the last discovery, read from what the run left on the device when rdf_test_paths is called
     * (the run itself does no more for them).  The chunk and list fields are those of a single-GPU run; a rank of a
     * sharded run among several reports 0. */
    uint32_t hclassed;             /* the binary heavy-only dependents took their refs from the class lists */
    uint64_t n_class_chunks;       /* k_class_eval work items: chunks of 64 members of the classes' pivot groups */
    uint64_t n_emit_tiles;         /* k_class_emit tiles of the class part (member tiles x list segments) */
    uint64_t max_class_list;       /* refs of the longest class list L'(m) */
    uint64_t n_multi_seg_lists;    /* class lists longer than one emission segment (CLS_LS refs) */
    /* K3's key items (RDFIND_EMIT_KEYS) of the last group build; a rank of a sharded run reports its own */
    uint64_t k3_key_items;         /* frequent binary keys the emission took as items behind the triples (0: switch off) */
    uint64_t k3_suppressed;        /* records the triples left to those items (they still count as n_records) */
    uint32_t group_form;           /* RDF_TEST_GROUPS_* of the last one-pass group build (RDFIND_GROUP_KV); 0: a range build */
} rdf_test_path_report;

rdf_status rdf_test_paths(rdf_ctx* ctx, rdf_test_path_report* out);

/* What the exchange of the last completed sharded run (rdf_shard_begin .. RDF_X_DONE) did on this rank
 * (RDF_ERR_STATE without one, or after a later run of another kind).  Every field but the last is a number the phases
 * hold on the host anyway: a run launches, copies and waits exactly as it did.  max_verify_per_dep is computed when the
 * call is made, from the verify offsets sh_phase15 left on the device (have_max_verify = 0, and the field 0, when they
 * are gone). */
typedef struct rdf_test_shard_report_t {
    uint32_t rank, nranks;
    uint64_t holder_survivors;   /* pairs this rank's holder pass kept (phase 5) */
    uint64_t routed_words;       /* words it routed: reports_sent + verify_sent */
    uint64_t reports_sent;       /* ... one report per survivor to the dependent's owner */
    uint64_t verify_sent;        /* ... and one verify word per other rank with a light group of the dependent */
    uint64_t reports_received;   /* holders' reports received as an owner (phase 15) */
    uint64_t verify_received;    /* verify pairs received (phase 15) */
    uint64_t verify_kept;        /* ... of which this rank's verify pass kept */
    uint64_t owner_reports;      /* phase 6: holders' and verifiers' reports this owner counted */
    uint64_t owner_kept;         /* ... distinct pairs reported by every rank with a light group (need-complete) */
    uint64_t unary_own;          /* ... of those, pairs of unary dependents (sent to every rank) */
    uint64_t binary_own;         /* ... and pairs of binary dependents (kept here) */
    uint64_t unary_gathered;     /* unary dependents' pairs of all ranks (phase 7) */
    uint64_t n_classes;          /* mask classes (the same on every rank) */
    uint64_t n_class_members;    /* class members this rank owns */
    uint64_t n_class_items;      /* class work items (chunks of 64 pivot members) of the classes pivoted here */
    uint64_t n_list_entries;     /* class list entries this rank contributed to the all-gather */
    uint64_t hot_entries;        /* entries of the hot owner table */
    uint64_t heavy_base;         /* this rank's first heavy bit */
    uint64_t heavy_columns;      /* heavy columns of this rank's join shard */
    uint32_t have_max_verify;
    uint64_t max_verify_per_dep; /* the most verify pairs received for one dependent */
} rdf_test_shard_report_t;

rdf_status rdf_test_shard_report(rdf_ctx* ctx, rdf_test_shard_report_t* out);

/* Frequent-condition counting (K1 / K2, counts.inl) on its own: which branches the last rdf_frequent_conditions took,
 * and the frequent unary set it left on the device.  All four calls need only that stage (RDF_ERR_STATE before it and
 * after rdf_release_scratch), not a whole run.
 *
 * rdf_test_fc_trace: off by default.  Only while it is on does rdf_frequent_conditions read the K1 and K2 slice lists
 * back (two copies and host waits more) to fill the slice fields of the report; off, the stage issues the launches and
 * host waits it always did, and those fields are zero. */
rdf_status rdf_test_fc_trace(rdf_ctx* ctx, int on);

typedef struct rdf_test_fc_report_t {
    uint32_t traced;      /* the stage ran with the trace on: the fields marked (t) are filled */
    uint32_t k1_form;     /* RDF_TEST_K1_* */
    uint32_t k1_bits;     /* key bits per K1 bucket: 14 or 15 (0: the atomic form has no buckets) */
    uint32_t k2_form;     /* RDF_TEST_K2_* (0: no triples) */
    uint32_t k2_bits;     /* bucket bits of K2's first level (the radix form: of its hash prefix) */
    uint32_t k2_sub;      /* bits of the second-level split (k_b2_split), 0 without one */
    uint64_t k1_buckets;  /* K1 buckets */
    uint64_t k1_slices;   /* (t) K1 counting slices (a bucket without records has one too) */
    uint64_t k1_multi;    /* (t) K1 buckets counted by more than one slice (ranked by k_u2_finish) */
    uint64_t k2_buckets;  /* K2 counting buckets (first level << sub) */
    uint64_t k2_multi;    /* (t) K2 buckets counted by more than one slice (all partials to the spill list) */
    uint64_t k2_spill;    /* spill entries handed to fc_sum_pairs: partials of multi-slice buckets + refused records */
} rdf_test_fc_report_t;

rdf_status rdf_test_fc_report(rdf_ctx* ctx, rdf_test_fc_report_t* out);

/* fval[0, U) (the values of the frequent unary conditions in rank order: subjects, predicates, objects, each ascending)
 * into fval_host[0, cap), *U_out = U, n3 = the frequent s / p / o counts.  cap < U: RDF_ERR_ARG, nothing copied. */
rdf_status rdf_test_copy_frequent_unary(rdf_ctx* ctx, uint32_t* fval_host, uint64_t cap, uint64_t* U_out, uint64_t* n3);

/* rank_out[i] = the global rank of unary key keys[i] = pos * V + value among the frequent conditions (0xffffffff: not
 * frequent), bit_out[i] = its bit of the frequency bitmap K2 reads.  A gather on the device: nothing sized by |V| moves.
 * A key >= 3V is refused (RDF_ERR_ARG) before anything runs; the outputs lie between canaries. */
rdf_status rdf_test_unary_lookup(rdf_ctx* ctx, const uint64_t* keys, uint64_t n, uint32_t* rank_out, uint32_t* bit_out,
                                 uint32_t* canaries_ok);

/* The key lookup of the last rdf_rewrite_terms: the tables staged in LDS, or read from global memory (a table too
 * large for LDS).  0: no call yet, or the last one had no keys or no terms. */
enum { RDF_TEST_RW_LDS = 1, RDF_TEST_RW_GLOBAL = 2 };
rdf_status rdf_test_rewrite_form(rdf_ctx* ctx, uint32_t* form);

/* Device time (ms) of the last result statistics (rdf_cind_stats_begin .. _end, rdf_cind_histogram), split:
 * [0] the explicit passes of its add calls, [1] their class passes, [2] the end.  For tools/cindstats_bench.py. */
rdf_status rdf_test_cind_stats_times(rdf_ctx* ctx, float* ms3);

#ifdef __cplusplus
}
#endif
#endif
