// The RDFIND_* environment switches: one table, one reader.  (DESIGN.md lists them for readers of the documents.)
//
// A row is SW(field, type, default, "NAME", parse, kind, "doc"): `parse` is an expression over the variable's value
// `v` (a C string, the variable is set) and the struct being filled `s` (s.field still holds the default); an unset
// variable leaves the default.  Kinds:
//   TEST  test hook: forces a path that large or differently shaped inputs take on their own
//   AB    selects a path (or a constant) the code never chooses itself; candidates for pruning
//   DIAG  diagnostic output
// Scope: the rows of RDF_CTX_SWITCHES are read when a context is created (rdf_ctx_create -> read_switches) and held
// by value in it, so two contexts of one process may differ.  The rows of RDF_PROC_SWITCHES are used where no context
// exists; they are read once per process, at their first use (proc_switches).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "common.hpp"

namespace rdf {

// a switch without a default value: unset leaves the decision to the code
template <typename T>
struct Opt {
    bool set = false;
    T v{};
};
static inline Opt<int> opt_int(const char* v) { return {true, atoi(v)}; }
static inline Opt<u64> opt_u64(const char* v) { return {true, strtoull(v, nullptr, 10)}; }
static inline Opt<std::string> opt_str(const char* v) { return {true, v}; }
static inline bool is_set(const char*) { return true; }  // any value, the empty one too
static inline u64 positive_or(const char* v, u64 dflt) { return atoll(v) > 0 ? (u64)atoll(v) : dflt; }
struct RankPhase {
    int rank = -1, phase = -1;
};
static inline RankPhase rank_phase(const char* v) {  // "rank:phase"; anything else: no rank
    RankPhase r;
    if (sscanf(v, "%d:%d", &r.rank, &r.phase) != 2) r = RankPhase();
    return r;
}

// clang-format off
#define RDF_CTX_SWITCHES(SW) \
    /* frequent conditions */ \
    SW(count_atomic, bool, false, "RDFIND_COUNT_PATHS", !strcmp(v, "atomic"), TEST, \
       "=atomic: the global-atomic counting kernels (the fallback of the partitioned K1 / K2 for |V| > 2^26 / 3)") \
    SW(u1_radix_min, u64, 0, "RDFIND_U1_RADIX_MIN", strtoull(v, nullptr, 10), TEST, \
       "3n from which K1 takes its radix form (0: the rule, U1_RADIX_MIN and the bucket count)") \
    SW(b2_split, int, 1, "RDFIND_B2_SPLIT", atoi(v), AB, \
       "0: K2 never groups its records by hash prefix (no k_b2_emit / k_b2_split)") \
    SW(b2_radix_min, u64, B2_RADIX_MIN, "RDFIND_B2_RADIX_MIN", strtoull(v, nullptr, 10), TEST, \
       "3n from which K2 groups compact records with the radix passes") \
    /* chunked ingest */ \
    SW(nt_dict_slots, u64, 1ull << 16, "RDFIND_NT_DICT_SLOTS", positive_or(v, s.nt_dict_slots), TEST, \
       "=<pow2>: initial slots of the chunked parse's persistent term table (small: tiny inputs rebuild it several times)") \
    SW(nt_fp_bits, int, 32, "RDFIND_NT_FP_BITS", std::max(0, std::min(atoi(v), 32)), TEST, \
       "=<0..32>: fingerprint bits the chunked parse compares before the bytes (0: every occupied slot is byte-compared)") \
    /* capture groups */ \
    SW(heavy_min, u64, 64, "RDFIND_HEAVY_MIN", positive_or(v, s.heavy_min), TEST, \
       "minimum heavy-group size (a power of two; smaller groups are cheaper by binary search than as bit columns)") \
    SW(group_range_records, u64, 0, "RDFIND_GROUP_RANGE", positive_or(v, s.group_range_records), TEST, \
       "build the capture groups in join ranges of at most that many K3 records (0: only from 2^32 / 9 triples, automatic size)") \
    SW(range_keep, bool, true, "RDFIND_RANGE_KEEP", atoi(v) != 0, TEST, \
       "0: pass 2 of a range build always re-emits (as when pass 1's records do not fit)") \
    SW(emit_onepass, bool, true, "RDFIND_EMIT_ONEPASS", atoi(v) != 0, TEST, \
       "0: K3 as count pass + write pass (as when the record buffers hold fewer than 9 records per triple)") \
    SW(emit_hist, bool, true, "RDFIND_EMIT_HIST", atoi(v) != 0, AB, \
       "0: the one-pass K3 compacts its regions and the record sort counts its first digit itself (no histogram from K3)") \
    SW(emit_keys, bool, true, "RDFIND_EMIT_KEYS", atoi(v) != 0, AB, \
       "0: K3 has no key items: every triple writes the two unary records its frequent binary keys determine") \
    SW(emit_grid, u64, 0, "RDFIND_EMIT_GRID", strtoull(v, nullptr, 10), TEST, \
       "=<blocks>: cap of K3's emission grid (small: a small input's blocks emit regions of several sort sub-tiles)") \
    SW(group_kv, bool, true, "RDFIND_GROUP_KV", atoi(v) != 0, AB, \
       "0: the one-pass group build keeps and sorts its records as u64 (dk, fk), not as u32 joins and captures") \
    /* cinds: the pivot pass and the light passes */ \
    SW(allow_hclass, bool, true, "RDFIND_HCLASS", strcmp(v, "0") != 0, AB, \
       "=0: binary heavy-only dependents are not emitted from class lists") \
    SW(dense_div, int, -1, "RDFIND_DENSE", atoi(v), AB, \
       "bitmaps for light groups of >= C / <divisor> members on every input (0: none; unset: by input, d_dense_flags)") \
    SW(dense_min, u64, LIGHT_DENSE_MIN, "RDFIND_DENSE_MIN", positive_or(v, s.dense_min), TEST, \
       "absolute minimum size of a dense light group (bitmaps for small groups too)") \
    SW(dense_bytes, u64, DENSE_BYTES, "RDFIND_DENSE_BYTES", (u64)atoll(v), TEST, \
       "cap of the dense bitmaps' bytes (rows past the cap stay member lists)") \
    SW(sig, int, 2, "RDFIND_SIG", atoi(v), AB, \
       "light-group signatures: 0 off, 1 tested by k_light and the packed path, 2 by k_light only") \
    SW(piv2, int, 1, "RDFIND_PIV2", atoi(v), AB, \
       "second pivots: 0 off, 1 checked by k_light and the packed path, 2 by k_light only") \
    SW(pivx, bool, true, "RDFIND_PIVX", atoi(v) != 0, AB, \
       "0: no extra pivots after the second one (there are none without RDFIND_PIV2 either)") \
    SW(pivx_n, Opt<int>, {}, "RDFIND_PIVX_N", opt_int(v), AB, \
       "how many of the computed extra pivots k_light checks (unset: all the variant takes)") \
    SW(pivx_packed, Opt<int>, {}, "RDFIND_PIVX_PACKED", opt_int(v), TEST, \
       "0 / 1: the packed path checks the first extra pivot (unset: on large-group inputs)") \
    SW(stage, Opt<int>, {}, "RDFIND_STAGE", opt_int(v), TEST, \
       "0 / 1: k_light stages light groups in LDS rows (unset: by the weighted mean light group size)") \
    SW(light_hiocc, Opt<int>, {}, "RDFIND_LIGHT_HIOCC", opt_int(v), TEST, \
       "0 / 1: the plain k_light at 6 waves per SIMD (unset: by input; never with the staging variant)") \
    SW(light_side, bool, true, "RDFIND_LIGHT_SIDE", atoi(v) != 0, AB, \
       "0: k_light_packed on the context stream, not beside k_light on the side stream") \
    SW(light_order, Opt<u64>, {}, "RDFIND_LIGHT_ORDER", opt_u64(v), TEST, \
       "k_light items of dependents with >= that many group entries go first (0: off; unset: the staging variant only)") \
    SW(sweep_f, int, LIGHT_SWEEP_F, "RDFIND_SWEEP_F", atoi(v), AB, \
       "CindView::sweep_f, the window range sweeps of the light kernels (0: off)") \
    SW(light2, Opt<int>, {}, "RDFIND_LIGHT2", opt_int(v), AB, \
       "0 / 1: the two light passes (unset: one pass while the sweeps are compiled in)") \
    SW(light_dedup, int, -1, "RDFIND_LIGHT_DEDUP", atoi(v) != 0 ? 1 : 0, TEST, \
       "0: every light dependent verified on its own, 1: once per class of equal group lists (unset: where the light pass stages)") \
    SW(dup_min, u32, 256, "RDFIND_DUP_MIN", (u32)std::max(1, atoi(v)), TEST, \
       "the shortest group list that looks for an equal one") \
    /* sharded runs */ \
    SW(holder_qbits, int, 2, "RDFIND_HOLDER_Q", std::max(0, std::min(atoi(v), 8)), AB, \
       "pivot-holder election on log-size buckets (holder_key; 0: exact sizes; at most 8)") \
    SW(hot_balance, bool, true, "RDFIND_HOT_BALANCE", atoi(v) != 0, AB, \
       "0: every join value's owner by hash (no hot table)") \
    /* CIND check */ \
    SW(check_lds_slots, Opt<u64>, {}, "RDFIND_CHECK_LDS_SLOTS", opt_u64(v), TEST, \
       "=<slots>: cap of the condition table rdf_check_cinds stages in LDS (0: always probed in global memory)") \
    SW(check_records, Opt<u64>, {}, "RDFIND_CHECK_RECORDS", opt_u64(v), TEST, \
       "=<records>: record budget of one rdf_check_cinds batch (unset: by the free HBM; small: tiny inputs take several batches)") \
    /* failures on request */ \
    SW(test_fail_launch, std::string, {}, "RDFIND_TEST_FAIL_LAUNCH", std::string(v), TEST, \
       "=<kernel>: that kernel is launched with an invalid configuration (k_b2_split)") \
    SW(test_oom_discovery, bool, false, "RDFIND_TEST_OOM_DISCOVERY", atoi(v) != 0, TEST, \
       "rdf_discover_cinds fails with RDF_ERR_OOM (the paged fallback of the program)") \
    SW(test_fail_shard, RankPhase, {}, "RDFIND_TEST_FAIL_SHARD", rank_phase(v), TEST, \
       "=rank:phase: that rank's rdf_shard_step fails with RDF_ERR_OOM at that phase (cross-rank failure agreement)") \
    /* diagnostics */ \
    SW(debug_light, bool, false, "RDFIND_DEBUG_LIGHT", is_set(v), DIAG, \
       "set: the light pass's choices (dense rows, variant, occupancy, extra pivots) on stderr") \
    SW(light2_log, bool, false, "RDFIND_LIGHT2_LOG", is_set(v), DIAG, \
       "set: one line per discovery on the light passes' items and survivors") \
    SW(light_dump, Opt<std::string>, {}, "RDFIND_LIGHT_DUMP", opt_str(v), DIAG, \
       "=<path>: per-item records of k_light (builds with RDF_LIGHT_STATS only; tools/light_items.py)")

#define RDF_PROC_SWITCHES(SW) \
    SW(sync_trace, bool, false, "RDFIND_SYNC_TRACE", is_set(v), DIAG, \
       "set: every host wait prints SYNC <line> <t_us> <wait_us> (tools/sync_trace.py)") \
    SW(spin, bool, false, "RDFIND_SPIN", atoi(v) != 0, AB, \
       "1: host waits poll the stream instead of blocking in hipStreamSynchronize") \
    SW(mem_report, bool, false, "RDFIND_MEM_REPORT", atoi(v) != 0, DIAG, \
       "1: after each run, the context's buffers of >= 256 MiB and the peak on stderr") \
    SW(part_digit, int, 9, "RDFIND_PART_DIGIT", std::max(8, std::min(10, atoi(v))), AB, \
       "digit bits of radix_partition_hashed (8..10)")
// clang-format on

#define RDF_SW_FIELD(field, type, dflt, name, parse, kind, doc) type field = dflt;
#define RDF_SW_READ(field, type, dflt, name, parse, kind, doc) \
    if (const char* v = getenv(name)) s.field = (parse);

struct ProcSwitches {
    RDF_PROC_SWITCHES(RDF_SW_FIELD)
};
inline const ProcSwitches& proc_switches() {
    static const ProcSwitches once = [] {
        ProcSwitches s;
        RDF_PROC_SWITCHES(RDF_SW_READ)
        return s;
    }();
    return once;
}

}  // namespace rdf
