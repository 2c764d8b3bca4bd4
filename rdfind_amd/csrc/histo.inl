// Dataset statistics on the resident triples (included by kernels.inl): rdf_condition_histogram, rdf_join_histogram,
// rdf_count_literals.  Integer keys, the radix sort of primitives.hip, and run lengths of the sorted keys; no per-key
// global atomics (the house rule of counts.inl) and nothing sized by |V|.
//
// Run lengths without atomics: k_histo_heads flags the first key of every run, an exclusive scan numbers the runs,
// k_histo_starts writes each run's first index to start[run] and the key count to start[number of runs], so a run's
// length is start[r + 1] - start[r] whatever blocks or waves the run spans.
//
// rdf_condition_histogram (CountConditions.scala:192-212), once per arity:
//   k_histo_unary_keys / k_histo_binary_keys   3 n condition keys; sorted on the bits they use
//   k_histo_level2                             one key kind << 32 | count per distinct condition; sorted again
//   k_histo_rows                               one (kind, count, times) row per distinct level-2 key
// then k_histo_fold_*: every row once more under kind 0, the rows sorted by (kind, count), the kind-0 rows of one count
// (at most six, one per kind) summed.
//
// rdf_join_histogram (RDFind.scala:449-452): k_histo_join_emit writes the join partners of CreateJoinPartners
// (histo_join_partners) as join << condbits | condition, the sort is join-major, and the number of distinct conditions
// of a join value is the number of record runs inside its join run (k_histo_join_starts, k_histo_sizes); the sizes go
// through the level-2 sort and k_histo_rows.

// binary condition key on 2 + 2 jb bits (bin_key with the value fields narrowed to the ids' bits): bt as in bin_key,
// 0 = (p, o), 1 = (s, o), 2 = (s, p)
__host__ __device__ inline u64 histo_bin_key(u64 bt, u64 v1, u64 v2, int jb) { return (bt << (2 * jb)) | (v1 << jb) | v2; }

// keys[pos n + i] = pos V + value: the unary conditions of triple i (pos 0 s, 1 p, 2 o)
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_unary_keys(const u32* __restrict__ s, const u32* __restrict__ p,
                                                                const u32* __restrict__ o, u64 n, u32 V, u64* keys) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * RDF_BLOCK) {
        keys[i] = s[i];
        keys[n + i] = (u64)V + p[i];
        keys[2 * n + i] = 2ull * V + o[i];
    }
}

// keys[bt n + i]: the binary conditions (p, o), (s, o), (s, p) of triple i
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_binary_keys(const u32* __restrict__ s, const u32* __restrict__ p,
                                                                 const u32* __restrict__ o, u64 n, int jb, u64* keys) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * RDF_BLOCK) {
        const u32 ts = s[i], tp = p[i], to = o[i];
        keys[i] = histo_bin_key(0, tp, to, jb);
        keys[n + i] = histo_bin_key(1, ts, to, jb);
        keys[2 * n + i] = histo_bin_key(2, ts, tp, jb);
    }
}

// flags[i] = 1 where sorted key i starts a run of equal keys >> shift
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_heads(const u64* __restrict__ keys, u64 m, int shift, u32* flags) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < m; i += (u64)gridDim.x * RDF_BLOCK)
        flags[i] = i == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift) ? 1u : 0u;
}

// start[run] = first index of the run, start[number of runs] = m; pos = the exclusive scan of flags, pos[m] its total
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_starts(const u32* __restrict__ flags, const u32* __restrict__ pos, u64 m,
                                                            u32* start) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i <= m; i += (u64)gridDim.x * RDF_BLOCK)
        if (i == m || flags[i]) start[pos[i]] = (u32)i;
}

// one level-2 key per distinct condition: kind << 32 | triples it occurs in.  UNARY: keys pos V + value, kind 1 << pos;
// else histo_bin_key keys, kind 6 (p, o), 5 (s, o), 3 (s, p)  (the ConditionCodes values)
template <bool UNARY>
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_level2(const u64* __restrict__ keys, const u32* __restrict__ start, u64 R,
                                                            u32 V, int jb, u64* out) {
    for (u64 r = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; r < R; r += (u64)gridDim.x * RDF_BLOCK) {
        const u32 b = start[r];
        const u64 key = keys[b], len = start[r + 1] - b;
        u64 kind;
        if (UNARY) {
            kind = key >= 2ull * V ? 4 : key >= V ? 2 : 1;
        } else {
            const u64 bt = key >> (2 * jb);
            kind = bt == 0 ? 6 : bt == 1 ? 5 : 3;
        }
        out[r] = (kind << 32) | len;
    }
}

// one row per run of the sorted level-2 keys: (key >> 32, key & 0xffffffff, run length)
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_rows(const u64* __restrict__ keys, const u32* __restrict__ start, u64 R,
                                                          rdf_hist_row* out) {
    for (u64 r = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; r < R; r += (u64)gridDim.x * RDF_BLOCK) {
        const u32 b = start[r];
        const u64 key = keys[b];
        rdf_hist_row row;
        row.kind = (u32)(key >> 32);
        row.value = (u32)key;
        row.times = start[r + 1] - b;
        out[r] = row;
    }
}

// kind 0 folded in: row r under its own kind and under kind 0, as kind << 61 | count << 29 | r (r < 2^29)
static constexpr int HISTO_FOLD_IDX_BITS = 29;
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_fold_keys(const rdf_hist_row* __restrict__ rows, u64 R, u64* out) {
    for (u64 r = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; r < R; r += (u64)gridDim.x * RDF_BLOCK) {
        const u64 cnt = (u64)rows[r].value << HISTO_FOLD_IDX_BITS;
        out[2 * r] = ((u64)rows[r].kind << 61) | cnt | r;
        out[2 * r + 1] = cnt | r;
    }
}

// sorted fold keys: every key of a kind >= 1 is a row, the kind-0 keys of one count are one row
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_fold_flags(const u64* __restrict__ keys, u64 M, u32* flags) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < M; i += (u64)gridDim.x * RDF_BLOCK) {
        const u64 k = keys[i];
        flags[i] = (k >> 61) != 0 || i == 0 || (k >> HISTO_FOLD_IDX_BITS) != (keys[i - 1] >> HISTO_FOLD_IDX_BITS) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(RDF_BLOCK) void k_histo_fold_rows(const u64* __restrict__ keys, u64 M,
                                                               const u32* __restrict__ flags, const u32* __restrict__ pos,
                                                               const rdf_hist_row* __restrict__ rows, rdf_hist_row* out) {
    const u64 imask = (1ull << HISTO_FOLD_IDX_BITS) - 1;
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < M; i += (u64)gridDim.x * RDF_BLOCK) {
        if (!flags[i]) continue;
        const u64 k = keys[i];
        if (k >> 61) {
            out[pos[i]] = rows[k & imask];
            continue;
        }
        rdf_hist_row row;  // kind 0: the sum over the kinds that have this count (a run of at most six keys)
        row.kind = 0;
        row.value = (u32)(k >> HISTO_FOLD_IDX_BITS);
        row.times = 0;
        for (u64 j = i; j < M && (keys[j] >> HISTO_FOLD_IDX_BITS) == (k >> HISTO_FOLD_IDX_BITS); ++j)
            row.times += rows[keys[j] & imask].times;
        out[pos[i]] = row;
    }
}

// ---- join lines ----

// first index of `key` in the sorted keys[0, nb) (the key is present)
__device__ inline u64 histo_lower_bound(const u64* __restrict__ keys, u64 nb, u64 key) {
    u64 lo = 0, hi = nb;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// id of the binary condition (bt, v1, v2) when its capture is emitted, else EMPTY64.  FIS: its index among the frequent
// binary conditions (after rdf_association_rules the table holds only those that no rule implies: mightBeFrequent &&
// !isAssociationRuleImplied, CreateJoinPartners.scala:100); otherwise every binary is emitted and the id is the key's
// first index in ubin, the sorted histo_bin_keys of all triples
template <bool FIS>
__device__ inline u64 histo_binary_id(u64 bt, u32 v1, u32 v2, const u64* __restrict__ lkeys, const u32* __restrict__ lvals,
                                      u64 lmask, const u64* __restrict__ ubin, u64 nb, int jb) {
    if (FIS) {
        const u32 b = bin_lookup(lkeys, lvals, lmask, bin_key(bt, v1, v2));
        return b == NONE32 ? EMPTY64 : (u64)b;
    }
    return histo_lower_bound(ubin, nb, histo_bin_key(bt, v1, v2, jb));
}

// CreateJoinPartners.flatMap (ALG/operators/CreateJoinPartners.scala:86-147) for one triple: per projection the binary
// capture when it is emitted, else the conditional unary, plus the always-emitted unary; at most two records per
// projection.  Record = join << (cb + 1) | condition; condition = t V + value for the unary capture type t (0 s[p],
// 1 s[o], 2 p[s], 3 p[o], 4 o[s], 5 o[p]) or 1 << cb | binary id.  Returns the record count.
template <bool FIS>
__device__ inline u32 histo_join_partners(u32 ts, u32 tp, u32 to, u32 V, const u32* __restrict__ frank,
                                          const u64* __restrict__ lkeys, const u32* __restrict__ lvals, u64 lmask,
                                          const u64* __restrict__ ubin, u64 nb, int jb, int proj, int cb, u64 (&rec)[6]) {
    u32 c = 0;
    bool fs = true, fp = true, fo = true;  // without the frequent conditions every value passes (:78)
    if (FIS) {
        fs = frank[ts] != NONE32;
        fp = frank[(u64)V + tp] != NONE32;
        fo = frank[2ull * V + to] != NONE32;
    }
    const int sh = cb + 1;
#define HISTO_UNARY(join, t, v) rec[c++] = ((u64)(join) << sh) | ((u64)(t) * V + (v))
#define HISTO_BINARY(join, b) rec[c++] = ((u64)(join) << sh) | (1ull << cb) | (b)
    if (proj & 4) {  // join on the object: o[s,p], else o[p]; o[s]
        if (fs) {
            const u64 b = fp ? histo_binary_id<FIS>(2, ts, tp, lkeys, lvals, lmask, ubin, nb, jb) : EMPTY64;
            if (b != EMPTY64) HISTO_BINARY(to, b);
            else if (fp) HISTO_UNARY(to, 5, tp);
            HISTO_UNARY(to, 4, ts);
        } else if (fp) {
            HISTO_UNARY(to, 5, tp);
        }
    }
    if (proj & 2) {  // join on the predicate: p[s,o], else p[o]; p[s]
        if (fs) {
            const u64 b = fo ? histo_binary_id<FIS>(1, ts, to, lkeys, lvals, lmask, ubin, nb, jb) : EMPTY64;
            if (b != EMPTY64) HISTO_BINARY(tp, b);
            else if (fo) HISTO_UNARY(tp, 3, to);
            HISTO_UNARY(tp, 2, ts);
        } else if (fo) {
            HISTO_UNARY(tp, 3, to);
        }
    }
    if (proj & 1) {  // join on the subject: s[p,o], else s[o]; s[p]
        if (fp) {
            const u64 b = fo ? histo_binary_id<FIS>(0, tp, to, lkeys, lvals, lmask, ubin, nb, jb) : EMPTY64;
            if (b != EMPTY64) HISTO_BINARY(ts, b);
            else if (fo) HISTO_UNARY(ts, 1, to);
            HISTO_UNARY(ts, 0, tp);
        } else if (fo) {
            HISTO_UNARY(ts, 1, to);
        }
    }
#undef HISTO_UNARY
#undef HISTO_BINARY
    return c;
}

// WRITE = false: cnt[i] = the records of triple i; true: they go to out[off[i], ...) (off: the scan of cnt; cap: slots)
template <bool FIS, bool WRITE>
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_join_emit(const u32* __restrict__ s, const u32* __restrict__ p,
                                                               const u32* __restrict__ o, u64 n, u32 V,
                                                               const u32* __restrict__ frank, const u64* __restrict__ lkeys,
                                                               const u32* __restrict__ lvals, u64 lmask,
                                                               const u64* __restrict__ ubin, u64 nb, int jb, int proj, int cb,
                                                               u32* cnt, const u32* __restrict__ off, u64* out, u64 cap) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * RDF_BLOCK) {
        u64 rec[6];
        const u32 c = histo_join_partners<FIS>(s[i], p[i], o[i], V, frank, lkeys, lvals, lmask, ubin, nb, jb, proj, cb, rec);
        if (!WRITE) {
            cnt[i] = c;
            continue;
        }
        const u64 q = off[i];
#pragma unroll
        for (u32 k = 0; k < 6; ++k)
            if (k < c && q + k < cap) out[q + k] = rec[k];
    }
}

// sorted records: flags = the join heads, pos1 = scan of the record heads, pos2 = scan of the join heads (both with
// their totals at [m]).  jstart[g] = distinct records before join line g, jstart[number of lines] = all of them
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_join_starts(const u32* __restrict__ flags, const u32* __restrict__ pos1,
                                                                 const u32* __restrict__ pos2, u64 m, u32* jstart) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i <= m; i += (u64)gridDim.x * RDF_BLOCK)
        if (i == m || flags[i]) jstart[pos2[i]] = pos1[i];
}

// out[g] = distinct conditions of join line g (a level-2 key of kind 0)
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_sizes(const u32* __restrict__ jstart, u64 G, u64* out) {
    for (u64 g = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; g < G; g += (u64)gridDim.x * RDF_BLOCK)
        out[g] = jstart[g + 1] - jstart[g];
}

// ---- literals ----

// *count += the terms whose first byte is '"' (CountDistinctValues.scala:112-119); one atomic per wave
__global__ __launch_bounds__(RDF_BLOCK) void k_histo_literals(const unsigned char* __restrict__ base,
                                                              const u64* __restrict__ toff, const u32* __restrict__ tlen, u64 V,
                                                              u64* count) {
    u32 mine = 0;
    for (u64 t = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; t < V; t += (u64)gridDim.x * RDF_BLOCK)
        mine += tlen[t] && base[toff[t]] == '"' ? 1u : 0u;
    const u32 total = wave_sum(mine);
    if (lane_id() == 0 && total) atomicAdd(count, (u64)total);
}
