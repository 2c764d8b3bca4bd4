// Result selection (included by kernels.inl): rdf_select_cinds and rdf_find_terms.  The CINDs whose dependent, ref
// and support match a query, taken from the result as it lies in HBM into a view of the same form (refs in runs of one
// dependent, compact ids).  A pending mask class of M members sharing a list of L refs costs O(M + L + its selected
// rows), never M x L.
//
// flags:            k_sel_flags, one pass over the C compact captures: depsel[c] (a dep pattern matches and the
//                   support lies in the bounds) and refsel[c]; the patterns staged in LDS, the code by k_cs_codes' rule
// explicit part:    k_sel_run_len (refs of the runs whose dependent is selected, 0 for the others) -> scan: the
//                   candidate refs, numbered through the selected runs only, in tiles of SEL_TILE.  k_sel_count reads
//                   each candidate once (per-run counts: one result-free atomic per run and wave; per-tile counts:
//                   plain stores) -> scans -> k_sel_write reads them again and writes the kept ones at tile base +
//                   ballot rank, k_sel_runs the kept runs' table entries.  A candidate finds its run by a search in the
//                   tile's run range, so one-ref runs and 10^5-ref runs cost the same per ref.
// pending classes:  k_sel_class_count (per class: selected members; if any, selected list entries) -> scan ->
//                   k_sel_class_compact (the selected list, order kept, so it stays sorted) -> k_sel_member_rows (per
//                   member: rows = |selected list| - its own selected self entry, and that entry's rank) -> scan ->
//                   k_sel_class_emit (one thread per output row: the selected list minus self) and k_sel_runs.
//                   A class without a selected member or list entry is skipped by a uniform branch.
// rdf_find_terms:   k_find_terms, one pass over the dictionary's V terms, the queries in LDS, atomicMin on a hit

static constexpr u32 SEL_TILE = 2048;               // candidate refs per tile (8 per thread)
static constexpr u32 SEL_FT_BYTES = 32u << 10;      // query bytes k_find_terms stages in LDS (longer sets: global)
static constexpr u32 SEL_FT_MAX = 2 * RDF_SEL_MAX_PATTERNS;

__device__ inline bool sel_match(const rdf_capture_pattern& p, u32 ci, u32 v1, u32 v2) {
    // (a unary capture has v2 = NONE32 = RDF_SEL_ANY, which no pattern value equals)
    return ((p.codes >> ci) & 1u) && (p.value1 == RDF_SEL_ANY || p.value1 == v1) && (p.value2 == RDF_SEL_ANY || p.value2 == v2);
}

// pats: the n_dep dep patterns, then the n_ref ref patterns
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_flags(const u32* __restrict__ fext, u32 C, u32 V, const u64* __restrict__ bkeys,
                                                         const u32* __restrict__ csup,
                                                         const rdf_capture_pattern* __restrict__ pats, u32 n_dep, u32 n_ref,
                                                         u32 lo, u32 hi, unsigned char* depsel, unsigned char* refsel) {
    __shared__ rdf_capture_pattern s_pat[2 * RDF_SEL_MAX_PATTERNS];
    for (u32 t = threadIdx.x; t < n_dep + n_ref; t += RDF_BLOCK) s_pat[t] = pats[t];
    __syncthreads();
    const u64 six = 6ull * V;
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < C; i += (u64)gridDim.x * RDF_BLOCK) {
        const u32 ext = fext[i];
        u32 ci, v1, v2;
        if (ext < six) {
            const u32 t = ext / V;
            ci = cs_unary_index(t);
            v1 = ext - t * V;
            v2 = NONE32;
        } else {
            const u64 k = bkeys[ext - six];
            ci = cs_binary_index((u32)bin_key_type(k));
            v1 = bin_key_v1(k);
            v2 = bin_key_v2(k);
        }
        bool d = n_dep == 0, r = n_ref == 0;
        for (u32 k = 0; k < n_dep && !d; ++k) d = sel_match(s_pat[k], ci, v1, v2);  // (LDS broadcast reads)
        for (u32 k = 0; k < n_ref && !r; ++k) r = sel_match(s_pat[n_dep + k], ci, v1, v2);
        const u32 sup = csup[i];
        depsel[i] = (unsigned char)(d && sup >= lo && sup <= hi);
        refsel[i] = (unsigned char)r;
    }
}

// w[r] = refs of run r if its dependent is selected, else 0 (the run's refs are then never read)
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_run_len(const u64* __restrict__ runoff, const u32* __restrict__ rundep, u64 R,
                                                           const unsigned char* __restrict__ depsel, u32* w) {
    for (u64 r = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; r < R; r += (u64)gridDim.x * RDF_BLOCK)
        w[r] = depsel[rundep[r]] ? (u32)(runoff[r + 1] - runoff[r]) : 0u;
}

// Candidate j of the tile's run range [lo, hi] (woff: the scanned k_sel_run_len weights; runs of weight 0 share their
// successor's offset and are never found): its run and whether its ref is selected.
__device__ inline bool sel_candidate(const u32* __restrict__ refs, const u64* __restrict__ runoff, const u64* __restrict__ woff,
                                     u64 lo, u64 hi, u64 j, const unsigned char* __restrict__ refsel, u64* run, u32* ref) {
    const u64 r = run_of(woff, lo, hi, j);
    const u32 v = refs[runoff[r] + (j - woff[r])];
    *run = r;
    *ref = v;
    return refsel[v] != 0;
}

// the run range of tile t into s_lo / s_hi (thread 0; the caller synchronises)
__device__ inline void sel_tile_range(const u64* __restrict__ woff, u64 R, u64 S, u64 t, u64* s_lo, u64* s_hi) {
    const u64 j0 = t * SEL_TILE, j1 = (j0 + SEL_TILE < S ? j0 + SEL_TILE : S) - 1;
    *s_lo = run_of(woff, 0, R - 1, j0);
    *s_hi = run_of(woff, *s_lo, R - 1, j1);
}

// count pass over the S candidates: rcnt[r] += kept refs of run r, tcnt[t] = kept refs of tile t.  The lanes of a wave
// hold consecutive candidates, so a run's lanes are consecutive: its first lane in the wave adds the run's kept lanes.
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_count(const u32* __restrict__ refs, const u64* __restrict__ runoff,
                                                         const u64* __restrict__ woff, u64 R, u64 S,
                                                         const unsigned char* __restrict__ refsel, u32* rcnt, u32* tcnt) {
    __shared__ u64 s_lo, s_hi;
    __shared__ u32 s_cnt;
    const int lane = lane_id();
    const u64 T = (S + SEL_TILE - 1) / SEL_TILE;
    for (u64 t = blockIdx.x; t < T; t += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) {
            sel_tile_range(woff, R, S, t, &s_lo, &s_hi);
            s_cnt = 0;
        }
        __syncthreads();
        u32 mine = 0;
        for (u32 k = 0; k < SEL_TILE / RDF_BLOCK; ++k) {
            const u64 j = t * SEL_TILE + (u64)k * RDF_BLOCK + threadIdx.x;
            const bool on = j < S;
            u64 r = 0;
            u32 v = 0;
            const bool keep = on && sel_candidate(refs, runoff, woff, s_lo, s_hi, j, refsel, &r, &v);
            const u64 kb = __ballot(keep);
            const u64 rp = __shfl_up(r, 1, RDF_WAVE);
            const u64 heads = __ballot(on && (lane == 0 || r != rp));
            if (on && ((heads >> lane) & 1ull)) {
                const u64 above = lane == RDF_WAVE - 1 ? 0ull : heads & (~0ull << (lane + 1));
                const u64 below_next = above ? (1ull << (__ffsll((long long)above) - 1)) - 1ull : ~0ull;
                const u32 n = (u32)__popcll(kb & below_next & ~((1ull << lane) - 1ull));
                if (n) (void)atomicAdd(&rcnt[r], n);
            }
            mine += keep ? 1u : 0u;
        }
        mine = wave_sum(mine);
        if (lane == 0 && mine) (void)atomicAdd(&s_cnt, mine);
        __syncthreads();
        if (threadIdx.x == 0) tcnt[t] = s_cnt;
    }
}

// rank of this thread's kept element among the block's (s_w: RDF_WAVES_PER_BLOCK words); *total = the block's kept
// elements.  Two barriers: s_w is reusable on return.
__device__ inline u32 sel_block_rank(bool keep, u32* s_w, u32* total) {
    const u64 b = __ballot(keep);
    const u32 wave = threadIdx.x / RDF_WAVE;
    if (lane_id() == 0) s_w[wave] = (u32)__popcll(b);
    __syncthreads();
    u32 before = 0, tot = 0;
#pragma unroll
    for (u32 w = 0; w < RDF_WAVES_PER_BLOCK; ++w) {
        const u32 x = s_w[w];
        before += w < wave ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return before + (u32)__popcll(b & lanemask_lt());
}

// write pass: the kept candidates in candidate order (= view order) at out[toff[t] + rank in the tile]
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_write(const u32* __restrict__ refs, const u64* __restrict__ runoff,
                                                         const u64* __restrict__ woff, u64 R, u64 S,
                                                         const unsigned char* __restrict__ refsel,
                                                         const u64* __restrict__ toff, u32* out) {
    __shared__ u64 s_lo, s_hi;
    __shared__ u32 s_w[RDF_WAVES_PER_BLOCK];
    const u64 T = (S + SEL_TILE - 1) / SEL_TILE;
    for (u64 t = blockIdx.x; t < T; t += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) sel_tile_range(woff, R, S, t, &s_lo, &s_hi);
        __syncthreads();
        u64 base = toff[t];
        if (toff[t + 1] == base) continue;  // (uniform: nothing kept in this tile)
        for (u32 k = 0; k < SEL_TILE / RDF_BLOCK; ++k) {
            const u64 j = t * SEL_TILE + (u64)k * RDF_BLOCK + threadIdx.x;
            u64 r = 0;
            u32 v = 0, tot = 0;
            const bool keep = j < S && sel_candidate(refs, runoff, woff, s_lo, s_hi, j, refsel, &r, &v);
            const u32 rank = sel_block_rank(keep, s_w, &tot);
            if (keep) out[base + rank] = v;
            base += tot;
        }
    }
}

__global__ __launch_bounds__(RDF_BLOCK) void k_sel_nonzero(const u32* __restrict__ cnt, u64 n, u32* flag) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * RDF_BLOCK) flag[i] = cnt[i] ? 1u : 0u;
}

// table entries of the kept runs: run r (cnt[r] > 0 rows from row off[r] of its part) is view run run0 + kpos[r]; its
// dependent comes from dep32[r] or the low word of dep64[r] (class members).  The last thread closes the table.
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_runs(const u32* __restrict__ cnt, const u64* __restrict__ off,
                                                        const u64* __restrict__ kpos, const u32* __restrict__ dep32,
                                                        const u64* __restrict__ dep64, u64 n, u64 row0, u64 run0,
                                                        u64* sel_runoff, u32* sel_rundep) {
    for (u64 r = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; r < n; r += (u64)gridDim.x * RDF_BLOCK) {
        if (!cnt[r]) continue;
        const u64 k = run0 + kpos[r];
        sel_runoff[k] = row0 + off[r];
        sel_rundep[k] = dep32 ? dep32[r] : (u32)dep64[r];
    }
}

// sum of v over the block (s_w: RDF_WAVES_PER_BLOCK words, reusable on return)
__device__ inline u32 sel_block_sum(u32 v, u32* s_w) {
    v = wave_sum(v);
    if (lane_id() == 0) s_w[threadIdx.x / RDF_WAVE] = v;
    __syncthreads();
    u32 tot = 0;
#pragma unroll
    for (u32 w = 0; w < RDF_WAVES_PER_BLOCK; ++w) tot += s_w[w];
    __syncthreads();
    return tot;
}

// per class m (one block each; layout as k_cs_class): lcnt[m] = selected list entries if a member is selected, else 0
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_class_count(u32 ncls, const u64* __restrict__ coff, const u64* __restrict__ cchoff,
                                                               const u64* __restrict__ lwoff, const u32* __restrict__ lists,
                                                               const u64* __restrict__ ckeys,
                                                               const unsigned char* __restrict__ depsel,
                                                               const unsigned char* __restrict__ refsel, u32* lcnt) {
    __shared__ u32 s_w[RDF_WAVES_PER_BLOCK];
    for (u64 m = blockIdx.x; m < ncls; m += gridDim.x) {
        const u64 k0 = coff[m], k1 = coff[m + 1];
        u32 nm = 0;
        for (u64 i = k0 + threadIdx.x; i < k1; i += RDF_BLOCK) nm += depsel[(u32)ckeys[i]];
        nm = sel_block_sum(nm, s_w);
        u32 nl = 0;
        if (nm) {  // (uniform over the block)
            const u64 lb = lwoff[cchoff[m]], le = lwoff[cchoff[m + 1]];
            for (u64 i = lb + threadIdx.x; i < le; i += RDF_BLOCK) nl += refsel[lists[i]];
            nl = sel_block_sum(nl, s_w);
        }
        if (threadIdx.x == 0) lcnt[m] = nl;
    }
}

// the selected entries of class m's list, order kept, at slist[sloff[m], sloff[m + 1])
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_class_compact(u32 ncls, const u64* __restrict__ cchoff,
                                                                 const u64* __restrict__ lwoff, const u32* __restrict__ lists,
                                                                 const unsigned char* __restrict__ refsel,
                                                                 const u64* __restrict__ sloff, u32* slist) {
    __shared__ u32 s_w[RDF_WAVES_PER_BLOCK];
    for (u64 m = blockIdx.x; m < ncls; m += gridDim.x) {
        u64 base = sloff[m];
        if (sloff[m + 1] == base) continue;  // (uniform)
        const u64 lb = lwoff[cchoff[m]], le = lwoff[cchoff[m + 1]];
        for (u64 b = lb; b < le; b += RDF_BLOCK) {
            const u64 i = b + threadIdx.x;
            const u32 v = i < le ? lists[i] : 0u;
            const bool keep = i < le && refsel[v];
            u32 tot = 0;
            const u32 rank = sel_block_rank(keep, s_w, &tot);
            if (keep) slist[base + rank] = v;
            base += tot;
        }
    }
}

// per member i: mc[i] = its selected rows (the selected list minus its own selected self entry), mrank[i] = that
// entry's position in the selected list (NONE32: none), found by a search: the selected list is sorted as the list is
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_member_rows(const u64* __restrict__ ckeys, u64 nmem,
                                                               const u32* __restrict__ selfpos,
                                                               const unsigned char* __restrict__ depsel,
                                                               const unsigned char* __restrict__ refsel,
                                                               const u64* __restrict__ sloff, const u32* __restrict__ slist,
                                                               u32* mc, u32* mrank) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < nmem; i += (u64)gridDim.x * RDF_BLOCK) {
        const u32 m = (u32)(ckeys[i] >> 32), d = (u32)ckeys[i];
        const u64 b = sloff[m], e = sloff[m + 1];
        u32 cnt = 0, rank = NONE32;
        if (e > b && depsel[d]) {
            cnt = (u32)(e - b);
            if (selfpos[i] != NONE32 && refsel[d]) {
                u64 lo = b, hi = e;
                while (lo < hi) {
                    const u64 mid = (lo + hi) >> 1;
                    if (slist[mid] < d) lo = mid + 1;
                    else hi = mid;
                }
                rank = (u32)(lo - b);
                --cnt;
            }
        }
        mc[i] = cnt;
        mrank[i] = rank;
    }
}

// the class rows [0, Sc), one thread each: row j belongs to member i = the last one with moff[i] <= j (members without
// rows share their successor's offset), and is entry j - moff[i] of its class's selected list with the self entry
// skipped.  Consecutive threads read and write consecutive words within a member.
__global__ __launch_bounds__(RDF_BLOCK) void k_sel_class_emit(const u64* __restrict__ ckeys, u64 nmem, const u64* __restrict__ moff,
                                                              u64 Sc, const u32* __restrict__ mrank,
                                                              const u64* __restrict__ sloff, const u32* __restrict__ slist,
                                                              u32* out) {
    __shared__ u64 s_lo, s_hi;
    for (u64 b = (u64)blockIdx.x * RDF_BLOCK; b < Sc; b += (u64)gridDim.x * RDF_BLOCK) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const u64 last = b + RDF_BLOCK - 1 < Sc ? b + RDF_BLOCK - 1 : Sc - 1;
            s_lo = run_of(moff, 0, nmem - 1, b);
            s_hi = run_of(moff, s_lo, nmem - 1, last);
        }
        __syncthreads();
        const u64 j = b + threadIdx.x;
        if (j < Sc) {
            const u64 i = run_of(moff, s_lo, s_hi, j);
            const u64 k = j - moff[i];
            const u32 sr = mrank[i];
            out[j] = slist[sloff[(u32)(ckeys[i] >> 32)] + k + (sr != NONE32 && k >= sr ? 1u : 0u)];
        }
    }
}

// ids[q] = the smallest id of a dictionary term equal to query q (ids preset to NONE32): one thread per term, the
// query offsets and (when they fit) bytes staged in LDS; lengths first, then bytes
__global__ __launch_bounds__(RDF_BLOCK) void k_find_terms(const char* __restrict__ dheap, const u64* __restrict__ dtoff, u64 V,
                                                          const char* __restrict__ qheap, const u64* __restrict__ qoff, u32 nq,
                                                          u32* ids) {
    __shared__ u64 s_off[SEL_FT_MAX + 1];
    __shared__ char s_q[SEL_FT_BYTES];
    for (u32 t = threadIdx.x; t <= nq; t += RDF_BLOCK) s_off[t] = qoff[t];
    __syncthreads();
    const u64 q0 = s_off[0], qbytes = s_off[nq] - q0;
    const bool staged = qbytes <= SEL_FT_BYTES;
    if (staged)
        for (u64 t = threadIdx.x; t < qbytes; t += RDF_BLOCK) s_q[t] = qheap[q0 + t];
    __syncthreads();
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < V; i += (u64)gridDim.x * RDF_BLOCK) {
        const u64 tb = dtoff[i], tl = dtoff[i + 1] - tb;
        for (u32 q = 0; q < nq; ++q) {
            const u64 qb = s_off[q];
            if (s_off[q + 1] - qb != tl) continue;
            const char* a = staged ? s_q + (qb - q0) : qheap + qb;
            u64 k = 0;
            while (k < tl && a[k] == dheap[tb + k]) ++k;
            if (k == tl) (void)atomicMin(&ids[q], (u32)i);
        }
    }
}
