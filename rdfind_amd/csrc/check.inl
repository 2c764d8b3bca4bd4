// CIND check (included by kernels.inl): rdf_check_cinds.  Which of M given (dep capture, ref capture) pairs hold in the
// resident triples, with supports, overlaps and the smallest violating values.  Plain set semantics: I(c) = the distinct
// values of c's projection attribute over the triples matching c's condition; no frequent conditions, no groups.
//
// captures:   k_chk_keys (2M capture keys ci << 60 | v1 << 30 | v2, validated; a side with an absent value: EMPTY64) ->
//             radix sort -> k_chk_cap_heads -> scan -> k_chk_cap_compact: the Q distinct captures; k_chk_sides: each
//             side's capture index by binary search
// table:      k_chk_table, open addressing keyed by condition (mask << 60 | v1 << 30 | v2), <= 1/4 full; a 16-B slot
//             holds the key and one capture index per projection of the condition (two for a unary one, one for a binary)
// match:      k_chk_match, one pass over s / p / o, four triples per lane (16-B loads when the arrays allow); each triple
//             probes its six conditions in the table (staged in LDS when it fits, else in global memory).  Count form:
//             matching triples per capture (in LDS beside the staged table, one global add per slot and block; else
//             one global add per distinct capture of a wave, chk_count_add).  Write form: capture << joinbits | value records at a block-aggregated cursor (one global
//             atomic per block and 256 triples)
// unique:     radix sort on capbits + joinbits bits -> k_histo_heads -> scan -> k_chk_values (the distinct values,
//             ascending per capture) and k_chk_qoff (per capture the offset of its values: supports are differences)
// intersect:  work item = (candidate, chunk of CHK_CHUNK dependent values), numbered by a scan.  k_chk_intersect narrows
//             the ref list to the chunk's value range with two searches, stages that range in LDS when it fits, counts
//             the hits by ballot and stores one violation count per item.  A scan over the items gives each its
//             candidate's violations before it; the example form runs again only for the items whose rank is below
//             n_examples and writes their violations at rank + position, so the examples are the smallest values.
// k_chk_rows / k_chk_classes: the rows and the three class counts.

static constexpr u32 CHK_LDS_SLOTS = 2048;  // slots of the LDS table: 32 KiB (+ 16 KiB of counters in the count form)
static constexpr u32 CHK_CHUNK = 1024;      // dependent values per work item (4 per thread)
static constexpr u32 CHK_REF_LDS = 4096;    // ref values a work item stages in LDS (16 KiB)
static constexpr u32 CHK_TRIPLES = 4;       // triples per lane and pass of k_chk_match
static constexpr int CHK_VBITS = 30;        // bits of a term id in a capture / condition key
static constexpr u64 CHK_VMASK = (1ull << CHK_VBITS) - 1;

// index of a capture code among 10 12 14 17 20 21 33 34 35 (ascending), or -1
__host__ __device__ inline int chk_code_index(u32 code) {
    switch (code) {
        case 10: return 0;
        case 12: return 1;
        case 14: return 2;
        case 17: return 3;
        case 20: return 4;
        case 21: return 5;
        case 33: return 6;
        case 34: return 7;
        case 35: return 8;
    }
    return -1;
}
// condition mask (s 1, p 2, o 4) and projection attribute of code index ci: code = projection << 3 | mask
__host__ __device__ inline u32 chk_index_code(u32 ci) {
    const u32 pr = ci / 3, k = ci % 3;  // per projection: the two unary conditions ascending, then the binary one
    const u32 proj = 1u << pr, rest = 7u & ~proj, lo = rest & (0u - rest), hi = rest & ~lo;
    return (proj << 3) | (k == 0 ? lo : k == 1 ? hi : rest);
}
// slot of projection `proj` in the condition `mask`'s table entry: the attributes outside the mask, ascending
__host__ __device__ inline u32 chk_proj_slot(u32 mask, u32 proj) {
    const u32 rest = 7u & ~mask;
    return (rest & (0u - rest)) == proj ? 0u : 1u;
}

// capture key of one side; *reason: 0 fine, 1 code, 2 unary with value2, 3 binary without, 4 id out of range
__device__ inline u64 chk_side_key(const rdf_capture_key& k, u32 V, u32* reason) {
    const int ci = chk_code_index(k.code);
    *reason = 0;
    if (ci < 0) {
        *reason = 1;
        return EMPTY64;
    }
    const bool binary = ci % 3 == 2;
    if (!binary && k.value2 != NONE32) *reason = 2;
    else if (binary && k.value2 == NONE32) *reason = 3;
    else if ((k.value1 != RDF_CHK_ABSENT && k.value1 >= V) || (binary && k.value2 != RDF_CHK_ABSENT && k.value2 >= V)) *reason = 4;
    if (*reason) return EMPTY64;
    if (k.value1 == RDF_CHK_ABSENT || (binary && k.value2 == RDF_CHK_ABSENT)) return EMPTY64;
    return ((u64)ci << 60) | ((u64)k.value1 << CHK_VBITS) | (binary ? (u64)k.value2 : 0ull);
}

// keys[2 i], keys[2 i + 1] = the capture keys of candidate i; *err = min over the invalid candidates of i << 3 | reason
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_keys(const rdf_cind_candidate* __restrict__ cands, u64 M, u32 V, u64* keys,
                                                        u64* err) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < M; i += (u64)gridDim.x * RDF_BLOCK) {
        const rdf_cind_candidate cd = cands[i];
        u32 r1, r2;
        keys[2 * i] = chk_side_key(cd.dep, V, &r1);
        keys[2 * i + 1] = chk_side_key(cd.ref, V, &r2);
        if (r1 | r2) (void)atomicMin(err, (i << 3) | (r1 ? r1 : r2));
    }
}

// flags[i] = 1 where sorted key i is a capture (not EMPTY64) and differs from its predecessor
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_cap_heads(const u64* __restrict__ keys, u64 m, u32* flags) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < m; i += (u64)gridDim.x * RDF_BLOCK)
        flags[i] = keys[i] != EMPTY64 && (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(RDF_BLOCK) void k_chk_cap_compact(const u64* __restrict__ keys, u64 m, const u32* __restrict__ flags,
                                                               const u32* __restrict__ pos, u64* ucap) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < m; i += (u64)gridDim.x * RDF_BLOCK)
        if (flags[i]) ucap[pos[i]] = keys[i];
}

// side[2 i], side[2 i + 1] = index of candidate i's dep / ref capture in ucap[0, Q) (NONE32: an empty side)
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_sides(const rdf_cind_candidate* __restrict__ cands, u64 M, u32 V,
                                                         const u64* __restrict__ ucap, u64 Q, u32* side) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < 2 * M; i += (u64)gridDim.x * RDF_BLOCK) {
        const rdf_cind_candidate& cd = cands[i >> 1];
        u32 r;
        const u64 key = chk_side_key((i & 1) ? cd.ref : cd.dep, V, &r);
        side[i] = key == EMPTY64 ? NONE32 : (u32)histo_lower_bound(ucap, Q, key);
    }
}

// the condition table: x = condition key (EMPTY64: free), y = capture index of projection slot 0 | slot 1 << 32
// (NONE32: no such capture).  Inserts the captures q with inb[q] (inb null: all); *nconds += the distinct conditions.
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_table(const u64* __restrict__ ucap, u64 Q, const unsigned char* __restrict__ inb,
                                                         ulonglong2* tab, u32 mask, u32* nconds) {
    for (u64 b = (u64)blockIdx.x * RDF_BLOCK; b < Q; b += (u64)gridDim.x * RDF_BLOCK) {
        const u64 q = b + threadIdx.x;
        bool fresh = false;
        if (q < Q && (!inb || inb[q])) {
            const u64 ck = ucap[q];
            const u32 code = chk_index_code((u32)(ck >> 60)), cm = code & 7u;
            const u64 key = ((u64)cm << 60) | (ck & ((1ull << 60) - 1));
            for (u32 h = (u32)mix64(key) & mask;; h = (h + 1) & mask) {
                const u64 old = atomicCAS(&tab[h].x, EMPTY64, key);
                if (old == EMPTY64 || old == key) {
                    ((u32*)&tab[h].y)[chk_proj_slot(cm, code >> 3)] = (u32)q;  // (one capture per condition and slot)
                    fresh = old == EMPTY64;
                    break;
                }
            }
        }
        const u64 fb = __ballot(fresh);
        if (fb && lane_id() == __ffsll((long long)fb) - 1) (void)atomicAdd(nconds, (u32)__popcll(fb));
    }
}

// the slot of `key` in the table (<= 1/4 full, so a free slot ends every probe), or NONE32
__device__ inline u32 chk_probe(const ulonglong2* tab, u32 mask, u64 key) {
    for (u32 h = (u32)mix64(key) & mask;; h = (h + 1) & mask) {
        const u64 k = tab[h].x;
        if (k == key) return h;
        if (k == EMPTY64) return NONE32;
    }
}

// cnt[c] += 1 for every lane with `on`.  A hot capture (s[p=rdf:type]) is most lanes' c, and their adds to one address
// would serialise in L2 (c2, a 1,000-row sample: 43 ms per-lane, 10.8 ms per wave and distinct c), so the wave's lanes
// with one c add once, into the block's CHK_PRIV LDS counters (pkey: capture or NONE32, pcnt; four probes, then the
// global counter), which the block flushes when it ends.  Called by all lanes of the wave.
static constexpr u32 CHK_PRIV = 1024;
__device__ inline void chk_count_add(u32* cnt, u32* pkey, u32* pcnt, u32 c, bool on) {
    u64 todo = __ballot(on);
    while (todo) {  // (uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const u32 lc = __shfl(c, leader, RDF_WAVE);
        const u64 same = __ballot(on && c == lc);
        if (lane_id() == leader) {
            const u32 add = (u32)__popcll(same);
            bool done = false;
            u32 h = hash32(lc) & (CHK_PRIV - 1);
            for (int t = 0; t < 4 && !done; ++t, h = (h + 1) & (CHK_PRIV - 1)) {
                const u32 old = atomicCAS(&pkey[h], NONE32, lc);
                if (old == NONE32 || old == lc) {
                    (void)atomicAdd(&pcnt[h], add);
                    done = true;
                }
            }
            if (!done) (void)atomicAdd(&cnt[lc], add);
        }
        todo &= ~same;
    }
}

// One pass over the triples.  WRITE = false: cnt[q] += the triples matching capture q.  WRITE = true: the records
// q << joinbits | value to out[0, cap) at *cursor (one atomic per block and 256 triples; *overflow when cap is too small).
// LDS: the table (tmask + 1 slots) is staged in dynamic LDS, followed in the count form by two counters per slot.
template <bool LDS, bool WRITE>
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_match(const u32* __restrict__ s, const u32* __restrict__ p,
                                                         const u32* __restrict__ o, u64 n, const ulonglong2* __restrict__ gtab,
                                                         u32 tmask, int joinbits, u32* cnt, u64* cursor, u64* out, u64 cap,
                                                         u32* overflow) {
    extern __shared__ ulonglong2 chk_dyn[];
    __shared__ u32 s_w[2][RDF_WAVES_PER_BLOCK];
    __shared__ u64 s_base[2];
    const ulonglong2* tab = gtab;
    u32* lcnt = nullptr;
    if (LDS) {
        for (u32 t = threadIdx.x; t <= tmask; t += RDF_BLOCK) chk_dyn[t] = gtab[t];
        tab = chk_dyn;
        if (!WRITE) {
            lcnt = (u32*)(chk_dyn + tmask + 1);
            for (u32 t = threadIdx.x; t < 2 * (tmask + 1); t += RDF_BLOCK) lcnt[t] = 0;
        }
        __syncthreads();
    }
    u32 *pkey = nullptr, *pcnt = nullptr;
    if (!LDS && !WRITE) {  // (dynamic LDS: the block's private counters)
        pkey = (u32*)chk_dyn;
        pcnt = pkey + CHK_PRIV;
        for (u32 t = threadIdx.x; t < CHK_PRIV; t += RDF_BLOCK) pkey[t] = NONE32, pcnt[t] = 0;
        __syncthreads();
    }
    const bool vec =((((uintptr_t)s) | ((uintptr_t)p) | ((uintptr_t)o)) & 15) == 0;
    const u32 wave = threadIdx.x / RDF_WAVE;
    u32 par = 0;
    const u64 per_block = (u64)RDF_BLOCK * CHK_TRIPLES;
    for (u64 b = (u64)blockIdx.x * per_block; b < n; b += (u64)gridDim.x * per_block) {
        const u64 i0 = b + (u64)threadIdx.x * CHK_TRIPLES;
        u32 ts[CHK_TRIPLES], tp[CHK_TRIPLES], to[CHK_TRIPLES];
        if (vec && i0 + CHK_TRIPLES <= n) {
            const uint4 a = *(const uint4*)(s + i0), c = *(const uint4*)(p + i0), d = *(const uint4*)(o + i0);
            ts[0] = a.x, ts[1] = a.y, ts[2] = a.z, ts[3] = a.w;
            tp[0] = c.x, tp[1] = c.y, tp[2] = c.z, tp[3] = c.w;
            to[0] = d.x, to[1] = d.y, to[2] = d.z, to[3] = d.w;
        } else {
#pragma unroll
            for (u32 k = 0; k < CHK_TRIPLES; ++k) {
                const bool on = i0 + k < n;
                ts[k] = on ? s[i0 + k] : 0u;
                tp[k] = on ? p[i0 + k] : 0u;
                to[k] = on ? o[i0 + k] : 0u;
            }
        }
#pragma unroll
        for (u32 k = 0; k < CHK_TRIPLES; ++k) {
            u64 rec[9];
            u32 have = 0;  // bit j: rec[j] is a record
            {
                const bool valid = i0 + k < n;
                const u64 vs = ts[k], vp = tp[k], vo = to[k];
                // the six conditions; the values of the projection slots 0 / 1 (a binary condition has slot 0 only)
                const u64 key[6] = {(1ull << 60) | (vs << CHK_VBITS), (2ull << 60) | (vp << CHK_VBITS), (4ull << 60) | (vo << CHK_VBITS),
                                    (3ull << 60) | (vs << CHK_VBITS) | vp, (5ull << 60) | (vs << CHK_VBITS) | vo,
                                    (6ull << 60) | (vp << CHK_VBITS) | vo};
                const u32 val0[6] = {tp[k], ts[k], ts[k], to[k], tp[k], ts[k]};
                const u32 val1[3] = {to[k], to[k], tp[k]};
#pragma unroll
                for (u32 j = 0; j < 6; ++j) {  // (every lane of the wave comes through: the global count form votes)
                    const u32 h = valid ? chk_probe(tab, tmask, key[j]) : NONE32;
                    const u64 caps = h != NONE32 ? tab[h].y : EMPTY64;
                    const u32 c0 = (u32)caps, c1 = (u32)(caps >> 32);
                    if (WRITE) {
                        if (c0 != NONE32) {
                            rec[j] = ((u64)c0 << joinbits) | val0[j];
                            have |= 1u << j;
                        }
                        if (j < 3 && c1 != NONE32) {
                            rec[6 + (j < 3 ? j : 0)] = ((u64)c1 << joinbits) | val1[j < 3 ? j : 0];
                            have |= 1u << (6 + j);
                        }
                    } else if (LDS) {
                        if (c0 != NONE32) (void)atomicAdd(&lcnt[2 * h], 1u);
                        if (c1 != NONE32) (void)atomicAdd(&lcnt[2 * h + 1], 1u);
                    } else {
                        chk_count_add(cnt, pkey, pcnt, c0, c0 != NONE32);
                        if (j < 3) chk_count_add(cnt, pkey, pcnt, c1, c1 != NONE32);
                    }
                }
            }
            if (WRITE) {
                // block-aggregated cursor: the block's records of this round get one range of `out`
                const u32 nr = (u32)__popc(have), incl = wave_inclusive_scan(nr);
                if (lane_id() == RDF_WAVE - 1) s_w[par][wave] = incl;
                __syncthreads();
                if (threadIdx.x == 0) {
                    u32 t = 0;
#pragma unroll
                    for (u32 w = 0; w < RDF_WAVES_PER_BLOCK; ++w) t += s_w[par][w];
                    s_base[par] = t ? atomicAdd(cursor, (u64)t) : 0ull;
                }
                __syncthreads();
                u64 at = s_base[par] + (incl - nr);
#pragma unroll
                for (u32 w = 0; w < RDF_WAVES_PER_BLOCK; ++w) at += w < wave ? s_w[par][w] : 0u;
#pragma unroll
                for (u32 j = 0; j < 9; ++j) {
                    if (!((have >> j) & 1u)) continue;
                    if (at < cap) out[at] = rec[j];
                    else *overflow = 1u;
                    ++at;
                }
                par ^= 1u;  // (the next round's writers use the other copy while this one may still be read)
            }
        }
    }
    if (!LDS && !WRITE) {
        __syncthreads();
        for (u32 t = threadIdx.x; t < CHK_PRIV; t += RDF_BLOCK)
            if (pkey[t] != NONE32 && pcnt[t]) (void)atomicAdd(&cnt[pkey[t]], pcnt[t]);
    }
    if (LDS && !WRITE) {
        __syncthreads();
        for (u32 t = threadIdx.x; t < 2 * (tmask + 1); t += RDF_BLOCK) {
            const u32 v = lcnt[t];
            if (!v) continue;
            const u64 caps = chk_dyn[t >> 1].y;
            (void)atomicAdd(&cnt[(t & 1) ? (u32)(caps >> 32) : (u32)caps], v);
        }
    }
}

// qval[pos[i]] = the value of sorted record i where it starts a run (flags, pos: heads and their scan)
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_values(const u64* __restrict__ rec, u64 R, const u32* __restrict__ flags,
                                                          const u32* __restrict__ pos, u64 jmask, u32* qval) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < R; i += (u64)gridDim.x * RDF_BLOCK)
        if (flags[i]) qval[pos[i]] = (u32)(rec[i] & jmask);
}

// qoff[q] = distinct records of the captures below q, q in [0, Q] (pos[R] = all of them): capture q's values are
// qval[qoff[q], qoff[q + 1]), ascending; a capture without records has none
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_qoff(const u64* __restrict__ rec, u64 R, const u32* __restrict__ pos, u64 Q,
                                                        int joinbits, u32* qoff) {
    for (u64 q = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; q <= Q; q += (u64)gridDim.x * RDF_BLOCK)
        qoff[q] = pos[histo_lower_bound(rec, R, q << joinbits)];
}

// inb[q] = 1 for the captures of candidates [c0, c1)
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_mark(const u32* __restrict__ side, u64 c0, u64 c1, unsigned char* inb) {
    for (u64 i = 2 * c0 + (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < 2 * c1; i += (u64)gridDim.x * RDF_BLOCK)
        if (side[i] != NONE32) inb[side[i]] = 1;
}

// w[q] = cnt[q] where inb[q] (inb null: everywhere)
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_masked(const u32* __restrict__ cnt, const unsigned char* __restrict__ inb, u64 Q,
                                                          u32* w) {
    for (u64 q = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; q < Q; q += (u64)gridDim.x * RDF_BLOCK)
        w[q] = !inb || inb[q] ? cnt[q] : 0u;
}

// w[i] = the records candidate i's two captures need on their own (an upper bound of what it adds to a batch)
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_weights(const u32* __restrict__ side, u64 M, const u32* __restrict__ cnt, u32* w) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < M; i += (u64)gridDim.x * RDF_BLOCK) {
        const u32 d = side[2 * i], r = side[2 * i + 1];
        w[i] = (d != NONE32 ? cnt[d] : 0u) + (r != NONE32 && r != d ? cnt[r] : 0u);
    }
}

__device__ inline u32 chk_len(const u32* __restrict__ qoff, u32 q) { return q == NONE32 ? 0u : qoff[q + 1] - qoff[q]; }

// nit[i - c0] = work items of candidate i in [c0, c1): chunks of CHK_CHUNK dependent values
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_items(const u32* __restrict__ side, u64 c0, u64 c1,
                                                         const u32* __restrict__ qoff, u32* nit) {
    for (u64 i = c0 + (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < c1; i += (u64)gridDim.x * RDF_BLOCK)
        nit[i - c0] = (chk_len(qoff, side[2 * i]) + CHK_CHUNK - 1) / CHK_CHUNK;
}

// first index in [lo, hi) of the ascending a[] with a[index] >= v (UPPER: > v)
template <bool UPPER, typename P>
__device__ inline u32 chk_bound(P a, u32 lo, u32 hi, u32 v) {
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (UPPER ? a[mid] <= v : a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One block per work item w of the batch's candidates [c0, c0 + Mb) (ioff: the scanned item counts, ioff[Mb] = W).
// EX = false: viol[w] = the item's dependent values that the ref lacks.  EX = true (vpre: the scan of viol): the items
// whose candidate has fewer than nex violations before them write theirs to ex[candidate * nex + rank ...).
template <bool EX>
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_intersect(const u64* __restrict__ ioff, u64 Mb, u64 W, u64 c0,
                                                             const u32* __restrict__ side, const u32* __restrict__ qoff,
                                                             const u32* __restrict__ qval, u32* viol,
                                                             const u64* __restrict__ vpre, u32 nex, u32* ex) {
    __shared__ u32 s_ref[CHK_REF_LDS];
    __shared__ u32 s_w[RDF_WAVES_PER_BLOCK];
    __shared__ u32 s_d0, s_d1, s_r0, s_r1, s_skip;
    __shared__ u64 s_cand, s_rank;
    for (u64 w = blockIdx.x; w < W; w += gridDim.x) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const u64 ci = run_of(ioff, 0, Mb - 1, w), cand = c0 + ci;
            const u32 dq = side[2 * cand], rq = side[2 * cand + 1];
            const u32 db = qoff[dq], de = qoff[dq + 1];  // (a candidate with items has a dependent with values)
            const u32 d0 = db + (u32)(w - ioff[ci]) * CHK_CHUNK, d1 = de - d0 > CHK_CHUNK ? d0 + CHK_CHUNK : de;
            u32 r0 = 0, r1 = 0;
            if (rq != NONE32) {
                r0 = chk_bound<false>(qval, qoff[rq], qoff[rq + 1], qval[d0]);
                r1 = chk_bound<true>(qval, r0, qoff[rq + 1], qval[d1 - 1]);
            }
            s_d0 = d0, s_d1 = d1, s_r0 = r0, s_r1 = r1, s_cand = cand;
            s_skip = 0;
            if (EX) {
                s_rank = vpre[w] - vpre[ioff[ci]];
                s_skip = s_rank >= nex || viol[w] == 0 ? 1u : 0u;
            }
        }
        __syncthreads();
        if (s_skip) continue;  // (uniform)
        const u32 d0 = s_d0, d1 = s_d1, r0 = s_r0, rn = s_r1 - s_r0;
        const bool staged = rn <= CHK_REF_LDS;
        if (staged) {
            for (u32 t = threadIdx.x; t < rn; t += RDF_BLOCK) s_ref[t] = qval[r0 + t];
            __syncthreads();
        }
        u32 hits = 0;  // (EX: the violations written so far, as a rank within the candidate)
        u64 rank = EX ? s_rank : 0;
        for (u32 b = d0; b < d1; b += RDF_BLOCK) {
            const u32 j = b + threadIdx.x;
            const bool on = j < d1;
            const u32 v = on ? qval[j] : 0u;
            bool found = false;
            if (on && rn) {
                if (staged) {
                    const u32 k = chk_bound<false>((const u32*)s_ref, 0u, rn, v);
                    found = k < rn && s_ref[k] == v;
                } else {
                    const u32 k = chk_bound<false>(qval, r0, r0 + rn, v);
                    found = k < r0 + rn && qval[k] == v;
                }
            }
            if (!EX) {
                hits += (u32)__popcll(__ballot(found));  // (the same in every lane of the wave)
            } else {
                u32 tot = 0;
                const u32 r = sel_block_rank(on && !found, s_w, &tot);
                if (on && !found && rank + r < nex) ex[s_cand * nex + rank + r] = v;
                rank += tot;
                if (rank >= nex) break;  // (uniform)
            }
        }
        if (!EX) {
            if (lane_id() == 0) s_w[threadIdx.x / RDF_WAVE] = hits;
            __syncthreads();
            if (threadIdx.x == 0) {
                u32 t = 0;
#pragma unroll
                for (u32 k = 0; k < RDF_WAVES_PER_BLOCK; ++k) t += s_w[k];
                viol[w] = (d1 - d0) - t;
            }
        }
    }
}

// the rows of candidates [c0, c0 + Mb): violations = the item violations between the candidate's first item and the next
// candidate's (vpre[W] = all of the batch's)
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_rows(u64 c0, u64 Mb, const u32* __restrict__ side, const u32* __restrict__ qoff,
                                                        const u64* __restrict__ ioff, const u64* __restrict__ vpre, u32 nex,
                                                        rdf_check_row* rows) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < Mb; i += (u64)gridDim.x * RDF_BLOCK) {
        const u64 cand = c0 + i;
        const u32 ds = chk_len(qoff, side[2 * cand]), rs = chk_len(qoff, side[2 * cand + 1]);
        const u32 v = (u32)(vpre[ioff[i + 1]] - vpre[ioff[i]]);
        rdf_check_row row;
        row.dep_support = ds;
        row.ref_support = rs;
        row.overlap = ds - v;
        row.n_examples = v < nex ? v : nex;
        rows[cand] = row;
    }
}

// cls[0] += holding rows, cls[1] += violated, cls[2] += empty (one atomic per class and block)
__global__ __launch_bounds__(RDF_BLOCK) void k_chk_classes(const rdf_check_row* __restrict__ rows, u64 M, u64* cls) {
    __shared__ u32 s_w[RDF_WAVES_PER_BLOCK];
    u32 h = 0, v = 0, e = 0;
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < M; i += (u64)gridDim.x * RDF_BLOCK) {
        const rdf_check_row r = rows[i];
        if (r.dep_support == 0) ++e;
        else if (r.overlap == r.dep_support) ++h;
        else ++v;
    }
    h = sel_block_sum(h, s_w);
    v = sel_block_sum(v, s_w);
    e = sel_block_sum(e, s_w);
    if (threadIdx.x == 0) {
        if (h) (void)atomicAdd(&cls[0], (u64)h);
        if (v) (void)atomicAdd(&cls[1], (u64)v);
        if (e) (void)atomicAdd(&cls[2], (u64)e);
    }
}
