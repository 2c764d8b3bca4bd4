// Result statistics (included by kernels.inl): rdf_cind_stats_begin / _add / _end, rdf_cind_histogram,
// rdf_copy_top_refs.  Integer reductions over the result as it lies in HBM, the class part unexpanded: a mask class of
// M members sharing a list of L refs is counted in O(M + L), never as its M x L rows.
//
// Accumulators (additive over the pages of a paged run, which partition the dependents and keep the compact ids):
//   nref[C]   refs of each dependent              indeg[C]   CINDs referencing each capture
//   cells[81] CINDs per (dependent code, ref code); the code index 0..8 numbers the codes 10 12 14 17 20 21 33 34 35
//             in ascending order (the codes by decode_capture's rule), so the cells ascend by dep code << 8 | ref code
// add, explicit part:   k_cs_run_refs (nref from the run lengths) and k_cs_explicit (one pass over the refs: a relaxed,
//                       result-free atomic add per ref into indeg, an 81-bin LDS histogram per block for the cells)
// add, pending classes: k_cs_class, one block per class: indeg[list entry] += M, indeg[self] -= 1, nref[member] += its
//                       count, cells += (members per code) x (list refs per code) - the self entries on the diagonal
// end:                  k_cs_level2 -> the run-length kernels of histo.inl (kinds 3 and 4), k_cs_support_keys -> sort ->
//                       scan -> k_cs_support_rows (kind 2: nref summed per support), k_cs_shape_rows (kind 1),
//                       k_cs_top_keys -> one sort (the top list)

static constexpr u32 CS_CODES = 9;
static constexpr u32 CS_CELLS = CS_CODES * CS_CODES;
// cells[CS_CELLS + 0 / 1]: dependents with refs / captures with references (k_cs_level2)
static constexpr u32 CS_NZ = CS_CELLS;
static constexpr u32 CS_SCALARS = CS_CELLS + 2;
static constexpr u64 CS_KIND_ZERO = 7;  // level-2 kind of the zero entries: sorts behind kinds 3 and 4, dropped

__host__ __device__ inline u32 cs_code_of(u32 idx) {
    return idx == 0 ? 10u : idx == 1 ? 12u : idx == 2 ? 14u : idx == 3 ? 17u : idx == 4 ? 20u : idx == 5 ? 21u
           : idx == 6 ? 33u : idx == 7 ? 34u : 35u;
}
// code index of unary type t (10 12 17 20 33 34) / binary type bt (14 21 35)
__host__ __device__ inline u32 cs_unary_index(u32 t) { return t + (t >= 2) + (t >= 4); }
__host__ __device__ inline u32 cs_binary_index(u32 bt) { return 3 * bt + 2; }

// code[c] = code index of compact capture c
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_codes(const u32* __restrict__ fext, u32 C, u32 V,
                                                        const u64* __restrict__ bkeys, unsigned char* code) {
    const u64 six = 6ull * V;
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < C; i += (u64)gridDim.x * RDF_BLOCK) {
        const u32 ext = fext[i];
        code[i] = (unsigned char)(ext < six ? cs_unary_index(ext / V) : cs_binary_index((u32)bin_key_type(bkeys[ext - six])));
    }
}

// hist[bin] += 1 for every lane with `on`, one LDS atomic per distinct bin of the wave (a run's refs mostly share one)
__device__ inline void cs_wave_count(u32* hist, u32 bin, bool on) {
    u64 todo = __ballot(on);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const u32 b = __shfl(bin, l, RDF_WAVE);
        const u64 same = __ballot(on && bin == b);
        if (lane_id() == l) atomicAdd(&hist[b], (u32)__popcll(same));
        todo &= ~same;
    }
}

// nref[rundep[r]] += length of run r, for the runs [0, R) of the explicit rows (a dependent may have several runs)
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_run_refs(const u64* __restrict__ runoff, const u32* __restrict__ rundep,
                                                           u64 R, u32* nref) {
    for (u64 r = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; r < R; r += (u64)gridDim.x * RDF_BLOCK) {
        const u64 len = runoff[r + 1] - runoff[r];
        if (len) atomicAdd(&nref[rundep[r]], (u32)len);
    }
}

// the explicit rows [0, n): indeg[ref] += 1 and the (dependent code, ref code) cells; dependents as in k_checksum.  A
// block counts at most n / gridDim.x + RDF_BLOCK rows, which its u32 LDS bins hold for n < 2^32 gridDim.x
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_explicit(const u32* __restrict__ refs, u64 n, const u64* __restrict__ runoff,
                                                           const u32* __restrict__ rundep, u64 R,
                                                           const unsigned char* __restrict__ code, u32* indeg, u64* cells) {
    __shared__ u64 s_lo, s_hi;
    __shared__ u32 s_cell[CS_CELLS];
    for (u32 t = threadIdx.x; t < CS_CELLS; t += RDF_BLOCK) s_cell[t] = 0;
    for (u64 b = (u64)blockIdx.x * RDF_BLOCK; b < n; b += (u64)gridDim.x * RDF_BLOCK) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const u64 last = b + RDF_BLOCK - 1 < n ? b + RDF_BLOCK - 1 : n - 1;
            s_lo = run_of(runoff, 0, R - 1, b);
            s_hi = run_of(runoff, s_lo, R - 1, last);
        }
        __syncthreads();
        const u64 i = b + threadIdx.x;
        const bool on = i < n;
        u32 cell = 0;
        if (on) {
            const u32 d = rundep[run_of(runoff, s_lo, s_hi, i)], r = refs[i];
            cell = (u32)code[d] * CS_CODES + code[r];
            (void)__hip_atomic_fetch_add(&indeg[r], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        cs_wave_count(s_cell, cell, on);
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < CS_CELLS; t += RDF_BLOCK)
        if (s_cell[t]) atomicAdd(&cells[t], (u64)s_cell[t]);
}

// the pending class part, one block per class m: members ckeys[coff[m], coff[m + 1]) (class << 32 | dependent), list
// lists[lwoff[cchoff[m]], lwoff[cchoff[m + 1]]); selfpos / mcnt per member as k_class_members left them.  A class
// without unary members (its list serves classed binary dependents only) adds nothing.
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_class(u32 ncls, const u64* __restrict__ coff, const u64* __restrict__ cchoff,
                                                        const u64* __restrict__ lwoff, const u32* __restrict__ lists,
                                                        const u64* __restrict__ ckeys, const u32* __restrict__ selfpos,
                                                        const u32* __restrict__ mcnt, const unsigned char* __restrict__ code,
                                                        u32* nref, u32* indeg, u64* cells) {
    __shared__ u32 s_mem[CS_CODES], s_list[CS_CODES], s_self[CS_CODES];
    for (u64 m = blockIdx.x; m < ncls; m += gridDim.x) {
        const u64 k0 = coff[m], k1 = coff[m + 1];
        if (k0 == k1) continue;  // (uniform over the block)
        const u64 lb = lwoff[cchoff[m]], le = lwoff[cchoff[m + 1]];
        __syncthreads();
        if (threadIdx.x < CS_CODES) s_mem[threadIdx.x] = s_list[threadIdx.x] = s_self[threadIdx.x] = 0;
        __syncthreads();
        const u32 M = (u32)(k1 - k0);
        for (u64 b = k0; b < k1; b += RDF_BLOCK) {
            const u64 i = b + threadIdx.x;
            const bool on = i < k1;
            u32 cd = 0;
            bool self = false;
            if (on) {
                const u32 d = (u32)ckeys[i];
                cd = code[d];
                self = selfpos[i] != NONE32;
                if (mcnt[i]) atomicAdd(&nref[d], mcnt[i]);
                if (self) (void)__hip_atomic_fetch_add(&indeg[d], 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            cs_wave_count(s_mem, cd, on);
            cs_wave_count(s_self, cd, self);
        }
        for (u64 b = lb; b < le; b += RDF_BLOCK) {
            const u64 i = b + threadIdx.x;
            const bool on = i < le;
            u32 cr = 0;
            if (on) {
                const u32 r = lists[i];
                cr = code[r];
                (void)__hip_atomic_fetch_add(&indeg[r], M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            cs_wave_count(s_list, cr, on);
        }
        __syncthreads();
        if (threadIdx.x < CS_CELLS) {
            const u32 dc = threadIdx.x / CS_CODES, rc = threadIdx.x % CS_CODES;
            const u64 v = (u64)s_mem[dc] * s_list[rc] - (dc == rc ? s_self[dc] : 0u);
            if (v) atomicAdd(&cells[threadIdx.x], v);
        }
    }
}

// level-2 keys of kinds 3 and 4: out[d] = 3 << 32 | nref[d], out[C + c] = 4 << 32 | indeg[c]; zero entries get kind
// CS_KIND_ZERO.  cells[CS_NZ + 0 / 1] += the non-zero entries of each.
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_level2(const u32* __restrict__ nref, const u32* __restrict__ indeg, u32 C,
                                                         u64* out, u64* cells) {
    u32 nz_ref = 0, nz_in = 0;
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < C; i += (u64)gridDim.x * RDF_BLOCK) {
        const u32 a = nref[i], b = indeg[i];
        out[i] = a ? ((u64)RDF_CS_REFS << 32) | a : CS_KIND_ZERO << 32;
        out[(u64)C + i] = b ? ((u64)RDF_CS_INDEGREE << 32) | b : CS_KIND_ZERO << 32;
        nz_ref += a ? 1u : 0u;
        nz_in += b ? 1u : 0u;
    }
    nz_ref = wave_sum(nz_ref);
    nz_in = wave_sum(nz_in);
    if (lane_id() == 0 && nz_ref) atomicAdd(&cells[CS_NZ], (u64)nz_ref);
    if (lane_id() == 0 && nz_in) atomicAdd(&cells[CS_NZ + 1], (u64)nz_in);
}

// support << 32 | dependent for the dependents with refs; the others get support NONE32 (behind every real support)
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_support_keys(const u32* __restrict__ nref, const u32* __restrict__ csup, u32 C,
                                                               u64* out) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < C; i += (u64)gridDim.x * RDF_BLOCK)
        out[i] = ((u64)(nref[i] ? csup[i] : NONE32) << 32) | i;
}

// w[i] = refs of the dependent of sorted support key i
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_support_weights(const u64* __restrict__ keys, u64 m,
                                                                  const u32* __restrict__ nref, u64* w) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < m; i += (u64)gridDim.x * RDF_BLOCK)
        w[i] = nref[(u32)keys[i]];
}

// one row per support run r of the sorted keys: (2, support, sum of the run's weights); wsum = the exclusive scan of
// the weights with the total at [m], start as k_histo_starts leaves it
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_support_rows(const u64* __restrict__ keys, const u32* __restrict__ start,
                                                               u64 R, const u64* __restrict__ wsum, rdf_hist_row* out) {
    for (u64 r = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; r < R; r += (u64)gridDim.x * RDF_BLOCK) {
        const u32 b = start[r];
        rdf_hist_row row;
        row.kind = RDF_CS_SUPPORT;
        row.value = (u32)(keys[b] >> 32);
        row.times = wsum[start[r + 1]] - wsum[b];
        out[r] = row;
    }
}

// the non-zero cells as rows (1, dep code << 8 | ref code, CINDs), ascending by value: one wave, cell t on lane t % 64
__global__ __launch_bounds__(RDF_WAVE) void k_cs_shape_rows(const u64* __restrict__ cells, rdf_hist_row* out) {
    u32 base = 0;
    for (u32 t0 = 0; t0 < CS_CELLS; t0 += RDF_WAVE) {
        const u32 t = t0 + threadIdx.x;
        const u64 v = t < CS_CELLS ? cells[t] : 0;
        const u64 nz = __ballot(v != 0);
        if (v) {
            rdf_hist_row row;
            row.kind = RDF_CS_SHAPE;
            row.value = (cs_code_of(t / CS_CODES) << 8) | cs_code_of(t % CS_CODES);
            row.times = v;
            out[base + __popcll(nz & lanemask_lt())] = row;
        }
        base += (u32)__popcll(nz);
    }
}

// (~indeg) << 32 | external capture id: ascending = descending in-degree, ties by ascending capture id
__global__ __launch_bounds__(RDF_BLOCK) void k_cs_top_keys(const u32* __restrict__ indeg, const u32* __restrict__ fext, u32 C,
                                                           u64* out) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < C; i += (u64)gridDim.x * RDF_BLOCK)
        out[i] = ((u64)(~indeg[i]) << 32) | fext[i];
}
