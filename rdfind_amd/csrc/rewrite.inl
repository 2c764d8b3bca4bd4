// rdf_rewrite_terms: --asciify-triples and --prefixes on the device dictionary (included by kernels.inl).
//
// Both are pure functions of one term (ALG/programs/RDFind.scala:239-267), so they run once per distinct term over the
// term table the parse left in HBM (term id i at src[term_off[i], +term_len[i])):
//   k_rw_len     per term: the asciified length, the longest key that is a prefix of the (asciified) term, the new
//                length, the error flags; nothing resident changes before the host has read the flags
//   k_rw_write   the new bytes into a scratch heap at the scanned offsets (short terms a lane each, long ones a wave)
//   k_rw_hash    the tokenizer's 64-bit hash (nt_hash) of the new bytes
//   k_nt_dict_insert<1> / k_nt_dict_rep<1> over the scratch heap with occurrence = old id: a class's slot ends holding
//                its smallest old id, so the new ids (scan of `first`) ascend with it, as a host re-encoding in id order
//   k_rw_compact the new term table and old id -> new id; k_nt_append_bytes packs the representatives' bytes
//   k_rw_remap   s / p / o through the map, 16 B per load and store
//
// AsciifyTriples.asciify (ALG/operators/AsciifyTriples.scala:17-37): every UTF-16 code unit c of the term becomes the
// bytes c & 0x7F, c >>= 7, ... until c == 0 (at least one byte); a code point >= U+10000 is its two surrogates.
// ShortenUrls.shorten (ALG/operators/ShortenUrls.scala:36-44): a term ending in '>' whose longest prefix key is k
// becomes value(k) + term[len(k) : len - 1].
//
// Key lookup: the FNV-1a hash of the term's first L bytes is kept incrementally; at the lengths L that some key has
// (a bitmap), the table of all keys (open addressing, full 64-bit hash per slot, load <= 1/2) is probed and a hit is
// byte-compared.  One pass over the first min(len, longest key) bytes, whatever the number of keys.  The table, the
// key offsets and the key bytes are staged in LDS when they fit (RW_LDS_*), else read from global memory.

static constexpr u32 RW_NONE = 0xffffffffu;
static constexpr u32 RW_LDS_SLOTS = 2048;   // table slots (<= 1024 keys) ...
static constexpr u32 RW_LDS_HEAP = 16384;   // ... key bytes ...
static constexpr u32 RW_LDS_MAXLEN = 1023;  // ... and longest key of the LDS-staged form (44 KB of LDS)
static constexpr u32 RW_LONG = 256;         // terms of more source bytes are written by a wave together

__host__ __device__ inline u64 rw_hash0() { return 0xcbf29ce484222325ull; }
__host__ __device__ inline u64 rw_hash_step(u64 h, u32 b) { return (h ^ b) * 0x100000001b3ull; }
__host__ __device__ inline u32 rw_slot(u64 h, u32 mask) { return (u32)mix64(h) & mask; }

// the key tables of one call (device or LDS addresses)
struct RwKeys {
    const u64* th;               // [mask + 1] the keys' hashes (where tk holds a key)
    const u32* tk;               // [mask + 1] key index or RW_NONE
    const u32* koff;             // [n_keys + 1] key byte offsets
    const u32* lenbits;          // bit L: some key has L bytes; maxlen / 32 + 1 words
    const unsigned char* kheap;  // the keys' bytes
    u32 mask, maxlen, n_keys, kbytes;
};

// one UTF-8 sequence at s[pos, end): its byte count and code point, 0 when it is not valid UTF-8 (overlong forms,
// surrogates and values above U+10FFFF included)
__device__ inline u32 rw_decode(const unsigned char* __restrict__ s, u64 pos, u64 end, u32* cp) {
    const u32 b0 = s[pos];
    if (b0 < 0x80) {
        *cp = b0;
        return 1;
    }
    const u32 need = b0 < 0xC2 ? 0u : b0 < 0xE0 ? 1u : b0 < 0xF0 ? 2u : b0 < 0xF5 ? 3u : 0u;
    if (!need || pos + need >= end) return 0;  // (a lead byte of 0x80..0xC1 or 0xF5.. or a sequence cut short)
    u32 v = b0 & (0x3Fu >> need);
    for (u32 k = 1; k <= need; ++k) {
        const u32 b = s[pos + k];
        if ((b & 0xC0) != 0x80) return 0;
        v = (v << 6) | (b & 0x3F);
    }
    if (need == 2 && (v < 0x800 || (v >= 0xD800 && v <= 0xDFFF))) return 0;
    if (need == 3 && (v < 0x10000 || v > 0x10FFFF)) return 0;
    *cp = v;
    return need + 1;
}

// the asciified bytes of one code point, packed lowest byte first (at most 6: two surrogates of 3 bytes)
__device__ inline u32 rw_asciify_cp(u32 cp, u64* out) {
    u32 unit[2], nu = 1;
    if (cp >= 0x10000) {
        cp -= 0x10000;
        unit[0] = 0xD800 + (cp >> 10);
        unit[1] = 0xDC00 + (cp & 0x3FF);
        nu = 2;
    } else {
        unit[0] = cp;
    }
    u64 ob = 0;
    u32 cnt = 0;
    for (u32 u = 0; u < nu; ++u) {
        u32 c = unit[u];
        for (int k = 0; k < 3; ++k) {  // a unit is < 2^16: at most three groups of 7 bits
            ob |= (u64)(c & 0x7F) << (8 * cnt);
            ++cnt;
            c >>= 7;
            if (!c) break;
        }
    }
    *out = ob;
    return cnt;
}

// the bytes of a term as the rewrite sees them: its own (ASC = false) or its asciified form
template <bool ASC>
struct RwStream {
    const unsigned char* s;
    u64 pos, end;
    u64 ob = 0;
    u32 cnt = 0;
    bool bad = false, nonascii = false;
    __device__ RwStream(const unsigned char* s_, u64 a, u64 e) : s(s_), pos(a), end(e) {}
    __device__ int next() {
        if (!ASC) return pos < end ? (int)s[pos++] : -1;
        if (!cnt) {
            if (pos >= end || bad) return -1;
            u32 cp = 0;
            const u32 nb = rw_decode(s, pos, end, &cp);
            if (!nb) {
                bad = true;
                return -1;
            }
            nonascii |= nb > 1;
            pos += nb;
            cnt = rw_asciify_cp(cp, &ob);
        }
        const int b = (int)(ob & 0xFF);
        ob >>= 8;
        --cnt;
        return b;
    }
};

// whether key k (L bytes) is a prefix of the term's stream
template <bool ASC>
__device__ inline bool rw_key_equal(const RwKeys& K, u32 k, const unsigned char* __restrict__ src, u64 a, u64 e, u32 L) {
    RwStream<ASC> it(src, a, e);
    const unsigned char* kb = K.kheap + K.koff[k];
    for (u32 i = 0; i < L; ++i)
        if (it.next() != (int)kb[i]) return false;
    return true;
}

// the key of L bytes with prefix hash h that the term starts with, or RW_NONE
template <bool ASC>
__device__ inline u32 rw_probe(const RwKeys& K, u64 h, u32 L, const unsigned char* __restrict__ src, u64 a, u64 e) {
    u32 sl = rw_slot(h, K.mask);
    for (u32 probe = 0; probe <= K.mask; ++probe, sl = (sl + 1) & K.mask) {
        const u32 k = K.tk[sl];
        if (k == RW_NONE) return RW_NONE;
        if (K.th[sl] == h && K.koff[k + 1] - K.koff[k] == L && rw_key_equal<ASC>(K, k, src, a, e, L)) return k;
    }
    return RW_NONE;
}

// Per term: matched key (km), new length (nlen).  err[0] / err[1] / err[2]: the smallest term id whose longest key
// covers the whole term / that is not valid UTF-8 (ASC) / whose new length does not fit 32 bits; err[3]: the number of
// terms whose bytes change (a key matched, or a non-ASCII character under ASC).
template <bool ASC, bool LDS>
__global__ __launch_bounds__(RDF_BLOCK) void k_rw_len(const unsigned char* __restrict__ src, const u64* __restrict__ toff,
                                                      const u32* __restrict__ tlen, u64 V, RwKeys G,
                                                      const u32* __restrict__ vlen, u32* nlen, u32* km, u64* err) {
    __shared__ u64 s_th[LDS ? RW_LDS_SLOTS : 1];
    __shared__ u32 s_tk[LDS ? RW_LDS_SLOTS : 1];
    __shared__ u32 s_koff[LDS ? RW_LDS_SLOTS / 2 + 1 : 1];
    __shared__ u32 s_bits[LDS ? RW_LDS_MAXLEN / 32 + 1 : 1];
    __shared__ u32 s_heap[LDS ? RW_LDS_HEAP / 4 : 1];
    RwKeys K = G;
    if (LDS) {  // (the host chose this form: every count below fits its array)
        for (u32 i = threadIdx.x; i <= G.mask; i += RDF_BLOCK) {
            s_th[i] = G.th[i];
            s_tk[i] = G.tk[i];
        }
        for (u32 i = threadIdx.x; i <= G.n_keys; i += RDF_BLOCK) s_koff[i] = G.koff[i];
        for (u32 i = threadIdx.x; i <= G.maxlen / 32; i += RDF_BLOCK) s_bits[i] = G.lenbits[i];
        for (u32 i = threadIdx.x; i < (G.kbytes + 3) / 4; i += RDF_BLOCK) s_heap[i] = ((const u32*)G.kheap)[i];
        __syncthreads();
        K.th = s_th;
        K.tk = s_tk;
        K.koff = s_koff;
        K.lenbits = s_bits;
        K.kheap = (const unsigned char*)s_heap;
    }
    for (u64 t0 = (u64)blockIdx.x * RDF_BLOCK; t0 < V; t0 += (u64)gridDim.x * RDF_BLOCK) {
        const u64 t = t0 + threadIdx.x;
        bool changed = false;
        if (t < V) {
            const u64 a = toff[t];
            const u32 n = tlen[t];
            u64 alen = 0, h = rw_hash0();
            u32 last = 0, best = RW_NONE;
            if (!ASC) {
                alen = n;
                last = n ? src[a + n - 1] : 0;
                const u32 lim = last == '>' && K.n_keys ? (n < K.maxlen ? n : K.maxlen) : 0;
                for (u32 i = 0; i < lim; ++i) {
                    h = rw_hash_step(h, src[a + i]);
                    const u32 L = i + 1;
                    if (K.lenbits[L >> 5] >> (L & 31) & 1) {
                        const u32 k = rw_probe<false>(K, h, L, src, a, a + n);
                        if (k != RW_NONE) best = k;
                    }
                }
            } else {
                RwStream<true> it(src, a, a + n);
                for (int b = it.next(); b >= 0; b = it.next()) {
                    ++alen;
                    last = (u32)b;
                    if (K.n_keys && alen <= K.maxlen) {
                        h = rw_hash_step(h, (u32)b);
                        const u32 L = (u32)alen;
                        if (K.lenbits[L >> 5] >> (L & 31) & 1) {
                            const u32 k = rw_probe<true>(K, h, L, src, a, a + n);
                            if (k != RW_NONE) best = k;
                        }
                    }
                }
                if (it.bad) atomicMin(&err[1], t);
                changed = it.nonascii;
                if (last != '>') best = RW_NONE;
            }
            u64 out = alen;
            if (best != RW_NONE) {
                const u32 kl = K.koff[best + 1] - K.koff[best];
                if (kl >= alen)
                    atomicMin(&err[0], t);
                else
                    out = (u64)vlen[best] + alen - kl - 1;
                changed = true;
            }
            if (out > 0xffffffffull) {
                atomicMin(&err[2], t);
                out = 0;
            }
            nlen[t] = (u32)out;
            km[t] = best;
        }
        const u32 nch = (u32)__popcll(__ballot(changed));
        if (lane_id() == 0 && nch) atomicAdd(&err[3], (u64)nch);
    }
}

// The new bytes of every term at dst[noff[t], +nlen[t]): value(km) followed by the term's stream without its first
// len(key) bytes and its final '>' (no key: the whole stream).  A wave takes 64 consecutive terms: a term of at most
// RW_LONG source bytes is written by its lane, the longer ones by the whole wave one after the other, 64 source bytes
// per step (under ASC each lane decodes the character that starts at its byte, and a wave scan places the bytes).
template <bool ASC>
__global__ __launch_bounds__(RDF_BLOCK) void k_rw_write(const unsigned char* __restrict__ src, const u64* __restrict__ toff,
                                                        const u32* __restrict__ tlen, u64 V, const u32* __restrict__ koff,
                                                        const u32* __restrict__ voff, const unsigned char* __restrict__ vheap,
                                                        const u32* __restrict__ km, const u32* __restrict__ nlen,
                                                        const u64* __restrict__ noff, unsigned char* dst) {
    const u64 wave = (u64)blockIdx.x * RDF_WAVES_PER_BLOCK + threadIdx.x / RDF_WAVE;
    const u64 nwaves = (u64)gridDim.x * RDF_WAVES_PER_BLOCK;
    const int lane = lane_id();
    for (u64 t0 = wave * RDF_WAVE; t0 < V; t0 += nwaves * RDF_WAVE) {
        const u64 t = t0 + lane;
        const bool live = t < V;
        u64 a = 0, d = 0, vsrc = 0;
        u32 n = 0, skip = 0, vl = 0, keep = 0;  // keep: stream bytes [skip, skip + keep) are written
        if (live) {
            a = toff[t];
            n = tlen[t];
            d = noff[t];
            const u32 k = km[t];
            keep = nlen[t];
            if (k != RW_NONE) {
                skip = koff[k + 1] - koff[k];
                vsrc = voff[k];
                vl = voff[k + 1] - voff[k];
                keep -= vl;
            }
        }
        const bool is_long = live && n > RW_LONG;
        if (live && !is_long) {
            for (u32 i = 0; i < vl; ++i) dst[d + i] = vheap[vsrc + i];
            RwStream<ASC> it(src, a, a + n);
            u64 idx = 0;
            for (int b = it.next(); b >= 0 && idx < (u64)skip + keep; b = it.next(), ++idx)
                if (idx >= skip) dst[d + vl + (idx - skip)] = (unsigned char)b;
        }
        u64 todo = __ballot(is_long);
        for (int round = 0; round < RDF_WAVE && todo; ++round) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const u64 wa = __shfl(a, l, RDF_WAVE), wd = __shfl(d, l, RDF_WAVE), wv = __shfl(vsrc, l, RDF_WAVE);
            const u32 wn = __shfl(n, l, RDF_WAVE), wskip = __shfl(skip, l, RDF_WAVE), wvl = __shfl(vl, l, RDF_WAVE);
            const u32 wkeep = __shfl(keep, l, RDF_WAVE);
            for (u32 i = lane; i < wvl; i += RDF_WAVE) dst[wd + i] = vheap[wv + i];
            u64 base = 0;  // stream bytes before this step
            for (u32 i0 = 0; i0 < wn; i0 += RDF_WAVE) {
                const u32 i = i0 + lane;
                u64 ob = 0;
                u32 cnt = 0;
                if (i < wn) {
                    const u32 b0 = src[wa + i];
                    if (!ASC) {
                        ob = b0;
                        cnt = 1;
                    } else if ((b0 & 0xC0) != 0x80) {  // the character starting here (k_rw_len found the term valid)
                        u32 cp = 0;
                        if (rw_decode(src, wa + i, wa + wn, &cp)) cnt = rw_asciify_cp(cp, &ob);
                    }
                }
                const u32 incl = wave_inclusive_scan(cnt);
                const u32 total = __shfl(incl, RDF_WAVE - 1, RDF_WAVE);
                const u64 first = base + incl - cnt;
                for (u32 k = 0; k < cnt; ++k) {
                    const u64 idx = first + k;
                    if (idx >= wskip && idx < (u64)wskip + wkeep)
                        dst[wd + wvl + (idx - wskip)] = (unsigned char)(ob >> (8 * k));
                }
                base += total;
            }
        }
    }
}

// the tokenizer's hash of the new bytes (what k_nt_tokenize writes into nhv), and the offsets as the dictionary
// kernels take them
__global__ __launch_bounds__(RDF_BLOCK) void k_rw_hash(const unsigned char* __restrict__ heap, const u64* __restrict__ noff,
                                                       const u32* __restrict__ nlen, u64 V, u64* hv) {
    for (u64 t = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; t < V; t += (u64)gridDim.x * RDF_BLOCK)
        hv[t] = nt_hash(NtGlobal{heap}, noff[t], nlen[t]);
}

// old id -> new id (the id of its class's smallest old id); per class representative: the row of the new term table
// and where its bytes lie in the scratch heap
__global__ __launch_bounds__(RDF_BLOCK) void k_rw_compact(const u32* __restrict__ rep, const u32* __restrict__ first,
                                                          const u32* __restrict__ fid, const u64* __restrict__ noff,
                                                          const u32* __restrict__ nlen, const u64* __restrict__ coff, u64 V,
                                                          u32* remap, u64* term_off, u32* term_len, u64* srcoff) {
    for (u64 t = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; t < V; t += (u64)gridDim.x * RDF_BLOCK) {
        remap[t] = fid[rep[t]];
        if (first[t]) {
            const u32 id = fid[t];
            term_off[id] = coff[t];
            term_len[id] = nlen[t];
            srcoff[id] = noff[t];
        }
    }
}

// s / p / o through the map in place: four ids per 16-B load and store, the last n % 4 ids one by one
__global__ __launch_bounds__(RDF_BLOCK) void k_rw_remap(u32* s, u32* p, u32* o, u64 n, const u32* __restrict__ remap) {
    const u64 n4 = n / 4;
    u32* const arr[3] = {s, p, o};
    for (int x = 0; x < 3; ++x) {
        uint4* v4 = (uint4*)arr[x];
        for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < n4; i += (u64)gridDim.x * RDF_BLOCK) {
            uint4 v = v4[i];
            v.x = remap[v.x];
            v.y = remap[v.y];
            v.z = remap[v.z];
            v.w = remap[v.w];
            v4[i] = v;
        }
        if (blockIdx.x == 0 && threadIdx.x < n - 4 * n4) {
            const u64 i = 4 * n4 + threadIdx.x;
            arr[x][i] = remap[arr[x][i]];
        }
    }
}
