// Test-only entry points (test_abi.h).  Included at the end of rdfind_hip.hip, which defines rdf_ctx; nothing in
// the pipeline calls them.

namespace {

// A device array of `count` elements of `esz` bytes that starts `skew` elements past a 16-byte aligned address, with
// RDF_TEST_CANARY pattern elements directly before and directly after it.  The whole allocation starts as the pattern.
struct TestArr {
    DevBuf buf;
    size_t esz = 0, count = 0, off = 0;  // off: the array's byte offset in buf
    hipError_t make(size_t elem_bytes, size_t elems, unsigned skew, hipStream_t st) {
        esz = elem_bytes;
        count = elems;
        off = (RDF_TEST_CANARY + skew) * esz;  // (hipMalloc aligns to 256 B and 64 elements are a multiple of 16 B)
        hipError_t e = buf.ensure(off + (count + RDF_TEST_CANARY) * esz);
        if (e != hipSuccess) return e;
        return hipMemsetAsync(buf.p, RDF_TEST_CANARY_BYTE, buf.cap, st);
    }
    char* data() const { return (char*)buf.p + off; }
    ~TestArr() { buf.release(); }
};

static bool all_pattern(const unsigned char* p, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i)
        if (p[i] != RDF_TEST_CANARY_BYTE) return false;
    return true;
}

// *ok &= the canaries on both sides of a[0, a.count) are intact (call after the stream has drained)
static hipError_t check_canaries(const TestArr& a, bool* ok) {
    const size_t cb = RDF_TEST_CANARY * a.esz;
    std::vector<unsigned char> h(2 * cb);
    hipError_t e = hipMemcpy(h.data(), a.data() - cb, cb, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h.data() + cb, a.data() + a.count * a.esz, cb, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !all_pattern(h.data(), h.size())) *ok = false;
    return e;
}

// *ok &= a[0, elems) still holds `want` (want == nullptr: the fill pattern)
static hipError_t check_contents(const TestArr& a, const void* want, size_t elems, bool* ok) {
    if (!elems) return hipSuccess;
    std::vector<unsigned char> h(elems * a.esz);
    hipError_t e = hipMemcpy(h.data(), a.data(), h.size(), hipMemcpyDeviceToHost);
    if (e == hipSuccess && !(want ? memcmp(h.data(), want, h.size()) == 0 : all_pattern(h.data(), h.size()))) *ok = false;
    return e;
}

static rdf_status prim_status(rdf_ctx* c, hipError_t e, const char* what) {
    if (e == hipSuccess) return RDF_OK;
    (void)hipGetLastError();
    return fail(c, e == hipErrorOutOfMemory ? RDF_ERR_OOM : RDF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// rdf_test_unary_lookup: rank[i] = frank[keys[i]] (global ranks after the stage), bit[i] = the key's fbits bit
__global__ __launch_bounds__(RDF_BLOCK) void k_test_unary_lookup(const u64* __restrict__ keys, u64 n,
                                                                 const u32* __restrict__ frank,
                                                                 const u64* __restrict__ fbits, u32* rank, u32* bit) {
    for (u64 i = (u64)blockIdx.x * RDF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * RDF_BLOCK) {
        rank[i] = frank[keys[i]];
        bit[i] = fbit(fbits, keys[i]) ? 1u : 0u;
    }
}

// the frequent-condition state these calls read: the stage is done, single GPU, and its buffers are still held
static rdf_status fc_state(rdf_ctx* c, const char* who) {
    if (c->stage < 2 || c->nranks != 1 || !c->frank.p || !c->fbits.p || !c->fval.p)
        return fail(c, RDF_ERR_STATE, std::string(who) + ": rdf_frequent_conditions must be called first");
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_test_scan(rdf_ctx* c, int kind, const void* in_host, uint64_t n, uint32_t in_skew, uint32_t out_skew,
                         int in_place, int want_total, void* out_host, uint64_t* total_out, uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || (n && (!in_host || !out_host)) || (want_total && !total_out))
        return fail(c, RDF_ERR_ARG, "rdf_test_scan: null argument");
    *canaries_ok = 0;
    if (kind < RDF_TEST_SCAN_U32_U32 || kind > RDF_TEST_SCAN_U64_U64 || in_skew > 3 || out_skew > 3)
        return fail(c, RDF_ERR_ARG, "rdf_test_scan: kind or skew out of range");
    const size_t isz = kind == RDF_TEST_SCAN_U64_U64 ? 8 : 4, osz = kind == RDF_TEST_SCAN_U32_U32 ? 4 : 8;
    if (in_place && (isz != osz || in_skew != out_skew))
        return fail(c, RDF_ERR_ARG, "rdf_test_scan: in place needs equal element types and skews");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    TestArr in, out, tot;
    const bool tail_total = in_place && want_total;  // the total at out[n]: one more element may be written
    HIP_TRY(c, in.make(isz, n + (tail_total ? 1 : 0), in_skew, st));
    if (!in_place) HIP_TRY(c, out.make(osz, n, out_skew, st));
    if (!in_place && want_total) HIP_TRY(c, tot.make(osz, 1, 0, st));
    if (n) HIP_TRY(c, hipMemcpyAsync(in.data(), in_host, n * isz, hipMemcpyHostToDevice, st));
    char* d_out = in_place ? in.data() : out.data();
    char* d_tot = !want_total ? nullptr : in_place ? in.data() + n * osz : tot.data();
    hipError_t e = kind == RDF_TEST_SCAN_U32_U32   ? exclusive_scan_u32(c->ws, (const u32*)in.data(), (u32*)d_out, n, (u32*)d_tot, st)
                   : kind == RDF_TEST_SCAN_U32_U64 ? exclusive_scan_u32_u64(c->ws, (const u32*)in.data(), (u64*)d_out, n, (u64*)d_tot, st)
                                                   : exclusive_scan_u64(c->ws, (const u64*)in.data(), (u64*)d_out, n, (u64*)d_tot, st);
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    HIP_TRY(c, check_canaries(in, &ok));
    if (!in_place) {
        HIP_TRY(c, check_canaries(out, &ok));
        HIP_TRY(c, check_contents(in, in_host, n, &ok));  // the input is read only
        if (want_total) HIP_TRY(c, check_canaries(tot, &ok));
    }
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "exclusive_scan"));
    if (n) HIP_TRY(c, hipMemcpy(out_host, d_out, n * osz, hipMemcpyDeviceToHost));
    if (want_total) {
        u64 t = 0;  // (little endian: a 4-byte total lands in the low half)
        HIP_TRY(c, hipMemcpy(&t, d_tot, osz, hipMemcpyDeviceToHost));
        *total_out = t;
    }
    return RDF_OK;
}

rdf_status rdf_test_scan_batch(rdf_ctx* c, int k, const uint32_t* in_host, uint64_t n, uint32_t skew_mask,
                               uint64_t* out_host, uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || (k > 0 && ((n && !in_host) || !out_host))) return fail(c, RDF_ERR_ARG, "rdf_test_scan_batch: null argument");
    *canaries_ok = 0;
    if (k < 0 || k > RDF_TEST_BATCH_CAP) return fail(c, RDF_ERR_ARG, "rdf_test_scan_batch: k out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int nb = std::max(k, 1);  // (k = 0 still gets one pair of arrays to watch)
    TestArr in[RDF_TEST_BATCH_CAP], out[RDF_TEST_BATCH_CAP];
    const u32* ip[RDF_TEST_BATCH_CAP] = {};
    u64* op[RDF_TEST_BATCH_CAP] = {};
    for (int j = 0; j < nb; ++j) {
        HIP_TRY(c, in[j].make(4, n, (skew_mask >> j) & 1u, st));
        HIP_TRY(c, out[j].make(8, n + 1, (skew_mask >> (4 + j)) & 1u, st));
        if (j < k && n) HIP_TRY(c, hipMemcpyAsync(in[j].data(), in_host + (u64)j * n, n * 4, hipMemcpyHostToDevice, st));
        ip[j] = (const u32*)in[j].data();
        op[j] = (u64*)out[j].data();
    }
    const hipError_t e = exclusive_scan_u32_u64_batch(c->ws, ip, op, k, n, st);
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    for (int j = 0; j < nb; ++j) {
        HIP_TRY(c, check_canaries(in[j], &ok));
        HIP_TRY(c, check_canaries(out[j], &ok));
        if (j < k) HIP_TRY(c, check_contents(in[j], in_host + (u64)j * n, n, &ok));
        if (e != hipSuccess) HIP_TRY(c, check_contents(out[j], nullptr, n + 1, &ok));  // a refused call writes nothing
    }
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "exclusive_scan_u32_u64_batch"));
    for (int j = 0; j < k; ++j)
        HIP_TRY(c, hipMemcpy(out_host + (u64)j * (n + 1), out[j].data(), (n + 1) * 8, hipMemcpyDeviceToHost));
    return RDF_OK;
}

rdf_status rdf_test_radix(rdf_ctx* c, int op, const void* keys_host, uint64_t n, int lo, int hi, uint64_t hmask,
                          void* out_host, uint64_t* n_out, uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || !n_out || (n && (!keys_host || !out_host))) return fail(c, RDF_ERR_ARG, "rdf_test_radix: null argument");
    *canaries_ok = 0;
    *n_out = 0;
    if (op < RDF_TEST_RADIX_SORT_BITS || op > RDF_TEST_RADIX_PART_U32 || n >= (1ull << 32))
        return fail(c, RDF_ERR_ARG, "rdf_test_radix: op or n out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t ksz = op == RDF_TEST_RADIX_PART_U32 ? 4 : 8;
    TestArr a, b, kept;  // the passes write a and b in turn
    HIP_TRY(c, a.make(ksz, n, 0, st));
    HIP_TRY(c, b.make(ksz, n, 0, st));
    HIP_TRY(c, kept.make(4, 1, 0, st));
    if (n) HIP_TRY(c, hipMemcpyAsync(a.data(), keys_host, n * ksz, hipMemcpyHostToDevice, st));
    u64 m = n;
    const char* res = nullptr;
    hipError_t e;
    if (op == RDF_TEST_RADIX_PART_U32) {
        u32 *keys = (u32*)a.data(), *tmp = (u32*)b.data();
        e = radix_partition_u32(c->ws, keys, tmp, n, lo, hi, st);
        res = (const char*)keys;
    } else {
        u64 *keys = (u64*)a.data(), *tmp = (u64*)b.data();
        e = op == RDF_TEST_RADIX_SORT_BITS   ? radix_sort_u64_bits(c->ws, keys, tmp, n, lo, hi, st)
            : op == RDF_TEST_RADIX_SORT_DROP ? radix_sort_u64_drop(c->ws, keys, tmp, n, hi, (u32*)kept.data(), &m, st)
                                             : radix_partition_hashed(c->ws, keys, tmp, n, hi, hmask, st);
        res = (const char*)keys;
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    HIP_TRY(c, check_canaries(a, &ok));
    HIP_TRY(c, check_canaries(b, &ok));
    HIP_TRY(c, check_canaries(kept, &ok));
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "radix primitive"));
    if (m > n) return fail(c, RDF_ERR_HIP, "rdf_test_radix: more keys kept than given");
    if (m) HIP_TRY(c, hipMemcpy(out_host, res, m * ksz, hipMemcpyDeviceToHost));
    *n_out = m;
    return RDF_OK;
}

int rdf_test_radix_passes(int bits) { return radix_sort_passes(bits); }

rdf_status rdf_test_radix_segments(rdf_ctx* c, const uint64_t* src_host, uint64_t src_n, const uint64_t* seg_base,
                                   uint64_t stride, const uint64_t* seg_cnt, uint32_t n_seg, int w0, int bits,
                                   int32_t hist_bump, uint32_t hist_bump_seg, uint32_t hist_bump_digit,
                                   uint64_t* out_host, uint64_t* n_out, uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || !n_out || !seg_cnt || (src_n && !src_host))
        return fail(c, RDF_ERR_ARG, "rdf_test_radix_segments: null argument");
    *canaries_ok = 0;
    *n_out = 0;
    if (w0 == 0) w0 = radix_first_width(bits);
    if (n_seg == 0 || n_seg > (1u << 16) || bits < 1 || bits > 64 || w0 < 1 || w0 > RS_MAX_BITS || w0 > bits ||
        src_n >= (1ull << 32))
        return fail(c, RDF_ERR_ARG, "rdf_test_radix_segments: segments, bits or width out of range");
    if (!seg_layout_ok(src_n, seg_base, stride, seg_cnt, n_seg))
        return fail(c, RDF_ERR_ARG, "rdf_test_radix_segments: a segment leaves the keys or overlaps another");
    std::vector<u32> hh;
    const u64 total = seg_host_histogram(src_host, seg_base, stride, seg_cnt, n_seg, w0, hh);
    if (total && !out_host) return fail(c, RDF_ERR_ARG, "rdf_test_radix_segments: null argument");
    if (hist_bump) {
        if (hist_bump_seg >= n_seg || hist_bump_digit >= (1u << w0))
            return fail(c, RDF_ERR_ARG, "rdf_test_radix_segments: the changed histogram entry is out of range");
        hh[(size_t)hist_bump_digit * radix_hist_stride(n_seg) + hist_bump_seg] += (u32)hist_bump;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    TestArr src, a, b, cnt, base, over;  // the first pass reads src and writes a; the later passes write b and a in turn
    HIP_TRY(c, src.make(8, src_n, 0, st));
    HIP_TRY(c, a.make(8, total, 0, st));
    HIP_TRY(c, b.make(8, total, 0, st));
    HIP_TRY(c, cnt.make(8, n_seg, 0, st));
    HIP_TRY(c, base.make(8, n_seg, 0, st));
    HIP_TRY(c, over.make(4, 1, 0, st));
    if (src_n) HIP_TRY(c, hipMemcpyAsync(src.data(), src_host, src_n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(cnt.data(), seg_cnt, n_seg * 8ull, hipMemcpyHostToDevice, st));
    if (seg_base) HIP_TRY(c, hipMemcpyAsync(base.data(), seg_base, n_seg * 8ull, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(over.data(), 0, 4, st));
    u64 *keys = (u64*)a.data(), *tmp = (u64*)b.data();
    hipError_t e = hipSuccess;
    u32* hist = radix_seg_hist(c->ws, n_seg, w0);
    if (!hist) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpyAsync(hist, hh.data(), hh.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = radix_seg_first_pass(c->ws, (const u64*)src.data(), src_n, keys, total, seg_base ? (const u64*)base.data() : nullptr,
                                 stride, (const u64*)cnt.data(), n_seg, w0, hist, (u32*)over.data(), st);
    u32 h_over = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h_over, over.data(), 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && !h_over) e = radix_sort_u64_rest(c->ws, keys, tmp, total, w0, bits, st);
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    HIP_TRY(c, check_canaries(src, &ok));
    HIP_TRY(c, check_contents(src, src_host, src_n, &ok));  // the segments are read only
    HIP_TRY(c, check_canaries(a, &ok));
    HIP_TRY(c, check_canaries(b, &ok));
    HIP_TRY(c, check_canaries(cnt, &ok));
    HIP_TRY(c, check_canaries(base, &ok));
    HIP_TRY(c, check_canaries(over, &ok));
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "radix segment sort"));
    if (h_over) return fail(c, RDF_ERR_LIMIT, "rdf_test_radix_segments: the histogram and the segments' keys disagree");
    if (total) HIP_TRY(c, hipMemcpy(out_host, keys, total * 8, hipMemcpyDeviceToHost));
    *n_out = total;
    return RDF_OK;
}

int rdf_test_record_tile(void) { return (int)KT_TILE; }

rdf_status rdf_test_keep_records(rdf_ctx* c, const uint64_t* keys_host, uint64_t n, int joinbits, uint64_t ncap, uint32_t ms,
                                 uint32_t* support_out, uint64_t* Jf_out, uint32_t* C_out, uint64_t* dk_out, uint64_t* fk_out,
                                 uint64_t* doff_out, uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || !support_out || !Jf_out || !C_out || !doff_out || (n && (!keys_host || !dk_out || !fk_out)))
        return fail(c, RDF_ERR_ARG, "rdf_test_keep_records: null argument");
    *canaries_ok = 0;
    *Jf_out = 0;
    *C_out = 0;
    if (joinbits < 1 || joinbits > 32 || ncap < 1 || ncap >= (1ull << 31) || n >= (1ull << 32) || ms < 1)
        return fail(c, RDF_ERR_ARG, "rdf_test_keep_records: joinbits, ncap, n or ms out of range");
    for (u64 i = 0; i < n; ++i)
        if ((keys_host[i] >> joinbits) >= ncap || (i && keys_host[i] < keys_host[i - 1]))
            return fail(c, RDF_ERR_ARG, "rdf_test_keep_records: the keys are not sorted or name a capture >= ncap");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const unsigned nt = (unsigned)((n + KT_TILE - 1) / KT_TILE);
    TestArr keys, sup, tfresh, tbase, flags, fidx, skip, fcap, info, csup, doff, dk, fk;
    HIP_TRY(c, keys.make(8, n, 0, st));
    HIP_TRY(c, sup.make(4, ncap, 0, st));
    HIP_TRY(c, tfresh.make(4, nt, 0, st));
    HIP_TRY(c, tbase.make(4, nt + 1ull, 0, st));
    HIP_TRY(c, flags.make(4, ncap, 0, st));
    HIP_TRY(c, fidx.make(4, ncap + 1, 0, st));
    HIP_TRY(c, skip.make(4, ncap + 1, 0, st));
    if (n) HIP_TRY(c, hipMemcpyAsync(keys.data(), keys_host, n * 8, hipMemcpyHostToDevice, st));
    const unsigned gc = grid_for(ncap, RDF_BLOCK, kGrid);
    // the counting pass and its scan (g_fresh_bounds)
    HIP_TRY(c, hipMemsetAsync(sup.data(), 0, ncap * 4, st));
    if (nt)
        hipLaunchKernelGGL(k_fresh_bounds, dim3(nt), dim3(RDF_BLOCK), 0, st, (const u64*)keys.data(), n, joinbits,
                           (u32*)tfresh.data(), (u32*)sup.data());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)tfresh.data(), (u32*)tbase.data(), nt, (u32*)tbase.data() + nt, st);
    // the frequent captures' compact ids (g_compact_captures) and the infrequent ones' fresh records before each capture
    hipLaunchKernelGGL(k_support_flags, dim3(gc), dim3(RDF_BLOCK), 0, st, (const u32*)sup.data(), ncap, ms, (u32*)flags.data());
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)flags.data(), (u32*)fidx.data(), ncap, (u32*)fidx.data() + ncap, st);
    hipLaunchKernelGGL(k_skip_counts, dim3(gc), dim3(RDF_BLOCK), 0, st, (const u32*)sup.data(), (const u32*)sup.data(), ncap, ms,
                       (u32*)flags.data());
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)flags.data(), (u32*)skip.data(), ncap, (u32*)skip.data() + ncap, st);
    u32 h[3] = {0, 0, 0};  // fresh records, those of infrequent captures, frequent captures
    if (e == hipSuccess) e = hipMemcpyAsync(&h[0], (u32*)tbase.data() + nt, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h[1], (u32*)skip.data() + ncap, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h[2], (u32*)fidx.data() + ncap, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    TRY(prim_status(c, e, "rdf_test_keep_records (counting pass)"));
    if (h[1] > h[0] || h[0] > n || h[2] > ncap) return fail(c, RDF_ERR_HIP, "rdf_test_keep_records: counts out of range");
    const u64 Jf = h[0] - h[1];
    const u32 C = h[2];
    HIP_TRY(c, fcap.make(4, C, 0, st));
    HIP_TRY(c, info.make(sizeof(CapInfo), C, 0, st));
    HIP_TRY(c, csup.make(4, C, 0, st));
    HIP_TRY(c, doff.make(8, C + 1ull, 0, st));
    HIP_TRY(c, dk.make(8, Jf, 0, st));
    HIP_TRY(c, fk.make(8, Jf, 0, st));
    hipLaunchKernelGGL(k_compact_captures, dim3(gc), dim3(RDF_BLOCK), 0, st, (const u32*)sup.data(), (const u32*)fidx.data(), ncap,
                       ms, (u32*)fcap.data(), (CapInfo*)info.data());
    // the writing pass, and the dependents' offsets from the frequent captures' record counts (g_compact_groups)
    if (nt)
        hipLaunchKernelGGL(k_keep_scatter, dim3(nt), dim3(RDF_BLOCK), 0, st, (const u64*)keys.data(), n, joinbits,
                           (const u32*)tbase.data(), (const u32*)skip.data(), (const u32*)sup.data(), ms, (const u32*)fidx.data(),
                           (u64*)dk.data(), (u64*)fk.data());
    if (C)
        hipLaunchKernelGGL(k_info_support_u32, dim3(grid_for(C, RDF_BLOCK, kGrid)), dim3(RDF_BLOCK), 0, st,
                           (const CapInfo*)info.data(), C, (u32*)csup.data());
    e = hipGetLastError();
    if (e == hipSuccess)
        e = exclusive_scan_u32_u64(c->ws, (const u32*)csup.data(), (u64*)doff.data(), C, (u64*)doff.data() + C, st);
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    for (const TestArr* a : {&keys, &sup, &tfresh, &tbase, &flags, &fidx, &skip, &fcap, &info, &csup, &doff, &dk, &fk})
        HIP_TRY(c, check_canaries(*a, &ok));
    HIP_TRY(c, check_contents(keys, keys_host, n, &ok));  // the records are read only
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "rdf_test_keep_records"));
    HIP_TRY(c, hipMemcpy(support_out, sup.data(), ncap * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(doff_out, doff.data(), (C + 1ull) * 8, hipMemcpyDeviceToHost));
    if (Jf) {
        HIP_TRY(c, hipMemcpy(dk_out, dk.data(), Jf * 8, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(fk_out, fk.data(), Jf * 8, hipMemcpyDeviceToHost));
    }
    *Jf_out = Jf;
    *C_out = C;
    return RDF_OK;
}

rdf_status rdf_test_group_build(rdf_ctx* c, const uint64_t* fk_host, uint64_t n, uint32_t V, uint64_t rbase, uint32_t gbase,
                                uint64_t* G_out, uint64_t* goff_out, uint32_t* gcap_out, uint32_t* gmap_out,
                                uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || !G_out || !goff_out || !gmap_out || (n && (!fk_host || !gcap_out)))
        return fail(c, RDF_ERR_ARG, "rdf_test_group_build: null argument");
    *canaries_ok = 0;
    *G_out = 0;
    if (V < 1 || n >= (1ull << 32) || rbase >= (1ull << 32) || (u64)gbase + n >= (1ull << 32))
        return fail(c, RDF_ERR_ARG, "rdf_test_group_build: V, n, rbase or gbase out of range");
    for (u64 i = 0; i < n; ++i)
        if ((fk_host[i] >> 32) >= V || (i && (fk_host[i] >> 32) < (fk_host[i - 1] >> 32)))
            return fail(c, RDF_ERR_ARG, "rdf_test_group_build: the records are not sorted by join value or name one >= V");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const unsigned nt = (unsigned)((n + KT_TILE - 1) / KT_TILE);
    TestArr fk, theads, tgbase, goff, gcap, gmap;
    HIP_TRY(c, fk.make(8, n, 0, st));
    HIP_TRY(c, theads.make(4, nt, 0, st));
    HIP_TRY(c, tgbase.make(4, nt + 1ull, 0, st));
    HIP_TRY(c, gcap.make(4, rbase + n, 0, st));
    HIP_TRY(c, gmap.make(4, V, 0, st));
    if (n) HIP_TRY(c, hipMemcpyAsync(fk.data(), fk_host, n * 8, hipMemcpyHostToDevice, st));
    if (nt) hipLaunchKernelGGL(k_group_flags, dim3(nt), dim3(RDF_BLOCK), 0, st, (const u64*)fk.data(), n, (u32*)theads.data());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)theads.data(), (u32*)tgbase.data(), nt, (u32*)tgbase.data() + nt, st);
    u32 G = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&G, (u32*)tgbase.data() + nt, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    TRY(prim_status(c, e, "rdf_test_group_build (counting pass)"));
    if (G > n) return fail(c, RDF_ERR_HIP, "rdf_test_group_build: more groups than records");
    HIP_TRY(c, goff.make(8, (u64)gbase + G + 1, 0, st));
    if (nt) {
        if (rbase || gbase)
            hipLaunchKernelGGL(k_group_build_at, dim3(nt), dim3(RDF_BLOCK), 0, st, (const u64*)fk.data(), n,
                               (const u32*)tgbase.data(), rbase, gbase, (u64*)goff.data(), (u32*)gcap.data(), (u32*)gmap.data());
        else
            hipLaunchKernelGGL(k_group_build, dim3(nt), dim3(RDF_BLOCK), 0, st, (const u64*)fk.data(), n,
                               (const u32*)tgbase.data(), (u64*)goff.data(), (u32*)gcap.data(), (u32*)gmap.data());
    }
    e = hipGetLastError();
    const u64 end = rbase + n;  // the end of the last group: the caller's to write, as in the pipeline
    HIP_TRY(c, hipMemcpyAsync((u64*)goff.data() + gbase + G, &end, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    for (const TestArr* a : {&fk, &theads, &tgbase, &goff, &gcap, &gmap}) HIP_TRY(c, check_canaries(*a, &ok));
    HIP_TRY(c, check_contents(fk, fk_host, n, &ok));      // the records are read only
    HIP_TRY(c, check_contents(gcap, nullptr, rbase, &ok));  // nothing before the range's records ...
    HIP_TRY(c, check_contents(goff, nullptr, gbase, &ok));  // ... or before its groups is written
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "rdf_test_group_build"));
    HIP_TRY(c, hipMemcpy(goff_out, (u64*)goff.data() + gbase, (G + 1ull) * 8, hipMemcpyDeviceToHost));
    if (n) HIP_TRY(c, hipMemcpy(gcap_out, (u32*)gcap.data() + rbase, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(gmap_out, gmap.data(), (u64)V * 4, hipMemcpyDeviceToHost));
    *G_out = G;
    return RDF_OK;
}

rdf_status rdf_test_radix_pairs(rdf_ctx* c, const uint32_t* keys_host, const uint32_t* vals_host, uint64_t n, int lo, int hi,
                                uint32_t* keys_out, uint32_t* vals_out, uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || (n && (!keys_host || !vals_host || !keys_out || !vals_out)))
        return fail(c, RDF_ERR_ARG, "rdf_test_radix_pairs: null argument");
    *canaries_ok = 0;
    if (n >= (1ull << 32) || lo < 0 || hi > 32 || hi < lo) return fail(c, RDF_ERR_ARG, "rdf_test_radix_pairs: n or bits out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    TestArr ki, vi, ko, vo, kt, vt;
    for (TestArr* a : {&ki, &vi, &ko, &vo, &kt, &vt}) HIP_TRY(c, a->make(4, n, 0, st));
    if (n) {
        HIP_TRY(c, hipMemcpyAsync(ki.data(), keys_host, n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(vi.data(), vals_host, n * 4, hipMemcpyHostToDevice, st));
    }
    const hipError_t e = radix_sort_pairs_u32(c->ws, (const u32*)ki.data(), (const u32*)vi.data(), (u32*)ko.data(),
                                              (u32*)vo.data(), (u32*)kt.data(), (u32*)vt.data(), n, lo, hi, st);
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    for (const TestArr* a : {&ki, &vi, &ko, &vo, &kt, &vt}) HIP_TRY(c, check_canaries(*a, &ok));
    HIP_TRY(c, check_contents(ki, keys_host, n, &ok));  // the input is read only
    HIP_TRY(c, check_contents(vi, vals_host, n, &ok));
    if (n < 2 || radix_sort_passes(hi - lo) <= 1) {  // no pass or a single one: straight into the output
        HIP_TRY(c, check_contents(kt, nullptr, n, &ok));
        HIP_TRY(c, check_contents(vt, nullptr, n, &ok));
    }
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "radix_sort_pairs_u32"));
    if (n) {
        HIP_TRY(c, hipMemcpy(keys_out, ko.data(), n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(vals_out, vo.data(), n * 4, hipMemcpyDeviceToHost));
    }
    return RDF_OK;
}

rdf_status rdf_test_group_kv(rdf_ctx* c, const uint64_t* keys_host, uint64_t n, int joinbits, uint64_t ncap, uint32_t ms,
                             uint32_t V, uint32_t* support_out, uint64_t* Jf_out, uint32_t* C_out, uint64_t* doff_out,
                             uint32_t* dgrp_out, uint64_t* G_out, uint64_t* goff_out, uint32_t* gcap_out, uint32_t* gmap_out,
                             uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || !support_out || !Jf_out || !C_out || !doff_out || !G_out || !goff_out || !gmap_out ||
        (n && (!keys_host || !dgrp_out || !gcap_out)))
        return fail(c, RDF_ERR_ARG, "rdf_test_group_kv: null argument");
    *canaries_ok = 0;
    *Jf_out = *G_out = 0;
    *C_out = 0;
    if (joinbits < 1 || joinbits > 32 || ncap < 1 || ncap >= (1ull << 31) || n >= (1ull << 32) || ms < 1 || V < 1 ||
        (u64)V > (1ull << joinbits))
        return fail(c, RDF_ERR_ARG, "rdf_test_group_kv: joinbits, ncap, n, ms or V out of range");
    const u64 jm = (1ull << joinbits) - 1;
    for (u64 i = 0; i < n; ++i)
        if ((keys_host[i] >> joinbits) >= ncap || (keys_host[i] & jm) >= V || (i && keys_host[i] < keys_host[i - 1]))
            return fail(c, RDF_ERR_ARG, "rdf_test_group_kv: the keys are not sorted or name a capture >= ncap or a join >= V");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const unsigned nt = (unsigned)((n + KT_TILE - 1) / KT_TILE);
    TestArr keys, sup, tfresh, tbase, flags, fidx, skip, fcap, info, csup, doff;
    HIP_TRY(c, keys.make(8, n, 0, st));
    HIP_TRY(c, sup.make(4, ncap, 0, st));
    HIP_TRY(c, tfresh.make(4, nt, 0, st));
    HIP_TRY(c, tbase.make(4, nt + 1ull, 0, st));
    HIP_TRY(c, flags.make(4, ncap, 0, st));
    HIP_TRY(c, fidx.make(4, ncap + 1, 0, st));
    HIP_TRY(c, skip.make(4, ncap + 1, 0, st));
    if (n) HIP_TRY(c, hipMemcpyAsync(keys.data(), keys_host, n * 8, hipMemcpyHostToDevice, st));
    const unsigned gc = grid_for(ncap, RDF_BLOCK, kGrid);
    // the counting pass, the frequent captures' compact ids and the skip counts, as rdf_test_keep_records runs them
    HIP_TRY(c, hipMemsetAsync(sup.data(), 0, ncap * 4, st));
    if (nt)
        hipLaunchKernelGGL(k_fresh_bounds, dim3(nt), dim3(RDF_BLOCK), 0, st, (const u64*)keys.data(), n, joinbits,
                           (u32*)tfresh.data(), (u32*)sup.data());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)tfresh.data(), (u32*)tbase.data(), nt, (u32*)tbase.data() + nt, st);
    hipLaunchKernelGGL(k_support_flags, dim3(gc), dim3(RDF_BLOCK), 0, st, (const u32*)sup.data(), ncap, ms, (u32*)flags.data());
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)flags.data(), (u32*)fidx.data(), ncap, (u32*)fidx.data() + ncap, st);
    hipLaunchKernelGGL(k_skip_counts, dim3(gc), dim3(RDF_BLOCK), 0, st, (const u32*)sup.data(), (const u32*)sup.data(), ncap, ms,
                       (u32*)flags.data());
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)flags.data(), (u32*)skip.data(), ncap, (u32*)skip.data() + ncap, st);
    u32 h[3] = {0, 0, 0};  // fresh records, those of infrequent captures, frequent captures
    if (e == hipSuccess) e = hipMemcpyAsync(&h[0], (u32*)tbase.data() + nt, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h[1], (u32*)skip.data() + ncap, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h[2], (u32*)fidx.data() + ncap, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    TRY(prim_status(c, e, "rdf_test_group_kv (counting pass)"));
    if (h[1] > h[0] || h[0] > n || h[2] > ncap) return fail(c, RDF_ERR_HIP, "rdf_test_group_kv: counts out of range");
    const u64 Jf = h[0] - h[1];
    const u32 C = h[2];
    const unsigned ng = (unsigned)((Jf + KT_TILE - 1) / KT_TILE);
    TestArr joins, caps, kt, vt, dgrp, gcap, theads, tgbase, goff, gmap;
    HIP_TRY(c, fcap.make(4, C, 0, st));
    HIP_TRY(c, info.make(sizeof(CapInfo), C, 0, st));
    HIP_TRY(c, csup.make(4, C, 0, st));
    HIP_TRY(c, doff.make(8, C + 1ull, 0, st));
    for (TestArr* a : {&joins, &caps, &kt, &vt, &dgrp, &gcap}) HIP_TRY(c, a->make(4, Jf, 0, st));
    HIP_TRY(c, theads.make(4, ng, 0, st));
    HIP_TRY(c, tgbase.make(4, ng + 1ull, 0, st));
    HIP_TRY(c, gmap.make(4, V, 0, st));
    hipLaunchKernelGGL(k_compact_captures, dim3(gc), dim3(RDF_BLOCK), 0, st, (const u32*)sup.data(), (const u32*)fidx.data(), ncap,
                       ms, (u32*)fcap.data(), (CapInfo*)info.data());
    if (nt)
        hipLaunchKernelGGL(k_keep_scatter_kv, dim3(nt), dim3(RDF_BLOCK), 0, st, (const u64*)keys.data(), n, joinbits,
                           (const u32*)tbase.data(), (const u32*)skip.data(), (const u32*)sup.data(), ms, (const u32*)fidx.data(),
                           (u32*)joins.data(), (u32*)caps.data());
    if (C)
        hipLaunchKernelGGL(k_info_support_u32, dim3(grid_for(C, RDF_BLOCK, kGrid)), dim3(RDF_BLOCK), 0, st,
                           (const CapInfo*)info.data(), C, (u32*)csup.data());
    e = hipGetLastError();
    if (e == hipSuccess)
        e = exclusive_scan_u32_u64(c->ws, (const u32*)csup.data(), (u64*)doff.data(), C, (u64*)doff.data() + C, st);
    // the pair sort (the sorted joins into dgrp, the sorted captures into gcap) and the group passes (g_compact_groups)
    if (e == hipSuccess)
        e = radix_sort_pairs_u32(c->ws, (const u32*)joins.data(), (const u32*)caps.data(), (u32*)dgrp.data(), (u32*)gcap.data(),
                                 (u32*)kt.data(), (u32*)vt.data(), Jf, 0, joinbits, st);
    if (ng) hipLaunchKernelGGL(k_group_flags_kv, dim3(ng), dim3(RDF_BLOCK), 0, st, (const u32*)dgrp.data(), Jf, (u32*)theads.data());
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess)
        e = exclusive_scan_u32(c->ws, (const u32*)theads.data(), (u32*)tgbase.data(), ng, (u32*)tgbase.data() + ng, st);
    u32 G = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&G, (u32*)tgbase.data() + ng, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    TRY(prim_status(c, e, "rdf_test_group_kv (group heads)"));
    if (G > Jf) return fail(c, RDF_ERR_HIP, "rdf_test_group_kv: more groups than records");
    HIP_TRY(c, goff.make(8, G + 1ull, 0, st));
    if (ng) {
        hipLaunchKernelGGL(k_group_build_kv, dim3(ng), dim3(RDF_BLOCK), 0, st, (const u32*)dgrp.data(), Jf,
                           (const u32*)tgbase.data(), (u64*)goff.data(), (u32*)gmap.data());
        hipLaunchKernelGGL(k_dgrp_kv, dim3(grid_for(Jf, RDF_BLOCK, kGrid)), dim3(RDF_BLOCK), 0, st, (const u32*)joins.data(), Jf,
                           (const u32*)gmap.data(), (u32*)dgrp.data());
    }
    e = hipGetLastError();
    HIP_TRY(c, hipMemcpyAsync((u64*)goff.data() + G, &Jf, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    for (const TestArr* a : {&keys, &sup, &tfresh, &tbase, &flags, &fidx, &skip, &fcap, &info, &csup, &doff, &joins, &caps, &kt,
                             &vt, &dgrp, &gcap, &theads, &tgbase, &goff, &gmap})
        HIP_TRY(c, check_canaries(*a, &ok));
    HIP_TRY(c, check_contents(keys, keys_host, n, &ok));  // the records are read only
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "rdf_test_group_kv"));
    HIP_TRY(c, hipMemcpy(support_out, sup.data(), ncap * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(doff_out, doff.data(), (C + 1ull) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(goff_out, goff.data(), (G + 1ull) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(gmap_out, gmap.data(), (u64)V * 4, hipMemcpyDeviceToHost));
    if (Jf) {
        HIP_TRY(c, hipMemcpy(dgrp_out, dgrp.data(), Jf * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(gcap_out, gcap.data(), Jf * 4, hipMemcpyDeviceToHost));
    }
    *Jf_out = Jf;
    *C_out = C;
    *G_out = G;
    return RDF_OK;
}

rdf_status rdf_test_paths(rdf_ctx* c, rdf_test_path_report* out) {
    if (!c || !out) return RDF_ERR_ARG;
    if (c->stage < 4) return fail(c, RDF_ERR_STATE, "no completed run");
    rdf_test_path_report r = {};
    r.k1_form = c->path_k1;
    r.k2_form = c->path_k2;
    r.k3_form = c->path_k3;
    r.dense_on = c->dense_on ? 1 : 0;
    r.light_stage = c->light_stage ? 1 : 0;
    r.light_hiocc = c->light_hiocc ? 1 : 0;
    r.n_dense = c->n_dense;
    r.n_dense_eligible = c->n_dense_eligible;
    r.n_dedup_members = c->n_dedup_members;
    r.n_light_items = c->lpaths.items;
    r.n_packed_octets = c->lpaths.packed_octets;
    r.n_mseg_chunks = c->lpaths.mseg_chunks;
    r.n_multi_items = c->n_multi_items;
    r.n_light_survivors = c->n_light_survivors;
    r.light_npx = (uint32_t)c->lpaths.light_npx;
    r.packed_npx = (uint32_t)c->lpaths.packed_npx;
    r.light_ordered = c->lpaths.ordered ? 1 : 0;
    r.light_side = c->lpaths.side ? 1 : 0;
    r.light_two_pass = c->lpaths.two_pass ? 1 : 0;
    r.sig_on = c->sig_on ? 1 : 0;
    r.piv2_on = c->piv2_on ? 1 : 0;
    r.k3_hist = c->k3_hist ? 1 : 0;
    r.k3_key_items = c->k3_key_items;
    r.k3_suppressed = c->k3_suppressed;
    r.group_form = c->path_group_kv;
    r.hclassed = c->hclassed ? 1 : 0;
    r.n_emit_tiles = c->pend_NT;
    // the class lists as the run left them: class m's is lists[lwoff[cchoff[m]], lwoff[cchoff[m + 1]]).  n_classes and
    // pend_NT belong to the last discovery because every discovery path sets both (d_classes_single / the sharded class
    // phases, and d_emit_rest), also to 0; stage >= 4 (above) says that such a run completed and rdf_release_scratch has
    // not freed its buffers since.  The capacities are checked so that a stale count can never read past a buffer.
    const u64 ncls = c->nranks == 1 ? c->n_classes : 0;
    if (ncls && (u64)c->cchoff.cap >= (ncls + 1) * 8) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<u64> ch(ncls + 1);
        HIP_TRY(c, hipMemcpy(ch.data(), c->cchoff.p, (ncls + 1) * 8, hipMemcpyDeviceToHost));
        const u64 WC = ch[ncls];
        if ((u64)c->lwoff.cap < (WC + 1) * 8) return fail(c, RDF_ERR_STATE, "rdf_test_paths: the class lists are gone");
        std::vector<u64> lw(WC + 1);
        HIP_TRY(c, hipMemcpy(lw.data(), c->lwoff.p, (WC + 1) * 8, hipMemcpyDeviceToHost));
        r.n_class_chunks = WC;
        for (u64 m = 0; m < ncls; ++m) {
            const u64 len = lw[ch[m + 1]] - lw[ch[m]];
            r.max_class_list = std::max<u64>(r.max_class_list, len);
            r.n_multi_seg_lists += len > CLS_LS;
        }
    }
    *out = r;
    return RDF_OK;
}

rdf_status rdf_test_shard_report(rdf_ctx* c, rdf_test_shard_report_t* out) {
    if (!c || !out) return RDF_ERR_ARG;
    if (!c->shrep_done || c->sh_phase != 9 || c->stage < 4)
        return fail(c, RDF_ERR_STATE, "rdf_test_shard_report: no completed sharded run");
    rdf_test_shard_report_t r = c->shrep;
    // the verify offsets as sh_phase15 left them: vcoff[0, C] of that run's C (shrep_vC says nothing has written the
    // buffer since; the capacity is checked so that a released buffer is never read)
    const u64 C = c->shrep_vC;
    if (C != ~0ull && C == c->C && (u64)c->vcoff.cap >= (C + 1) * 8) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<u64> off(C + 1);
        HIP_TRY(c, hipMemcpy(off.data(), c->vcoff.p, (C + 1) * 8, hipMemcpyDeviceToHost));
        for (u64 d = 0; d < C; ++d) r.max_verify_per_dep = std::max<u64>(r.max_verify_per_dep, off[d + 1] - off[d]);
        r.have_max_verify = 1;
    }
    *out = r;
    return RDF_OK;
}

rdf_status rdf_test_fc_trace(rdf_ctx* c, int on) {
    if (!c) return RDF_ERR_ARG;
    c->fc_trace = on != 0;
    return RDF_OK;
}

rdf_status rdf_test_fc_report(rdf_ctx* c, rdf_test_fc_report_t* out) {
    if (!c || !out) return RDF_ERR_ARG;
    if (c->stage < 2) return fail(c, RDF_ERR_STATE, "rdf_test_fc_report: rdf_frequent_conditions must be called first");
    *out = c->fcrep;
    out->k1_form = c->path_k1;
    out->k2_form = c->path_k2;
    return RDF_OK;
}

rdf_status rdf_test_copy_frequent_unary(rdf_ctx* c, uint32_t* fval_host, uint64_t cap, uint64_t* U_out, uint64_t* n3) {
    if (!c) return RDF_ERR_ARG;
    if (!U_out || !n3 || (cap && !fval_host)) return fail(c, RDF_ERR_ARG, "rdf_test_copy_frequent_unary: null argument");
    TRY(fc_state(c, "rdf_test_copy_frequent_unary"));
    *U_out = c->U;
    for (int t = 0; t < 3; ++t) n3[t] = c->fstats.n_frequent_unary[t];
    if (cap < c->U) return fail(c, RDF_ERR_ARG, "rdf_test_copy_frequent_unary: fval_host holds fewer than U values");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->U) HIP_TRY(c, ctx_copy(c, fval_host, c->fval.p, (size_t)c->U * 4, hipMemcpyDeviceToHost));
    return RDF_OK;
}

rdf_status rdf_test_unary_lookup(rdf_ctx* c, const uint64_t* keys, uint64_t n, uint32_t* rank_out, uint32_t* bit_out,
                                 uint32_t* canaries_ok) {
    if (!c) return RDF_ERR_ARG;
    if (!canaries_ok || (n && (!keys || !rank_out || !bit_out)))
        return fail(c, RDF_ERR_ARG, "rdf_test_unary_lookup: null argument");
    *canaries_ok = 0;
    TRY(fc_state(c, "rdf_test_unary_lookup"));
    const u64 K = 3ull * (c->V ? c->V : 1);
    for (u64 i = 0; i < n; ++i)
        if (keys[i] >= K) return fail(c, RDF_ERR_ARG, "rdf_test_unary_lookup: a key is not below 3V");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    TestArr dk, dr, db;
    HIP_TRY(c, dk.make(8, n, 0, st));
    HIP_TRY(c, dr.make(4, n, 0, st));
    HIP_TRY(c, db.make(4, n, 0, st));
    if (n) {
        HIP_TRY(c, hipMemcpyAsync(dk.data(), keys, n * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_test_unary_lookup, dim3(grid_for(n, RDF_BLOCK, kGrid)), dim3(RDF_BLOCK), 0, st,
                           (const u64*)dk.data(), n, c->frank.as<u32>(), c->fbits.as<u64>(), (u32*)dr.data(),
                           (u32*)db.data());
    }
    const hipError_t e = n ? hipGetLastError() : hipSuccess;
    HIP_TRY(c, hipStreamSynchronize(st));
    bool ok = true;
    HIP_TRY(c, check_canaries(dk, &ok));
    HIP_TRY(c, check_contents(dk, keys, n, &ok));  // the keys are read only
    HIP_TRY(c, check_canaries(dr, &ok));
    HIP_TRY(c, check_canaries(db, &ok));
    *canaries_ok = ok ? 1 : 0;
    TRY(prim_status(c, e, "k_test_unary_lookup"));
    if (n) {
        HIP_TRY(c, hipMemcpy(rank_out, dr.data(), n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(bit_out, db.data(), n * 4, hipMemcpyDeviceToHost));
    }
    return RDF_OK;
}

rdf_status rdf_test_rewrite_form(rdf_ctx* c, uint32_t* form) {
    if (!c || !form) return RDF_ERR_ARG;
    *form = c->rw_form;
    return RDF_OK;
}

rdf_status rdf_test_cind_stats_times(rdf_ctx* c, float* ms3) {
    if (!c || !ms3) return RDF_ERR_ARG;
    for (int i = 0; i < 3; ++i) ms3[i] = c->cs_ms[i];
    return RDF_OK;
}

}  // extern "C"
