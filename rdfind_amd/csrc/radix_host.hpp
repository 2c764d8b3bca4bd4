// Host-side arithmetic of the radix sort (pass count, digit widths, histogram layout) and the host histogram of keys
// that lie in segments.  Plain C++ without HIP: primitives.hip and the test ABI use it, and tools/radix_host_check.cpp
// runs it alone under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace rdf {

// passes of a sort of `bits` key bits with digits of at most dmax bits
inline int radix_passes_for(int bits, int dmax) { return bits > 0 && dmax > 0 ? (bits + dmax - 1) / dmax : 0; }
// width of pass p (0-based): as even as possible, the wider digits first (43 bits, dmax 9: 9+9+9+8+8)
inline int radix_pass_width(int bits, int dmax, int p) {
    const int passes = radix_passes_for(bits, dmax);
    if (p < 0 || p >= passes) return 0;
    return bits / passes + (p < bits % passes ? 1 : 0);
}
// the digit-major histogram's row stride for `columns` tiles or segments: rows stay 16-byte aligned
inline uint32_t radix_hist_stride(uint32_t columns) { return (columns + 3u) & ~3u; }

// Segment b: cnt[b] keys from base[b] (base null: from b * stride).  True when every segment lies inside [0, src_n) and
// no two overlap (empty segments may lie anywhere inside).
inline bool seg_layout_ok(uint64_t src_n, const uint64_t* base, uint64_t stride, const uint64_t* cnt, uint32_t n_seg) {
    std::vector<std::pair<uint64_t, uint64_t>> iv;  // [begin, end) of the non-empty segments
    for (uint32_t b = 0; b < n_seg; ++b) {
        const uint64_t lo = base ? base[b] : (uint64_t)b * stride;
        if (cnt[b] > src_n || lo > src_n - cnt[b]) return false;
        if (cnt[b]) iv.emplace_back(lo, lo + cnt[b]);
    }
    for (size_t i = 0; i < iv.size(); ++i)
        for (size_t j = i + 1; j < iv.size(); ++j)
            if (iv[i].first < iv[j].second && iv[j].first < iv[i].second) return false;
    return true;
}

// hist[d * radix_hist_stride(n_seg) + b] = segment b's keys whose low w bits are d (w in 1..16); the padding columns
// are 0.  The layout must have passed seg_layout_ok.  Returns the keys' number.
inline uint64_t seg_host_histogram(const uint64_t* src, const uint64_t* base, uint64_t stride, const uint64_t* cnt,
                                   uint32_t n_seg, int w, std::vector<uint32_t>& hist) {
    const uint32_t rs = radix_hist_stride(n_seg);
    const uint64_t dmask = (1ull << w) - 1ull;
    hist.assign((size_t)rs << w, 0u);
    uint64_t total = 0;
    for (uint32_t b = 0; b < n_seg; ++b) {
        const uint64_t lo = base ? base[b] : (uint64_t)b * stride;
        for (uint64_t i = 0; i < cnt[b]; ++i) ++hist[(size_t)(src[lo + i] & dmask) * rs + b];
        total += cnt[b];
    }
    return total;
}

}  // namespace rdf
