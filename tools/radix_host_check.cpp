// Stand-alone check of rdfind_amd/csrc/radix_host.hpp (the radix sort's pass and width arithmetic, the histogram layout and
// the host histogram of keys in segments), meant to run under the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/radix_host_check.cpp -o radix_host_check
// Exit status 0: every check held.  tests/test_radix_host.py builds and runs it that way.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "../rdfind_amd/csrc/radix_host.hpp"

using namespace rdf;

static int failures = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            ++failures;                                            \
        }                                                          \
    } while (0)

static void widths() {
    for (int dmax = 8; dmax <= 10; ++dmax)
        for (int bits = 0; bits <= 64; ++bits) {
            const int passes = radix_passes_for(bits, dmax);
            CHECK(passes == (bits + dmax - 1) / dmax);
            int sum = 0, prev = dmax;
            for (int p = 0; p < passes; ++p) {
                const int w = radix_pass_width(bits, dmax, p);
                CHECK(w >= 1 && w <= dmax && w <= prev);  // the wider digits first
                prev = w;
                sum += w;
            }
            CHECK(sum == bits);
            CHECK(radix_pass_width(bits, dmax, passes) == 0 && radix_pass_width(bits, dmax, -1) == 0);
        }
    const int want[5] = {9, 9, 9, 8, 8};  // the flagship's 43-bit records
    for (int p = 0; p < 5; ++p) CHECK(radix_pass_width(43, 9, p) == want[p]);
    CHECK(radix_passes_for(43, 9) == 5 && radix_passes_for(17, 9) == 2 && radix_pass_width(17, 9, 0) == 9);
    for (uint32_t c = 0; c < 70; ++c) CHECK(radix_hist_stride(c) >= c && radix_hist_stride(c) % 4 == 0 && radix_hist_stride(c) < c + 4);
}

static void histograms() {
    std::mt19937_64 rng(12345);
    const uint64_t lens[][6] = {{0, 1, 4095, 4096, 4097, 3 * 4096 + 5}, {7, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
    for (const auto& len : lens)
        for (int n_seg : {1, 3, 5, 6})
            for (int w : {1, 8, 9, 10})
                for (int strided = 0; strided < 2; ++strided) {
                    std::vector<uint64_t> cnt(len, len + n_seg), base(n_seg);
                    const uint64_t stride = *std::max_element(cnt.begin(), cnt.end()) + 3;
                    uint64_t at = 2;
                    for (int b = 0; b < n_seg; ++b) {
                        base[b] = strided ? (uint64_t)b * stride : at;
                        at += cnt[b] + 1 + rng() % 9;
                    }
                    const uint64_t src_n = strided ? stride * n_seg : at;
                    std::vector<uint64_t> src(src_n);
                    for (auto& k : src) k = rng();
                    const uint64_t* bp = strided ? nullptr : base.data();
                    CHECK(seg_layout_ok(src_n, bp, stride, cnt.data(), (uint32_t)n_seg));
                    std::vector<uint32_t> hist;
                    const uint64_t total = seg_host_histogram(src.data(), bp, stride, cnt.data(), (uint32_t)n_seg, w, hist);
                    CHECK(total == std::accumulate(cnt.begin(), cnt.end(), (uint64_t)0));
                    const uint32_t rs = radix_hist_stride((uint32_t)n_seg);
                    CHECK(hist.size() == ((size_t)rs << w));
                    for (int b = 0; b < (int)rs; ++b) {  // every column sums to its segment's length, the padding to 0
                        uint64_t col = 0;
                        for (size_t d = 0; d < ((size_t)1 << w); ++d) col += hist[d * rs + b];
                        CHECK(col == (b < n_seg ? cnt[b] : 0));
                    }
                    // one digit recounted by hand
                    const uint64_t d0 = src[base[n_seg - 1]] & ((1ull << w) - 1);
                    uint32_t by_hand = 0;
                    for (uint64_t i = 0; i < cnt[n_seg - 1]; ++i) by_hand += (src[base[n_seg - 1] + i] & ((1ull << w) - 1)) == d0;
                    if (cnt[n_seg - 1]) CHECK(hist[d0 * rs + (n_seg - 1)] == by_hand);
                }
    // layouts that must be refused: past the end, overlapping, a count that would wrap the bound
    const uint64_t c2[2] = {60, 60}, b2[2] = {0, 50}, c1[1] = {10}, b1[1] = {95}, cw[1] = {~0ull}, bw[1] = {1};
    CHECK(!seg_layout_ok(100, b2, 0, c2, 2));
    CHECK(!seg_layout_ok(100, b1, 0, c1, 1));
    CHECK(!seg_layout_ok(100, bw, 0, cw, 1));
    CHECK(!seg_layout_ok(100, nullptr, 50, c2, 2));
    CHECK(seg_layout_ok(120, nullptr, 60, c2, 2));
    const uint64_t ce[2] = {0, 100}, be[2] = {100, 0};  // an empty segment may sit at the very end
    CHECK(seg_layout_ok(100, be, 0, ce, 2));
}

int main() {
    widths();
    histograms();
    if (failures) {
        std::fprintf(stderr, "radix_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::puts("radix_host_check ok");
    return 0;
}
