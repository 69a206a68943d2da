// bundles_pass.h with the blob count of a stripe bundle against the formulas written out here once more: a bundle stages its table row
// and its indices once and its values and its witness n_blobs times; roots and bad are per (stripe, blob) cell, the status words per
// (bundle, blob), the gather table per stripe.  Blob counts 1, 3, 16 and 256; the factor 1 must reproduce the plan without a factor
// field by field.  Stand-alone (UBSan: tests/test_stripe_bundles_sanitizers.py); prints OK.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "bundles_pass.h"

using namespace frieda;

static long checks = 0;
static uint32_t g_log_cell;
static size_t g_budget, g_n, g_blobs;
#define EXPECT(cond)                                                                                        \
    do {                                                                                                    \
        checks++;                                                                                           \
        if (!(cond)) {                                                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                        \
            printf("  log_cell %u bundles %zu budget %zu blobs %zu\n", g_log_cell, g_n, g_budget, g_blobs); \
            exit(1);                                                                                        \
        }                                                                                                   \
    } while (0)

static size_t al(size_t b) { return (b + 255) / 256 * 256; }
// table row + indices, once; values + witness, once per blob (hashes are counted per blob)
static size_t staged(uint32_t c, size_t stripes, size_t hashes, size_t k) { return 12 + 4 * stripes + k * ((((size_t)16) << c) * stripes + 32 * hashes); }

static bool same_plan(const BundlesPassPlan& a, const BundlesPassPlan& b) {
    return a.i_idx == b.i_idx && a.i_tab == b.i_tab && a.i_val == b.i_val && a.i_wit == b.i_wit && a.in_bytes == b.in_bytes && a.res_bytes == b.res_bytes &&
           a.p_res == b.p_res && a.p_tab == b.p_tab && a.pinned == b.pinned && a.a_in == b.a_in && a.a_roots == b.a_roots && a.a_bad == b.a_bad &&
           a.a_res == b.a_res && a.a_tab == b.a_tab && a.arena == b.arena;
}

static void check_plan(uint32_t c, const BundlesPassCount& n, size_t k, const BundlesPassPlan* call) {
    const BundlesPassPlan p = bundles_pass_plan(c, n, k);
    size_t at = 0;
    EXPECT(p.i_idx == at);
    at += al(4 * n.cells);  // the indices: once, whatever k is
    EXPECT(p.i_tab == at);
    at += al(12 * n.bundles);
    EXPECT(p.i_val == at);
    at += al((((size_t)16) << c) * n.cells * k);
    EXPECT(p.i_wit == at);
    at += al(32 * n.hashes * k);
    EXPECT(p.in_bytes == at);
    EXPECT(p.i_tab % 256 == 0 && p.i_val % 256 == 0 && p.i_wit % 256 == 0 && p.in_bytes % 256 == 0);
    if (n.hashes == 0) EXPECT(p.in_bytes == p.i_wit);  // an empty witness
    EXPECT(p.res_bytes == 4 * n.bundles * k);          // a status word per (bundle, blob)
    EXPECT(p.p_res == p.in_bytes && p.p_tab == p.in_bytes + al(4 * n.bundles * k));
    EXPECT(p.pinned == p.p_tab + 8 * n.cells);  // a gather row per stripe at the most
    at = 0;
    EXPECT(p.a_in == at);
    at += al(p.in_bytes);
    EXPECT(p.a_roots == at);
    at += al(32 * n.cells * k);
    EXPECT(p.a_bad == at);
    at += al(4 * n.cells * k);
    EXPECT(p.a_res == at);
    at += al(4 * n.bundles * k);
    EXPECT(p.a_tab == at);
    at += al(8 * n.cells);
    EXPECT(p.arena == at);
    if (call) EXPECT(p.arena <= call->arena && p.pinned <= call->pinned);
    if (k == 1) EXPECT(same_plan(p, bundles_pass_plan(c, n)));  // today's plan
}

// a whole call: the passes partition the bundles, none straddles, every pass but a lone oversized bundle is within the budget and could
// not have taken the next bundle, every pass fits the call's one plan
static void walk(uint32_t c, const std::vector<BundleSize>& sz, size_t budget, size_t k) {
    g_log_cell = c, g_budget = budget, g_n = sz.size(), g_blobs = k;
    const BundlesPassCount top = bundles_call_count(c, sz.data(), sz.size(), budget, k);
    const BundlesPassPlan call = bundles_pass_plan(c, top, k);
    size_t first = 0, passes = 0, seen_cells = 0, seen_hashes = 0;
    BundlesPassCount mx;
    while (first < sz.size()) {
        const size_t end = bundles_pass_end(c, sz.data(), sz.size(), first, budget, k);
        EXPECT(end > first && end <= sz.size());  // one bundle is always admitted
        if (k == 1) EXPECT(end == bundles_pass_end(c, sz.data(), sz.size(), first, budget));
        size_t sum = 0, cells = 0, hashes = 0;
        uint32_t biggest = 0;
        for (size_t b = first; b < end; b++) {
            EXPECT(bundle_staged_bytes(c, sz[b], k) == staged(c, sz[b].cells, sz[b].hashes, k));
            if (k == 1) EXPECT(bundle_staged_bytes(c, sz[b]) == staged(c, sz[b].cells, sz[b].hashes, 1));
            sum += staged(c, sz[b].cells, sz[b].hashes, k), cells += sz[b].cells, hashes += sz[b].hashes, biggest = std::max(biggest, sz[b].cells);
        }
        EXPECT(end == first + 1 || sum <= budget);
        if (end < sz.size()) EXPECT(sum + staged(c, sz[end].cells, sz[end].hashes, k) > budget);  // (greedy: the next one did not fit)
        const BundlesPassCount n = bundles_pass_count(sz.data(), first, end);
        EXPECT(n.cells == cells && n.hashes == hashes && n.bundles == end - first && n.max_cells == biggest);
        check_plan(c, n, k, &call);
        mx.cells = std::max(mx.cells, cells), mx.hashes = std::max(mx.hashes, hashes), mx.bundles = std::max(mx.bundles, end - first);
        mx.max_cells = std::max(mx.max_cells, biggest);
        seen_cells += cells, seen_hashes += hashes, first = end, passes++;
    }
    EXPECT(first == sz.size());
    size_t all_cells = 0, all_hashes = 0;
    for (const BundleSize& z : sz) all_cells += z.cells, all_hashes += z.hashes;
    EXPECT(seen_cells == all_cells && seen_hashes == all_hashes);
    EXPECT(top.cells == mx.cells && top.hashes == mx.hashes && top.bundles == mx.bundles && top.max_cells == mx.max_cells);
    if (budget == 1) EXPECT(passes == sz.size());
    if (k == 1) {
        const BundlesPassCount old = bundles_call_count(c, sz.data(), sz.size(), budget);
        EXPECT(old.cells == top.cells && old.hashes == top.hashes && old.bundles == top.bundles && old.max_cells == top.max_cells);
    }
}

int main() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&rng]() {
        rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
        return rng;
    };
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 300, 1024};
    for (size_t k : {(size_t)1, (size_t)3, (size_t)16, (size_t)256}) {
        for (uint32_t c : {0u, 1u, 3u, 6u, 10u}) {
            for (uint32_t depth : {0u, 1u, 12u, 24u}) {
                for (size_t nb : {(size_t)1, (size_t)2, (size_t)7, (size_t)40}) {
                    std::vector<BundleSize> sz;
                    for (size_t b = 0; b < nb; b++) {
                        const uint32_t s = sizes[next() % 7];
                        // any per-blob witness length a bundle of s stripes at this depth can have: 0 .. s * depth
                        sz.push_back(BundleSize{s, depth ? next() % ((uint64_t)s * depth + 1) : 0});
                    }
                    const size_t one = staged(c, sz[0].cells, sz[0].hashes, k);
                    size_t all = 0;
                    for (const BundleSize& z : sz) all += staged(c, z.cells, z.hashes, k);
                    for (size_t budget : {(size_t)1, one, one - 1, one + 1, all, all - 1, all / 2 + 1, (size_t)32 << 20}) walk(c, sz, budget, k);
                    g_log_cell = c, g_budget = one, g_n = nb, g_blobs = k;
                    EXPECT(bundles_pass_end(c, sz.data(), sz.size(), 0, one, k) == 1);
                    EXPECT(bundles_pass_end(c, sz.data(), sz.size(), 0, one - 1, k) == 1);
                    EXPECT(bundles_pass_end(c, sz.data(), sz.size(), 0, all, k) == nb);
                    if (nb > 1) EXPECT(bundles_pass_end(c, sz.data(), sz.size(), 0, all - 1, k) < nb);
                }
            }
        }
        // plans on their own, the empty witness included
        for (uint32_t c : {0u, 3u, 10u})
            for (size_t cells : {(size_t)1, (size_t)65, (size_t)5000})
                for (size_t hashes : {(size_t)0, (size_t)1, (size_t)9, (size_t)70000}) {
                    BundlesPassCount n;
                    n.cells = cells, n.bundles = std::max<size_t>(1, cells / 60), n.hashes = hashes, n.max_cells = 1;
                    g_log_cell = c, g_budget = 0, g_n = n.bundles, g_blobs = k;
                    check_plan(c, n, k, nullptr);
                }
    }
    // the staged bytes of the record's shape: 16 blobs, one bundle of 513 stripes of 64 entries, 1673 hashes per blob
    EXPECT(bundle_staged_bytes(6, BundleSize{513, 1673}, 16) == 12 + 4 * 513 + 16 * (1024 * (size_t)513 + 32 * (size_t)1673));
    printf("OK %ld checks\n", checks);
    return 0;
}
