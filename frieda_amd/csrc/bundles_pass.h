// bundles_pass.h — the arithmetic of one pass of the bundle verifier (bundles_host.cpp: verify_bundles_passes, the one driver of cell
// bundles and stripe bundles, which calls everything here with the factor max(n_blobs, 1)): which bundles a pass takes,
// where the pieces of its staged image lie, and what it asks of the pinned block and the arena.  No HIP, no context: the cuts run on
// the CPU against the formulas written out again (tests/cpp/test_bundles_pass.cpp).  cells_pass.h is the same for separate cells.
//
// Only well-formed bundles are staged (bundles_host.h decides MALFORMED first), so a pass sees a list of sizes: cells and witness hashes
// per bundle.  A bundle stages 12 + cells * (4 + vb) + 32 * hashes bytes (vb = 16 << log_cell): its table row, its indices, its values
// and its witness.  A pass takes bundles in order while their sum stays within the budget `pass_bytes`; a bundle never straddles two
// passes, and one bundle is always admitted.  Passes differ in their mix of cells and hashes, so the call plans its arena and pinned
// block once from the largest cell count, bundle count and hash count any of its passes has (every offset below grows with each of
// the three): every pass fits that plan.
// Staged image (pinned block -> arena, one copy): indices | the bundle table (first cell, cell count, first witness hash: three words a
// row) | values, cell-major as given | the witness as given; every piece from a 256-byte boundary.  Behind it in the pinned block: one
// status word per bundle as it comes back, then the gather table the host builds from the statuses (two words per cell of an accepted
// bundle).  In the arena behind the image: roots (32 bytes a cell), bad (a word a cell), the status words, the gather table.
//
// Stripe bundles (stripe_bundles_host.cpp's exports) go through the same driver with a factor n_blobs (default 1: the single-blob form):
// a bundle's k stripes are cell j of EVERY blob, so it stages its table row and its indices once and its values and its witness n_blobs
// times, 12 + cells * 4 + n_blobs * (cells * vb + 32 * hashes) bytes with `hashes` counted per blob; roots and bad are per (stripe, blob)
// cell, there is a status word per (bundle, blob), and the gather table has a row per stripe.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace frieda {

struct BundleSize {
    uint32_t cells;
    uint64_t hashes;
};

inline size_t bundles_al(size_t b) { return (b + 255) & ~(size_t)255; }

inline size_t bundle_staged_bytes(uint32_t log_cell, const BundleSize& z, size_t n_blobs = 1) {
    return 12 + (size_t)z.cells * 4 + n_blobs * ((size_t)z.cells * ((size_t)16 << log_cell) + 32 * (size_t)z.hashes);
}

// the end (exclusive) of the pass that begins at bundle `first` < n
inline size_t bundles_pass_end(uint32_t log_cell, const BundleSize* sz, size_t n, size_t first, size_t pass_bytes, size_t n_blobs = 1) {
    size_t end = first + 1, sum = bundle_staged_bytes(log_cell, sz[first], n_blobs);
    while (end < n) {
        const size_t next = bundle_staged_bytes(log_cell, sz[end], n_blobs);
        if (next > pass_bytes || sum > pass_bytes - next) break;
        sum += next, end++;
    }
    return end;
}

struct BundlesPassCount {
    size_t cells = 0, bundles = 0, hashes = 0;
    uint32_t max_cells = 0;  // the largest bundle: sizes the walk's LDS
};
inline BundlesPassCount bundles_pass_count(const BundleSize* sz, size_t first, size_t end) {
    BundlesPassCount c;
    for (size_t b = first; b < end; b++) c.cells += sz[b].cells, c.hashes += (size_t)sz[b].hashes, c.bundles++, c.max_cells = std::max(c.max_cells, sz[b].cells);
    return c;
}
// the component-wise largest pass of the call: what the one plan of the call is made from
inline BundlesPassCount bundles_call_count(uint32_t log_cell, const BundleSize* sz, size_t n, size_t pass_bytes, size_t n_blobs = 1) {
    BundlesPassCount m;
    for (size_t first = 0; first < n;) {
        const size_t end = bundles_pass_end(log_cell, sz, n, first, pass_bytes, n_blobs);
        const BundlesPassCount c = bundles_pass_count(sz, first, end);
        m.cells = std::max(m.cells, c.cells), m.bundles = std::max(m.bundles, c.bundles), m.hashes = std::max(m.hashes, c.hashes);
        m.max_cells = std::max(m.max_cells, c.max_cells);
        first = end;
    }
    return m;
}

struct BundlesPassPlan {
    size_t i_idx, i_tab, i_val, i_wit, in_bytes;          // the staged image
    size_t res_bytes, p_res, p_tab, pinned;               // pinned block: statuses at p_res, gather table at p_tab, `pinned` bytes in all
    size_t a_in, a_roots, a_bad, a_res, a_tab, arena;     // arena offsets, `arena` bytes in all
};

// c counts indices (`cells`) and per-blob hashes; n_blobs multiplies what a bundle holds once per blob
inline BundlesPassPlan bundles_pass_plan(uint32_t log_cell, const BundlesPassCount& c, size_t n_blobs = 1) {
    BundlesPassPlan p;
    p.i_idx = 0, p.i_tab = bundles_al(4 * c.cells), p.i_val = p.i_tab + bundles_al(12 * c.bundles);
    p.i_wit = p.i_val + bundles_al(((size_t)16 << log_cell) * c.cells * n_blobs), p.in_bytes = p.i_wit + bundles_al(32 * c.hashes * n_blobs);
    p.res_bytes = 4 * c.bundles * n_blobs;
    p.p_res = p.in_bytes, p.p_tab = p.p_res + bundles_al(p.res_bytes), p.pinned = p.p_tab + 8 * c.cells;
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t o = off;
        off = bundles_al(off + bytes);
        return o;
    };
    p.a_in = take(p.in_bytes), p.a_roots = take(32 * c.cells * n_blobs), p.a_bad = take(4 * c.cells * n_blobs), p.a_res = take(p.res_bytes), p.a_tab = take(8 * c.cells);
    p.arena = off;
    return p;
}

}  // namespace frieda
