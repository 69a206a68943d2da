// bundles_host.h — cell bundles on the host, without HIP: the malformed rule, the witness count, the per-level offsets the opener
// uploads, and the host verifier.  Compiles with a plain C++ compiler (tests/cpp/fuzz_bundles.cpp runs it under ASan + UBSan).
//
// A bundle is k cells of one blob at one log_cell, 1 <= k <= FRIEDA_MAX_BUNDLE_CELLS, indices strictly ascending, with ONE hash
// witness: stwo's (MerkleProver::decommit) for the tree cut at level d = log_domain - log_cell with the indices as positions, i.e. the
// tables E_1 .. E_d of queries_dev.h, E_s read at tree level d - s + 1, bottom-up and ascending within a level.
//
// Two statements of the same object live here on purpose.  The COUNTS come from the emit rule (position i contributes to E_s iff it
// is the first of its parent group and a right child, or the last and a left child): every level independently, as the opener's
// waves compute them.  The VERIFIER is the bottom-up merge (MerkleVerifier::verify): a queue of (position, hash) per level, per parent
// in ascending order the child that is not in the queue is taken from the witness.  It shares no code with the kernels (walk_dev.h);
// the tests cross-check the two.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/frieda_hip.h"
#include "blake2s.h"

namespace frieda {

// ---- the malformed rule: one function for every entry point and both verifiers; null when the bundle is well formed ----
inline const char* bundle_shape_error(uint32_t log_domain, uint32_t log_cell) {
    if (log_domain > FRIEDA_MAX_LOG_DOMAIN) return "log_domain out of range";
    if (log_cell > log_domain || log_cell > FRIEDA_MAX_LOG_OPEN_CELL) return "log_cell out of range";
    return nullptr;
}
inline const char* bundle_malformed(uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, size_t k) {
    if (const char* bad = bundle_shape_error(log_domain, log_cell)) return bad;
    if (k == 0) return "empty bundle";
    if (k > FRIEDA_MAX_BUNDLE_CELLS) return "more than FRIEDA_MAX_BUNDLE_CELLS cells";
    const uint32_t bits = log_domain - log_cell;
    for (size_t i = 0; i < k; i++) {
        if (((uint64_t)cell_index[i] >> bits) != 0) return "cell index out of range";
        if (i && cell_index[i - 1] >= cell_index[i]) return "cell indices not strictly ascending";
    }
    return nullptr;
}

// |E_s| of the strictly ascending p[0 .. k), 1 <= s: the emit rule of queries_dev.h
inline size_t bundle_level_count(const uint32_t* p, size_t k, uint32_t s) {
    size_t cnt = 0;
    for (size_t i = 0; i < k; i++) {
        const uint32_t v = p[i] >> s, bit = (p[i] >> (s - 1)) & 1u;
        const bool first = i == 0 || (p[i - 1] >> s) != v;
        const bool last = i + 1 == k || (p[i + 1] >> s) != v;
        cnt += (first && bit) || (last && !bit) ? 1 : 0;  // (never both: a lone entry is a left or a right child)
    }
    return cnt;
}
// the witness length of a well-formed bundle: |E_1| + ... + |E_depth|; base[s - 1] (optional, depth entries) = first + |E_1| + ... + |E_{s-1}|
inline uint64_t bundle_witness_count(uint32_t depth, const uint32_t* p, size_t k, uint64_t first = 0, uint64_t* base = nullptr) {
    uint64_t acc = first;
    for (uint32_t s = 1; s <= depth; s++) {
        if (base) base[s - 1] = acc;
        acc += bundle_level_count(p, k, s);
    }
    return acc - first;
}

// ---- the structure of a call: the *_first arrays start at 0 and never decrease; null when it holds ----
inline const char* bundles_call_error(const uint32_t* bundle_first, const uint64_t* witness_first, uint32_t n_bundles) {
    if (bundle_first[0] != 0) return "bundle_first does not start at 0";
    if (witness_first && witness_first[0] != 0) return "witness_first does not start at 0";
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (bundle_first[b + 1] < bundle_first[b]) return "bundle_first decreases";
        if (witness_first && witness_first[b + 1] < witness_first[b]) return "witness_first decreases";
    }
    return nullptr;
}

// MALFORMED or not, for every bundle of a structurally sound call, before anything is hashed: by the rule above, or a witness whose
// length is not what the indices give.  out_status[b] = FRIEDA_BUNDLE_MALFORMED, or FRIEDA_BUNDLE_REJECTED for the verifier to decide.
inline void bundles_classify(uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, const uint32_t* bundle_first, uint32_t n_bundles,
                             const uint64_t* witness_first, uint8_t* out_status) {
    for (uint32_t b = 0; b < n_bundles; b++) {
        const uint32_t* p = cell_index + bundle_first[b];
        const size_t k = bundle_first[b + 1] - bundle_first[b];
        bool bad = bundle_malformed(log_domain, log_cell, p, k) != nullptr;
        if (!bad) bad = bundle_witness_count(log_domain - log_cell, p, k) != witness_first[b + 1] - witness_first[b];
        out_status[b] = bad ? FRIEDA_BUNDLE_MALFORMED : FRIEDA_BUNDLE_REJECTED;
    }
}

// ---- the host verifier ----
namespace bundledetail {
inline void node_words(const uint32_t* l, const uint32_t* r, uint32_t* out) {
    uint32_t m[16], h[8];
    memcpy(m, l, 32);
    memcpy(m + 8, r, 32);
    b2_merkle_block_lat(m, h);
    memcpy(out, h, 32);
}
// the subtree root over the 2^c leaves of one cell v[4][2^c]; false when a word is not a canonical M31
inline bool cell_root(uint32_t c, const uint32_t* v, std::vector<uint32_t>& lvl, uint32_t* root) {
    const size_t cs = (size_t)1 << c;
    for (size_t i = 0; i < 4 * cs; i++)
        if (v[i] >= P31) return false;
    lvl.resize(8 * cs);
    for (size_t j = 0; j < cs; j++) {
        const uint32_t m[16] = {v[j], v[cs + j], v[2 * cs + j], v[3 * cs + j], 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t h[8];
        b2_merkle_block_lat(m, h);
        memcpy(&lvl[8 * j], h, 32);
    }
    for (size_t w = cs >> 1; w >= 1; w >>= 1)
        for (size_t j = 0; j < w; j++) node_words(&lvl[16 * j], &lvl[16 * j + 8], &lvl[8 * j]);
    memcpy(root, lvl.data(), 32);
    return true;
}
}  // namespace bundledetail

struct BundleScratch {
    std::vector<uint32_t> lvl, pos, hash;
};

// One WELL-FORMED bundle (bundle_malformed is null): every word canonical, and the cells' subtree roots merged upward with the
// witness consumed in order give exactly `want`.  n_witness is what the caller holds; nothing is read beyond it.
// n_blobs (default 1): cell i's values lie n_blobs cells apart — one blob's cells of a stripe bundle, whose values are stripe-major.
inline bool bundle_accept(const uint32_t want[8], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, size_t k, const uint32_t* values,
                          const uint8_t* witness, uint64_t n_witness, BundleScratch& sc, size_t n_blobs = 1) {
    const size_t vw = ((size_t)4 << log_cell) * n_blobs;
    sc.pos.resize(k);
    sc.hash.resize(8 * k);
    for (size_t i = 0; i < k; i++) {
        if (!bundledetail::cell_root(log_cell, values + i * vw, sc.lvl, &sc.hash[8 * i])) return false;
        sc.pos[i] = cell_index[i];
    }
    uint64_t used = 0;
    size_t cn = k;
    uint32_t sib[8];
    for (uint32_t lv = log_domain - log_cell; lv > 0; lv--) {
        size_t out = 0;
        for (size_t i = 0; i < cn;) {
            const uint32_t x = sc.pos[i];
            const uint32_t *l, *r;
            size_t step = 1;
            if (x & 1u) {  // a right child whose left neighbour is not known (it would have been merged with it)
                if (used >= n_witness) return false;
                memcpy(sib, witness + 32 * used++, 32);
                l = sib, r = &sc.hash[8 * i];
            } else if (i + 1 < cn && sc.pos[i + 1] == x + 1) {
                l = &sc.hash[8 * i], r = &sc.hash[8 * (i + 1)];
                step = 2;
            } else {
                if (used >= n_witness) return false;
                memcpy(sib, witness + 32 * used++, 32);
                l = &sc.hash[8 * i], r = sib;
            }
            uint32_t h[8];
            bundledetail::node_words(l, r, h);  // (h is a copy: entry `out` <= i may be one of the operands)
            memcpy(&sc.hash[8 * out], h, 32);
            sc.pos[out++] = x >> 1;
            i += step;
        }
        cn = out;
    }
    return used == n_witness && cn == 1 && memcmp(sc.hash.data(), want, 32) == 0;
}

// Every bundle of a structurally sound call (bundles_call_error is null, shape in range): one status byte each
inline void verify_cell_bundles_host(const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                                     const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                     const uint64_t* witness_first, uint8_t* out_status) {
    uint32_t want[8];
    memcpy(want, commitment, 32);
    bundles_classify(log_domain, log_cell, cell_index, bundle_first, n_bundles, witness_first, out_status);
    BundleScratch sc;
    const size_t vw = (size_t)4 << log_cell;
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (out_status[b] == FRIEDA_BUNDLE_MALFORMED) continue;
        const size_t first = bundle_first[b], k = bundle_first[b + 1] - first;
        const uint64_t nw = witness_first[b + 1] - witness_first[b];
        const uint8_t* wit = nw ? witness + 32 * witness_first[b] : nullptr;
        out_status[b] = bundle_accept(want, log_domain, log_cell, cell_index + first, k, values + first * vw, wit, nw, sc) ? FRIEDA_BUNDLE_ACCEPTED
                                                                                                                         : FRIEDA_BUNDLE_REJECTED;
    }
}

// ---- stripe bundles: k stripes of a block of n_blobs blobs (a stripe is cell j of every blob) with one witness per blob ----
// values [stripes][n_blobs][4][2^log_cell]; witness_first counts hashes PER BLOB: bundle b's block starts at hash n_blobs * witness_first[b],
// blob j's piece is the W_b = witness_first[b + 1] - witness_first[b] hashes at j * W_b inside it, and is that blob's cell-bundle witness.
// the argument rule of the verifiers and the rebuild: null pointers and the call's own structure; null when it holds
inline const char* stripe_bundles_args_error(const uint8_t* commitments, uint32_t n_blobs, uint32_t max_blobs, uint32_t log_domain, uint32_t log_cell,
                                             const uint32_t* stripe_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values,
                                             const uint8_t* witness, const uint64_t* witness_first, const uint8_t* out_status) {
    if (n_blobs == 0 || n_blobs > max_blobs) return "n_blobs out of range";
    if (!commitments || !bundle_first || !witness_first || !out_status) return "null argument";
    if (const char* bad = bundle_shape_error(log_domain, log_cell)) return bad;
    if (const char* bad = bundles_call_error(bundle_first, witness_first, n_bundles)) return bad;
    if (bundle_first[n_bundles] && (!stripe_index || !values)) return "null argument";
    if (witness_first[n_bundles] && !witness) return "null argument";
    if (witness_first[n_bundles] > ((uint64_t)1 << 40) / n_blobs) return "witness_first out of range";
    return nullptr;
}

// Every (bundle, blob) of a structurally sound call: out_status[n_bundles][n_blobs].  MALFORMED depends on the indices and W_b alone: it
// is decided once per bundle and written to the bundle's whole row; else byte (b, j) is the single-blob verifier's on blob j's piece.
inline void verify_stripe_bundles_host(const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* stripe_index,
                                       const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                       const uint64_t* witness_first, uint8_t* out_status) {
    std::vector<uint8_t> cls(n_bundles);
    bundles_classify(log_domain, log_cell, stripe_index, bundle_first, n_bundles, witness_first, cls.data());
    BundleScratch sc;
    const size_t vw = (size_t)4 << log_cell;
    for (uint32_t b = 0; b < n_bundles; b++) {
        uint8_t* st = out_status + (size_t)b * n_blobs;
        if (cls[b] == FRIEDA_BUNDLE_MALFORMED) {
            memset(st, FRIEDA_BUNDLE_MALFORMED, n_blobs);
            continue;
        }
        const size_t first = bundle_first[b], k = bundle_first[b + 1] - first;
        const uint64_t nw = witness_first[b + 1] - witness_first[b];
        for (uint32_t j = 0; j < n_blobs; j++) {
            uint32_t want[8];
            memcpy(want, commitments + 32 * (size_t)j, 32);
            const uint8_t* wit = nw ? witness + 32 * (n_blobs * witness_first[b] + j * nw) : nullptr;
            st[j] = bundle_accept(want, log_domain, log_cell, stripe_index + first, k, values + (first * n_blobs + j) * vw, wit, nw, sc, n_blobs)
                        ? FRIEDA_BUNDLE_ACCEPTED
                        : FRIEDA_BUNDLE_REJECTED;
        }
    }
}

}  // namespace frieda
