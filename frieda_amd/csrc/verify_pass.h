// verify_pass.h — the arithmetic of one pass of the proof verifier (verify_many.cpp: verify_many): which proofs a pass takes, which
// of the two launch shapes it runs, what the split shape asks of the arena, and how the events of the split shape's two launches become
// the one status of the sequential verifier.  No HIP, no context: the cut and the rule run on the CPU against the formulas written out
// again (tests/cpp/test_verify_pass.cpp); verify_split.hip includes the rule (constexpr functions only).
//
// The cut.  The kernel-eligible proofs of a call go pass by pass, in the caller's order.  A pass takes proofs while the staged words
// (a header and the image per proof) stay within `pass_bytes`; a lone larger proof is a pass of its own.  A pass of at most `split_max`
// proofs (0: never) takes the split shape — one wave per proof for the value chain, then one wave per (proof, layer) for the Merkle
// walks — and the chain hands every layer's assembled pairs to the walks through a scratch of
//     proofs * max_layers * q_cap * VERIFY_SPLIT_ENTRY_BYTES      (the pass's largest layer count and query capacity: one pitch)
// bytes, 1.4 MiB per proof at 1024 queries and 40 layers.  A split pass is therefore cut again, to the longest prefix whose scratch stays
// within `scratch_cap`; a lone proof is always admitted.  (A prefix of a pass that may split is itself at most split_max proofs.)
//
// The rule.  verifier.cpp::verify, and verify_many_kernel after it, return at the first failing event in this order:
//     0            the proof of work
//     1 + 2 li     the value stage of layer li (witness counts, the fold; at li = 0 also QueryEvalsExhausted)
//     2 + 2 li     the Merkle walk of layer li
//     3            (a proof without inner layers: INVARIANT once layer 0 has passed — the slot of the value stage it does not have)
//     3 + 2 nl     the last-layer checks (nl = the number of inner layers)
// An event is a key: the order in the high bits, the status in the low two, so that the smallest key is the first event.  The chain
// wave stores the key of its first event, or VERIFY_KEY_ACCEPTED; it stops there, so the layers behind that event have no walk.  A walk
// wave that fails lowers the stored key to its own (atomicMin).  What is left decodes to the status.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace frieda {

constexpr size_t VERIFY_PASS_BYTES = (size_t)32 << 20;          // staging budget of one upload
constexpr size_t VERIFY_SPLIT_SCRATCH_CAP = (size_t)256 << 20;  // most scratch a split pass may ask of the arena
constexpr size_t VERIFY_SPLIT_ENTRY_WORDS = 9;                  // a pair of a layer: v, then l and r (4 words each)
constexpr size_t VERIFY_SPLIT_ENTRY_BYTES = 4 * VERIFY_SPLIT_ENTRY_WORDS;

// ---- the rule ----
constexpr uint32_t VERIFY_KEY_ACCEPTED = 0xFFFFFFFFu;
constexpr uint32_t verify_key(uint32_t order, uint32_t status) { return (order << 2) | status; }
constexpr uint32_t verify_order_pow() { return 0; }
constexpr uint32_t verify_order_values(uint32_t li) { return 1 + 2 * li; }
constexpr uint32_t verify_order_walk(uint32_t li) { return 2 + 2 * li; }
constexpr uint32_t verify_order_no_inner() { return 3; }
constexpr uint32_t verify_order_last(uint32_t n_inner) { return 3 + 2 * n_inner; }
// the status of a stored key; `accepted`: the status word for VERIFY_KEY_ACCEPTED (k::VERIFY_ACCEPTED)
constexpr uint32_t verify_key_status(uint32_t key, uint32_t accepted) { return key == VERIFY_KEY_ACCEPTED ? accepted : (key & 3u); }
// is `key` something the two launches can leave for a proof of n_inner inner layers: "accepted", or an event up to the last-layer
// checks with REJECTED (0) or INVARIANT (2)?  (The host's guard against a row nobody wrote.)
constexpr bool verify_key_valid(uint32_t key, uint32_t n_inner) {
    return key == VERIFY_KEY_ACCEPTED || ((key >> 2) <= verify_order_last(n_inner) && ((key & 3u) == 0u || (key & 3u) == 2u));
}

// ---- the cut ----
struct VerifyPassItem {
    size_t words;        // staged words of the proof: header + image
    uint32_t n_queries;  // 1 .. VERIFY_MAX_QUERIES
    uint32_t n_layers;   // first layer + inner layers
};

struct VerifyPassCut {
    size_t end = 0;           // the pass is [first, end)
    size_t words = 0;         // staged words of the pass
    uint32_t q_cap = 64;      // >= 64, a power of two, >= every n_queries of the pass
    uint32_t max_layers = 0;  // the largest n_layers of the pass
    bool split = false;
    size_t scratch_bytes = 0;  // split only: the pairs; the counts are 4 * proofs * max_layers bytes beside them
};

inline uint32_t verify_q_cap(uint32_t q_cap, uint32_t n_queries) {
    while (q_cap < n_queries) q_cap <<= 1;
    return q_cap;
}

inline size_t verify_split_scratch_bytes(size_t n_proofs, uint32_t max_layers, uint32_t q_cap) {
    return n_proofs * max_layers * q_cap * VERIFY_SPLIT_ENTRY_BYTES;
}

// item(i): the VerifyPassItem of the i-th eligible proof, i in [first, n)
template <class Item>
VerifyPassCut verify_pass_cut(Item item, size_t first, size_t n, size_t pass_bytes, size_t split_max, size_t scratch_cap) {
    VerifyPassCut c;
    c.end = first;
    while (c.end < n) {
        const VerifyPassItem it = item(c.end);
        if (c.end > first && 4 * (c.words + it.words) > pass_bytes) break;
        c.words += it.words;
        c.q_cap = verify_q_cap(c.q_cap, it.n_queries);
        if (it.n_layers > c.max_layers) c.max_layers = it.n_layers;
        c.end++;
    }
    if (split_max == 0 || c.end - first > split_max) return c;
    // the split shape: the longest prefix whose scratch fits
    VerifyPassCut s;
    s.split = true;
    s.end = first;
    while (s.end < c.end) {
        const VerifyPassItem it = item(s.end);
        const uint32_t q = verify_q_cap(s.q_cap, it.n_queries), ml = it.n_layers > s.max_layers ? it.n_layers : s.max_layers;
        if (s.end > first && verify_split_scratch_bytes(s.end - first + 1, ml, q) > scratch_cap) break;
        s.words += it.words;
        s.q_cap = q;
        s.max_layers = ml;
        s.end++;
    }
    s.scratch_bytes = verify_split_scratch_bytes(s.end - first, s.max_layers, s.q_cap);
    return s;
}

}  // namespace frieda
