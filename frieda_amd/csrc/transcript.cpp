// transcript.cpp — the variable-length parts of the Fiat–Shamir transcript shared by prover and verifier:
// Blake2sChannel::mix_felts and stwo core/queries.rs::Queries::{generate, fold}.  PARITY UNPINNED (see channel.h).
#include <stddef.h>

#include <algorithm>

#include "host.h"

namespace frieda {

// Blake2sChannel::mix_felts (channel.h) over a vector of QM31
void channel_mix_felts(Channel& ch, const std::vector<QM31>& felts) {
    static_assert(sizeof(QM31) == 4 * sizeof(uint32_t) && offsetof(QM31, a) == 0 && offsetof(QM31, b) == 4 && offsetof(QM31, c) == 8 &&
                      offsetof(QM31, d) == 12,
                  "a QM31 is four consecutive uint32_t: a, b, c, d");
    ch.mix_felts(reinterpret_cast<const uint32_t*>(felts.data()), (uint32_t)felts.size());
}

// Queries::generate
std::vector<uint32_t> generate_queries(Channel& ch, uint32_t log_domain_size, uint32_t n_queries) {
    std::vector<uint32_t> q;
    uint32_t mask = (1u << log_domain_size) - 1;
    while (q.size() < n_queries) {
        uint32_t w[8];
        ch.draw_random_words(w);
        for (int i = 0; i < 8 && q.size() < n_queries; i++) q.push_back(w[i] & mask);
    }
    std::sort(q.begin(), q.end());
    q.erase(std::unique(q.begin(), q.end()), q.end());
    return q;
}
// Queries::fold
std::vector<uint32_t> fold_queries(const std::vector<uint32_t>& q, uint32_t n_folds) {
    std::vector<uint32_t> r;
    for (uint32_t v : q)
        if (r.empty() || r.back() != (v >> n_folds)) r.push_back(v >> n_folds);
    return r;
}

}  // namespace frieda
