// block_proof.h against its rules written out here once more: the stripe indices a proof's queries give (duplicates, both leaves of one
// pair, a single query, any order), the combination sum over k of rho^k v_k against powers computed one by one, the block challenge
// against the channel calls spelled out, and the wire image — round trip, every truncation, one byte more, and every single corruption
// of a header field or of an index that the malformed rule must catch.  Stand-alone; prints OK.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "block_proof.h"

using namespace frieda;

static long checks = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        checks++;                                                     \
        if (!(cond)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static std::vector<uint32_t> indices_of(std::vector<uint32_t> q) {
    std::vector<uint32_t> idx{99, 98};  // (whatever it held before)
    block_stripe_indices(q.data(), q.size(), idx);
    return idx;
}

static void test_indices() {
    EXPECT((indices_of({0}) == std::vector<uint32_t>{0}));
    EXPECT((indices_of({7}) == std::vector<uint32_t>{3}));
    EXPECT((indices_of({6, 7}) == std::vector<uint32_t>{3}));            // both leaves of one pair
    EXPECT((indices_of({5, 5, 4, 9}) == std::vector<uint32_t>{2, 4}));   // duplicates, any order
    EXPECT((indices_of({1, 2, 3, 4}) == std::vector<uint32_t>{0, 1, 2}));
    EXPECT(indices_of({}).empty());
    EXPECT((indices_of({0xFFFFFFFFu, 0}) == std::vector<uint32_t>{0, 0x7FFFFFFFu}));
    std::mt19937 rng(7);
    for (int round = 0; round < 200; round++) {
        const uint32_t n = 1 + rng() % 40, bits = 1 + rng() % 12;
        std::vector<uint32_t> q(n);
        for (uint32_t& v : q) v = rng() & ((1u << bits) - 1);
        const std::vector<uint32_t> idx = indices_of(q);
        for (size_t i = 0; i < idx.size(); i++) {
            EXPECT(i == 0 || idx[i - 1] < idx[i]);
            bool found = false;
            for (uint32_t v : q) found = found || (v >> 1) == idx[i];
            EXPECT(found);
        }
        for (uint32_t v : q) {
            bool found = false;
            for (uint32_t x : idx) found = found || x == (v >> 1);
            EXPECT(found);
        }
        EXPECT(bundle_malformed(bits, 1, idx.data(), idx.size()) == nullptr);  // what the opener and the verifier will ask of them
    }
}

static void test_combine() {
    std::mt19937 rng(11);
    const uint32_t edge[] = {0, 1, P31 - 1};
    for (int round = 0; round < 300; round++) {
        const uint32_t K = 1 + rng() % 20;
        QM31 rho{rng() % P31, rng() % P31, rng() % P31, rng() % P31};
        if (round < 81) rho = QM31{edge[round % 3], edge[round / 3 % 3], edge[round / 9 % 3], edge[round / 27 % 3]};
        std::vector<uint32_t> values(8 * (size_t)K);  // one stripe: [K][4][2]
        for (uint32_t& v : values) v = (rng() & 1) ? edge[rng() % 3] : rng() % P31;
        for (uint32_t e = 0; e < 2; e++) {
            QM31 want{0, 0, 0, 0}, power{1, 0, 0, 0};
            for (uint32_t k = 0; k < K; k++) {
                const uint32_t* v = &values[8 * (size_t)k + e];
                want = qm_add(want, qm_mul(power, QM31{v[0], v[2], v[4], v[6]}));
                EXPECT(qm_eq(power, qm_pow(rho, k)));
                power = qm_mul(power, rho);
            }
            EXPECT(qm_eq(block_combine(values.data() + e, K, 8, rho), want));
        }
    }
}

static void test_challenge() {
    for (uint32_t K : {1u, 2u, 3u, 17u}) {
        std::vector<uint8_t> roots(32 * (size_t)K);
        for (size_t i = 0; i < roots.size(); i++) roots[i] = (uint8_t)(31 * i + 7 * K);
        Channel ch;
        ch.init();
        ch.mix_u64(K);
        for (uint32_t k = 0; k < K; k++) {
            uint32_t w[8];
            memcpy(w, &roots[32 * (size_t)k], 32);  // (a little-endian host)
            ch.mix_root(w);
        }
        const QM31 want = ch.draw_felt(), got = block_challenge(roots.data(), K);
        EXPECT(qm_eq(got, want));
        EXPECT(got.a < P31 && got.b < P31 && got.c < P31 && got.d < P31);
        if (K >= 2) {
            std::vector<uint8_t> swapped = roots;
            for (int i = 0; i < 32; i++) std::swap(swapped[i], swapped[32 + i]);
            EXPECT(!qm_eq(block_challenge(swapped.data(), K), got));
            EXPECT(!qm_eq(block_challenge(roots.data(), K - 1), got));
        }
    }
}

static void test_wire() {
    // a small image: 2 blobs, the stripes {1, 4, 5} of a 2^4 domain (8 cells of 2), a stand-in of 40 bytes for the proof image
    const uint32_t log_domain = 4, n_blobs = 2;
    const std::vector<uint32_t> idx{1, 4, 5};
    const uint64_t W = bundle_witness_count(log_domain - 1, idx.data(), idx.size());
    EXPECT(W == 3);  // level 1: cell 0 and (4, 5 merge: nothing); level 2: node 1 and node 3; level 3: the two halves merge
    BlockWire w;
    EXPECT(block_wire_layout(n_blobs, (uint32_t)idx.size(), W, 40, w));
    EXPECT(w.off_proof == 32 && w.off_index == 72 && w.off_values == 84 && w.off_witness == 84 + 32 * 3 * 2 && w.total == w.off_witness + 32 * 3 * 2);
    std::vector<uint8_t> img(w.total);
    for (size_t i = 0; i < img.size(); i++) img[i] = (uint8_t)(i * 13 + 1);
    block_wire_write_header(img.data(), w);
    memcpy(img.data() + w.off_index, idx.data(), 4 * idx.size());
    // round trip
    BlockWire r;
    EXPECT(block_wire_read(img.data(), img.size(), r));
    EXPECT(r.n_blobs == n_blobs && r.n_stripes == 3 && r.W == W && r.proof_bytes == 40 && r.total == w.total && r.off_witness == w.off_witness);
    std::vector<uint32_t> got(r.n_stripes);
    memcpy(got.data(), img.data() + r.off_index, 4 * got.size());
    EXPECT(got == idx && block_wire_indices_ok(log_domain, got.data(), r.n_stripes, r.W));
    // every truncation and one byte more; each from a buffer of exactly that size, so that a read past the end is the sanitizer's
    for (size_t len = 0; len <= img.size() + 1; len++) {
        if (len == img.size()) continue;
        std::vector<uint8_t> cut(img.begin(), img.begin() + std::min(len, img.size()));
        cut.resize(len, 0);
        EXPECT(!block_wire_read(cut.data(), cut.size(), r));
    }
    EXPECT(!block_wire_read(nullptr, 0, r));
    // every single-bit corruption of every header field: magic, version, n_blobs, n_stripes, W, proof_bytes
    for (size_t byte = 0; byte < BLOCK_PROOF_HEADER_BYTES; byte++)
        for (int bit = 0; bit < 8; bit++) {
            std::vector<uint8_t> bad = img;
            bad[byte] ^= (uint8_t)(1u << bit);
            EXPECT(!block_wire_read(bad.data(), bad.size(), r));
        }
    // counts out of range never lay out
    EXPECT(!block_wire_layout(0, 3, W, 40, r) && !block_wire_layout(65536, 3, W, 40, r));
    EXPECT(!block_wire_layout(2, 0, 0, 40, r) && !block_wire_layout(2, FRIEDA_MAX_BUNDLE_CELLS + 1, W, 40, r));
    EXPECT(!block_wire_layout(2, 3, ~(uint64_t)0, 40, r) && !block_wire_layout(2, 3, W, ~(uint64_t)0, r));
    // the indices: the bundle's malformed rule and the witness count
    EXPECT(!block_wire_indices_ok(log_domain, idx.data(), 3, W + 1) && !block_wire_indices_ok(log_domain, idx.data(), 3, W - 1));
    EXPECT(!block_wire_indices_ok(log_domain, idx.data(), 0, 0));
    EXPECT(!block_wire_indices_ok(0, idx.data(), 1, 0));
    for (size_t i = 0; i < idx.size(); i++) {
        std::vector<uint32_t> bad = idx;
        bad[i] = 8;  // out of range for 8 cells (and not ascending unless last)
        EXPECT(!block_wire_indices_ok(log_domain, bad.data(), 3, W));
        bad[i] = 0x80000001u;
        EXPECT(!block_wire_indices_ok(log_domain, bad.data(), 3, W));
        if (i) {
            bad = idx;
            bad[i] = idx[i - 1];  // repeated
            EXPECT(!block_wire_indices_ok(log_domain, bad.data(), 3, W));
            bad[i] = idx[i - 1] - 1;  // descending
            EXPECT(!block_wire_indices_ok(log_domain, bad.data(), 3, W));
        }
    }
    // an index moved to another legal place changes the witness count here: {1, 4, 5} -> {1, 4, 6}
    const uint32_t moved[3] = {1, 4, 6};
    EXPECT(bundle_malformed(log_domain, 1, moved, 3) == nullptr && !block_wire_indices_ok(log_domain, moved, 3, W));
    // the whole domain opened: no witness at all
    const uint32_t all[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    EXPECT(block_wire_indices_ok(log_domain, all, 8, 0) && !block_wire_indices_ok(log_domain, all, 8, 1));
}

int main() {
    test_indices();
    test_combine();
    test_challenge();
    test_wire();
    printf("%ld checks\nOK\n", checks);
    return 0;
}
