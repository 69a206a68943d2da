// block_proof.h — block proofs on the host, without HIP: the block challenge, the stripe indices a proof's queries give, the client's
// combination check and the wire image.  Compiles with a plain C++ compiler (tests/cpp/test_block_proof_plan.cpp runs it under ASan +
// UBSan), as prove_jobs_plan.h and verify_pass.h do.
//
// A BLOCK PROOF answers for the n_blobs commitments of a block with ONE FRI proof: the proof of g = sum over k of rho^k f_k (the
// aggregate handle of frieda_aggregate_encoded; rho drawn from all the commitments), and the values of every f_k where that proof opened
// g, as one stripe bundle at log_cell 1.  FRI's first layer opens the bit-reversed evaluation in pairs {2 i, 2 i + 1}: pair i IS cell i at
// log_cell 1, so the stripes are the ascending distinct q >> 1 of the proof's first-layer queries q.
//
// Wire image (little-endian; the arrays in the layouts of frieda_verify_stripe_bundles):
//   u32 magic "FBP1" | u32 version 1 | u32 n_blobs | u32 n_stripes | u64 W (witness hashes per blob) | u64 proof_bytes
//   proof image [proof_bytes]                         
//   stripe_index u32 [n_stripes]
//   values u32 [n_stripes][n_blobs][4][2]
//   witness [n_blobs][W][32]
// Nothing follows the witness: a reader accepts an image of exactly that length, whose indices pass the bundle's malformed rule for the
// proof's domain and whose W is the count the indices give.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bundles_host.h"
#include "channel.h"

namespace frieda {

// rho: a default channel, mix_u64(n_blobs), mix_root(commitment k) for k = 0 .. n_blobs - 1, one draw_felt.  commitments[n_blobs][32].
inline QM31 block_challenge(const uint8_t* commitments, uint32_t n_blobs) {
    Channel ch;
    ch.init();
    ch.mix_u64(n_blobs);
    for (uint32_t k = 0; k < n_blobs; k++) {
        uint32_t w[8];
        const uint8_t* c = commitments + 32 * (size_t)k;
        for (int i = 0; i < 8; i++) w[i] = (uint32_t)c[4 * i] | ((uint32_t)c[4 * i + 1] << 8) | ((uint32_t)c[4 * i + 2] << 16) | ((uint32_t)c[4 * i + 3] << 24);
        ch.mix_root(w);
    }
    return ch.draw_felt();
}

inline QM31 qm_pow(QM31 x, uint64_t e) {
    QM31 r{1, 0, 0, 0};
    while (e) {
        if (e & 1) r = qm_mul(r, x);
        x = qm_mul(x, x);
        e >>= 1;
    }
    return r;
}

// the stripes of a proof: the ascending distinct q >> 1 over its first-layer queries (any order, repeats allowed)
inline void block_stripe_indices(const uint32_t* queries, size_t n_queries, std::vector<uint32_t>& idx) {
    idx.resize(n_queries);
    for (size_t i = 0; i < n_queries; i++) idx[i] = queries[i] >> 1;
    std::sort(idx.begin(), idx.end());
    idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
}

// sum over k of rho^k * v_k, v_k = the four words at values[k * stride + c * 2] (c = 0 .. 3): one entry of one opened pair, the blobs
// of a stripe `stride` = 8 words apart.  Horner from the last blob down, as the kernel does.
inline QM31 block_combine(const uint32_t* values, uint32_t n_blobs, size_t stride, QM31 rho) {
    QM31 acc{0, 0, 0, 0};
    for (uint32_t k = n_blobs; k-- > 0;) {
        const uint32_t* v = values + (size_t)k * stride;
        acc = qm_add(qm_mul(acc, rho), QM31{v[0], v[2], v[4], v[6]});
    }
    return acc;
}

// ---- the wire image ----
constexpr uint32_t BLOCK_PROOF_MAGIC = 0x31504246u;  // "FBP1"
constexpr uint32_t BLOCK_PROOF_VERSION = 1;
constexpr size_t BLOCK_PROOF_HEADER_BYTES = 32;
constexpr uint32_t BLOCK_PROOF_MAX_BLOBS = 65535;

struct BlockWire {
    uint32_t n_blobs = 0, n_stripes = 0;
    uint64_t W = 0, proof_bytes = 0;
    size_t off_proof = 0, off_index = 0, off_values = 0, off_witness = 0, total = 0;
};

namespace blockdetail {
inline void put32(uint8_t* p, uint32_t v) {
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}
inline void put64(uint8_t* p, uint64_t v) {
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
inline uint32_t get32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t get64(const uint8_t* p) { return (uint64_t)get32(p) | ((uint64_t)get32(p + 4) << 32); }
}  // namespace blockdetail

// the offsets of an image of these counts; false when a count is out of range (then nothing can be laid out)
inline bool block_wire_layout(uint32_t n_blobs, uint32_t n_stripes, uint64_t W, uint64_t proof_bytes, BlockWire& w) {
    if (n_blobs == 0 || n_blobs > BLOCK_PROOF_MAX_BLOBS || n_stripes == 0 || n_stripes > FRIEDA_MAX_BUNDLE_CELLS) return false;
    if (W > (uint64_t)FRIEDA_MAX_BUNDLE_CELLS * FRIEDA_MAX_LOG_DOMAIN || proof_bytes > ((uint64_t)1 << 32)) return false;
    w.n_blobs = n_blobs, w.n_stripes = n_stripes, w.W = W, w.proof_bytes = proof_bytes;
    w.off_proof = BLOCK_PROOF_HEADER_BYTES;
    w.off_index = w.off_proof + (size_t)proof_bytes;
    w.off_values = w.off_index + 4 * (size_t)n_stripes;
    w.off_witness = w.off_values + 32 * (size_t)n_stripes * n_blobs;
    w.total = w.off_witness + 32 * (size_t)W * n_blobs;
    return true;
}
inline void block_wire_write_header(uint8_t* buf, const BlockWire& w) {
    using namespace blockdetail;
    put32(buf, BLOCK_PROOF_MAGIC), put32(buf + 4, BLOCK_PROOF_VERSION), put32(buf + 8, w.n_blobs), put32(buf + 12, w.n_stripes);
    put64(buf + 16, w.W), put64(buf + 24, w.proof_bytes);
}
// header, ranges and the exact-length rule; the proof image and the indices are the caller's next steps (block_wire_indices_ok)
inline bool block_wire_read(const uint8_t* buf, size_t len, BlockWire& w) {
    using namespace blockdetail;
    if (!buf || len < BLOCK_PROOF_HEADER_BYTES) return false;
    if (get32(buf) != BLOCK_PROOF_MAGIC || get32(buf + 4) != BLOCK_PROOF_VERSION) return false;
    if (!block_wire_layout(get32(buf + 8), get32(buf + 12), get64(buf + 16), get64(buf + 24), w)) return false;
    return w.total == len;
}
// the bundle's malformed rule for the stripes of a proof on a 2^log_domain domain: 1 .. 1024 strictly ascending indices below
// 2^(log_domain - 1), and W the witness count they give
inline bool block_wire_indices_ok(uint32_t log_domain, const uint32_t* idx, uint32_t n_stripes, uint64_t W) {
    if (log_domain < 1 || bundle_malformed(log_domain, 1, idx, n_stripes)) return false;
    return bundle_witness_count(log_domain - 1, idx, n_stripes) == W;
}

}  // namespace frieda
