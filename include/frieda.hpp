// frieda.hpp — header-only C++17 mirror of frieda's public Rust API over the C ABI (frieda_hip.h).
//
//   frieda::api::commit(data, log_blowup_factor) -> Commitment                         (/root/reference/src/lib.rs:31)
//   frieda::api::generate_proof(data, seed, pcs_config) -> Proof                       (src/lib.rs:36)
//   frieda::proof::commit_and_generate_proof(data, seed, pcs_config) -> {Commitment, Proof}   (src/proof.rs:32)
//   frieda::api::verify(proof, seed) -> bool                                           (src/lib.rs:41)
//
// Same names, argument meaning and error behaviour: where the reference panics, frieda::Panic is thrown; verifier
// rejections return false.  Option<u64> is std::optional<uint64_t>.  A thread-local default context (device 0) backs the
// free functions; construct frieda::Context for other devices / streams.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "frieda_hip.h"

namespace frieda {

using Commitment = std::array<uint8_t, 32>;  // src/commit.rs:9

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& what) : std::runtime_error(what), status(s) {}
};
struct Panic : Error {  // the reference implementation panics here (FRIEDA_ERR_INVARIANT)
    using Error::Error;
};

inline void check(int status, const frieda_ctx* ctx = nullptr) {
    if (status == FRIEDA_OK) return;
    std::string msg = std::string("frieda_hip: ") + frieda_status_string(status);
    if (ctx) msg += std::string(": ") + frieda_last_error(ctx);
    if (status == FRIEDA_ERR_INVARIANT) throw Panic(status, msg);
    throw Error(status, msg);
}

// stwo FriConfig / PcsConfig as constructed at src/proof.rs:109-116
struct FriConfig {
    uint32_t log_blowup_factor = 4, log_last_layer_degree_bound = 0;
    size_t n_queries = 20;
};
struct PcsConfig {
    uint32_t pow_bits = 20;
    FriConfig fri_config;
    frieda_pcs_config c() const {
        return {pow_bits, fri_config.log_blowup_factor, fri_config.log_last_layer_degree_bound, (uint32_t)fri_config.n_queries};
    }
};

struct QM31 {
    uint32_t v[4];
    bool operator==(const QM31& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2] && v[3] == o.v[3]; }
    bool operator!=(const QM31& o) const { return !(*this == o); }
};

// frieda::proof::Proof (src/proof.rs:19-26); the fields the reference's tests mutate are exposed as accessors
class Proof {
  public:
    Proof() = default;
    explicit Proof(frieda_proof* h) : h_(h) {}
    Proof(const Proof& o) { check(frieda_proof_clone(o.h_, &h_)); }
    Proof(Proof&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Proof& operator=(Proof o) {
        std::swap(h_, o.h_);
        return *this;
    }
    ~Proof() { frieda_proof_free(h_); }

    uint64_t proof_of_work() const { return frieda_proof_proof_of_work(h_); }
    void set_proof_of_work(uint64_t v) { frieda_proof_set_proof_of_work(h_, v); }
    uint32_t log_size_bound() const { return frieda_proof_log_size_bound(h_); }
    size_t n_inner_layers() const { return frieda_proof_n_inner_layers(h_); }
    Commitment first_layer_commitment() const {
        Commitment c;
        const uint8_t* p = frieda_proof_layer_commitment(h_, 0);
        for (int i = 0; i < 32; i++) c[i] = p[i];
        return c;
    }
    std::vector<QM31> evaluations() const {
        size_t n = frieda_proof_n_evaluations(h_);
        std::vector<QM31> out(n);
        const uint32_t* p = frieda_proof_evaluations(h_);
        for (size_t i = 0; i < n; i++)
            for (int c = 0; c < 4; c++) out[i].v[c] = p[4 * i + c];
        return out;
    }
    void set_evaluations(const std::vector<QM31>& ev) {
        check(frieda_proof_resize_evaluations(h_, ev.size()));
        uint32_t* p = frieda_proof_evaluations(h_);
        for (size_t i = 0; i < ev.size(); i++)
            for (int c = 0; c < 4; c++) p[4 * i + c] = ev[i].v[c];
    }
    std::vector<uint8_t> serialize() const {
        std::vector<uint8_t> b(frieda_proof_serialize(h_, nullptr, 0));
        frieda_proof_serialize(h_, b.data(), b.size());
        return b;
    }
    static Proof deserialize(const std::vector<uint8_t>& b) {
        frieda_proof* h = nullptr;
        check(frieda_proof_deserialize(b.data(), b.size(), &h));
        return Proof(h);
    }
    const frieda_proof* handle() const { return h_; }

  private:
    frieda_proof* h_ = nullptr;
};

// An encoded blob on the device (frieda_encoded): evaluations + first-layer tree + root in an allocation of its own — the half of a proof
// that does not depend on the seed.  Made by Context::encode, only read by Context::prove_seeds (several contexts may share one).
class Encoded {
  public:
    Encoded() = default;
    explicit Encoded(frieda_encoded* h) : h_(h) {}
    Encoded(const Encoded&) = delete;
    Encoded& operator=(const Encoded&) = delete;
    Encoded(Encoded&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Encoded& operator=(Encoded&& o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }
    ~Encoded() { frieda_encoded_free(h_); }
    Commitment commitment() const {
        Commitment c;
        check(frieda_encoded_commitment(h_, c.data()));
        return c;
    }
    size_t bytes() const { return frieda_encoded_bytes(h_); }
    // {log_size_bound, log_domain} of the encoded codeword (frieda_encoded_shape)
    std::pair<uint32_t, uint32_t> shape() const {
        uint32_t l = 0, n = 0;
        check(frieda_encoded_shape(h_, &l, &n));
        return {l, n};
    }
    // the number of blobs an aggregate handle (Context::aggregate_encoded) combines; 0 for a blob's own handle
    uint32_t aggregate_of() const { return frieda_encoded_aggregate_of(h_); }
    const frieda_encoded* handle() const { return h_; }

  private:
    frieda_encoded* h_ = nullptr;
};

// A block proof (frieda_block_proof): ONE FRI proof for all blobs of a block — the proof of the aggregate handle under a seed and the
// blobs opened where it was queried, as one stripe bundle at log_cell 1.  A protocol of this project, not of the reference
// (include/frieda_hip.h, "block proofs").  Made by Context::prove_block_seeds or from its wire image; checked by verify_block.
class BlockProof {
  public:
    BlockProof() = default;
    explicit BlockProof(frieda_block_proof* h) : h_(h) {}
    BlockProof(const BlockProof&) = delete;
    BlockProof& operator=(const BlockProof&) = delete;
    BlockProof(BlockProof&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    BlockProof& operator=(BlockProof&& o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }
    ~BlockProof() { frieda_block_proof_free(h_); }
    // the FRI part: owned by the block proof (frieda_proof_clone for a copy)
    const frieda_proof* fri() const { return frieda_block_proof_fri(h_); }
    uint32_t n_blobs() const { return frieda_block_proof_n_blobs(h_); }
    uint32_t n_stripes() const { return frieda_block_proof_n_stripes(h_); }
    uint64_t witness_hashes() const { return frieda_block_proof_witness_hashes(h_); }  // per blob
    // the opening part in the layouts of frieda_verify_stripe_bundles: [n_stripes], [n_stripes][n_blobs][4][2], [n_blobs][witness_hashes][32]
    const uint32_t* stripe_index() const { return frieda_block_proof_stripe_index(h_); }
    const uint32_t* values() const { return frieda_block_proof_values(h_); }
    const uint8_t* witness() const { return frieda_block_proof_witness(h_); }
    std::vector<uint8_t> serialize() const {
        std::vector<uint8_t> b(frieda_block_proof_serialize(h_, nullptr, 0));
        frieda_block_proof_serialize(h_, b.data(), b.size());
        return b;
    }
    static BlockProof deserialize(const std::vector<uint8_t>& b) {
        frieda_block_proof* h = nullptr;
        check(frieda_block_proof_deserialize(b.data(), b.size(), &h));
        return BlockProof(h);
    }
    const frieda_block_proof* handle() const { return h_; }

  private:
    frieda_block_proof* h_ = nullptr;
};

// rho of a block: the Fiat-Shamir challenge over all its commitments, in order (frieda_block_challenge; host only)
inline QM31 block_challenge(const std::vector<Commitment>& commitments) {
    QM31 rho{};
    check(frieda_block_challenge(commitments.empty() ? nullptr : commitments.data()->data(), (uint32_t)commitments.size(), rho.v));
    return rho;
}
// The client's check of a block proof (frieda_verify_block; host only): true when accepted; *reason (optional) receives FRIEDA_BLOCK_OK
// or the first failing step, FRIEDA_BLOCK_SHAPE / _FRI / _INDICES / _BUNDLE / _COMBINATION.
inline bool verify_block(const std::vector<Commitment>& commitments, const BlockProof& bp, std::optional<uint64_t> seed, uint32_t* reason = nullptr) {
    int ok = 0;
    uint64_t s = seed.value_or(0);
    check(frieda_verify_block(commitments.empty() ? nullptr : commitments.data()->data(), (uint32_t)commitments.size(), bp.handle(), seed ? &s : nullptr, &ok, reason));
    return ok != 0;
}

class Context {
  public:
    explicit Context(int device = 0, void* stream = nullptr) { check(frieda_ctx_create(device, stream, &h_)); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { frieda_ctx_destroy(h_); }

    // a tuning / A-B option of this context alone, named like the environment variable that sets its default ("FRIEDA_HOST_DECOMMIT", ...)
    void set_option(const char* name, int64_t value) { check(frieda_ctx_set_option(h_, name, value), h_); }

    Commitment commit(const uint8_t* data, size_t len, uint32_t log_blowup_factor) {
        Commitment root;
        check(frieda_commit(h_, data, len, log_blowup_factor, root.data()), h_);
        return root;
    }
    std::pair<Commitment, Proof> commit_and_generate_proof(const uint8_t* data, size_t len, std::optional<uint64_t> seed,
                                                           const PcsConfig& cfg) {
        Commitment root;
        frieda_proof* p = nullptr;
        uint64_t s = seed.value_or(0);
        check(frieda_commit_and_generate_proof(h_, data, len, seed ? &s : nullptr, cfg.c(), root.data(), &p), h_);
        return {root, Proof(p)};
    }
    // `count` equal-length blobs, blob i at data + i * stride: every kernel is launched once for the whole batch
    std::vector<Commitment> commit_batch(const uint8_t* data, size_t stride, size_t len, uint32_t count, uint32_t log_blowup_factor) {
        std::vector<Commitment> roots(count);
        if (count) check(frieda_commit_batch(h_, data, stride, len, count, log_blowup_factor, roots.data()->data()), h_);
        return roots;
    }
    std::vector<std::pair<Commitment, Proof>> commit_and_generate_proof_batch(const uint8_t* data, size_t stride, size_t len, uint32_t count,
                                                                              const uint64_t* seeds_or_null, const PcsConfig& cfg) {
        std::vector<std::pair<Commitment, Proof>> out;
        if (!count) return out;
        std::vector<Commitment> roots(count);
        std::vector<frieda_proof*> ps(count, nullptr);
        check(frieda_commit_and_generate_proof_batch(h_, data, stride, len, count, seeds_or_null, cfg.c(), roots.data()->data(), ps.data()), h_);
        out.reserve(count);
        for (uint32_t i = 0; i < count; i++) out.emplace_back(roots[i], Proof(ps[i]));
        return out;
    }
    // One blob under many seeds (a provider serving sampling clients): encode once — encode_device for a blob already on the device
    // (frieda_encode_device) —, then proof i == commit_and_generate_proof(data, seeds[i], cfg).second byte for byte.  The split form
    // (frieda_prove_seeds_begin / frieda_prove_seeds_finish) overlaps two contexts; frieda_commit_and_generate_proofs_for_seeds is the
    // one-call convenience; frieda_seeds_workspace_bytes sizes a call.
    Encoded encode(const uint8_t* data, size_t len, uint32_t log_blowup_factor) {
        frieda_encoded* e = nullptr;
        check(frieda_encode(h_, data, len, log_blowup_factor, &e), h_);
        return Encoded(e);
    }
    Encoded encode_device(const void* d_data, size_t len, uint32_t log_blowup_factor) {
        frieda_encoded* e = nullptr;
        check(frieda_encode_device(h_, d_data, len, log_blowup_factor, &e), h_);
        return Encoded(e);
    }
    std::vector<Proof> prove_seeds(const Encoded& enc, const std::vector<uint64_t>& seeds, const PcsConfig& cfg) {
        std::vector<frieda_proof*> ps(seeds.size(), nullptr);
        check(frieda_prove_seeds(h_, enc.handle(), seeds.data(), (uint32_t)seeds.size(), cfg.c(), ps.data()), h_);
        std::vector<Proof> out;
        out.reserve(ps.size());
        for (frieda_proof* p : ps) out.emplace_back(p);
        return out;
    }
    // A block under many seeds in ONE call (frieda_prove_seeds_blobs): every handle of `encs` (one shape) under every seed of the one
    // list; proof b * seeds.size() + s == prove_seeds(*encs[b], {seeds[s]}, cfg)[0] byte for byte.  frieda_seeds_blobs_workspace_bytes sizes
    // a call; the split form is frieda_prove_seeds_blobs_begin / frieda_prove_seeds_blobs_finish.
    std::vector<Proof> prove_seeds_blobs(const std::vector<const Encoded*>& encs, const std::vector<uint64_t>& seeds, const PcsConfig& cfg) {
        std::vector<const frieda_encoded*> hs;
        hs.reserve(encs.size());
        for (const Encoded* e : encs) hs.push_back(e ? e->handle() : nullptr);
        std::vector<frieda_proof*> ps(encs.size() * seeds.size(), nullptr);
        check(frieda_prove_seeds_blobs(h_, hs.data(), (uint32_t)encs.size(), seeds.data(), (uint32_t)seeds.size(), cfg.c(), ps.data()), h_);
        std::vector<Proof> out;
        out.reserve(ps.size());
        for (frieda_proof* p : ps) out.emplace_back(p);
        return out;
    }
    // Block proofs (include/frieda_hip.h, "block proofs"): the aggregate handle of a block — once per block, whatever the seeds — and
    // one BlockProof per seed for the whole block: seeds.size() fold chains instead of encs.size() * seeds.size().
    Encoded aggregate_encoded(const std::vector<const Encoded*>& encs) {
        std::vector<const frieda_encoded*> hs;
        hs.reserve(encs.size());
        for (const Encoded* e : encs) hs.push_back(e ? e->handle() : nullptr);
        frieda_encoded* g = nullptr;
        check(frieda_aggregate_encoded(h_, hs.data(), (uint32_t)encs.size(), &g), h_);
        return Encoded(g);
    }
    std::vector<BlockProof> prove_block_seeds(const Encoded& agg, const std::vector<const Encoded*>& encs, const std::vector<uint64_t>& seeds,
                                              const PcsConfig& cfg) {
        std::vector<const frieda_encoded*> hs;
        hs.reserve(encs.size());
        for (const Encoded* e : encs) hs.push_back(e ? e->handle() : nullptr);
        std::vector<frieda_block_proof*> ps(seeds.size(), nullptr);
        check(frieda_prove_block_seeds(h_, agg.handle(), hs.data(), (uint32_t)encs.size(), seeds.data(), (uint32_t)seeds.size(), cfg.c(), ps.data()), h_);
        std::vector<BlockProof> out;
        out.reserve(ps.size());
        for (frieda_block_proof* p : ps) out.emplace_back(p);
        return out;
    }
    // Any list of jobs in ONE call (frieda_prove_jobs): proof j == prove_seeds(*encs[blob_index[j]], {seeds[j]}, cfg)[0] byte for byte,
    // in the caller's order; the call cuts itself into passes (frieda_prove_jobs_plan says how, frieda_prove_jobs_workspace_bytes sizes
    // a pass); the split, one-pass form is frieda_prove_jobs_begin / frieda_prove_jobs_finish.
    std::vector<Proof> prove_jobs(const std::vector<const Encoded*>& encs, const std::vector<uint32_t>& blob_index, const std::vector<uint64_t>& seeds,
                                  const PcsConfig& cfg) {
        if (blob_index.size() != seeds.size()) throw Error(FRIEDA_ERR_ARG, "prove_jobs: one seed per job");
        std::vector<const frieda_encoded*> hs;
        hs.reserve(encs.size());
        for (const Encoded* e : encs) hs.push_back(e ? e->handle() : nullptr);
        std::vector<frieda_proof*> ps(seeds.size(), nullptr);
        check(frieda_prove_jobs(h_, hs.data(), (uint32_t)encs.size(), blob_index.data(), seeds.data(), (uint32_t)seeds.size(), cfg.c(), ps.data()), h_);
        std::vector<Proof> out;
        out.reserve(ps.size());
        for (frieda_proof* p : ps) out.emplace_back(p);
        return out;
    }
    // The reconstructor's half of the README's sampling flow (/root/reference/README.md:56-69): any >= 2^log_coef + 2 distinct
    // (position, value) pairs of the bit-reversed codeword — e.g. pooled from api::verify_samples of proofs with different seeds —
    // give the blob's `len` bytes back (frieda_reconstruct_points_device: no linear system, every pair checked against the result;
    // pairs that are not values of one polynomial throw Error).  Repeated positions are ignored (the first one counts).
    std::vector<uint8_t> reconstruct_from_samples(const std::vector<uint32_t>& positions, const std::vector<QM31>& values, uint32_t log_coef,
                                                  uint32_t log_domain, size_t len) {
        if (positions.size() != values.size() || positions.empty()) throw Error(FRIEDA_ERR_ARG, "reconstruct_from_samples: one value per position");
        std::vector<uint32_t> flat(4 * values.size());
        for (size_t i = 0; i < values.size(); i++)
            for (int c = 0; c < 4; c++) flat[4 * i + c] = values[i].v[c];  // [n_points][4 columns][1 entry]
        DeviceBuffer d_cells(h_, 4 * flat.size()), d_out(h_, len + 8);
        check(frieda_dev_upload(h_, d_cells.ptr, flat.data(), 4 * flat.size()), h_);
        check(frieda_reconstruct_points_device(h_, static_cast<const uint32_t*>(d_cells.ptr), positions.data(), (uint32_t)positions.size(), 0, log_coef,
                                               log_domain, len, d_out.ptr),
              h_);
        std::vector<uint8_t> out(len);
        if (len) check(frieda_dev_download(h_, out.data(), d_out.ptr, len), h_);
        return out;
    }
    // Many proofs verified in one call on the GPU (frieda_verify_many): one status byte per proof — FRIEDA_VERIFY_REJECTED, FRIEDA_VERIFY_ACCEPTED,
    // FRIEDA_VERIFY_INVARIANT (api::verify would throw Panic), FRIEDA_VERIFY_WRONG_COMMITMENT — each what api::verify gives for that proof.
    // seeds: empty (None for all) or one per proof; expected_commitment: optional.
    std::vector<uint8_t> verify_many(const std::vector<const Proof*>& proofs, const std::vector<uint64_t>& seeds = {},
                                     const Commitment* expected_commitment = nullptr) {
        std::vector<uint8_t> status(proofs.size());
        if (proofs.empty()) return status;
        if (!seeds.empty() && seeds.size() != proofs.size()) throw Error(FRIEDA_ERR_ARG, "verify_many: one seed per proof");
        std::vector<const frieda_proof*> hs;
        for (const Proof* p : proofs) hs.push_back(p->handle());
        check(frieda_verify_many(h_, hs.data(), seeds.empty() ? nullptr : seeds.data(), (uint32_t)hs.size(),
                                 expected_commitment ? expected_commitment->data() : nullptr, status.data()),
              h_);
        return status;
    }
    // The proofs of a block against a table of commitments (frieda_verify_blobs_many): status[i] is what verify_many gives for proof i alone
    // with commitments[blob_index[i]] (FRIEDA_VERIFY_WRONG_COMMITMENT included); blob_index empty: proof i belongs to commitment i and
    // there is one proof per commitment.  accepted_per_blob (optional) receives per blob the number of ACCEPTED proofs that name it.
    // Error(FRIEDA_ERR_ARG) before anything runs: an index beyond the table, no index with proofs.size() != commitments.size(), proofs
    // but no commitments, a proof in flight on the context.
    std::vector<uint8_t> verify_blobs_many(const std::vector<const Proof*>& proofs, const std::vector<Commitment>& commitments,
                                           const std::vector<uint32_t>& blob_index = {}, const std::vector<uint64_t>& seeds = {},
                                           std::vector<uint32_t>* accepted_per_blob = nullptr) {
        if (!seeds.empty() && seeds.size() != proofs.size()) throw Error(FRIEDA_ERR_ARG, "verify_blobs_many: one seed per proof");
        if (!blob_index.empty() && blob_index.size() != proofs.size()) throw Error(FRIEDA_ERR_ARG, "verify_blobs_many: one blob index per proof");
        std::vector<const frieda_proof*> hs;
        for (const Proof* p : proofs) hs.push_back(p->handle());
        std::vector<uint8_t> table(32 * commitments.size() + 1), status(hs.size());
        for (size_t b = 0; b < commitments.size(); b++) std::copy(commitments[b].begin(), commitments[b].end(), table.begin() + 32 * b);
        std::vector<uint32_t> acc(commitments.size());
        check(frieda_verify_blobs_many(h_, hs.data(), seeds.empty() ? nullptr : seeds.data(), (uint32_t)hs.size(), table.data(),
                                       (uint32_t)commitments.size(), blob_index.empty() ? nullptr : blob_index.data(), status.data(), acc.data()),
              h_);
        if (accepted_per_blob) *accepted_per_blob = acc;
        return status;
    }
    // the same as verify_many + the positions every accepted proof sampled (frieda_verify_samples_many; empty for a proof that is not accepted)
    std::pair<std::vector<uint8_t>, std::vector<std::vector<uint32_t>>> verify_samples_many(const std::vector<const Proof*>& proofs,
                                                                                            const std::vector<uint64_t>& seeds = {},
                                                                                            const Commitment* expected_commitment = nullptr) {
        std::vector<uint8_t> status(proofs.size());
        std::vector<std::vector<uint32_t>> out(proofs.size());
        if (proofs.empty()) return {status, out};
        if (!seeds.empty() && seeds.size() != proofs.size()) throw Error(FRIEDA_ERR_ARG, "verify_samples_many: one seed per proof");
        std::vector<const frieda_proof*> hs;
        size_t pitch = 1;
        for (const Proof* p : proofs) {
            hs.push_back(p->handle());
            pitch = std::max<size_t>(pitch, frieda_proof_pcs_config(p->handle()).n_queries);
        }
        std::vector<uint32_t> pos(pitch * hs.size()), n(hs.size());
        check(frieda_verify_samples_many(h_, hs.data(), seeds.empty() ? nullptr : seeds.data(), (uint32_t)hs.size(),
                                         expected_commitment ? expected_commitment->data() : nullptr, status.data(), pos.data(), pitch, n.data()),
              h_);
        for (size_t i = 0; i < hs.size(); i++) out[i].assign(pos.begin() + i * pitch, pos.begin() + i * pitch + n[i]);
        return {status, out};
    }
    // the sampling client's whole flow (frieda_reconstruct_from_proofs): verify against the commitment, pool the verified samples, rebuild
    // the blob's `len` bytes and check that they commit to expected_commitment; throws Error when the verified points do not suffice
    std::vector<uint8_t> reconstruct_from_proofs(const std::vector<const Proof*>& proofs, const std::vector<uint64_t>& seeds,
                                                 const Commitment& expected_commitment, size_t len, std::vector<uint8_t>* out_status = nullptr,
                                                 size_t* n_points = nullptr) {
        if (!seeds.empty() && seeds.size() != proofs.size()) throw Error(FRIEDA_ERR_ARG, "reconstruct_from_proofs: one seed per proof");
        std::vector<const frieda_proof*> hs;
        for (const Proof* p : proofs) hs.push_back(p->handle());
        std::vector<uint8_t> status(hs.size() + 1), out(len + 1);
        size_t np = 0;
        const int rc = frieda_reconstruct_from_proofs(h_, hs.data(), seeds.empty() ? nullptr : seeds.data(), (uint32_t)hs.size(), expected_commitment.data(),
                                                      len, out.data(), status.data(), &np);
        status.resize(hs.size());
        if (out_status) *out_status = status;
        if (n_points) *n_points = np;
        check(rc, h_);
        out.resize(len);
        return out;
    }
    // every point the accepted proofs authenticate (frieda_verify_pairs_many): per proof the ascending positions of both members of every
    // opened first-layer pair and their values; empty for a proof that is not accepted
    struct PairRows {
        std::vector<uint8_t> status;
        std::vector<std::vector<uint32_t>> positions;
        std::vector<std::vector<QM31>> values;
    };
    PairRows verify_pairs_many(const std::vector<const Proof*>& proofs, const std::vector<uint64_t>& seeds = {}, const Commitment* expected_commitment = nullptr) {
        PairRows out{std::vector<uint8_t>(proofs.size()), std::vector<std::vector<uint32_t>>(proofs.size()), std::vector<std::vector<QM31>>(proofs.size())};
        if (proofs.empty()) return out;
        if (!seeds.empty() && seeds.size() != proofs.size()) throw Error(FRIEDA_ERR_ARG, "verify_pairs_many: one seed per proof");
        std::vector<const frieda_proof*> hs;
        size_t pitch = 1;
        for (const Proof* p : proofs) {
            hs.push_back(p->handle());
            pitch = std::max<size_t>(pitch, 2 * (size_t)frieda_proof_pcs_config(p->handle()).n_queries);
        }
        std::vector<uint32_t> pos(pitch * hs.size()), val(4 * pitch * hs.size()), n(hs.size());
        check(frieda_verify_pairs_many(h_, hs.data(), seeds.empty() ? nullptr : seeds.data(), (uint32_t)hs.size(),
                                       expected_commitment ? expected_commitment->data() : nullptr, out.status.data(), pos.data(), val.data(), pitch, n.data()),
              h_);
        for (size_t i = 0; i < hs.size(); i++) {
            out.positions[i].assign(pos.begin() + i * pitch, pos.begin() + i * pitch + n[i]);
            out.values[i].resize(n[i]);
            for (size_t j = 0; j < n[i]; j++)
                for (int c = 0; c < 4; c++) out.values[i][j].v[c] = val[4 * (i * pitch + j) + c];
        }
        return out;
    }
    // frieda_reconstruct_from_proof_pairs: reconstruct_from_proofs with the pair points as the pool (about half as many proofs needed)
    std::vector<uint8_t> reconstruct_from_proof_pairs(const std::vector<const Proof*>& proofs, const std::vector<uint64_t>& seeds,
                                                      const Commitment& expected_commitment, size_t len, std::vector<uint8_t>* out_status = nullptr,
                                                      size_t* n_points = nullptr) {
        if (!seeds.empty() && seeds.size() != proofs.size()) throw Error(FRIEDA_ERR_ARG, "reconstruct_from_proof_pairs: one seed per proof");
        std::vector<const frieda_proof*> hs;
        for (const Proof* p : proofs) hs.push_back(p->handle());
        std::vector<uint8_t> status(hs.size() + 1), out(len + 1);
        size_t np = 0;
        const int rc = frieda_reconstruct_from_proof_pairs(h_, hs.data(), seeds.empty() ? nullptr : seeds.data(), (uint32_t)hs.size(),
                                                           expected_commitment.data(), len, out.data(), status.data(), &np);
        status.resize(hs.size());
        if (out_status) *out_status = status;
        if (n_points) *n_points = np;
        check(rc, h_);
        out.resize(len);
        return out;
    }
    // ---- authenticated cells (frieda_open_cells, frieda_verify_cells*, frieda_reconstruct_from_opened_cells) ----
    // values[n_cells][4][2^log_cell] cell-major, paths[n_cells][log_domain - log_cell][32] bottom-up
    struct OpenedCells {
        std::vector<uint32_t> values;
        std::vector<uint8_t> paths;
    };
    // a short vector must not reach the library: values / paths have exactly the shape of the cell list
    static void check_cell_shapes(const char* who, uint32_t log_domain, uint32_t log_cell, size_t n_cells, size_t n_values, size_t n_path_bytes) {
        if (log_cell > log_domain || log_cell > FRIEDA_MAX_LOG_OPEN_CELL) throw Error(FRIEDA_ERR_ARG, std::string(who) + ": log_cell out of range");
        if (n_values != (n_cells * 4) << log_cell || n_path_bytes != n_cells * 32 * (size_t)(log_domain - log_cell))
            throw Error(FRIEDA_ERR_ARG, std::string(who) + ": values / paths do not have the shape of the cell list");
    }
    OpenedCells open_cells(const Encoded& enc, uint32_t log_cell, const std::vector<uint32_t>& cell_index) {
        const uint32_t n = enc.shape().second;
        if (log_cell > n) throw Error(FRIEDA_ERR_ARG, "open_cells: log_cell beyond log_domain");
        OpenedCells out{std::vector<uint32_t>((cell_index.size() * 4) << log_cell), std::vector<uint8_t>(cell_index.size() * 32 * (n - log_cell))};
        check(frieda_open_cells(h_, enc.handle(), log_cell, cell_index.data(), (uint32_t)cell_index.size(), out.values.data(), out.paths.data()), h_);
        return out;
    }
    // one status byte per cell (FRIEDA_CELL_ACCEPTED / _REJECTED), verified on the GPU; verify_cells below is the host form
    std::vector<uint8_t> verify_cells_many(const Commitment& commitment, uint32_t log_domain, uint32_t log_cell, const std::vector<uint32_t>& cell_index,
                                           const std::vector<uint32_t>& values, const std::vector<uint8_t>& paths) {
        check_cell_shapes("verify_cells_many", log_domain, log_cell, cell_index.size(), values.size(), paths.size());
        std::vector<uint8_t> status(cell_index.size());
        check(frieda_verify_cells_many(h_, commitment.data(), log_domain, log_cell, cell_index.data(), (uint32_t)cell_index.size(), values.data(), paths.data(),
                                       status.data()),
              h_);
        return status;
    }
    std::vector<uint8_t> reconstruct_from_opened_cells(const Commitment& commitment, uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                                       const std::vector<uint32_t>& cell_index, const std::vector<uint32_t>& values,
                                                       const std::vector<uint8_t>& paths, std::vector<uint8_t>* out_status = nullptr,
                                                       size_t* n_cells_used = nullptr) {
        size_t n_felts = 0, n_padded = 0;
        uint32_t log_size = 0;
        check(frieda_codec_shape(len, &n_felts, &n_padded, &log_size));
        check_cell_shapes("reconstruct_from_opened_cells", log_size + log_blowup_factor, log_cell, cell_index.size(), values.size(), paths.size());
        std::vector<uint8_t> status(cell_index.size() + 1), out(len + 1);
        size_t used = 0;
        const int rc = frieda_reconstruct_from_opened_cells(h_, commitment.data(), log_blowup_factor, len, log_cell, cell_index.data(), (uint32_t)cell_index.size(),
                                                            values.data(), paths.data(), out.data(), status.data(), &used);
        status.resize(cell_index.size());
        if (out_status) *out_status = status;
        if (n_cells_used) *n_cells_used = used;
        check(rc, h_);
        out.resize(len);
        return out;
    }
    // ---- the cells of a block: many blobs of one shape in one call (frieda_open_cells_blobs, frieda_verify_cells_blobs*,
    // frieda_reconstruct_blobs_from_opened_stripes).  Cell i of a call is cell cell_index[i] of blob blob_index[i].
    static std::vector<uint8_t> flat_commitments(const std::vector<Commitment>& commitments) {
        std::vector<uint8_t> flat(32 * commitments.size());
        for (size_t b = 0; b < commitments.size(); b++) std::copy(commitments[b].begin(), commitments[b].end(), flat.begin() + 32 * b);
        return flat;
    }
    OpenedCells open_cells_blobs(const std::vector<const Encoded*>& encs, uint32_t log_cell, const std::vector<uint32_t>& blob_index,
                                 const std::vector<uint32_t>& cell_index) {
        if (encs.empty() || blob_index.size() != cell_index.size()) throw Error(FRIEDA_ERR_ARG, "open_cells_blobs: one blob number per cell, at least one blob");
        std::vector<const frieda_encoded*> handles;
        for (const Encoded* e : encs) handles.push_back(e ? e->handle() : nullptr);
        if (!encs[0]) throw Error(FRIEDA_ERR_ARG, "open_cells_blobs: null blob");
        const uint32_t n = encs[0]->shape().second;
        if (log_cell > n) throw Error(FRIEDA_ERR_ARG, "open_cells_blobs: log_cell beyond log_domain");
        OpenedCells out{std::vector<uint32_t>((cell_index.size() * 4) << log_cell), std::vector<uint8_t>(cell_index.size() * 32 * (n - log_cell))};
        check(frieda_open_cells_blobs(h_, handles.data(), (uint32_t)handles.size(), log_cell, blob_index.data(), cell_index.data(), (uint32_t)cell_index.size(),
                                      out.values.data(), out.paths.data()),
              h_);
        return out;
    }
    std::vector<uint8_t> verify_cells_blobs_many(const std::vector<Commitment>& commitments, uint32_t log_domain, uint32_t log_cell,
                                                 const std::vector<uint32_t>& blob_index, const std::vector<uint32_t>& cell_index,
                                                 const std::vector<uint32_t>& values, const std::vector<uint8_t>& paths) {
        if (blob_index.size() != cell_index.size()) throw Error(FRIEDA_ERR_ARG, "verify_cells_blobs_many: one blob number per cell");
        check_cell_shapes("verify_cells_blobs_many", log_domain, log_cell, cell_index.size(), values.size(), paths.size());
        const std::vector<uint8_t> flat = flat_commitments(commitments);
        std::vector<uint8_t> status(cell_index.size());
        check(frieda_verify_cells_blobs_many(h_, flat.data(), (uint32_t)commitments.size(), log_domain, log_cell, blob_index.data(), cell_index.data(),
                                             (uint32_t)cell_index.size(), values.data(), paths.data(), status.data()),
              h_);
        return status;
    }
    // values[n_stripes][n_blobs][4][2^log_cell], paths[n_stripes][n_blobs][log_domain - log_cell][32] -> blob b's bytes at [b]
    std::vector<std::vector<uint8_t>> reconstruct_blobs_from_opened_stripes(const std::vector<Commitment>& commitments, uint32_t log_blowup_factor, size_t len,
                                                                            uint32_t log_cell, const std::vector<uint32_t>& stripe_index,
                                                                            const std::vector<uint32_t>& values, const std::vector<uint8_t>& paths,
                                                                            std::vector<uint8_t>* out_status = nullptr, size_t* n_stripes_used = nullptr) {
        size_t n_felts = 0, n_padded = 0;
        uint32_t log_size = 0;
        check(frieda_codec_shape(len, &n_felts, &n_padded, &log_size));
        const size_t K = commitments.size(), cells = stripe_index.size() * K;
        check_cell_shapes("reconstruct_blobs_from_opened_stripes", log_size + log_blowup_factor, log_cell, cells, values.size(), paths.size());
        const std::vector<uint8_t> flat = flat_commitments(commitments);
        std::vector<uint8_t> status(cells + 1), out(len * K + 1);
        size_t used = 0;
        const int rc = frieda_reconstruct_blobs_from_opened_stripes(h_, flat.data(), (uint32_t)K, log_blowup_factor, len, log_cell, stripe_index.data(),
                                                                    (uint32_t)stripe_index.size(), values.data(), paths.data(), out.data(), status.data(), &used);
        status.resize(cells);
        if (out_status) *out_status = status;
        if (n_stripes_used) *n_stripes_used = used;
        check(rc, h_);
        std::vector<std::vector<uint8_t>> blobs(K);
        for (size_t b = 0; b < K; b++) blobs[b].assign(out.begin() + b * len, out.begin() + (b + 1) * len);
        return blobs;
    }
    // ---- stripe bundles: k stripes of a block under one shared hash witness per blob (frieda_open_stripe_bundles,
    // frieda_verify_stripe_bundles*, frieda_reconstruct_blobs_from_stripe_bundles).  Stripe t of a call belongs to bundle b when
    // bundle_first[b] <= t < bundle_first[b + 1]; values[stripes][K][4][2^log_cell]; witness_first counts hashes per blob; bundle b's witness
    // block starts at hash K * witness_first[b], blob j's piece lies j * W_b hashes into it.
    struct OpenedStripeBundles {
        std::vector<uint32_t> values;
        std::vector<uint8_t> witness;         // K * witness_first.back() hashes of 32 bytes
        std::vector<uint64_t> witness_first;  // [n_bundles + 1]
    };
    // the sizes a stripe-bundles call reads: a short array must not reach the library
    static void check_stripe_bundle_shapes(const char* fn, size_t K, uint32_t log_cell, const std::vector<uint32_t>& stripe_index,
                                           const std::vector<uint32_t>& bundle_first, size_t n_values, size_t n_witness_bytes,
                                           const std::vector<uint64_t>* witness_first) {
        if (K == 0 || bundle_first.empty() || bundle_first.back() > stripe_index.size() || log_cell > FRIEDA_MAX_LOG_OPEN_CELL)
            throw Error(FRIEDA_ERR_ARG, std::string(fn) + ": bundle_first has n_bundles + 1 entries, none beyond the stripe list");
        if (!witness_first) return;
        if (witness_first->size() != bundle_first.size() || n_values != ((stripe_index.size() * K * 4) << log_cell))
            throw Error(FRIEDA_ERR_ARG, std::string(fn) + ": values / witness_first do not have the shape of the stripe list");
        for (uint64_t w : *witness_first)
            if (w > n_witness_bytes / 32 / K) throw Error(FRIEDA_ERR_ARG, std::string(fn) + ": witness_first beyond the witness");
    }
    OpenedStripeBundles open_stripe_bundles(const std::vector<const Encoded*>& encs, uint32_t log_cell, const std::vector<uint32_t>& stripe_index,
                                            const std::vector<uint32_t>& bundle_first) {
        std::vector<const frieda_encoded*> handles;
        for (const Encoded* e : encs) handles.push_back(e ? e->handle() : nullptr);
        check_stripe_bundle_shapes("open_stripe_bundles", encs.size(), log_cell, stripe_index, bundle_first, 0, 0, nullptr);
        const uint32_t nb = (uint32_t)bundle_first.size() - 1, K = (uint32_t)handles.size();
        OpenedStripeBundles out;
        out.witness_first.assign(nb + 1, 0);
        if (nb == 0) return out;
        check(frieda_open_stripe_bundles(h_, handles.data(), K, log_cell, stripe_index.data(), bundle_first.data(), nb, nullptr, nullptr, 0, out.witness_first.data()), h_);
        const size_t total = (size_t)K * out.witness_first.back();
        out.values.resize(((stripe_index.size() * K * 4) << log_cell) + 1);
        out.witness.resize(32 * total + 1);
        check(frieda_open_stripe_bundles(h_, handles.data(), K, log_cell, stripe_index.data(), bundle_first.data(), nb, out.values.data(), out.witness.data(), total,
                                         out.witness_first.data()),
              h_);
        out.values.resize(out.values.size() - 1), out.witness.resize(32 * total);
        return out;
    }
    // status[n_bundles][K]
    std::vector<uint8_t> verify_stripe_bundles_many(const std::vector<Commitment>& commitments, uint32_t log_domain, uint32_t log_cell,
                                                    const std::vector<uint32_t>& stripe_index, const std::vector<uint32_t>& bundle_first,
                                                    const std::vector<uint32_t>& values, const std::vector<uint8_t>& witness,
                                                    const std::vector<uint64_t>& witness_first) {
        const size_t K = commitments.size();
        check_stripe_bundle_shapes("verify_stripe_bundles_many", K, log_cell, stripe_index, bundle_first, values.size(), witness.size(), &witness_first);
        const std::vector<uint8_t> flat = flat_commitments(commitments);
        const uint32_t nb = (uint32_t)bundle_first.size() - 1;
        std::vector<uint8_t> status((size_t)nb * K + 1);
        check(frieda_verify_stripe_bundles_many(h_, flat.data(), (uint32_t)K, log_domain, log_cell, stripe_index.data(), bundle_first.data(), nb, values.data(),
                                                witness.data(), witness_first.data(), status.data()),
              h_);
        status.resize((size_t)nb * K);
        return status;
    }
    std::vector<std::vector<uint8_t>> reconstruct_blobs_from_stripe_bundles(const std::vector<Commitment>& commitments, uint32_t log_blowup_factor, size_t len,
                                                                            uint32_t log_cell, const std::vector<uint32_t>& stripe_index,
                                                                            const std::vector<uint32_t>& bundle_first, const std::vector<uint32_t>& values,
                                                                            const std::vector<uint8_t>& witness, const std::vector<uint64_t>& witness_first,
                                                                            std::vector<uint8_t>* out_status = nullptr, size_t* n_stripes_used = nullptr) {
        const size_t K = commitments.size();
        check_stripe_bundle_shapes("reconstruct_blobs_from_stripe_bundles", K, log_cell, stripe_index, bundle_first, values.size(), witness.size(), &witness_first);
        const std::vector<uint8_t> flat = flat_commitments(commitments);
        const uint32_t nb = (uint32_t)bundle_first.size() - 1;
        std::vector<uint8_t> status((size_t)nb * K + 1), out(len * K + 1);
        size_t used = 0;
        const int rc = frieda_reconstruct_blobs_from_stripe_bundles(h_, flat.data(), (uint32_t)K, log_blowup_factor, len, log_cell, stripe_index.data(),
                                                                    bundle_first.data(), nb, values.data(), witness.data(), witness_first.data(), out.data(),
                                                                    status.data(), &used);
        status.resize((size_t)nb * K);
        if (out_status) *out_status = status;
        if (n_stripes_used) *n_stripes_used = used;
        check(rc, h_);
        std::vector<std::vector<uint8_t>> blobs(K);
        for (size_t b = 0; b < K; b++) blobs[b].assign(out.begin() + b * len, out.begin() + (b + 1) * len);
        return blobs;
    }
    // ---- encoded handles for a block in one call, and straight from a rebuild (frieda_encode_batch, frieda_rebuild_encoded_*): the
    // handles of a call share one reference-counted allocation; every Encoded frees its own share's reference ----
    // blob b at data + b * stride
    std::vector<Encoded> encode_batch(const uint8_t* data, size_t stride, size_t len, uint32_t count, uint32_t log_blowup_factor) {
        std::vector<frieda_encoded*> hs(count, nullptr);
        check(frieda_encode_batch(h_, data, stride, len, count, log_blowup_factor, hs.data()), h_);
        return adopt(hs);
    }
    // what a rebuild_encoded_* call returns: the twin's bytes (empty with want_bytes = false: nothing is packed or downloaded) and the handles
    struct RebuiltEncoded {
        std::vector<std::vector<uint8_t>> bytes;
        std::vector<Encoded> encs;
    };
    RebuiltEncoded rebuild_encoded_from_opened_cells(const Commitment& commitment, uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                                     const std::vector<uint32_t>& cell_index, const std::vector<uint32_t>& values,
                                                     const std::vector<uint8_t>& paths, bool want_bytes = true, std::vector<uint8_t>* out_status = nullptr,
                                                     size_t* n_cells_used = nullptr) {
        size_t n_felts = 0, n_padded = 0;
        uint32_t log_size = 0;
        check(frieda_codec_shape(len, &n_felts, &n_padded, &log_size));
        check_cell_shapes("rebuild_encoded_from_opened_cells", log_size + log_blowup_factor, log_cell, cell_index.size(), values.size(), paths.size());
        std::vector<uint8_t> status(cell_index.size() + 1), out(len + 1);
        size_t used = 0;
        frieda_encoded* e = nullptr;
        const int rc = frieda_rebuild_encoded_from_opened_cells(h_, commitment.data(), log_blowup_factor, len, log_cell, cell_index.data(),
                                                                (uint32_t)cell_index.size(), values.data(), paths.data(), want_bytes ? out.data() : nullptr,
                                                                status.data(), &used, &e);
        return rebuilt(rc, 1, len, want_bytes, out, status, cell_index.size(), used, &e, out_status, n_cells_used);
    }
    RebuiltEncoded rebuild_encoded_from_cell_bundles(const Commitment& commitment, uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                                     const std::vector<uint32_t>& cell_index, const std::vector<uint32_t>& bundle_first,
                                                     const std::vector<uint32_t>& values, const std::vector<uint8_t>& witness,
                                                     const std::vector<uint64_t>& witness_first, bool want_bytes = true,
                                                     std::vector<uint8_t>* out_status = nullptr, size_t* n_cells_used = nullptr) {
        check_stripe_bundle_shapes("rebuild_encoded_from_cell_bundles", 1, log_cell, cell_index, bundle_first, values.size(), witness.size(), &witness_first);
        const uint32_t nb = (uint32_t)bundle_first.size() - 1;
        std::vector<uint8_t> status((size_t)nb + 1), out(len + 1);
        size_t used = 0;
        frieda_encoded* e = nullptr;
        const int rc = frieda_rebuild_encoded_from_cell_bundles(h_, commitment.data(), log_blowup_factor, len, log_cell, cell_index.data(), bundle_first.data(), nb,
                                                                values.data(), witness.data(), witness_first.data(), want_bytes ? out.data() : nullptr,
                                                                status.data(), &used, &e);
        return rebuilt(rc, 1, len, want_bytes, out, status, nb, used, &e, out_status, n_cells_used);
    }
    RebuiltEncoded rebuild_encoded_blobs_from_opened_stripes(const std::vector<Commitment>& commitments, uint32_t log_blowup_factor, size_t len,
                                                             uint32_t log_cell, const std::vector<uint32_t>& stripe_index, const std::vector<uint32_t>& values,
                                                             const std::vector<uint8_t>& paths, bool want_bytes = true,
                                                             std::vector<uint8_t>* out_status = nullptr, size_t* n_stripes_used = nullptr) {
        size_t n_felts = 0, n_padded = 0;
        uint32_t log_size = 0;
        check(frieda_codec_shape(len, &n_felts, &n_padded, &log_size));
        const size_t K = commitments.size(), cells = stripe_index.size() * K;
        if (K == 0) throw Error(FRIEDA_ERR_ARG, "rebuild_encoded_blobs_from_opened_stripes: at least one blob");
        check_cell_shapes("rebuild_encoded_blobs_from_opened_stripes", log_size + log_blowup_factor, log_cell, cells, values.size(), paths.size());
        const std::vector<uint8_t> flat = flat_commitments(commitments);
        std::vector<uint8_t> status(cells + 1), out(len * K + 1);
        size_t used = 0;
        std::vector<frieda_encoded*> es(K, nullptr);
        const int rc = frieda_rebuild_encoded_blobs_from_opened_stripes(h_, flat.data(), (uint32_t)K, log_blowup_factor, len, log_cell, stripe_index.data(),
                                                                        (uint32_t)stripe_index.size(), values.data(), paths.data(),
                                                                        want_bytes ? out.data() : nullptr, status.data(), &used, es.data());
        return rebuilt(rc, K, len, want_bytes, out, status, cells, used, es.data(), out_status, n_stripes_used);
    }
    RebuiltEncoded rebuild_encoded_blobs_from_stripe_bundles(const std::vector<Commitment>& commitments, uint32_t log_blowup_factor, size_t len,
                                                             uint32_t log_cell, const std::vector<uint32_t>& stripe_index,
                                                             const std::vector<uint32_t>& bundle_first, const std::vector<uint32_t>& values,
                                                             const std::vector<uint8_t>& witness, const std::vector<uint64_t>& witness_first,
                                                             bool want_bytes = true, std::vector<uint8_t>* out_status = nullptr,
                                                             size_t* n_stripes_used = nullptr) {
        const size_t K = commitments.size();
        check_stripe_bundle_shapes("rebuild_encoded_blobs_from_stripe_bundles", K, log_cell, stripe_index, bundle_first, values.size(), witness.size(), &witness_first);
        const std::vector<uint8_t> flat = flat_commitments(commitments);
        const uint32_t nb = (uint32_t)bundle_first.size() - 1;
        std::vector<uint8_t> status((size_t)nb * K + 1), out(len * K + 1);
        size_t used = 0;
        std::vector<frieda_encoded*> es(K, nullptr);
        const int rc = frieda_rebuild_encoded_blobs_from_stripe_bundles(h_, flat.data(), (uint32_t)K, log_blowup_factor, len, log_cell, stripe_index.data(),
                                                                        bundle_first.data(), nb, values.data(), witness.data(), witness_first.data(),
                                                                        want_bytes ? out.data() : nullptr, status.data(), &used, es.data());
        return rebuilt(rc, K, len, want_bytes, out, status, (size_t)nb * K, used, es.data(), out_status, n_stripes_used);
    }

  private:
    static std::vector<Encoded> adopt(const std::vector<frieda_encoded*>& hs) {
        std::vector<Encoded> out;
        out.reserve(hs.size());  // (no throw between here and the last adoption: reserve did the allocating)
        for (frieda_encoded* h : hs) out.emplace_back(h);
        return out;
    }
    // the shared tail of the rebuild_encoded_* wrappers: statuses and counts out first (also on an error), then the check, then the results
    RebuiltEncoded rebuilt(int rc, size_t K, size_t len, bool want_bytes, const std::vector<uint8_t>& out, std::vector<uint8_t>& status, size_t n_status,
                           size_t used, frieda_encoded* const* es, std::vector<uint8_t>* out_status, size_t* n_used) {
        status.resize(n_status);
        if (out_status) *out_status = status;
        if (n_used) *n_used = used;
        check(rc, h_);
        RebuiltEncoded r;
        r.encs = adopt(std::vector<frieda_encoded*>(es, es + K));
        if (want_bytes) {
            r.bytes.resize(K);
            for (size_t b = 0; b < K; b++) r.bytes[b].assign(out.begin() + b * len, out.begin() + (b + 1) * len);
        }
        return r;
    }

  public:
    // Level B openings over caller device buffers (frieda_dev_gather, frieda_dev_gather_hashes, frieda_merkle_decommit)
    // rows[i * ncols + c] = column c at idx[i]
    std::vector<uint32_t> dev_gather(const uint32_t* d_cols, size_t stride, uint32_t ncols, const std::vector<uint64_t>& idx) {
        std::vector<uint32_t> out(idx.size() * ncols);
        check(frieda_dev_gather(h_, d_cols, stride, ncols, idx.data(), idx.size(), out.data()), h_);
        return out;
    }
    std::vector<std::array<uint8_t, 32>> dev_gather_hashes(const void* d_layer, size_t layer_len, const std::vector<uint64_t>& idx) {
        std::vector<std::array<uint8_t, 32>> out(idx.size());
        check(frieda_dev_gather_hashes(h_, d_layer, layer_len, idx.data(), idx.size(), idx.empty() ? nullptr : out.data()->data()), h_);
        return out;
    }
    // MerkleProver::decommit of a leaf-columns tree: {queried values [n_pos * ncols], hash witness}
    std::pair<std::vector<uint32_t>, std::vector<std::array<uint8_t, 32>>> merkle_decommit(const std::vector<const void*>& d_layers, uint32_t log_size,
                                                                                           const uint32_t* d_cols, uint32_t ncols, size_t stride,
                                                                                           const std::vector<uint32_t>& positions) {
        std::vector<uint32_t> values(positions.size() * ncols);
        size_t n = 0;
        const size_t bound = positions.size() * (size_t)log_size;
        std::vector<std::array<uint8_t, 32>> hashes(bound);
        check(frieda_merkle_decommit(h_, d_layers.data(), log_size, d_cols, ncols, stride, positions.data(), positions.size(), values.data(),
                                     bound ? hashes.data()->data() : nullptr, bound, &n),
              h_);
        hashes.resize(n);
        return {values, hashes};
    }
    frieda_ctx* handle() { return h_; }

  private:
    struct DeviceBuffer {  // frieda_dev_alloc / frieda_dev_free (Level B column storage), scoped
        frieda_ctx* ctx;
        void* ptr = nullptr;
        DeviceBuffer(frieda_ctx* c, size_t bytes) : ctx(c) { check(frieda_dev_alloc(c, bytes ? bytes : 1, &ptr), c); }
        DeviceBuffer(const DeviceBuffer&) = delete;
        DeviceBuffer& operator=(const DeviceBuffer&) = delete;
        ~DeviceBuffer() { frieda_dev_free(ctx, ptr); }
    };
    frieda_ctx* h_ = nullptr;
};

// A batch of independent blobs across the GPUs of one node (frieda_multi): blob i -> devices[i mod n]; roots gathered with RCCL.
class MultiContext {
  public:
    explicit MultiContext(const std::vector<int>& devices) { check(frieda_multi_create(devices.data(), (uint32_t)devices.size(), &h_)); }
    MultiContext(const MultiContext&) = delete;
    MultiContext& operator=(const MultiContext&) = delete;
    ~MultiContext() { frieda_multi_destroy(h_); }

    frieda_multi* handle() { return h_; }  // for the C entry points this class does not wrap (owned by the object)
    bool uses_rccl() const { return frieda_multi_uses_rccl(h_) != 0; }
    uint64_t gather_count() const { return frieda_multi_gather_count(h_); }
    uint32_t device_count() const { return frieda_multi_device_count(h_); }
    // a tuning option (frieda_ctx_set_option) on device slot d, e.g. the batch policy's "FRIEDA_BATCH_BUDGET_MB"
    void set_option(uint32_t device_slot, const char* name, int64_t value) {
        frieda_ctx* c = frieda_multi_ctx(h_, device_slot);
        if (!c) throw Error(FRIEDA_ERR_ARG, "no such device slot");
        check(frieda_ctx_set_option(c, name, value));
    }
    // hands the device workspaces the handle keeps between calls (two per device, up to the batch budget each) back; the next call allocates again
    void release_workspace() { mcheck(frieda_multi_release_workspace(h_)); }
    // the CPUs the worker thread of device slot d is pinned to (its GPU's NUMA node); empty: not pinned
    std::vector<int> near_cpus(uint32_t device_slot) const {
        std::vector<int> v(frieda_multi_near_cpus(h_, device_slot, nullptr, 0));
        if (!v.empty()) frieda_multi_near_cpus(h_, device_slot, v.data(), v.size());
        return v;
    }
    std::vector<Commitment> commit_many(const std::vector<std::vector<uint8_t>>& blobs, uint32_t log_blowup_factor) {
        std::vector<const uint8_t*> ptrs;
        std::vector<size_t> lens;
        for (const auto& b : blobs) ptrs.push_back(b.data()), lens.push_back(b.size());
        std::vector<Commitment> roots(blobs.size());
        if (!blobs.empty()) mcheck(frieda_commit_many(h_, ptrs.data(), lens.data(), (uint32_t)blobs.size(), log_blowup_factor, roots.data()->data()));
        return roots;
    }
    std::vector<std::pair<Commitment, Proof>> prove_many(const std::vector<std::vector<uint8_t>>& blobs, const uint64_t* seeds_or_null,
                                                         const PcsConfig& cfg) {
        std::vector<const uint8_t*> ptrs;
        std::vector<size_t> lens;
        for (const auto& b : blobs) ptrs.push_back(b.data()), lens.push_back(b.size());
        std::vector<std::pair<Commitment, Proof>> out;
        if (blobs.empty()) return out;
        std::vector<Commitment> roots(blobs.size());
        std::vector<frieda_proof*> ps(blobs.size(), nullptr);
        mcheck(frieda_prove_many(h_, ptrs.data(), lens.data(), (uint32_t)blobs.size(), seeds_or_null, cfg.c(), roots.data()->data(), ps.data()));
        for (size_t i = 0; i < blobs.size(); i++) out.emplace_back(roots[i], Proof(ps[i]));
        return out;
    }

  private:
    void mcheck(int status) {
        if (status == FRIEDA_OK) return;
        const std::string detail = frieda_multi_last_error(h_);
        if (status == FRIEDA_ERR_INVARIANT) throw Panic(status, detail);
        throw Error(status, detail);
    }
    frieda_multi* h_ = nullptr;
};

inline Context& default_context() {
    thread_local Context ctx(0);
    return ctx;
}

namespace proof {
inline std::pair<Commitment, Proof> commit_and_generate_proof(const std::vector<uint8_t>& data, std::optional<uint64_t> seed,
                                                              const PcsConfig& cfg) {
    return default_context().commit_and_generate_proof(data.data(), data.size(), seed, cfg);
}
}  // namespace proof

namespace api {
inline Commitment commit(const std::vector<uint8_t>& data, uint32_t log_blowup_factor) {
    return default_context().commit(data.data(), data.size(), log_blowup_factor);
}
inline Proof generate_proof(const std::vector<uint8_t>& data, std::optional<uint64_t> seed, const PcsConfig& cfg) {
    return proof::commit_and_generate_proof(data, seed, cfg).second;
}
inline bool verify(const Proof& proof, std::optional<uint64_t> seed) {
    int ok = 0;
    uint64_t s = seed.value_or(0);
    check(frieda_verify(proof.handle(), seed ? &s : nullptr, &ok));
    return ok != 0;
}
// verify + where the accepted proof sampled: evaluations()[i] sits at position [i] of the bit-reversed codeword; nullopt when the proof
// is rejected (the sampling client's half of the README's flow; pooled pairs feed frieda_reconstruct_points_device)
inline std::optional<std::vector<uint32_t>> verify_samples(const Proof& proof, std::optional<uint64_t> seed) {
    int ok = 0;
    uint64_t s = seed.value_or(0);
    std::vector<uint32_t> pos(proof.evaluations().size() + 1);
    size_t n = 0;
    check(frieda_verify_samples(proof.handle(), seed ? &s : nullptr, &ok, pos.data(), pos.size(), &n));
    if (!ok) return std::nullopt;
    pos.resize(n);
    return pos;
}
// verify + every point the accepted proof authenticates (frieda_verify_pairs): the ascending positions of both members of every opened
// first-layer pair and their values; nullopt when the proof is rejected
inline std::optional<std::pair<std::vector<uint32_t>, std::vector<QM31>>> verify_pairs(const Proof& proof, std::optional<uint64_t> seed) {
    int ok = 0;
    uint64_t s = seed.value_or(0);
    const size_t cap = 2 * (size_t)frieda_proof_pcs_config(proof.handle()).n_queries + 1;
    std::vector<uint32_t> pos(cap), val(4 * cap);
    size_t n = 0;
    check(frieda_verify_pairs(proof.handle(), seed ? &s : nullptr, &ok, pos.data(), val.data(), cap, &n));
    if (!ok) return std::nullopt;
    pos.resize(n);
    std::vector<QM31> values(n);
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 4; c++) values[i].v[c] = val[4 * i + c];
    return std::make_pair(pos, values);
}
// host verifier of opened cells (frieda_verify_cells): one status byte per cell, no context
inline std::vector<uint8_t> verify_cells(const Commitment& commitment, uint32_t log_domain, uint32_t log_cell, const std::vector<uint32_t>& cell_index,
                                         const std::vector<uint32_t>& values, const std::vector<uint8_t>& paths) {
    Context::check_cell_shapes("verify_cells", log_domain, log_cell, cell_index.size(), values.size(), paths.size());
    std::vector<uint8_t> status(cell_index.size());
    check(frieda_verify_cells(commitment.data(), log_domain, log_cell, cell_index.data(), (uint32_t)cell_index.size(), values.data(), paths.data(), status.data()));
    return status;
}
// host verifier of the cells of many blobs (frieda_verify_cells_blobs): cell i is cell cell_index[i] of blob blob_index[i]
inline std::vector<uint8_t> verify_cells_blobs(const std::vector<Commitment>& commitments, uint32_t log_domain, uint32_t log_cell,
                                               const std::vector<uint32_t>& blob_index, const std::vector<uint32_t>& cell_index,
                                               const std::vector<uint32_t>& values, const std::vector<uint8_t>& paths) {
    if (blob_index.size() != cell_index.size()) throw Error(FRIEDA_ERR_ARG, "verify_cells_blobs: one blob number per cell");
    Context::check_cell_shapes("verify_cells_blobs", log_domain, log_cell, cell_index.size(), values.size(), paths.size());
    const std::vector<uint8_t> flat = Context::flat_commitments(commitments);
    std::vector<uint8_t> status(cell_index.size());
    check(frieda_verify_cells_blobs(flat.data(), (uint32_t)commitments.size(), log_domain, log_cell, blob_index.data(), cell_index.data(),
                                    (uint32_t)cell_index.size(), values.data(), paths.data(), status.data()));
    return status;
}
// host verifier of stripe bundles (frieda_verify_stripe_bundles): status[n_bundles][K]
inline std::vector<uint8_t> verify_stripe_bundles(const std::vector<Commitment>& commitments, uint32_t log_domain, uint32_t log_cell,
                                                  const std::vector<uint32_t>& stripe_index, const std::vector<uint32_t>& bundle_first,
                                                  const std::vector<uint32_t>& values, const std::vector<uint8_t>& witness,
                                                  const std::vector<uint64_t>& witness_first) {
    const size_t K = commitments.size();
    Context::check_stripe_bundle_shapes("verify_stripe_bundles", K, log_cell, stripe_index, bundle_first, values.size(), witness.size(), &witness_first);
    const std::vector<uint8_t> flat = Context::flat_commitments(commitments);
    const uint32_t nb = (uint32_t)bundle_first.size() - 1;
    std::vector<uint8_t> status((size_t)nb * K + 1);
    check(frieda_verify_stripe_bundles(flat.data(), (uint32_t)K, log_domain, log_cell, stripe_index.data(), bundle_first.data(), nb, values.data(), witness.data(),
                                       witness_first.data(), status.data()));
    status.resize((size_t)nb * K);
    return status;
}
}  // namespace api

}  // namespace frieda
