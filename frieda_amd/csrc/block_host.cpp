// block_host.cpp — block proofs: one FRI proof for all blobs of a block.  The host side of aggregate.hip and the exports
// frieda_block_challenge, frieda_aggregate_encoded, frieda_encoded_aggregate_of, frieda_test_aggregate_with_rho,
// frieda_prove_block_seeds, frieda_verify_block and the frieda_block_proof_* accessors.
//
// A provider of a block of K blobs of one shape owes every sampling client one proximity proof per commitment: K fold chains per seed.
// Batched FRI removes the factor K.  The K codewords stay committed as they are; rho is drawn from the K commitments (block_proof.h);
// ONE FRI instance runs over g = sum over k of rho^k f_k; where that proof was queried every f_k is opened against its own commitment,
// and the client checks the linear combination there.
//   aggregate_encoded   g as an ordinary handle in a slab of its own: the K evaluation pointers go to the device as a table in the
//                       arena, aggregate.hip writes the evaluation, the tree build of a lone call (tree_first_layer) the tree and the
//                       root; one synchronisation.  Every call that takes a handle takes it: they read the evaluation and the tree.
//   prove_block_seeds   frieda_prove_seeds on g (first synchronisation), the query positions of every proof by replaying its transcript
//                       (no proof is verified to learn them), then the S stripe bundles of the K blobs at log_cell 1 — bundle s is seed
//                       s — through frieda_open_stripe_bundles: one launch chain (second synchronisation).
//   verify_block        host only: frieda_verify_pairs' verifier on the FRI part, the indices, frieda_verify_stripe_bundles' verifier
//                       on the opening part, then sum rho^k value_k against the pair values the FRI verifier hashed.
// The protocol is this project's own: the reference proves one column per FriProver::commit.
#include <string.h>

#include <memory>

#include "block_proof.h"
#include "host.h"

struct frieda_block_proof {
    frieda_proof* fri = nullptr;  // owned
    uint32_t n_blobs = 0;
    uint64_t W = 0;                        // witness hashes per blob
    std::vector<uint32_t> index, values;   // [n_stripes], [n_stripes][n_blobs][4][2]
    std::vector<uint8_t> witness;          // [n_blobs][W][32]
    ~frieda_block_proof() { frieda_proof_free(fri); }
};

namespace frieda {

namespace {

// the argument rules of a block of handles (frieda_prove_seeds_blobs_begin's): one shape, on ctx's device
int block_handles(Ctx* ctx, const char* fn, const frieda_encoded* const* encs, uint32_t n_blobs, std::vector<const Encoded*>& es) {
    if (!encs) return ctx->fail(FRIEDA_ERR_ARG, std::string(fn) + "null list of encoded blobs");
    if (n_blobs == 0 || n_blobs > BLOCK_PROOF_MAX_BLOBS) return ctx->fail(FRIEDA_ERR_ARG, std::string(fn) + "n_blobs out of range");
    es.resize(n_blobs);
    for (uint32_t b = 0; b < n_blobs; b++) {
        if (!encs[b] || !encs[b]->e.d) return ctx->fail(FRIEDA_ERR_ARG, std::string(fn) + "null encoded blob");
        es[b] = &encs[b]->e;
        if (es[b]->len != es[0]->len || es[b]->log_blowup != es[0]->log_blowup)
            return ctx->fail(FRIEDA_ERR_ARG, std::string(fn) + "the encoded blobs of a block have one length and one blowup");
        if (es[b]->device != ctx->device) return ctx->fail(FRIEDA_ERR_ARG, std::string(fn) + "the encoded blob lives on another device");
    }
    return FRIEDA_OK;
}

QM31 handles_challenge(const std::vector<const Encoded*>& es) {
    std::vector<uint8_t> roots(32 * es.size());
    for (size_t b = 0; b < es.size(); b++) memcpy(&roots[32 * b], es[b]->root, 32);
    return block_challenge(roots.data(), (uint32_t)es.size());
}

int aggregate_encoded(Ctx* ctx, const std::vector<const Encoded*>& es, QM31 rho, frieda_encoded** out) {
    const uint32_t K = (uint32_t)es.size(), n = es[0]->n;
    const size_t N = (size_t)1 << n;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t tb = sizeof(uint32_t*) * (size_t)K, o_root_pin = (tb + 255) & ~(size_t)255;
    ArenaPlan plan;
    const size_t o_tab = plan.take(tb);
    int rc = ctx->ensure_arena(plan.off);
    if (rc == FRIEDA_OK) rc = ensure_pinned(ctx, o_root_pin + 4096);
    if (rc) return rc;
    // the slab of one, its tree under the threshold of a lone call (what build_tree applies to a Launch of batch 1)
    EncodedBlock one;
    rc = one.alloc(ctx, es[0]->len, es[0]->log_blowup, es[0]->L, n, 1, k::tree_skip_threshold(ctx->tuning, 1));
    if (rc) return rc;
    Encoded& g = one.e[0];
    g.aggregate_of = K;
    g.aggregate_rho = rho;
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    const uint32_t** table = reinterpret_cast<const uint32_t**>(pin);
    for (uint32_t b = 0; b < K; b++) table[b] = es[b]->eval();
    k::AggregateArgs a{};
    a.evals = reinterpret_cast<const uint32_t* const*>(ctx->arena + o_tab);
    a.n_blobs = K;
    a.log_n = n;
    a.out = reinterpret_cast<uint32_t*>(g.d);
    a.chunk = (K + k::AGG_SPLIT - 1) / k::AGG_SPLIT;
    a.rho = qm_matrix(rho);
    for (uint32_t x = 1; x < k::AGG_SPLIT; x++) a.rho_pow[x - 1] = qm_matrix(qm_pow(rho, (uint64_t)x * a.chunk));
    // few positions under many blobs: fewer waves than the chip has SIMDs and a long chain in each — split the chain
    const uint32_t mode = ctx->tuning.agg_split;
    const bool split = n >= 2 && (mode == 2 || (mode == 0 && K >= 8 && n < 18));
    hipStream_t s = ctx->stream;
    auto run = [&]() -> int {
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + o_tab, pin, tb, hipMemcpyHostToDevice, s));
        k::aggregate(ctx->launch(), a, split);
        k::tree_first_layer(ctx->launch(), g.eval(), N, n, g.d + g.o_tree, nullptr, nullptr, 0, g.d + g.o_root);
        FR_HIP(ctx, hipMemcpyAsync(pin + o_root_pin, g.d + g.o_root, 32, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        FR_HIP(ctx, hipGetLastError());
        return FRIEDA_OK;
    };
    rc = run();
    if (rc != FRIEDA_OK) {
        (void)hipStreamSynchronize(s);  // (before the slab goes)
        return rc;
    }
    rc = one.publish(pin + o_root_pin, out);
    return rc == FRIEDA_OK ? rc : ctx->fail(rc, "host allocation failed");
}

int aggregate_entry(frieda_ctx* ctx, const char* fn, const frieda_encoded* const* encs, uint32_t n_blobs, const uint32_t* rho_given, frieda_encoded** out) {
    if (!ctx || !out) return FRIEDA_ERR_ARG;
    *out = nullptr;
    FR_GUARD_BEGIN
    FR_NO_JOB(&ctx->c);
    std::vector<const Encoded*> es;
    if (const int rc = block_handles(&ctx->c, fn, encs, n_blobs, es)) return rc;
    QM31 rho;
    if (rho_given) {
        for (int i = 0; i < 4; i++)
            if (rho_given[i] >= P31) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "rho is not four canonical M31 words");
        rho = QM31{rho_given[0], rho_given[1], rho_given[2], rho_given[3]};
    } else {
        rho = handles_challenge(es);
    }
    return aggregate_encoded(&ctx->c, es, rho, out);
    FR_GUARD_END(ctx)
}

// The first-layer query positions of a proof, from its transcript alone: seed, layer roots (an alpha drawn after each), last layer,
// nonce, generate_queries — the verifier's replay (verifier.cpp) without a single hash of the openings.
void proof_queries(const ProofData& p, const uint64_t* seed, std::vector<uint32_t>& queries) {
    auto words = [](const Hash32& h, uint32_t (&w)[8]) {
        for (int i = 0; i < 8; i++) w[i] = (uint32_t)h[4 * i] | ((uint32_t)h[4 * i + 1] << 8) | ((uint32_t)h[4 * i + 2] << 16) | ((uint32_t)h[4 * i + 3] << 24);
    };
    Channel ch;
    ch.init();
    if (seed) ch.mix_u64(*seed);
    uint32_t w[8];
    words(p.first_layer.commitment, w);
    ch.mix_root(w);
    (void)ch.draw_felt();
    for (const LayerProof& lp : p.inner_layers) {
        words(lp.commitment, w);
        ch.mix_root(w);
        (void)ch.draw_felt();
    }
    channel_mix_felts(ch, p.last_layer_poly);
    ch.mix_u64(p.proof_of_work);
    queries = generate_queries(ch, p.log_size_bound + p.pcs_config.log_blowup_factor, p.pcs_config.n_queries);
}

int prove_block_seeds(frieda_ctx* ctx, const frieda_encoded* agg, const frieda_encoded* const* encs, uint32_t n_blobs, const uint64_t* seeds, uint32_t n_seeds,
                      frieda_pcs_config cfg, frieda_block_proof** out) {
    const char* const fn = "prove_block_seeds: ";
    Ctx* c = &ctx->c;
    FR_NO_JOB(c);
    if (!agg || !agg->e.d) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "null aggregate handle");
    if (!seeds) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "null seeds");
    if (n_seeds == 0 || n_seeds > 65535) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "n_seeds out of range");
    std::vector<const Encoded*> es;
    if (const int rc = block_handles(c, fn, encs, n_blobs, es)) return rc;
    if (cfg.n_queries > FRIEDA_MAX_BUNDLE_CELLS) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "n_queries above FRIEDA_MAX_BUNDLE_CELLS");
    if (agg->e.len != es[0]->len || agg->e.log_blowup != es[0]->log_blowup) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "the aggregate is of another shape");
    if (agg->e.aggregate_of != n_blobs) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "the handle is not an aggregate of n_blobs blobs");
    if (!qm_eq(agg->e.aggregate_rho, handles_challenge(es))) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "the aggregate was not made from these commitments");
    if (es[0]->n < 1) return c->fail(FRIEDA_ERR_ARG, std::string(fn) + "shape out of range");

    // the FRI part: the proofs of g, one pass (every rule of frieda_prove_seeds applies as there)
    struct Proofs {
        std::vector<frieda_proof*> p;
        ~Proofs() {
            for (frieda_proof* x : p) frieda_proof_free(x);
        }
    } fri;
    fri.p.assign(n_seeds, nullptr);
    int rc = frieda_prove_seeds(ctx, agg, seeds, n_seeds, cfg, fri.p.data());
    if (rc != FRIEDA_OK) return rc;

    // where each proof opened g, and the S bundles of the K blobs there in ONE call: bundle s is seed s
    std::vector<uint32_t> index, first(n_seeds + 1, 0), q, idx;
    for (uint32_t s = 0; s < n_seeds; s++) {
        proof_queries(fri.p[s]->p, &seeds[s], q);
        block_stripe_indices(q.data(), q.size(), idx);
        index.insert(index.end(), idx.begin(), idx.end());
        first[s + 1] = (uint32_t)index.size();
    }
    std::vector<uint64_t> wfirst(n_seeds + 1, 0);
    rc = frieda_open_stripe_bundles(ctx, encs, n_blobs, 1, index.data(), first.data(), n_seeds, nullptr, nullptr, 0, wfirst.data());
    if (rc != FRIEDA_OK) return rc;
    std::vector<uint32_t> values(8 * index.size() * n_blobs);
    std::vector<uint8_t> witness(32 * (size_t)wfirst[n_seeds] * n_blobs + 32);  // (never empty: the call wants a pointer)
    rc = frieda_open_stripe_bundles(ctx, encs, n_blobs, 1, index.data(), first.data(), n_seeds, values.data(), witness.data(), (size_t)wfirst[n_seeds] * n_blobs,
                                    wfirst.data());
    if (rc != FRIEDA_OK) return rc;

    std::vector<std::unique_ptr<frieda_block_proof>> bps(n_seeds);
    for (uint32_t s = 0; s < n_seeds; s++) {
        bps[s].reset(new frieda_block_proof());
        frieda_block_proof& bp = *bps[s];
        bp.fri = fri.p[s];
        fri.p[s] = nullptr;
        bp.n_blobs = n_blobs;
        bp.W = wfirst[s + 1] - wfirst[s];
        bp.index.assign(index.begin() + first[s], index.begin() + first[s + 1]);
        bp.values.assign(values.begin() + 8 * (size_t)first[s] * n_blobs, values.begin() + 8 * (size_t)first[s + 1] * n_blobs);
        const uint8_t* wp = witness.data() + 32 * (size_t)wfirst[s] * n_blobs;
        bp.witness.assign(wp, wp + 32 * (size_t)bp.W * n_blobs);
    }
    for (uint32_t s = 0; s < n_seeds; s++) out[s] = bps[s].release();
    return FRIEDA_OK;
}

// the client's check; *reason names the first failing step
int verify_block(const uint8_t* commitments, uint32_t n_blobs, const frieda_block_proof& bp, const uint64_t* seed, int* ok, uint32_t* reason) {
    *ok = 0;
    const ProofData& p = bp.fri->p;
    const uint64_t n64 = (uint64_t)p.log_size_bound + p.pcs_config.log_blowup_factor;
    const size_t n_stripes = bp.index.size();
    *reason = FRIEDA_BLOCK_SHAPE;
    if (n_blobs == 0 || n_blobs != bp.n_blobs || n64 < 1 || n64 > FRIEDA_MAX_LOG_DOMAIN) return FRIEDA_OK;
    if (n_stripes == 0 || n_stripes > FRIEDA_MAX_BUNDLE_CELLS || bp.values.size() != 8 * n_stripes * n_blobs || bp.witness.size() != 32 * (size_t)bp.W * n_blobs)
        return FRIEDA_OK;
    const uint32_t n = (uint32_t)n64;
    *reason = FRIEDA_BLOCK_FRI;
    std::vector<uint32_t> q, idx;
    PairPoints pp;
    int fri_ok = 0;
    const int rc = verify(p, seed, &fri_ok, &q, &pp);
    if (rc != FRIEDA_OK || !fri_ok) return rc;
    if (q.size() != p.evaluations.size()) return FRIEDA_ERR_INVARIANT;  // (the rule of frieda_verify_pairs)
    *reason = FRIEDA_BLOCK_INDICES;
    block_stripe_indices(q.data(), q.size(), idx);
    if (idx != bp.index) return FRIEDA_OK;
    *reason = FRIEDA_BLOCK_BUNDLE;
    const uint32_t first[2] = {0, (uint32_t)n_stripes};
    const uint64_t wfirst[2] = {0, bp.W};
    std::vector<uint8_t> status(n_blobs, FRIEDA_BUNDLE_REJECTED);
    if (stripe_bundles_args_error(commitments, n_blobs, BLOCK_PROOF_MAX_BLOBS, n, 1, bp.index.data(), first, 1, bp.values.data(), bp.witness.data(), wfirst, status.data()))
        return FRIEDA_OK;
    verify_stripe_bundles_host(commitments, n_blobs, n, 1, bp.index.data(), first, 1, bp.values.data(), bp.witness.data(), wfirst, status.data());
    for (uint32_t j = 0; j < n_blobs; j++)
        if (status[j] != FRIEDA_BUNDLE_ACCEPTED) return FRIEDA_OK;
    *reason = FRIEDA_BLOCK_COMBINATION;
    // the FRI verifier's pair points: both members of every opened pair, ascending — entry 2 t + e is position 2 index[t] + e
    if (pp.pos.size() != 2 * n_stripes) return FRIEDA_OK;
    const QM31 rho = block_challenge(commitments, n_blobs);
    for (size_t t = 0; t < n_stripes; t++)
        for (uint32_t e = 0; e < 2; e++) {
            if (pp.pos[2 * t + e] != 2 * bp.index[t] + e) return FRIEDA_OK;
            if (!qm_eq(block_combine(bp.values.data() + 8 * t * n_blobs + e, n_blobs, 8, rho), pp.val[2 * t + e])) return FRIEDA_OK;
        }
    *reason = FRIEDA_BLOCK_OK;
    *ok = 1;
    return FRIEDA_OK;
}

}  // namespace

}  // namespace frieda

using namespace frieda;

extern "C" {

int frieda_block_challenge(const uint8_t* commitments, uint32_t n_blobs, uint32_t out_rho[4]) {
    if (!commitments || !out_rho || n_blobs == 0 || n_blobs > BLOCK_PROOF_MAX_BLOBS) return FRIEDA_ERR_ARG;
    const QM31 rho = block_challenge(commitments, n_blobs);
    out_rho[0] = rho.a, out_rho[1] = rho.b, out_rho[2] = rho.c, out_rho[3] = rho.d;
    return FRIEDA_OK;
}

int frieda_aggregate_encoded(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, frieda_encoded** out) {
    return aggregate_entry(ctx, "aggregate_encoded: ", encs, n_blobs, nullptr, out);
}
int frieda_test_aggregate_with_rho(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, const uint32_t rho[4], frieda_encoded** out) {
    if (!rho) return FRIEDA_ERR_ARG;
    return aggregate_entry(ctx, "test_aggregate_with_rho: ", encs, n_blobs, rho, out);
}
uint32_t frieda_encoded_aggregate_of(const frieda_encoded* enc) { return enc ? enc->e.aggregate_of : 0; }

int frieda_prove_block_seeds(frieda_ctx* ctx, const frieda_encoded* agg, const frieda_encoded* const* encs, uint32_t n_blobs, const uint64_t* seeds,
                             uint32_t n_seeds, frieda_pcs_config cfg, frieda_block_proof** out) {
    if (!ctx || !out) return FRIEDA_ERR_ARG;
    if (n_seeds >= 1 && n_seeds <= 65535) memset(out, 0, sizeof(frieda_block_proof*) * n_seeds);
    FR_GUARD_BEGIN
    return prove_block_seeds(ctx, agg, encs, n_blobs, seeds, n_seeds, cfg, out);
    FR_GUARD_END(ctx)
}

int frieda_verify_block(const uint8_t* commitments, uint32_t n_blobs, const frieda_block_proof* bp, const uint64_t* seed, int* ok, uint32_t* out_reason) {
    if (!commitments || !bp || !bp->fri || !ok) return FRIEDA_ERR_ARG;
    frieda_ctx* none = nullptr;
    uint32_t reason = FRIEDA_BLOCK_SHAPE;
    *ok = 0;
    FR_GUARD_BEGIN
    const int rc = verify_block(commitments, n_blobs, *bp, seed, ok, &reason);
    if (out_reason) *out_reason = reason;
    return rc;
    FR_GUARD_END(none)
}

void frieda_block_proof_free(frieda_block_proof* bp) { delete bp; }
const frieda_proof* frieda_block_proof_fri(const frieda_block_proof* bp) { return bp ? bp->fri : nullptr; }
uint32_t frieda_block_proof_n_blobs(const frieda_block_proof* bp) { return bp ? bp->n_blobs : 0; }
uint32_t frieda_block_proof_n_stripes(const frieda_block_proof* bp) { return bp ? (uint32_t)bp->index.size() : 0; }
const uint32_t* frieda_block_proof_stripe_index(const frieda_block_proof* bp) { return bp ? bp->index.data() : nullptr; }
const uint32_t* frieda_block_proof_values(const frieda_block_proof* bp) { return bp ? bp->values.data() : nullptr; }
const uint8_t* frieda_block_proof_witness(const frieda_block_proof* bp) { return bp ? bp->witness.data() : nullptr; }
uint64_t frieda_block_proof_witness_hashes(const frieda_block_proof* bp) { return bp ? bp->W : 0; }

size_t frieda_block_proof_serialize(const frieda_block_proof* bp, uint8_t* buf, size_t cap) {
    if (!bp || !bp->fri) return 0;
    try {
        const std::vector<uint8_t> img = serialize_proof(bp->fri->p);
        BlockWire w;
        if (!block_wire_layout(bp->n_blobs, (uint32_t)bp->index.size(), bp->W, img.size(), w)) return 0;
        if (buf && cap >= w.total) {
            block_wire_write_header(buf, w);
            memcpy(buf + w.off_proof, img.data(), img.size());
            memcpy(buf + w.off_index, bp->index.data(), 4 * bp->index.size());
            memcpy(buf + w.off_values, bp->values.data(), 4 * bp->values.size());
            if (!bp->witness.empty()) memcpy(buf + w.off_witness, bp->witness.data(), bp->witness.size());
        }
        return w.total;
    } catch (...) {
        return 0;
    }
}

int frieda_block_proof_deserialize(const uint8_t* buf, size_t len, frieda_block_proof** out) {
    if (!buf || !out) return FRIEDA_ERR_ARG;
    *out = nullptr;
    frieda_ctx* none = nullptr;
    FR_GUARD_BEGIN
    BlockWire w;
    if (!block_wire_read(buf, len, w)) return FRIEDA_ERR_ARG;
    std::unique_ptr<frieda_block_proof> bp(new frieda_block_proof());
    if (frieda_proof_deserialize(buf + w.off_proof, (size_t)w.proof_bytes, &bp->fri) != FRIEDA_OK) return FRIEDA_ERR_ARG;
    const ProofData& p = bp->fri->p;
    const uint64_t n = (uint64_t)p.log_size_bound + p.pcs_config.log_blowup_factor;
    if (n < 1 || n > FRIEDA_MAX_LOG_DOMAIN) return FRIEDA_ERR_ARG;
    bp->n_blobs = w.n_blobs;
    bp->W = w.W;
    bp->index.resize(w.n_stripes);
    memcpy(bp->index.data(), buf + w.off_index, 4 * (size_t)w.n_stripes);
    if (!block_wire_indices_ok((uint32_t)n, bp->index.data(), w.n_stripes, w.W)) return FRIEDA_ERR_ARG;
    bp->values.resize(8 * (size_t)w.n_stripes * w.n_blobs);
    memcpy(bp->values.data(), buf + w.off_values, 4 * bp->values.size());
    bp->witness.assign(buf + w.off_witness, buf + w.total);
    *out = bp.release();
    return FRIEDA_OK;
    FR_GUARD_END(none)
}

}  // extern "C"
