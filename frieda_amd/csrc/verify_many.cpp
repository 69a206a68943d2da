// verify_many.cpp — frieda_verify_many / frieda_verify_samples_many / frieda_reconstruct_from_proofs and their pair forms
// (frieda_verify_pairs_many / frieda_reconstruct_from_proof_pairs): the host side of verify.hip.
//
// Per proof the result is that of verifier.cpp::verify, whatever the route.  The checks that hash nothing and that the reference makes
// before anything else run here (the L, L + B range, InvalidNumFriLayers, LastLayerDegreeInvalid): such a proof has its status without
// being sent.  (The power-of-two rule of the last layer and the empty inner_layers assertion come AFTER the first layer's checks in the
// reference — a proof that is also short of evaluations panics first — so the kernel applies them, in the reference's order.)  Proofs of
// a shape the kernel does not take (more than VERIFY_MAX_QUERIES queries, a last layer above DT_MAX_LAST_POLY, more than DT_MAX_LAYERS
// layers, no queries at all) go through verify() inside the same call.  The rest is flattened into the context's pinned staging block
// in passes bounded by VERIFY_PASS_BYTES — header, layer table, words — uploaded, verified by one launch per pass (or, for a pass of at
// most FRIEDA_VERIFY_SPLIT_MAX proofs, by the two launches of verify_split.hip: verify_pass.h has the cut and the status rule), and one
// status word and the sampled positions per proof come back.  In pairs mode the kernel also leaves both members of every opened first-layer pair in a
// per-pass buffer; once the statuses are known, a gather launch copies the rows of the accepted proofs into the call's PairPool.
#include <string.h>

#include <algorithm>
#include <unordered_map>

#include "dev_transcript.h"
#include "host.h"
#include "verify_pass.h"

namespace frieda {

namespace {

size_t image_words(const ProofData& p) {
    size_t w = 4 * (p.inner_layers.size() + 1);
    auto layer = [](const LayerProof& l) { return 8 + 4 * l.fri_witness.size() + 8 * l.hash_witness.size(); };
    w += layer(p.first_layer);
    for (const LayerProof& l : p.inner_layers) w += layer(l);
    return w + 4 * p.last_layer_poly.size() + 4 * p.evaluations.size();
}

void pack_layer(const LayerProof& l, uint32_t* base, uint32_t* tab, size_t& off) {
    tab[0] = (uint32_t)l.fri_witness.size();
    tab[1] = (uint32_t)l.hash_witness.size();
    tab[2] = (uint32_t)l.column_witness.size();
    tab[3] = (uint32_t)off;
    memcpy(base + off, l.commitment.data(), 32);
    off += 8;
    if (!l.fri_witness.empty()) memcpy(base + off, l.fri_witness.data(), 16 * l.fri_witness.size());
    off += 4 * l.fri_witness.size();
    if (!l.hash_witness.empty()) memcpy(base + off, l.hash_witness.data(), 32 * l.hash_witness.size());
    off += 8 * l.hash_witness.size();
}

void pack_proof(const ProofData& p, const uint64_t* seed, uint32_t* base, k::VerifyHeader& h, size_t off_words) {
    memset(&h, 0, sizeof h);
    h.off_words = (uint32_t)off_words;
    h.n = p.log_size_bound + p.pcs_config.log_blowup_factor;
    h.n_inner = (uint32_t)p.inner_layers.size();
    h.n_queries = p.pcs_config.n_queries;
    h.pow_bits = p.pcs_config.pow_bits;
    h.has_seed = seed ? 1u : 0u;
    h.seed_lo = seed ? (uint32_t)*seed : 0u;
    h.seed_hi = seed ? (uint32_t)(*seed >> 32) : 0u;
    h.nonce_lo = (uint32_t)p.proof_of_work;
    h.nonce_hi = (uint32_t)(p.proof_of_work >> 32);
    h.n_last = (uint32_t)p.last_layer_poly.size();
    h.n_evals = (uint32_t)p.evaluations.size();
    size_t off = 4 * (p.inner_layers.size() + 1);
    pack_layer(p.first_layer, base, base, off);
    for (size_t i = 0; i < p.inner_layers.size(); i++) pack_layer(p.inner_layers[i], base, base + 4 * (i + 1), off);
    h.off_last = (uint32_t)off;
    if (h.n_last) memcpy(base + off, p.last_layer_poly.data(), 16 * (size_t)h.n_last);
    off += 4 * (size_t)h.n_last;
    h.off_evals = (uint32_t)off;
    if (h.n_evals) memcpy(base + off, p.evaluations.data(), 16 * (size_t)h.n_evals);
}

// the checks of verify() that precede every hash; true: `status` is final
bool structural_status(const ProofData& p, uint8_t& status) {
    const uint32_t B = p.pcs_config.log_blowup_factor, last = p.pcs_config.log_last_layer_degree_bound, L = p.log_size_bound;
    if (L < 1 || (uint64_t)L + B < 2 || (uint64_t)L + B > 30) {
        status = k::VERIFY_INVARIANT;
        return true;
    }
    status = k::VERIFY_REJECTED;
    uint32_t bound = L - 1;
    for (size_t i = 0; i < p.inner_layers.size(); i++) {
        if (bound < 1) return true;  // InvalidNumFriLayers
        bound -= 1;
    }
    if (bound != last) return true;
    if (p.last_layer_poly.size() > ((size_t)1 << last)) return true;  // LastLayerDegreeInvalid
    return false;
}

bool device_shape(const ProofData& p) {
    const uint32_t nq = p.pcs_config.n_queries;
    return nq >= 1 && nq <= k::VERIFY_MAX_QUERIES && p.last_layer_poly.size() <= DT_MAX_LAST_POLY && p.inner_layers.size() + 1 <= DT_MAX_LAYERS &&
           image_words(p) < ((size_t)1 << 30);
}

void host_route(const ProofData& p, const uint64_t* seed, bool samples, uint8_t& status, std::vector<uint32_t>* pos, PairPoints* pairs) {
    int ok = 0;
    std::vector<uint32_t> q;
    const int rc = verify(p, seed, &ok, &q, pairs);
    if (rc != FRIEDA_OK)
        status = k::VERIFY_INVARIANT;
    else if (!ok)
        status = k::VERIFY_REJECTED;
    else if (samples && q.size() != p.evaluations.size())
        status = k::VERIFY_INVARIANT;  // frieda_verify_samples: an accepted proof has one evaluation per distinct query
    else
        status = k::VERIFY_ACCEPTED;
    if (pos && status == k::VERIFY_ACCEPTED) *pos = std::move(q);
    if (pairs && status != k::VERIFY_ACCEPTED) pairs->pos.clear(), pairs->val.clear();
}

int init_device_tables(Ctx* ctx) {
    static std::mutex mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> g(mu);
    if (std::find(done.begin(), done.end(), ctx->device) != done.end()) return FRIEDA_OK;
    CPoint t[31];
    for (uint32_t b = 0; b < 31; b++) t[b] = point_from_index(1u << b);
    FR_HIP(ctx, k::verify_many_init(t));
    FR_HIP(ctx, k::verify_split_init(t));
    done.push_back(ctx->device);
    return FRIEDA_OK;
}

int pool_alloc(Ctx* ctx, PairPool& pool) {
    if (pool.buf.p || !pool.cap) return FRIEDA_OK;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    return pool.alloc(ctx, pool.cap, 16, "poison(pair pool)");
}

}  // namespace

int PairPool::upload_host_rows(Ctx* ctx) {
    bool any = false;
    for (size_t i = 0; i < host.size(); i++) {
        if (host[i].pos.empty()) continue;
        if (!any) {
            const int rc = pool_alloc(ctx, *this);
            if (rc) return rc;
            any = true;
        }
        FR_HIP(ctx, hipMemcpyAsync(d_pos() + off[i], host[i].pos.data(), 4 * host[i].pos.size(), hipMemcpyHostToDevice, ctx->stream));
        FR_HIP(ctx, hipMemcpyAsync(d_val() + 4 * off[i], host[i].val.data(), 16 * host[i].val.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    if (any) FR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return FRIEDA_OK;
}

int verify_many(Ctx* ctx, const ProofData* const* proofs, const uint64_t* seeds, uint32_t count, const uint8_t* const* expected_commitments, bool samples,
                uint8_t* out_status, std::vector<std::vector<uint32_t>>* positions, PairPool* pairs) {
    if (positions) positions->assign(count, {});
    if (pairs) {
        pairs->off.assign(count, 0);
        pairs->cnt.assign(count, 0);
        pairs->host.clear();
        pairs->host.resize(count);
        pairs->n = pairs->cap = 0;
    }
    // the pool is filled in the caller's order: a proof's offset is fixed once every accepted proof before it has its count (the host
    // route runs first, the kernel's proofs come in ascending order pass by pass)
    uint32_t cursor = 0;
    auto place_up_to = [&](uint32_t end) {
        for (; cursor < end; cursor++) {
            pairs->off[cursor] = pairs->n;
            pairs->n += pairs->cnt[cursor];
        }
    };
    std::vector<uint32_t> dev;  // indices of the proofs the kernel takes
    std::vector<uint32_t> host;
    for (uint32_t i = 0; i < count; i++) {
        const ProofData& p = *proofs[i];
        if (expected_commitments && expected_commitments[i] && memcmp(p.first_layer.commitment.data(), expected_commitments[i], 32) != 0) {
            out_status[i] = k::VERIFY_WRONG_COMMITMENT;
            continue;
        }
        if (structural_status(p, out_status[i])) continue;
        (device_shape(p) ? dev : host).push_back(i);
    }
    if (dev.size() < ctx->tuning.verify_device_min || dev.empty()) {
        host.insert(host.end(), dev.begin(), dev.end());
        dev.clear();
    }
    for (uint32_t i : host) {
        host_route(*proofs[i], seeds ? seeds + i : nullptr, samples, out_status[i], positions ? &(*positions)[i] : nullptr, pairs ? &pairs->host[i] : nullptr);
        if (pairs) pairs->cnt[i] = (uint32_t)pairs->host[i].pos.size();
    }
    if (pairs) {
        for (uint32_t i : host) pairs->cap += 2 * (size_t)proofs[i]->pcs_config.n_queries;
        for (uint32_t i : dev) pairs->cap += 2 * (size_t)proofs[i]->pcs_config.n_queries;
    }
    if (dev.empty()) {
        if (pairs) place_up_to(count);
        return FRIEDA_OK;
    }

    FR_HIP(ctx, hipSetDevice(ctx->device));
    int rc = init_device_tables(ctx);
    if (rc) return rc;
    if (pairs) {
        rc = pool_alloc(ctx, *pairs);
        if (rc) return rc;
    }
    hipStream_t s = ctx->stream;
    const size_t hdr_words = sizeof(k::VerifyHeader) / 4, head = pairs ? 3 : 2;  // (head: words of an output row before the queries)
    // (the staging budget of one upload; a lone larger proof is a pass of its own; test hook: Tuning::test_verify_pass_bytes)
    const size_t pass_bytes = ctx->tuning.test_verify_pass_bytes ? (size_t)ctx->tuning.test_verify_pass_bytes : VERIFY_PASS_BYTES;
    const size_t scratch_cap = ctx->tuning.test_verify_scratch_bytes ? (size_t)ctx->tuning.test_verify_scratch_bytes : VERIFY_SPLIT_SCRATCH_CAP;
    auto item = [&](size_t e) {
        const ProofData& p = *proofs[dev[e]];
        return VerifyPassItem{hdr_words + image_words(p), p.pcs_config.n_queries, (uint32_t)p.inner_layers.size() + 1};
    };
    for (size_t first = 0; first < dev.size();) {
        // the proofs of this pass and its launch shape (verify_pass.h)
        const VerifyPassCut cut = verify_pass_cut(item, first, dev.size(), pass_bytes, ctx->tuning.verify_split_max, scratch_cap);
        const size_t end = cut.end, words = cut.words;
        const uint32_t q_cap = cut.q_cap;
        const size_t np = end - first, in_bytes = (4 * words + 255) & ~(size_t)255, out_bytes = 4 * np * (head + (size_t)q_cap);
        const size_t tab_bytes = pairs ? 12 * np : 0, row = 2 * (size_t)q_cap;  // (row: entries of a proof in the pass's pair buffer)
        if (words >= ((size_t)1 << 32)) return ctx->fail(FRIEDA_ERR_ARG, "verify_many: one proof beyond 2^32 words");
        ArenaPlan ap;
        const size_t a_in = ap.take(in_bytes), a_out = ap.take(out_bytes);
        const size_t a_pp = ap.take(pairs ? 4 * np * row : 0), a_pv = ap.take(pairs ? 16 * np * row : 0), a_tab = ap.take(tab_bytes);
        const size_t a_cnt = ap.take(cut.split ? 4 * np * cut.max_layers : 0), a_sp = ap.take(cut.scratch_bytes);
        rc = ctx->ensure_arena(ap.off);
        if (rc) return rc;
        rc = ensure_pinned(ctx, in_bytes + out_bytes + tab_bytes);
        if (rc) return rc;
        uint32_t* pin = static_cast<uint32_t*>(ctx->pinned);
        k::VerifyHeader* hdr = reinterpret_cast<k::VerifyHeader*>(pin);
        size_t off = hdr_words * np;
        for (size_t j = 0; j < np; j++) {
            const uint32_t i = dev[first + j];
            pack_proof(*proofs[i], seeds ? seeds + i : nullptr, pin + off, hdr[j], off);
            off += image_words(*proofs[i]);
        }
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, 4 * words, hipMemcpyHostToDevice, s));
        k::VerifyArgs va;
        va.img = reinterpret_cast<const uint32_t*>(ctx->arena + a_in);
        va.out = reinterpret_cast<uint32_t*>(ctx->arena + a_out);
        va.q_cap = q_cap;
        if (pairs) {
            va.pair_pos = reinterpret_cast<uint32_t*>(ctx->arena + a_pp);
            va.pair_val = reinterpret_cast<uint32_t*>(ctx->arena + a_pv);
        }
        if (cut.split) {
            k::VerifySplitArgs sa;
            sa.v = va;
            sa.max_layers = cut.max_layers;
            sa.cnt = reinterpret_cast<uint32_t*>(ctx->arena + a_cnt);
            sa.pairs = reinterpret_cast<uint32_t*>(ctx->arena + a_sp);
            k::verify_split(ctx->launch(), sa, (uint32_t)np);
        } else {
            k::verify_many(ctx->launch(), va, (uint32_t)np);
        }
        FR_HIP(ctx, hipGetLastError());
        uint32_t* res = pin + in_bytes / 4;
        FR_HIP(ctx, hipMemcpyAsync(res, ctx->arena + a_out, out_bytes, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        uint32_t* tab = res + out_bytes / 4;
        uint32_t n_rows = 0;
        for (size_t j = 0; j < np; j++) {
            const uint32_t i = dev[first + j];
            const uint32_t* r = res + j * (head + (size_t)q_cap);
            // (split: the key of the first event; a word that is no key of this proof decodes to "no status")
            const uint32_t word = !cut.split ? r[0] : verify_key_valid(r[0], (uint32_t)proofs[i]->inner_layers.size()) ? verify_key_status(r[0], k::VERIFY_ACCEPTED) : 0xFFFFFFFFu;
            uint8_t st = (uint8_t)word;
            if (word > k::VERIFY_INVARIANT) return ctx->fail(FRIEDA_ERR_INVARIANT, "verify_many: the kernel left no status");
            if (st == k::VERIFY_ACCEPTED && samples && r[1] != proofs[i]->evaluations.size()) st = k::VERIFY_INVARIANT;
            out_status[i] = st;
            if (positions && st == k::VERIFY_ACCEPTED) (*positions)[i].assign(r + head, r + head + r[1]);
            if (pairs && st == k::VERIFY_ACCEPTED) {
                if (r[2] == 0 || r[2] > r[1] || r[1] > proofs[i]->pcs_config.n_queries) return ctx->fail(FRIEDA_ERR_INVARIANT, "verify_many: the kernel left no pair count");
                pairs->cnt[i] = 2 * r[2];
                place_up_to(i + 1);
                if (pairs->off[i] + pairs->cnt[i] > pairs->cap || pairs->cap > 0xFFFFFFFFull) return ctx->fail(FRIEDA_ERR_INVARIANT, "verify_many: pair pool overrun");
                tab[3 * n_rows] = (uint32_t)j, tab[3 * n_rows + 1] = pairs->cnt[i], tab[3 * n_rows + 2] = (uint32_t)pairs->off[i];
                n_rows++;
            }
        }
        if (n_rows) {
            // (the table sits in the pinned block the next pass overwrites: wait for the copy)
            FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_tab, tab, 12 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            k::verify_pairs_gather(ctx->launch(), reinterpret_cast<const uint32_t*>(ctx->arena + a_tab), n_rows, va.pair_pos, va.pair_val, q_cap,
                                   pairs->d_pos(), pairs->d_val());
            FR_HIP(ctx, hipGetLastError());
            FR_HIP(ctx, hipStreamSynchronize(s));
        }
        first = end;
    }
    if (pairs) place_up_to(count);
    return FRIEDA_OK;
}

}  // namespace frieda

using namespace frieda;

extern "C" {

// the commitment pointer per proof of the one-commitment entry points: the same for all, or none
struct SameCommitment {
    std::vector<const uint8_t*> v;
    SameCommitment(const uint8_t* c, uint32_t count) : v(c ? count : 0, c) {}
    const uint8_t* const* get() const { return v.empty() ? nullptr : v.data(); }
};

// commitments: NULL (nothing is compared) or per proof the 32 bytes its first-layer commitment must equal
static int verify_many_common(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                              const uint8_t* const* commitments, bool samples, uint8_t* out_status, std::vector<std::vector<uint32_t>>* positions,
                              PairPool* pairs = nullptr) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (count == 0) return FRIEDA_OK;
    if (!proofs || !out_status) return FRIEDA_ERR_ARG;
    for (uint32_t i = 0; i < count; i++)
        if (!proofs[i]) return ctx->c.fail(FRIEDA_ERR_ARG, "null proof " + std::to_string(i));
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    std::vector<const ProofData*> ps(count);
    for (uint32_t i = 0; i < count; i++) ps[i] = &proofs[i]->p;
    return verify_many(&ctx->c, ps.data(), seeds, count, commitments, samples, out_status, positions, pairs);
    FR_GUARD_END(ctx)
}

int frieda_verify_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                       const uint8_t* expected_commitment, uint8_t* out_status) {
    return verify_many_common(ctx, proofs, seeds, count, SameCommitment(expected_commitment, count).get(), false, out_status, nullptr);
}

int frieda_verify_blobs_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count, const uint8_t* commitments,
                             uint32_t n_blobs, const uint32_t* blob_index, uint8_t* out_status, uint32_t* out_accepted_per_blob) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (!commitments) return ctx->c.fail(FRIEDA_ERR_ARG, "verify_blobs_many: no commitments");
    if (count > 0 && n_blobs == 0) return ctx->c.fail(FRIEDA_ERR_ARG, "verify_blobs_many: proofs but no blobs");
    if (!blob_index && count != n_blobs) return ctx->c.fail(FRIEDA_ERR_ARG, "verify_blobs_many: without blob_index proof i belongs to commitment i: count must be n_blobs");
    if (count > 0 && !out_status) return FRIEDA_ERR_ARG;
    for (uint32_t i = 0; blob_index && i < count; i++)
        if (blob_index[i] >= n_blobs) return ctx->c.fail(FRIEDA_ERR_ARG, "blob_index " + std::to_string(i) + " beyond n_blobs");
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    std::vector<const uint8_t*> coms(count);
    for (uint32_t i = 0; i < count; i++) coms[i] = commitments + 32 * (size_t)(blob_index ? blob_index[i] : i);
    const int rc = verify_many_common(ctx, proofs, seeds, count, coms.data(), false, out_status, nullptr);
    if (rc != FRIEDA_OK) return rc;
    if (out_accepted_per_blob) {
        std::fill(out_accepted_per_blob, out_accepted_per_blob + n_blobs, 0u);
        for (uint32_t i = 0; i < count; i++)
            if (out_status[i] == k::VERIFY_ACCEPTED) out_accepted_per_blob[blob_index ? blob_index[i] : i]++;
    }
    return FRIEDA_OK;
    FR_GUARD_END(ctx)
}

int frieda_verify_samples_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                               const uint8_t* expected_commitment, uint8_t* out_status, uint32_t* out_positions, size_t pitch,
                               uint32_t* out_n_positions) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (count == 0) return FRIEDA_OK;
    if (!proofs || !out_status || !out_positions || !out_n_positions) return FRIEDA_ERR_ARG;
    for (uint32_t i = 0; i < count; i++) {
        if (!proofs[i]) return ctx->c.fail(FRIEDA_ERR_ARG, "null proof " + std::to_string(i));
        if (pitch < proofs[i]->p.pcs_config.n_queries) return ctx->c.fail(FRIEDA_ERR_ARG, "pitch smaller than n_queries of proof " + std::to_string(i));
    }
    FR_GUARD_BEGIN
    std::vector<std::vector<uint32_t>> pos;
    const int rc = verify_many_common(ctx, proofs, seeds, count, SameCommitment(expected_commitment, count).get(), true, out_status, &pos);
    if (rc != FRIEDA_OK) return rc;
    for (uint32_t i = 0; i < count; i++) {
        out_n_positions[i] = (uint32_t)pos[i].size();
        if (!pos[i].empty()) memcpy(out_positions + (size_t)i * pitch, pos[i].data(), 4 * pos[i].size());
    }
    return FRIEDA_OK;
    FR_GUARD_END(ctx)
}

int frieda_reconstruct_from_proofs(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                                   const uint8_t expected_commitment[32], size_t len, uint8_t* out_bytes, uint8_t* out_status, size_t* n_points) {
    if (!ctx || !proofs || !expected_commitment || !out_status || !n_points || count == 0 || (len && !out_bytes)) return FRIEDA_ERR_ARG;
    *n_points = 0;
    FR_GUARD_BEGIN
    std::vector<std::vector<uint32_t>> pos;
    int rc = verify_many_common(ctx, proofs, seeds, count, SameCommitment(expected_commitment, count).get(), true, out_status, &pos);
    if (rc != FRIEDA_OK) return rc;
    // pool the verified (position, evaluation) pairs: first occurrence of a position kept
    bool have_shape = false;
    uint32_t L = 0, B = 0;
    std::vector<uint32_t> index, cells;
    std::unordered_map<uint32_t, uint32_t> seen;
    for (uint32_t i = 0; i < count; i++) {
        if (out_status[i] != k::VERIFY_ACCEPTED) continue;
        const ProofData& p = proofs[i]->p;
        if (!have_shape) {
            L = p.log_size_bound, B = p.pcs_config.log_blowup_factor;
            have_shape = true;
        } else if (p.log_size_bound != L || p.pcs_config.log_blowup_factor != B) {
            *n_points = index.size();  // the points pooled before the proof that disagrees
            return ctx->c.fail(FRIEDA_ERR_ARG, "accepted proofs disagree on the shape of the codeword");
        }
        for (size_t j = 0; j < pos[i].size(); j++) {
            if (!seen.emplace(pos[i][j], (uint32_t)index.size()).second) continue;
            index.push_back(pos[i][j]);
            const QM31& e = p.evaluations[j];
            cells.insert(cells.end(), {e.a, e.b, e.c, e.d});
        }
    }
    *n_points = index.size();
    if (!have_shape) return ctx->c.fail(FRIEDA_ERR_ARG, "no proof was accepted");
    if (index.size() < ((size_t)1 << L) + 2)
        return ctx->c.fail(FRIEDA_ERR_ARG, std::to_string(index.size()) + " distinct verified points, " + std::to_string(((size_t)1 << L) + 2) + " needed");
    if ((8 * len + 29) / 30 > ((size_t)4 << L)) return ctx->c.fail(FRIEDA_ERR_ARG, "len does not fit the polynomial");
    FR_HIP(&ctx->c, hipSetDevice(ctx->c.device));
    DevBuf d_cells;
    rc = d_cells.alloc(&ctx->c, 4 * cells.size(), "poison(rebuilt bytes)");
    if (rc != FRIEDA_OK) return rc;
    return rebuild_blob(ctx, len, B, expected_commitment, "the rebuilt blob does not commit to expected_commitment (wrong len?)", out_bytes, [&](uint8_t* d_out) {
        const int up = frieda_dev_upload(ctx, d_cells.p, cells.data(), 4 * cells.size());
        if (up != FRIEDA_OK) return up;
        return frieda_reconstruct_points_device(ctx, static_cast<const uint32_t*>(d_cells.p), index.data(), (uint32_t)index.size(), 0, L, L + B, len, d_out);
    });
    FR_GUARD_END(ctx)
}

int frieda_verify_pairs_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                             const uint8_t* expected_commitment, uint8_t* out_status, uint32_t* out_positions, uint32_t* out_values, size_t pitch,
                             uint32_t* out_n_points) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (count == 0) return FRIEDA_OK;
    if (!proofs || !out_status || !out_positions || !out_values || !out_n_points) return FRIEDA_ERR_ARG;
    for (uint32_t i = 0; i < count; i++) {
        if (!proofs[i]) return ctx->c.fail(FRIEDA_ERR_ARG, "null proof " + std::to_string(i));
        if (pitch < 2 * (size_t)proofs[i]->p.pcs_config.n_queries)
            return ctx->c.fail(FRIEDA_ERR_ARG, "pitch smaller than 2 * n_queries of proof " + std::to_string(i));
    }
    FR_GUARD_BEGIN
    PairPool pool;
    const int rc = verify_many_common(ctx, proofs, seeds, count, SameCommitment(expected_commitment, count).get(), true, out_status, nullptr, &pool);
    if (rc != FRIEDA_OK) return rc;
    // the gathered rows of the kernel's proofs come back in one copy each (the entries between them, kept for host-route proofs, are not read)
    std::vector<uint32_t> pos, val;
    if (pool.buf.p && pool.n) {
        pos.resize(pool.n);
        val.resize(4 * pool.n);
        FR_HIP(&ctx->c, hipMemcpyAsync(pos.data(), pool.d_pos(), 4 * pool.n, hipMemcpyDeviceToHost, ctx->c.stream));
        FR_HIP(&ctx->c, hipMemcpyAsync(val.data(), pool.d_val(), 16 * pool.n, hipMemcpyDeviceToHost, ctx->c.stream));
        FR_HIP(&ctx->c, hipStreamSynchronize(ctx->c.stream));
    }
    for (uint32_t i = 0; i < count; i++) {
        const size_t n = pool.cnt[i];
        out_n_points[i] = (uint32_t)n;
        if (!n) continue;
        const PairPoints& h = pool.host[i];
        memcpy(out_positions + (size_t)i * pitch, h.pos.empty() ? pos.data() + pool.off[i] : h.pos.data(), 4 * n);
        memcpy(out_values + 4 * (size_t)i * pitch, h.pos.empty() ? val.data() + 4 * pool.off[i] : reinterpret_cast<const uint32_t*>(h.val.data()), 16 * n);
    }
    return FRIEDA_OK;
    FR_GUARD_END(ctx)
}

int frieda_reconstruct_from_proof_pairs(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                                        const uint8_t expected_commitment[32], size_t len, uint8_t* out_bytes, uint8_t* out_status, size_t* n_points) {
    if (!ctx || !proofs || !expected_commitment || !out_status || !n_points || count == 0 || (len && !out_bytes)) return FRIEDA_ERR_ARG;
    *n_points = 0;
    FR_GUARD_BEGIN
    PairPool pool;
    int rc = verify_many_common(ctx, proofs, seeds, count, SameCommitment(expected_commitment, count).get(), true, out_status, nullptr, &pool);
    if (rc != FRIEDA_OK) return rc;
    rc = pool.upload_host_rows(&ctx->c);
    if (rc != FRIEDA_OK) return rc;
    bool have_shape = false;
    uint32_t L = 0, B = 0, nd = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (out_status[i] != k::VERIFY_ACCEPTED) continue;
        const ProofData& p = proofs[i]->p;
        if (!have_shape) {
            L = p.log_size_bound, B = p.pcs_config.log_blowup_factor;
            have_shape = true;
        } else if (p.log_size_bound != L || p.pcs_config.log_blowup_factor != B) {
            // the points pooled before the proof that disagrees: a prefix of the pool, which is in the caller's order
            rc = count_distinct_points(ctx, pool.d_pos(), (uint32_t)pool.off[i], L + B, &nd);
            if (rc != FRIEDA_OK) return rc;
            *n_points = nd;
            return ctx->c.fail(FRIEDA_ERR_ARG, "accepted proofs disagree on the shape of the codeword");
        }
    }
    if (!have_shape) return ctx->c.fail(FRIEDA_ERR_ARG, "no proof was accepted");
    const size_t need = ((size_t)1 << L) + 2;
    auto too_few = [&]() { return ctx->c.fail(FRIEDA_ERR_ARG, std::to_string(nd) + " distinct verified points, " + std::to_string(need) + " needed"); };
    if ((8 * len + 29) / 30 > ((size_t)4 << L) || pool.n == 0) {
        rc = count_distinct_points(ctx, pool.d_pos(), (uint32_t)pool.n, L + B, &nd);
        if (rc != FRIEDA_OK) return rc;
        *n_points = nd;
        return nd < need ? too_few() : ctx->c.fail(FRIEDA_ERR_ARG, "len does not fit the polynomial");
    }
    return rebuild_blob(ctx, len, B, expected_commitment, "the rebuilt blob does not commit to expected_commitment (wrong len?)", out_bytes, [&](uint8_t* d_out) {
        rc = reconstruct_pooled(ctx, pool.d_val(), pool.d_pos(), (uint32_t)pool.n, 1, 0, L, L + B, len, d_out, 0, &nd);
        *n_points = nd;
        return rc == FRIEDA_ERR_ARG && nd < need ? too_few() : rc;
    });
    FR_GUARD_END(ctx)
}

}  // extern "C"
