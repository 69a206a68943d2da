// bundles_host.cpp — cell bundles: the host side of bundles.hip and its exports (frieda_cell_bundle_witness_count, frieda_open_cell_bundles,
// frieda_verify_cell_bundles, frieda_verify_cell_bundles_many, frieda_reconstruct_from_cell_bundles).
//
// A bundle is the answer to one request: k cells of one blob under one shared hash witness (bundles_host.h), accepted or not as a whole.
// A call carries n_bundles of them back to back: cell i belongs to bundle b when bundle_first[b] <= i < bundle_first[b + 1], and
// witness_first counts the same way in hashes.  The per-cell calls (cells_host.cpp) stay for callers who want independent cells.
//
// The provider's call computes every count and offset on the host — the witness length depends on the indices alone — and the kernels
// fill in hashes.  The verifier decides MALFORMED on the host before anything is hashed or staged (bundles_host.h: the one function the
// host verifier calls too), stages the well-formed bundles in passes cut by bundles_pass.h, and runs cells_roots + a walk per pass;
// with a pool, the cells of a pass's accepted bundles are gathered into it before the next pass overwrites the values.
//
// What this form shares with stripe bundles (stripe_bundles_host.cpp) lives here and is declared in host.h: the pass driver
// verify_bundles_passes (n_blobs 0: this form, bundle_walk + cells_gather; n_blobs >= 1: stripe_bundle_walk + cells_stripe_gather) and the
// openers' front, table fill and end (open_bundles_front / _fill / _finish).  The rebuilds end in rebuild_from_pool (cells_host.cpp).
#include <string.h>

#include <algorithm>

#include "bundles_host.h"
#include "bundles_pass.h"
#include "cells_pass.h"
#include "host.h"

namespace frieda {

static_assert(sizeof(k::BundleRow) == 12, "the bundle table is three words a row (bundles_pass.h)");
static_assert(k::BUNDLE_MAX_CELLS == FRIEDA_MAX_BUNDLE_CELLS, "one cap");

// ---- the openers' shared pieces ----
int open_bundles_front(frieda_ctx* ctx, const char* fn, uint32_t log_domain, uint32_t n_blobs, uint32_t log_cell, const uint32_t* index,
                       const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* out_values, const uint8_t* out_witness, size_t cap_hashes,
                       uint64_t* out_witness_first, std::vector<uint64_t>& wfirst, bool* go) {
    *go = false;
    if (!bundle_first || !out_witness_first || (out_witness && !out_values)) return FRIEDA_ERR_ARG;
    if (const char* bad = bundle_shape_error(log_domain, log_cell)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (const char* bad = bundles_call_error(bundle_first, nullptr, n_bundles)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (bundle_first[n_bundles] && !index) return FRIEDA_ERR_ARG;
    // the malformed rule and the witness counts: once per bundle, whatever n_blobs is
    wfirst.assign((size_t)n_bundles + 1, 0);
    for (uint32_t b = 0; b < n_bundles; b++) {
        const uint32_t* p = index + bundle_first[b];
        const size_t k = bundle_first[b + 1] - bundle_first[b];
        if (const char* bad = bundle_malformed(log_domain, log_cell, p, k)) return ctx->c.fail(FRIEDA_ERR_ARG, fn + ("bundle " + std::to_string(b) + ": ") + bad);
        wfirst[b + 1] = wfirst[b] + bundle_witness_count(log_domain - log_cell, p, k);
    }
    if (!out_witness) {  // the size query: nothing is launched
        memcpy(out_witness_first, wfirst.data(), 8 * wfirst.size());
        return FRIEDA_OK;
    }
    const uint64_t hashes = (uint64_t)n_blobs * wfirst[n_bundles];
    if (hashes > cap_hashes)
        return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "the witness takes " + std::to_string(hashes) + " hashes, cap_hashes is " + std::to_string(cap_hashes));
    *go = true;
    return FRIEDA_OK;
}

void open_bundles_fill(k::BundleRow* rows, uint64_t* base, uint32_t depth, uint32_t n_blobs, const uint32_t* index, const uint32_t* bundle_first,
                       uint32_t n_bundles, const uint64_t* wfirst) {
    for (uint32_t b = 0; b < n_bundles; b++) {
        rows[b] = k::BundleRow{bundle_first[b], bundle_first[b + 1] - bundle_first[b], n_blobs ? (uint32_t)wfirst[b] : 0};
        bundle_witness_count(depth, index + bundle_first[b], rows[b].n_cells, std::max<uint64_t>(n_blobs, 1) * wfirst[b], base + (size_t)b * depth);
    }
}

int open_bundles_finish(Ctx* ctx, size_t in_bytes, size_t a_out, size_t vb, size_t wb, uint32_t* out_values, uint8_t* out_witness) {
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    FR_HIP(ctx, hipGetLastError());
    FR_HIP(ctx, hipMemcpyAsync(pin + in_bytes, ctx->arena + a_out, cells_al(vb) + wb, hipMemcpyDeviceToHost, ctx->stream));
    FR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out_values, pin + in_bytes, vb);
    if (wb) memcpy(out_witness, pin + in_bytes + cells_al(vb), wb);
    return FRIEDA_OK;
}

// ---- the pass driver of both forms (host.h) ----
int verify_bundles_passes(Ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                          const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness, const uint64_t* witness_first,
                          uint8_t* out_status, CellPool* pool) {
    const bool stripes = n_blobs != 0;
    const size_t nb = stripes ? n_blobs : 1;  // the status bytes of a bundle; what multiplies its values and its witness (bundles_pass.h)
    const std::string fn = stripes ? "verify_stripe_bundles" : "verify_cell_bundles";
    std::vector<uint8_t> cls(n_bundles);
    bundles_classify(log_domain, log_cell, cell_index, bundle_first, n_bundles, witness_first, cls.data());
    std::vector<uint32_t> good;  // the bundles that are staged
    std::vector<BundleSize> sz;
    size_t good_cells = 0;
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (cls[b] == FRIEDA_BUNDLE_MALFORMED) {
            memset(out_status + (size_t)b * nb, FRIEDA_BUNDLE_MALFORMED, nb);
            continue;
        }
        good.push_back(b);
        sz.push_back(BundleSize{bundle_first[b + 1] - bundle_first[b], witness_first[b + 1] - witness_first[b]});
        good_cells += sz.back().cells;
    }
    if (pool) pool->n = 0;
    if (good.empty()) return FRIEDA_OK;
    const size_t vb = ((size_t)16 << log_cell) * nb;  // the values of one cell, or of one stripe
    FR_HIP(ctx, hipSetDevice(ctx->device));
    if (pool) {
        const int rc = pool->alloc(ctx, good_cells, vb, stripes ? "poison(stripe pool)" : "poison(cell pool)");
        if (rc) return rc;
    }
    size_t budget = ctx->tuning.test_verify_pass_bytes ? (size_t)ctx->tuning.test_verify_pass_bytes : CELLS_PASS_BYTES;
    // (stripes: at most 2^30 bytes a pass: the cells and the (bundle, blob) waves of a pass stay 32-bit whatever the test hook asks for)
    if (stripes) budget = std::min<size_t>(budget, (size_t)1 << 30);
    hipStream_t s = ctx->stream;
    DevBuf coms;  // stripes: the commitments, per-call device memory read by every pass
    {
        // one plan for the call: the component-wise largest pass
        const BundlesPassPlan p = bundles_pass_plan(log_cell, bundles_call_count(log_cell, sz.data(), sz.size(), budget, nb), nb);
        int rc = ctx->ensure_arena(p.arena);
        if (rc) return rc;
        rc = ensure_pinned(ctx, stripes ? std::max(p.pinned, 32 * nb) : p.pinned);
        if (rc) return rc;
        if (stripes) {
            rc = coms.alloc(ctx, 32 * nb, "poison(commitments)");
            if (rc) return rc;
            memcpy(ctx->pinned, commitments, 32 * nb);
            FR_HIP(ctx, hipMemcpyAsync(coms.p, ctx->pinned, 32 * nb, hipMemcpyHostToDevice, s));
            FR_HIP(ctx, hipStreamSynchronize(s));  // (the first pass stages over the pinned block)
        }
    }
    auto one_pass = [&](size_t first, size_t end) -> int {
        const BundlesPassCount cnt = bundles_pass_count(sz.data(), first, end);
        const BundlesPassPlan p = bundles_pass_plan(log_cell, cnt, nb);
        uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
        k::BundleRow* rows = reinterpret_cast<k::BundleRow*>(pin + p.i_tab);
        size_t co = 0, ho = 0;  // cells (stripes) and per-blob hashes staged so far
        for (size_t g = first; g < end; g++) {
            const uint32_t b = good[g];
            rows[g - first] = k::BundleRow{(uint32_t)co, sz[g].cells, (uint32_t)ho};
            memcpy(pin + p.i_idx + 4 * co, cell_index + bundle_first[b], 4 * (size_t)sz[g].cells);
            memcpy(pin + p.i_val + vb * co, reinterpret_cast<const uint8_t*>(values) + vb * bundle_first[b], vb * sz[g].cells);
            if (sz[g].hashes) memcpy(pin + p.i_wit + 32 * nb * ho, witness + 32 * nb * witness_first[b], 32 * nb * (size_t)sz[g].hashes);
            co += sz[g].cells, ho += (size_t)sz[g].hashes;
        }
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_in, pin, p.in_bytes, hipMemcpyHostToDevice, s));
        const uint32_t* d_values = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_val);
        const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_idx);
        k::CellsVerifyArgs ra{};  // (cells_roots reads values and writes roots / bad: it knows neither index, witness nor commitment)
        ra.values = d_values, ra.roots = reinterpret_cast<uint32_t*>(ctx->arena + p.a_roots), ra.bad = reinterpret_cast<uint32_t*>(ctx->arena + p.a_bad);
        ra.n = log_domain, ra.log_cell = log_cell, ra.n_cells = (uint32_t)(cnt.cells * nb);
        auto walk_args = [&](auto wa) {  // what BundleWalkArgs and StripeBundleWalkArgs have in common
            wa.values = d_values, wa.roots = ra.roots, wa.bad = ra.bad, wa.idx = d_idx;
            wa.rows = reinterpret_cast<const k::BundleRow*>(ctx->arena + p.a_in + p.i_tab);
            wa.witness = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_wit);
            wa.status = reinterpret_cast<uint32_t*>(ctx->arena + p.a_res);
            wa.n = log_domain, wa.log_cell = log_cell, wa.n_cells = ra.n_cells, wa.n_bundles = (uint32_t)cnt.bundles;
            wa.n_hashes = (uint32_t)cnt.hashes, wa.max_cells = cnt.max_cells;
            return wa;
        };
        FR_HIP(ctx, hipMemsetAsync(ctx->arena + p.a_res, 0xFF, p.res_bytes, s));  // (a word the kernel did not write is neither 0 nor 1)
        k::cells_roots(ctx->launch(), ra);
        if (stripes) {
            k::StripeBundleWalkArgs wa = walk_args(k::StripeBundleWalkArgs{});
            wa.commitments = static_cast<const uint32_t*>(coms.p), wa.n_blobs = n_blobs;
            k::stripe_bundle_walk(ctx->launch(), wa);
        } else {
            k::BundleWalkArgs wa = walk_args(k::BundleWalkArgs{});
            memcpy(wa.commitment, commitments, 32);
            k::bundle_walk(ctx->launch(), wa);
        }
        FR_HIP(ctx, hipGetLastError());
        const uint32_t* res = reinterpret_cast<const uint32_t*>(pin + p.p_res);
        FR_HIP(ctx, hipMemcpyAsync(pin + p.p_res, ctx->arena + p.a_res, p.res_bytes, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        uint32_t* tab = reinterpret_cast<uint32_t*>(pin + p.p_tab);
        uint32_t n_rows = 0;
        for (size_t g = first; g < end; g++) {
            uint8_t* st = out_status + (size_t)good[g] * nb;
            bool used = true;
            for (size_t j = 0; j < nb; j++) {
                const uint32_t w = res[(g - first) * nb + j];
                if (w > 1) return ctx->fail(FRIEDA_ERR_INVARIANT, fn + ": the kernel left no status");
                st[j] = w ? FRIEDA_BUNDLE_ACCEPTED : FRIEDA_BUNDLE_REJECTED;
                used = used && w;
            }
            if (!pool || !used) continue;
            const k::BundleRow& r = rows[g - first];  // a gather row per cell (stripe) of a used bundle: (slot of the pass, entry of the pool)
            for (uint32_t i = 0; i < r.n_cells; i++, n_rows++) tab[2 * n_rows] = r.first_cell + i, tab[2 * n_rows + 1] = (uint32_t)pool->n++;
        }
        if (n_rows) {
            const uint32_t* d_tab = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_tab);
            FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_tab, tab, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            if (stripes)
                k::cells_stripe_gather(ctx->launch(), d_tab, n_rows, d_values, d_idx, 1, n_blobs, log_cell, pool->d_idx(), pool->d_val());
            else
                k::cells_gather(ctx->launch(), d_tab, n_rows, d_values, d_idx, log_cell, pool->d_idx(), pool->d_val());
            FR_HIP(ctx, hipGetLastError());
            FR_HIP(ctx, hipStreamSynchronize(s));  // (the table sits in the pinned block the next pass overwrites: wait for the copy)
        }
        return FRIEDA_OK;
    };
    for (size_t first = 0; first < sz.size();) {
        const size_t end = bundles_pass_end(log_cell, sz.data(), sz.size(), first, budget, nb);
        const int rc = one_pass(first, end);
        if (rc != FRIEDA_OK) {
            (void)hipStreamSynchronize(s);  // (a pass ends drained; a failed one is drained here, before `coms` and the caller's pool go)
            return rc;
        }
        first = end;
    }
    return FRIEDA_OK;
}

namespace {

// Provider.  One upload (indices | bundle table | per-(bundle, level) witness offsets), the launches, one download (values | witness),
// one synchronisation.  wfirst[n_bundles + 1]: the witness offsets the caller computed from the indices.
int open_cell_bundles(Ctx* ctx, const Encoded* enc, uint32_t log_cell, const uint32_t* cell_index, const uint32_t* bundle_first, uint32_t n_bundles,
                      const std::vector<uint64_t>& wfirst, uint32_t* out_values, uint8_t* out_witness) {
    const uint32_t n = enc->n, depth = n - log_cell, n_cells = bundle_first[n_bundles];
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ib = 4 * (size_t)n_cells, rb = sizeof(k::BundleRow) * (size_t)n_bundles, lb = 8 * (size_t)n_bundles * depth;
    const size_t vb = ((size_t)16 << log_cell) * n_cells, wb = 32 * (size_t)wfirst[n_bundles];
    const size_t i_rows = cells_al(ib), i_base = i_rows + cells_al(rb), in_bytes = i_base + cells_al(lb);
    ArenaPlan ap;
    const size_t a_in = ap.take(in_bytes), a_out = ap.take(cells_al(vb) + wb);
    int rc = ctx->ensure_arena(ap.off);
    if (rc) return rc;
    rc = ensure_pinned(ctx, in_bytes + cells_al(vb) + wb);
    if (rc) return rc;
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    memcpy(pin, cell_index, ib);
    open_bundles_fill(reinterpret_cast<k::BundleRow*>(pin + i_rows), reinterpret_cast<uint64_t*>(pin + i_base), depth, 0, cell_index, bundle_first, n_bundles,
                      wfirst.data());
    FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(ctx->arena + a_in);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(ctx->arena + a_out);
    uint4* d_wit = reinterpret_cast<uint4*>(ctx->arena + a_out + cells_al(vb));
    k::cells_open_values(ctx->launch(), k::CellsOpenArgs{enc->eval(), enc->tree(), n, log_cell, enc->skip_log, n_cells, d_idx, d_out, nullptr});
    if (wb)
        k::bundle_open_witness(ctx->launch(), k::BundleOpenArgs{enc->eval(), enc->tree(), n, log_cell, enc->skip_log, n_bundles, d_idx,
                                                                reinterpret_cast<const k::BundleRow*>(ctx->arena + a_in + i_rows),
                                                                reinterpret_cast<const uint64_t*>(ctx->arena + a_in + i_base), d_wit});
    return open_bundles_finish(ctx, in_bytes, a_out, vb, wb, out_values, out_witness);
}

// the argument rule the two verifiers and the rebuild share: null pointers and the call's own structure; null when it holds
const char* verify_bundles_args_error(const uint8_t* commitment, uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                                      const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                      const uint64_t* witness_first, const uint8_t* out_status) {
    if (!commitment || !bundle_first || !witness_first || !out_status) return "null argument";
    if (const char* bad = bundle_shape_error(log_domain, log_cell)) return bad;
    if (const char* bad = bundles_call_error(bundle_first, witness_first, n_bundles)) return bad;
    if (bundle_first[n_bundles] && (!cell_index || !values)) return "null argument";
    if (witness_first[n_bundles] && !witness) return "null argument";
    if (witness_first[n_bundles] > ((uint64_t)1 << 40)) return "witness_first out of range";
    return nullptr;
}

}  // namespace

}  // namespace frieda

using namespace frieda;

extern "C" {
int frieda_cell_bundle_witness_count(uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells, size_t* n_hashes) {
    if (!n_hashes || (n_cells && !cell_index)) return FRIEDA_ERR_ARG;
    if (bundle_malformed(log_domain, log_cell, cell_index, n_cells)) return FRIEDA_ERR_ARG;
    *n_hashes = (size_t)bundle_witness_count(log_domain - log_cell, cell_index, n_cells);
    return FRIEDA_OK;
}

int frieda_open_cell_bundles(frieda_ctx* ctx, const frieda_encoded* enc, uint32_t log_cell, const uint32_t* cell_index, const uint32_t* bundle_first,
                             uint32_t n_bundles, uint32_t* out_values, uint8_t* out_witness, size_t cap_hashes, uint64_t* out_witness_first) {
    if (!ctx || !enc) return FRIEDA_ERR_ARG;
    if (n_bundles == 0) return FRIEDA_OK;
    FR_GUARD_BEGIN
    std::vector<uint64_t> wfirst;
    bool go;
    int rc = open_bundles_front(ctx, "open_cell_bundles: ", enc->e.n, 1, log_cell, cell_index, bundle_first, n_bundles, out_values, out_witness, cap_hashes,
                                out_witness_first, wfirst, &go);
    if (!go) return rc;
    FR_NO_JOB(&ctx->c);
    if (ctx->c.device != enc->e.device) return ctx->c.fail(FRIEDA_ERR_ARG, "open_cell_bundles: the context is not on the encoded blob's device");
    rc = open_cell_bundles(&ctx->c, &enc->e, log_cell, cell_index, bundle_first, n_bundles, wfirst, out_values, out_witness);
    if (rc == FRIEDA_OK) memcpy(out_witness_first, wfirst.data(), 8 * wfirst.size());
    return rc;
    FR_GUARD_END(ctx)
}

int frieda_verify_cell_bundles(const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, const uint32_t* bundle_first,
                               uint32_t n_bundles, const uint32_t* values, const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_status) {
    if (n_bundles == 0) return FRIEDA_OK;
    if (verify_bundles_args_error(commitment, log_domain, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first, out_status))
        return FRIEDA_ERR_ARG;
    try {
        verify_cell_bundles_host(commitment, log_domain, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first, out_status);
    } catch (const std::bad_alloc&) {
        return FRIEDA_ERR_NOMEM;
    }
    return FRIEDA_OK;
}

int frieda_verify_cell_bundles_many(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                                    const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                    const uint64_t* witness_first, uint8_t* out_status) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (n_bundles == 0) return FRIEDA_OK;
    if (const char* bad = verify_bundles_args_error(commitment, log_domain, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first, out_status))
        return ctx->c.fail(FRIEDA_ERR_ARG, std::string("verify_cell_bundles_many: ") + bad);
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    return verify_bundles_passes(&ctx->c, commitment, 0, log_domain, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first, out_status,
                                 nullptr);
    FR_GUARD_END(ctx)
}

namespace {
// frieda_reconstruct_from_cell_bundles (out_enc == nullptr: out_bytes required) and frieda_rebuild_encoded_from_cell_bundles (the tail
// that returns the handle; out_bytes optional)
int reconstruct_from_cell_bundles(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                  const uint32_t* cell_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                  const uint64_t* witness_first, uint8_t* out_bytes, uint8_t* out_status, size_t* n_cells_used, frieda_encoded** out_enc) {
    if (!ctx || !commitment || !n_cells_used || (len && !out_bytes && !out_enc)) return FRIEDA_ERR_ARG;
    *n_cells_used = 0;
    const char* const fn = out_enc ? "rebuild_encoded_from_cell_bundles: " : "reconstruct_from_cell_bundles: ";
    uint32_t L, n;
    if (const int rc = rebuild_shape(ctx, fn, log_blowup_factor, len, &L, &n)) return rc;
    if (n_bundles)
        if (const char* bad = verify_bundles_args_error(commitment, n, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first, out_status))
            return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (!n_bundles)
        if (const char* bad = bundle_shape_error(n, log_cell)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    CellPool pool;
    if (n_bundles)
        if (const int rc = verify_bundles_passes(&ctx->c, commitment, 0, n, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first,
                                                 out_status, &pool))
            return rc;
    return rebuild_from_pool(ctx, pool, commitment, 0, log_blowup_factor, len, log_cell, "distinct cells in accepted bundles", out_bytes, out_enc, n_cells_used);
    FR_GUARD_END(ctx)
}
}  // namespace

int frieda_reconstruct_from_cell_bundles(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                         const uint32_t* cell_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values,
                                         const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_bytes, uint8_t* out_status, size_t* n_cells_used) {
    return reconstruct_from_cell_bundles(ctx, commitment, log_blowup_factor, len, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first,
                                         out_bytes, out_status, n_cells_used, nullptr);
}
int frieda_rebuild_encoded_from_cell_bundles(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                             const uint32_t* cell_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values,
                                             const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_bytes, uint8_t* out_status,
                                             size_t* n_cells_used, frieda_encoded** out_enc) {
    if (!out_enc) return FRIEDA_ERR_ARG;
    *out_enc = nullptr;
    return reconstruct_from_cell_bundles(ctx, commitment, log_blowup_factor, len, log_cell, cell_index, bundle_first, n_bundles, values, witness, witness_first,
                                         out_bytes, out_status, n_cells_used, out_enc);
}

}  // extern "C"
