// stripe_bundles_host.cpp — stripe bundles: the host side of stripe_bundles.hip and its exports (frieda_open_stripe_bundles,
// frieda_verify_stripe_bundles, frieda_verify_stripe_bundles_many, frieda_reconstruct_blobs_from_stripe_bundles).
//
// A stripe bundle is the answer to one request over a block of n_blobs blobs of one shape: k stripes (a stripe is cell j of every blob)
// with one shared hash witness per blob.  Every blob of a bundle has the same indices, so the malformed rule, the witness length W_b and
// the per-level offsets are computed once per bundle (bundles_host.h), never once per (bundle, blob).  Layouts: values
// [stripes][n_blobs][4][2^log_cell], stripe-major; witness_first counts hashes per blob; bundle b's witness block starts at hash
// n_blobs * witness_first[b], blob j's piece — byte for byte that blob's cell-bundle witness — at j * W_b inside it.
//
// The device verifier and the rebuild run the pass driver of bundles_host.cpp (verify_bundles_passes, n_blobs >= 1: also for a block of
// one blob).  MALFORMED is decided on the host, once per bundle, before anything is staged; a well-formed bundle stages its indices once
// and its values and witness n_blobs times (bundles_pass.h with the factor n_blobs); a pass runs cells_roots over all its cells and
// stripe_bundle_walk, one wave per (bundle, blob).  The host has every pass's status words anyway: it ANDs them per bundle, and with a
// pool the stripes of the USED bundles (all n_blobs bytes ACCEPTED) are gathered into it by cells_stripe_gather before the next pass
// overwrites the values.  This file keeps the exports, their argument rules and the opener; the opener's front, table fill and end are
// bundles_host.cpp's too (open_bundles_front / _fill / _finish), and the rebuild ends in rebuild_from_pool (cells_host.cpp).
#include <string.h>

#include "bundles_host.h"
#include "cells_pass.h"
#include "host.h"

namespace frieda {

namespace {

constexpr uint32_t SB_MAX_BLOBS = 65536, SB_REBUILD_MAX_BLOBS = 256;  // (the point reconstruction takes at most 1024 columns)

// Provider.  One upload (per-pair stripe indices | per-pair blob numbers | the blob table | the shared indices | the bundle table | the
// per-(bundle, level) witness offsets), the launches, one download (values | witness), one synchronisation.
int open_stripe_bundles(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, uint32_t log_cell, const uint32_t* stripe_index,
                        const uint32_t* bundle_first, uint32_t n_bundles, const std::vector<uint64_t>& wfirst, uint32_t* out_values, uint8_t* out_witness) {
    const uint32_t n = encs[0]->n, depth = n - log_cell, n_stripes = bundle_first[n_bundles];
    const uint32_t n_cells = n_stripes * n_blobs;  // (the caller checked the product)
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pb = 4 * (size_t)n_cells, tb = sizeof(k::CellsBlobRow) * (size_t)n_blobs, ib = 4 * (size_t)n_stripes;
    const size_t rb = sizeof(k::BundleRow) * (size_t)n_bundles, lb = 8 * (size_t)n_bundles * depth;
    const size_t vb = ((size_t)16 << log_cell) * n_cells, wb = 32 * (size_t)n_blobs * wfirst[n_bundles];
    const size_t i_bidx = cells_al(pb), i_tab = i_bidx + cells_al(pb), i_idx = i_tab + cells_al(tb), i_rows = i_idx + cells_al(ib);
    const size_t i_base = i_rows + cells_al(rb), in_bytes = i_base + cells_al(lb);
    ArenaPlan ap;
    const size_t a_in = ap.take(in_bytes), a_out = ap.take(cells_al(vb) + wb);
    int rc = ctx->ensure_arena(ap.off);
    if (rc) return rc;
    rc = ensure_pinned(ctx, in_bytes + cells_al(vb) + wb);
    if (rc) return rc;
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    uint32_t* pair_idx = reinterpret_cast<uint32_t*>(pin);
    uint32_t* pair_blob = reinterpret_cast<uint32_t*>(pin + i_bidx);
    for (uint32_t t = 0; t < n_stripes; t++)
        for (uint32_t j = 0; j < n_blobs; j++) pair_idx[(size_t)t * n_blobs + j] = stripe_index[t], pair_blob[(size_t)t * n_blobs + j] = j;
    k::CellsBlobRow* table = reinterpret_cast<k::CellsBlobRow*>(pin + i_tab);
    for (uint32_t j = 0; j < n_blobs; j++) table[j] = k::CellsBlobRow{encs[j]->eval(), encs[j]->tree(), encs[j]->skip_log, 0};
    memcpy(pin + i_idx, stripe_index, ib);
    // once per bundle: the offsets of blob 0's piece; blob j's lie j * W_b further on
    open_bundles_fill(reinterpret_cast<k::BundleRow*>(pin + i_rows), reinterpret_cast<uint64_t*>(pin + i_base), depth, n_blobs, stripe_index, bundle_first,
                      n_bundles, wfirst.data());
    FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    const k::CellsBlobRow* d_table = reinterpret_cast<const k::CellsBlobRow*>(ctx->arena + a_in + i_tab);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(ctx->arena + a_out);
    uint4* d_wit = reinterpret_cast<uint4*>(ctx->arena + a_out + cells_al(vb));
    k::cells_open_blobs_values(ctx->launch(), k::CellsOpenBlobsArgs{d_table, reinterpret_cast<const uint32_t*>(ctx->arena + a_in + i_bidx),
                                                                    reinterpret_cast<const uint32_t*>(ctx->arena + a_in), n, log_cell, n_cells, d_out, nullptr});
    if (wb)
        k::stripe_bundle_open_witness(ctx->launch(),
                                      k::StripeBundleOpenArgs{d_table, n, log_cell, n_blobs, n_bundles, (uint32_t)wfirst[n_bundles],
                                                              reinterpret_cast<const uint32_t*>(ctx->arena + a_in + i_idx),
                                                              reinterpret_cast<const k::BundleRow*>(ctx->arena + a_in + i_rows),
                                                              reinterpret_cast<const uint64_t*>(ctx->arena + a_in + i_base), d_wit});
    return open_bundles_finish(ctx, in_bytes, a_out, vb, wb, out_values, out_witness);
}

// what the three verifying entry points refuse beyond stripe_bundles_args_error: counts the 32-bit tables of a pass cannot hold
const char* stripe_bundles_size_error(uint32_t n_blobs, const uint32_t* bundle_first, uint32_t n_bundles, const uint64_t* witness_first) {
    if ((uint64_t)bundle_first[n_bundles] * n_blobs > 0xFFFFFFFFull) return "more than 2^32 cells";
    if (witness_first[n_bundles] > 0xFFFFFFFFull) return "witness_first out of range";
    return nullptr;
}

}  // namespace

}  // namespace frieda

using namespace frieda;

extern "C" {
int frieda_open_stripe_bundles(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, uint32_t log_cell, const uint32_t* stripe_index,
                               const uint32_t* bundle_first, uint32_t n_bundles, uint32_t* out_values, uint8_t* out_witness, size_t cap_hashes,
                               uint64_t* out_witness_first) {
    if (!ctx || !encs || n_blobs == 0 || n_blobs > SB_MAX_BLOBS) return FRIEDA_ERR_ARG;
    for (uint32_t j = 0; j < n_blobs; j++)
        if (!encs[j]) return FRIEDA_ERR_ARG;
    FR_GUARD_BEGIN
    const char* const fn = "open_stripe_bundles: ";
    const uint32_t n = encs[0]->e.n;
    std::vector<const Encoded*> blobs(n_blobs);
    for (uint32_t j = 0; j < n_blobs; j++) {
        if (encs[j]->e.n != n) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "the blobs of a call must have one log_domain");
        if (encs[j]->e.device != ctx->c.device) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "the context is not on the encoded blobs' device");
        blobs[j] = &encs[j]->e;
    }
    if (n_bundles == 0) return FRIEDA_OK;
    std::vector<uint64_t> wfirst;
    bool go;
    int rc = open_bundles_front(ctx, fn, n, n_blobs, log_cell, stripe_index, bundle_first, n_bundles, out_values, out_witness, cap_hashes, out_witness_first, wfirst, &go);
    if (!go) return rc;
    if (const char* bad = stripe_bundles_size_error(n_blobs, bundle_first, n_bundles, wfirst.data())) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    FR_NO_JOB(&ctx->c);
    rc = open_stripe_bundles(&ctx->c, blobs.data(), n_blobs, log_cell, stripe_index, bundle_first, n_bundles, wfirst, out_values, out_witness);
    if (rc == FRIEDA_OK) memcpy(out_witness_first, wfirst.data(), 8 * wfirst.size());
    return rc;
    FR_GUARD_END(ctx)
}

int frieda_verify_stripe_bundles(const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* stripe_index,
                                 const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                 const uint64_t* witness_first, uint8_t* out_status) {
    if (n_bundles == 0) return FRIEDA_OK;
    if (stripe_bundles_args_error(commitments, n_blobs, SB_MAX_BLOBS, log_domain, log_cell, stripe_index, bundle_first, n_bundles, values, witness, witness_first,
                                  out_status))
        return FRIEDA_ERR_ARG;
    try {
        verify_stripe_bundles_host(commitments, n_blobs, log_domain, log_cell, stripe_index, bundle_first, n_bundles, values, witness, witness_first, out_status);
    } catch (const std::bad_alloc&) {
        return FRIEDA_ERR_NOMEM;
    }
    return FRIEDA_OK;
}

int frieda_verify_stripe_bundles_many(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell,
                                      const uint32_t* stripe_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values,
                                      const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_status) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (n_bundles == 0) return FRIEDA_OK;
    const char* const fn = "verify_stripe_bundles_many: ";
    if (const char* bad = stripe_bundles_args_error(commitments, n_blobs, SB_MAX_BLOBS, log_domain, log_cell, stripe_index, bundle_first, n_bundles, values, witness,
                                                    witness_first, out_status))
        return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (const char* bad = stripe_bundles_size_error(n_blobs, bundle_first, n_bundles, witness_first)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    return verify_bundles_passes(&ctx->c, commitments, n_blobs, log_domain, log_cell, stripe_index, bundle_first, n_bundles, values, witness, witness_first,
                                 out_status, nullptr);
    FR_GUARD_END(ctx)
}

namespace {
// frieda_reconstruct_blobs_from_stripe_bundles (out_encs == nullptr: its tail rebuild_blobs_from_stripes) and
// frieda_rebuild_encoded_blobs_from_stripe_bundles (out_encs[n_blobs], all NULL on entry; out_bytes optional)
int reconstruct_blobs_from_stripe_bundles(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                                          uint32_t log_cell, const uint32_t* stripe_index, const uint32_t* bundle_first, uint32_t n_bundles,
                                          const uint32_t* values, const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_bytes,
                                          uint8_t* out_status, size_t* n_stripes_used, frieda_encoded** out_encs) {
    if (!ctx || !commitments || !n_stripes_used || (len && !out_bytes && !out_encs)) return FRIEDA_ERR_ARG;
    *n_stripes_used = 0;
    const char* const fn = out_encs ? "rebuild_encoded_blobs_from_stripe_bundles: " : "reconstruct_blobs_from_stripe_bundles: ";
    if (n_blobs == 0 || n_blobs > SB_REBUILD_MAX_BLOBS) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "n_blobs out of range (1 .. 256)");
    uint32_t L, n;
    if (const int rc = rebuild_shape(ctx, fn, log_blowup_factor, len, &L, &n)) return rc;
    if (n_bundles) {
        if (const char* bad = stripe_bundles_args_error(commitments, n_blobs, SB_REBUILD_MAX_BLOBS, n, log_cell, stripe_index, bundle_first, n_bundles, values, witness,
                                                        witness_first, out_status))
            return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
        if (const char* bad = stripe_bundles_size_error(n_blobs, bundle_first, n_bundles, witness_first)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
        // the pooled values are the point reconstruction's sample buffer: at most 2^32 words (its positions are 32-bit)
        if ((uint64_t)bundle_first[n_bundles] * n_blobs > (0x100000000ull >> (log_cell + 2))) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "more than 2^32 value words");
    } else if (const char* bad = bundle_shape_error(n, log_cell)) {
        return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    }
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    CellPool pool;
    if (n_bundles)
        if (const int rc = verify_bundles_passes(&ctx->c, commitments, n_blobs, n, log_cell, stripe_index, bundle_first, n_bundles, values, witness, witness_first,
                                                 out_status, &pool))
            return rc;
    return rebuild_from_pool(ctx, pool, commitments, n_blobs, log_blowup_factor, len, log_cell, "distinct stripes in fully accepted bundles", out_bytes, out_encs,
                             n_stripes_used);
    FR_GUARD_END(ctx)
}
}  // namespace

int frieda_reconstruct_blobs_from_stripe_bundles(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                                                 uint32_t log_cell, const uint32_t* stripe_index, const uint32_t* bundle_first, uint32_t n_bundles,
                                                 const uint32_t* values, const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_bytes,
                                                 uint8_t* out_status, size_t* n_stripes_used) {
    return reconstruct_blobs_from_stripe_bundles(ctx, commitments, n_blobs, log_blowup_factor, len, log_cell, stripe_index, bundle_first, n_bundles, values, witness,
                                                 witness_first, out_bytes, out_status, n_stripes_used, nullptr);
}
int frieda_rebuild_encoded_blobs_from_stripe_bundles(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor,
                                                     size_t len, uint32_t log_cell, const uint32_t* stripe_index, const uint32_t* bundle_first,
                                                     uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                                     const uint64_t* witness_first, uint8_t* out_bytes, uint8_t* out_status,
                                                     size_t* n_stripes_used, frieda_encoded** out_encs) {
    if (!out_encs) return FRIEDA_ERR_ARG;
    if (n_blobs >= 1 && n_blobs <= SB_REBUILD_MAX_BLOBS) memset(out_encs, 0, sizeof(frieda_encoded*) * n_blobs);
    return reconstruct_blobs_from_stripe_bundles(ctx, commitments, n_blobs, log_blowup_factor, len, log_cell, stripe_index, bundle_first, n_bundles, values, witness,
                                                 witness_first, out_bytes, out_status, n_stripes_used, out_encs);
}

}  // extern "C"
