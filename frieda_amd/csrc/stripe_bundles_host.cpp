// stripe_bundles_host.cpp — stripe bundles: the host side of stripe_bundles.hip and its exports (frieda_open_stripe_bundles,
// frieda_verify_stripe_bundles, frieda_verify_stripe_bundles_many, frieda_reconstruct_blobs_from_stripe_bundles).
//
// A stripe bundle is the answer to one request over a block of n_blobs blobs of one shape: k stripes (a stripe is cell j of every blob)
// with one shared hash witness per blob.  Every blob of a bundle has the same indices, so the malformed rule, the witness length W_b and
// the per-level offsets are computed once per bundle (bundles_host.h), never once per (bundle, blob).  Layouts: values
// [stripes][n_blobs][4][2^log_cell], stripe-major; witness_first counts hashes per blob; bundle b's witness block starts at hash
// n_blobs * witness_first[b], blob j's piece — byte for byte that blob's cell-bundle witness — at j * W_b inside it.
//
// One pass driver serves the device verifier and the rebuild.  MALFORMED is decided on the host, once per bundle, before anything is
// staged; a well-formed bundle stages its indices once and its values and witness n_blobs times (bundles_pass.h with the factor
// n_blobs); a pass runs cells_roots over all its cells and stripe_bundle_walk, one wave per (bundle, blob).  The host has every pass's
// status words anyway: it ANDs them per bundle, and with a pool the stripes of the USED bundles (all n_blobs bytes ACCEPTED) are gathered
// into it by cells_stripe_gather before the next pass overwrites the values.
#include <string.h>

#include <algorithm>

#include "bundles_host.h"
#include "bundles_pass.h"
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
    hipStream_t s = ctx->stream;
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    uint32_t* pair_idx = reinterpret_cast<uint32_t*>(pin);
    uint32_t* pair_blob = reinterpret_cast<uint32_t*>(pin + i_bidx);
    for (uint32_t t = 0; t < n_stripes; t++)
        for (uint32_t j = 0; j < n_blobs; j++) pair_idx[(size_t)t * n_blobs + j] = stripe_index[t], pair_blob[(size_t)t * n_blobs + j] = j;
    k::CellsBlobRow* table = reinterpret_cast<k::CellsBlobRow*>(pin + i_tab);
    for (uint32_t j = 0; j < n_blobs; j++) table[j] = k::CellsBlobRow{encs[j]->eval(), encs[j]->tree(), encs[j]->skip_log, 0};
    memcpy(pin + i_idx, stripe_index, ib);
    k::BundleRow* rows = reinterpret_cast<k::BundleRow*>(pin + i_rows);
    uint64_t* base = reinterpret_cast<uint64_t*>(pin + i_base);
    for (uint32_t b = 0; b < n_bundles; b++) {
        rows[b] = k::BundleRow{bundle_first[b], bundle_first[b + 1] - bundle_first[b], (uint32_t)wfirst[b]};
        // once per bundle: the offsets of blob 0's piece; blob j's lie j * W_b further on
        bundle_witness_count(depth, stripe_index + bundle_first[b], rows[b].n_cells, (uint64_t)n_blobs * wfirst[b], base + (size_t)b * depth);
    }
    FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, in_bytes, hipMemcpyHostToDevice, s));
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
    FR_HIP(ctx, hipGetLastError());
    FR_HIP(ctx, hipMemcpyAsync(pin + in_bytes, ctx->arena + a_out, cells_al(vb) + wb, hipMemcpyDeviceToHost, s));
    FR_HIP(ctx, hipStreamSynchronize(s));
    memcpy(out_values, pin + in_bytes, vb);
    if (wb) memcpy(out_witness, pin + in_bytes + cells_al(vb), wb);
    return FRIEDA_OK;
}

// out_status[n_bundles][n_blobs].  MALFORMED on the host (the bundle's whole row), the rest from the kernels, staged in passes
// (bundles_pass.h, factor n_blobs).  Uses the arena and the pinned block (callers: FR_NO_JOB).  pool (optional): receives, in the caller's
// order, the stripes of the bundles whose n_blobs bytes are all ACCEPTED.
int verify_stripe_bundles_passes(Ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell,
                                 const uint32_t* stripe_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                 const uint64_t* witness_first, uint8_t* out_status, CellPool* pool) {
    std::vector<uint8_t> cls(n_bundles);
    bundles_classify(log_domain, log_cell, stripe_index, bundle_first, n_bundles, witness_first, cls.data());
    std::vector<uint32_t> good;  // the bundles that are staged
    std::vector<BundleSize> sz;
    size_t good_stripes = 0;
    for (uint32_t b = 0; b < n_bundles; b++) {
        if (cls[b] == FRIEDA_BUNDLE_MALFORMED) {
            memset(out_status + (size_t)b * n_blobs, FRIEDA_BUNDLE_MALFORMED, n_blobs);
            continue;
        }
        good.push_back(b);
        sz.push_back(BundleSize{bundle_first[b + 1] - bundle_first[b], witness_first[b + 1] - witness_first[b]});
        good_stripes += sz.back().cells;
    }
    if (pool) pool->n = 0;
    if (good.empty()) return FRIEDA_OK;
    const size_t vb = ((size_t)16 << log_cell) * n_blobs;  // the values of one stripe
    FR_HIP(ctx, hipSetDevice(ctx->device));
    if (pool) {
        const int rc = pool->alloc(ctx, good_stripes, vb, "poison(stripe pool)");
        if (rc) return rc;
    }
    // (at most 2^30 bytes a pass: the cells and the (bundle, blob) waves of a pass stay 32-bit whatever the test hook asks for)
    const size_t budget = std::min<size_t>(ctx->tuning.test_verify_pass_bytes ? (size_t)ctx->tuning.test_verify_pass_bytes : CELLS_PASS_BYTES, (size_t)1 << 30);
    hipStream_t s = ctx->stream;
    DevBuf coms;  // the commitments: per-call device memory, read by every pass
    {
        // one plan for the call: the component-wise largest pass
        const BundlesPassPlan p = bundles_pass_plan(log_cell, bundles_call_count(log_cell, sz.data(), sz.size(), budget, n_blobs), n_blobs);
        int rc = ctx->ensure_arena(p.arena);
        if (rc) return rc;
        rc = ensure_pinned(ctx, std::max(p.pinned, 32 * (size_t)n_blobs));
        if (rc) return rc;
        rc = coms.alloc(ctx, 32 * (size_t)n_blobs, "poison(commitments)");
        if (rc) return rc;
        memcpy(ctx->pinned, commitments, 32 * (size_t)n_blobs);
        FR_HIP(ctx, hipMemcpyAsync(coms.p, ctx->pinned, 32 * (size_t)n_blobs, hipMemcpyHostToDevice, s));
        FR_HIP(ctx, hipStreamSynchronize(s));  // (the first pass stages over the pinned block)
    }
    // every exit below has drained the stream before `coms` goes: a pass ends with a synchronisation, and a failed call is followed by one
    auto drained = [&](int rc) {
        if (rc != FRIEDA_OK) (void)hipStreamSynchronize(s);
        return rc;
    };
    auto one_pass = [&](size_t first, size_t end) -> int {
        const BundlesPassCount cnt = bundles_pass_count(sz.data(), first, end);
        const BundlesPassPlan p = bundles_pass_plan(log_cell, cnt, n_blobs);
        uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
        k::BundleRow* rows = reinterpret_cast<k::BundleRow*>(pin + p.i_tab);
        size_t so = 0, ho = 0;  // stripes and per-blob hashes staged so far
        for (size_t g = first; g < end; g++) {
            const uint32_t b = good[g];
            rows[g - first] = k::BundleRow{(uint32_t)so, sz[g].cells, (uint32_t)ho};
            memcpy(pin + p.i_idx + 4 * so, stripe_index + bundle_first[b], 4 * (size_t)sz[g].cells);
            memcpy(pin + p.i_val + vb * so, reinterpret_cast<const uint8_t*>(values) + vb * bundle_first[b], vb * sz[g].cells);
            if (sz[g].hashes)
                memcpy(pin + p.i_wit + 32 * n_blobs * ho, witness + 32 * n_blobs * witness_first[b], 32 * (size_t)n_blobs * (size_t)sz[g].hashes);
            so += sz[g].cells, ho += (size_t)sz[g].hashes;
        }
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_in, pin, p.in_bytes, hipMemcpyHostToDevice, s));
        const uint32_t* d_values = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_val);
        const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_idx);
        uint32_t* d_roots = reinterpret_cast<uint32_t*>(ctx->arena + p.a_roots);
        uint32_t* d_bad = reinterpret_cast<uint32_t*>(ctx->arena + p.a_bad);
        k::CellsVerifyArgs ra{};  // (cells_roots reads values and writes roots / bad: it knows neither index, witness nor commitment)
        ra.values = d_values, ra.roots = d_roots, ra.bad = d_bad;
        ra.n = log_domain, ra.log_cell = log_cell, ra.n_cells = (uint32_t)(cnt.cells * n_blobs);
        k::StripeBundleWalkArgs wa{};
        wa.values = d_values, wa.roots = d_roots, wa.bad = d_bad, wa.idx = d_idx;
        wa.rows = reinterpret_cast<const k::BundleRow*>(ctx->arena + p.a_in + p.i_tab);
        wa.witness = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_wit);
        wa.commitments = static_cast<const uint32_t*>(coms.p);
        wa.status = reinterpret_cast<uint32_t*>(ctx->arena + p.a_res);
        wa.n = log_domain, wa.log_cell = log_cell, wa.n_cells = ra.n_cells, wa.n_blobs = n_blobs, wa.n_bundles = (uint32_t)cnt.bundles;
        wa.n_hashes = (uint32_t)cnt.hashes, wa.max_cells = cnt.max_cells;
        FR_HIP(ctx, hipMemsetAsync(ctx->arena + p.a_res, 0xFF, p.res_bytes, s));  // (a word the kernel did not write is neither 0 nor 1)
        k::cells_roots(ctx->launch(), ra);
        k::stripe_bundle_walk(ctx->launch(), wa);
        FR_HIP(ctx, hipGetLastError());
        const uint32_t* res = reinterpret_cast<const uint32_t*>(pin + p.p_res);
        FR_HIP(ctx, hipMemcpyAsync(pin + p.p_res, ctx->arena + p.a_res, p.res_bytes, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        uint32_t* tab = reinterpret_cast<uint32_t*>(pin + p.p_tab);
        uint32_t n_rows = 0;
        for (size_t g = first; g < end; g++) {
            uint8_t* st = out_status + (size_t)good[g] * n_blobs;
            bool used = true;
            for (uint32_t j = 0; j < n_blobs; j++) {
                const uint32_t w = res[(g - first) * n_blobs + j];
                if (w > 1) return ctx->fail(FRIEDA_ERR_INVARIANT, "verify_stripe_bundles: the kernel left no status");
                st[j] = w ? FRIEDA_BUNDLE_ACCEPTED : FRIEDA_BUNDLE_REJECTED;
                used = used && w;
            }
            if (!pool || !used) continue;
            const k::BundleRow& r = rows[g - first];  // a gather row per stripe of a used bundle: (stripe of the pass, entry of the pool)
            for (uint32_t i = 0; i < r.n_cells; i++, n_rows++) tab[2 * n_rows] = r.first_cell + i, tab[2 * n_rows + 1] = (uint32_t)pool->n++;
        }
        if (n_rows) {
            const uint32_t* d_tab = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_tab);
            FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_tab, tab, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            k::cells_stripe_gather(ctx->launch(), d_tab, n_rows, d_values, d_idx, 1, n_blobs, log_cell, pool->d_idx(), pool->d_val());
            FR_HIP(ctx, hipGetLastError());
            FR_HIP(ctx, hipStreamSynchronize(s));  // (the table sits in the pinned block the next pass overwrites: wait for the copy)
        }
        return FRIEDA_OK;
    };
    for (size_t first = 0; first < sz.size();) {
        const size_t end = bundles_pass_end(log_cell, sz.data(), sz.size(), first, budget, n_blobs);
        const int rc = drained(one_pass(first, end));
        if (rc != FRIEDA_OK) return rc;
        first = end;
    }
    return FRIEDA_OK;
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
    if (!bundle_first || !out_witness_first || (out_witness && !out_values)) return FRIEDA_ERR_ARG;
    if (const char* bad = bundle_shape_error(n, log_cell)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (const char* bad = bundles_call_error(bundle_first, nullptr, n_bundles)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (bundle_first[n_bundles] && !stripe_index) return FRIEDA_ERR_ARG;
    // the malformed rule and the witness counts: once per bundle, whatever n_blobs is
    std::vector<uint64_t> wfirst(n_bundles + 1, 0);
    for (uint32_t b = 0; b < n_bundles; b++) {
        const uint32_t* p = stripe_index + bundle_first[b];
        const size_t k = bundle_first[b + 1] - bundle_first[b];
        if (const char* bad = bundle_malformed(n, log_cell, p, k)) return ctx->c.fail(FRIEDA_ERR_ARG, fn + ("bundle " + std::to_string(b) + ": ") + bad);
        wfirst[b + 1] = wfirst[b] + bundle_witness_count(n - log_cell, p, k);
    }
    if (!out_witness) {  // the size query: nothing is launched
        memcpy(out_witness_first, wfirst.data(), 8 * wfirst.size());
        return FRIEDA_OK;
    }
    if ((uint64_t)n_blobs * wfirst[n_bundles] > cap_hashes)
        return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "the witness takes " + std::to_string((uint64_t)n_blobs * wfirst[n_bundles]) + " hashes, cap_hashes is " +
                                               std::to_string(cap_hashes));
    if (const char* bad = stripe_bundles_size_error(n_blobs, bundle_first, n_bundles, wfirst.data())) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    FR_NO_JOB(&ctx->c);
    const int rc = open_stripe_bundles(&ctx->c, blobs.data(), n_blobs, log_cell, stripe_index, bundle_first, n_bundles, wfirst, out_values, out_witness);
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
    return verify_stripe_bundles_passes(&ctx->c, commitments, n_blobs, log_domain, log_cell, stripe_index, bundle_first, n_bundles, values, witness, witness_first,
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
    if (log_blowup_factor > FRIEDA_MAX_LOG_DOMAIN || len > ((size_t)1 << 40)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "shape out of range");
    const uint32_t L = codec_shape(len).log_size, n = L + log_blowup_factor;
    if (L < 1 || n < 2 || n + 1 > FRIEDA_MAX_LOG_DOMAIN) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "shape out of range");
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
    const size_t need = log_cell ? (((size_t)1 << L) >> log_cell) + 1 : ((size_t)1 << L) + 2;
    uint32_t nd = 0;
    auto too_few = [&]() {
        return ctx->c.fail(FRIEDA_ERR_ARG, std::to_string(nd) + " distinct stripes in fully accepted bundles, " + std::to_string(need) + " needed");
    };
    if (n_bundles == 0) return too_few();
    CellPool pool;
    int rc = verify_stripe_bundles_passes(&ctx->c, commitments, n_blobs, n, log_cell, stripe_index, bundle_first, n_bundles, values, witness, witness_first,
                                          out_status, &pool);
    if (rc != FRIEDA_OK) return rc;
    if (pool.n == 0) return too_few();
    rc = out_encs ? rebuild_encoded_from_pool(ctx, pool, commitments, n_blobs, log_blowup_factor, len, log_cell, nullptr, out_bytes, &nd, out_encs)
                  : rebuild_blobs_from_stripes(ctx, pool, commitments, n_blobs, log_blowup_factor, len, log_cell, out_bytes, &nd);
    *n_stripes_used = nd;
    return rc == FRIEDA_ERR_ARG && nd < need ? too_few() : rc;
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
