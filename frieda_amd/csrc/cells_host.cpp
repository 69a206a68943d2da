// cells_host.cpp — authenticated cells: the host side of cells.hip and its exports (frieda_open_cells, frieda_verify_cells,
// frieda_verify_cells_many, frieda_reconstruct_from_opened_cells, and their forms over the blobs of a block: frieda_open_cells_blobs,
// frieda_verify_cells_blobs, frieda_verify_cells_blobs_many, frieda_reconstruct_blobs_from_opened_stripes).
//
// A cell with its path is a self-contained message (values, index, path): every cell carries its own n - log_cell siblings, nothing is
// shared between the cells of a call, and a cell's status never depends on the others.  The host verifier and the kernels hash the
// same way (blake2s.h): a leaf is the four column words of one position, a node its two children.
//
// One opener, one host verifier and one pass driver serve both forms.  Blobs of a block: cell i of a call is cell cell_index[i] of blob
// blob_index[i]; the single-blob calls are the same code without blob numbers, and launch the single-blob kernels.  The driver
// (verify_cells_passes) stages a call through the pinned block and the arena in passes cut by cells_pass.h; with a pool, what a pass
// accepted — cells, or whole stripes (cell j of every blob) — is gathered into it before the next pass overwrites the staged values.
//
// The rebuilds from a pool — the two here and the two from bundles (bundles_host.cpp, stripe_bundles_host.cpp) — share their shape rule
// (rebuild_shape) and their tail (rebuild_from_pool: the dispatch to rebuild_blob, rebuild_blobs_from_stripes or rebuild_encoded_from_pool,
// how many entries the reconstruction needs, and the "too few" message); an entry point keeps its argument checks, its verify call and
// its noun.
#include <string.h>

#include <algorithm>

#include "cells_pass.h"
#include "host.h"

namespace frieda {

namespace {

// compress(0, left || right) / compress(0, leaf words || 0 x 12) on words, as the kernels do
void node_words(const uint32_t* l, const uint32_t* r, uint32_t* out) {
    uint32_t m[16], h[8];
    memcpy(m, l, 32);
    memcpy(m + 8, r, 32);
    b2_merkle_block_lat(m, h);
    memcpy(out, h, 32);
}

bool host_cell_ok(const uint32_t want[8], uint32_t n, uint32_t c, uint32_t index, const uint32_t* v, const uint8_t* path, std::vector<uint32_t>& lvl) {
    const size_t cs = (size_t)1 << c;
    for (size_t i = 0; i < 4 * cs; i++)
        if (v[i] >= P31) return false;
    lvl.resize(8 * cs);
    for (size_t j = 0; j < cs; j++) {
        const uint32_t m[16] = {v[j], v[cs + j], v[2 * cs + j], v[3 * cs + j], 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t h[8];
        b2_merkle_block_lat(m, h);
        memcpy(&lvl[8 * j], h, 32);
    }
    for (size_t w = cs >> 1; w >= 1; w >>= 1)
        for (size_t j = 0; j < w; j++) node_words(&lvl[16 * j], &lvl[16 * j + 8], &lvl[8 * j]);  // (writes entry j after reading 2j, 2j + 1: j <= 2j)
    uint32_t h[8], sib[8];
    memcpy(h, lvl.data(), 32);
    for (uint32_t s = 0; s < n - c; s++) {
        memcpy(sib, path + 32 * (size_t)s, 32);
        if ((index >> s) & 1)
            node_words(sib, h, h);
        else
            node_words(h, sib, h);
    }
    return memcmp(h, want, 32) == 0;
}

// cell i's commitment: the call's one (blob_index null), or commitments[blob_index[i]]
void verify_cells_host(const uint8_t* commitments, uint32_t log_domain, uint32_t log_cell, const uint32_t* blob_index, const uint32_t* cell_index,
                       uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status) {
    const size_t vw = (size_t)4 << log_cell, pb = 32 * (size_t)(log_domain - log_cell);
    std::vector<uint32_t> lvl;
    for (uint32_t i = 0; i < n_cells; i++) {
        uint32_t want[8];
        memcpy(want, commitments + (blob_index ? 32 * (size_t)blob_index[i] : 0), 32);
        out_status[i] = host_cell_ok(want, log_domain, log_cell, cell_index[i], values + i * vw, paths + i * pb, lvl) ? FRIEDA_CELL_ACCEPTED : FRIEDA_CELL_REJECTED;
    }
}

// One status byte per cell from the kernels, staged in passes (cells_pass.h).  Uses the arena and the pinned block (callers: FR_NO_JOB).
//   n_blobs 0        one commitment, in the kernel arguments (blob_index is not read)
//   n_blobs >= 1     commitments[n_blobs][32], uploaded once; cell i belongs to blob blob_index[i]
//   ... and a pool   stripes: the cells are [n_cells / n_blobs][n_blobs], stripe t is cell cell_index[t] of every blob (blob_index is not read)
// pool (optional): receives, in the caller's order, the accepted cells (one commitment) or the stripes whose cells are ALL accepted.
int verify_cells_passes(Ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* blob_index,
                        const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status, CellPool* pool) {
    const CellsPassShape shape{log_cell, log_domain - log_cell, n_blobs, n_blobs && pool};
    const size_t vb = shape.value_bytes(), pb = shape.path_bytes();
    const std::string fn = n_blobs ? "verify_cells_blobs" : "verify_cells";
    FR_HIP(ctx, hipSetDevice(ctx->device));
    if (pool) {
        pool->n = 0;
        const int rc = pool->alloc(ctx, n_cells / shape.group(), vb * shape.group(), "poison(cell pool)");
        if (rc) return rc;
    }
    const size_t per_pass = cells_per_pass(shape, n_cells, ctx->tuning.test_verify_pass_bytes ? (size_t)ctx->tuning.test_verify_pass_bytes : CELLS_PASS_BYTES);
    hipStream_t s = ctx->stream;
    {
        // one plan for the call, sized by its largest pass (the first)
        const CellsPassPlan p = cells_pass_plan(shape, per_pass);
        int rc = ctx->ensure_arena(p.arena);
        if (rc) return rc;
        rc = ensure_pinned(ctx, p.pinned);
        if (rc) return rc;
        if (n_blobs) {
            memcpy(ctx->pinned, commitments, 32 * (size_t)n_blobs);
            FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_com, ctx->pinned, 32 * (size_t)n_blobs, hipMemcpyHostToDevice, s));
            FR_HIP(ctx, hipStreamSynchronize(s));  // (the first pass stages over the pinned block)
        }
    }
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    for (size_t first = 0; first < n_cells; first += per_pass) {
        const size_t np = std::min(per_pass, (size_t)n_cells - first);
        const CellsPassPlan p = cells_pass_plan(shape, np);
        uint32_t* pin_idx = reinterpret_cast<uint32_t*>(pin + p.i_idx);
        uint32_t* pin_bidx = reinterpret_cast<uint32_t*>(pin + p.i_bidx);
        if (shape.stripes) {
            for (size_t j = 0; j < np; j++) pin_idx[j] = cell_index[(first + j) / n_blobs], pin_bidx[j] = (uint32_t)((first + j) % n_blobs);
        } else {
            memcpy(pin_idx, cell_index + first, 4 * np);
            if (n_blobs) memcpy(pin_bidx, blob_index + first, 4 * np);
        }
        memcpy(pin + p.i_val, reinterpret_cast<const uint8_t*>(values) + vb * first, vb * np);
        for (size_t j = 0; j < np; j++)  // the paths transposed to level-major: the walk's lanes read neighbouring hashes
            for (uint32_t lv = 0; lv < shape.depth; lv++) memcpy(pin + p.i_path + 32 * (lv * np + j), paths + pb * (first + j) + 32 * (size_t)lv, 32);
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_in, pin, p.in_bytes, hipMemcpyHostToDevice, s));
        k::CellsVerifyArgs va;
        va.values = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_val);
        va.paths = reinterpret_cast<const uint4*>(ctx->arena + p.a_in + p.i_path);
        va.idx = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_idx);
        va.roots = reinterpret_cast<uint32_t*>(ctx->arena + p.a_roots);
        va.bad = reinterpret_cast<uint32_t*>(ctx->arena + p.a_bad);
        va.status = reinterpret_cast<uint32_t*>(ctx->arena + p.a_res);
        va.n = log_domain;
        va.log_cell = log_cell;
        va.n_cells = (uint32_t)np;
        FR_HIP(ctx, hipMemsetAsync(ctx->arena + p.a_res, 0xFF, p.res_bytes, s));  // (a word the kernels did not write is neither 0 nor 1)
        if (n_blobs) {
            memset(va.commitment, 0, 32);  // (not read: the walk takes the cell's commitment from the table)
            k::cells_verify_blobs(ctx->launch(), va, reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_bidx),
                                  reinterpret_cast<const uint32_t*>(ctx->arena + p.a_com));
        } else {
            memcpy(va.commitment, commitments, 32);
            k::cells_verify(ctx->launch(), va);
        }
        if (shape.stripes) k::cells_stripe_accept(ctx->launch(), va.status, (uint32_t)p.n_stripes, n_blobs, va.status + cells_al(4 * np) / 4);
        FR_HIP(ctx, hipGetLastError());
        const uint32_t* res = reinterpret_cast<const uint32_t*>(pin + p.p_res);
        FR_HIP(ctx, hipMemcpyAsync(pin + p.p_res, ctx->arena + p.a_res, p.res_bytes, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        for (size_t j = 0; j < np; j++) {
            if (res[j] > 1) return ctx->fail(FRIEDA_ERR_INVARIANT, fn + ": the kernel left no status");
            out_status[first + j] = res[j] ? FRIEDA_CELL_ACCEPTED : FRIEDA_CELL_REJECTED;
        }
        if (!pool) continue;
        // what numbers the pool entries: the status words, or the accept words of the stripes
        const uint32_t* mark = shape.stripes ? res + cells_al(4 * np) / 4 : res;
        uint32_t* tab = reinterpret_cast<uint32_t*>(pin + p.p_tab);
        uint32_t n_rows = 0;
        for (size_t t = 0; t < p.n_rows; t++) {
            if (mark[t] > 1) return ctx->fail(FRIEDA_ERR_INVARIANT, fn + ": the kernel left no stripe status");
            if (mark[t]) {
                tab[2 * n_rows] = (uint32_t)t, tab[2 * n_rows + 1] = (uint32_t)pool->n++;
                n_rows++;
            }
        }
        if (n_rows) {
            const uint32_t* d_tab = reinterpret_cast<const uint32_t*>(ctx->arena + p.a_tab);
            FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_tab, tab, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            if (shape.stripes)
                k::cells_stripe_gather(ctx->launch(), d_tab, n_rows, va.values, va.idx, n_blobs, n_blobs, log_cell, pool->d_idx(), pool->d_val());
            else
                k::cells_gather(ctx->launch(), d_tab, n_rows, va.values, va.idx, log_cell, pool->d_idx(), pool->d_val());
            FR_HIP(ctx, hipGetLastError());
            FR_HIP(ctx, hipStreamSynchronize(s));  // (the table sits in the pinned block the next pass overwrites: wait for the copy)
        }
    }
    return FRIEDA_OK;
}

// Provider: cell i is cell cell_index[i] of encs[blob_index[i]] — or, blob_index null, of encs[0]: then the indices alone are staged and
// the single-blob kernels run.  One upload (indices, and with blob numbers those and a table row per blob: evaluation, tree, skip
// threshold), the launches, one download (values | paths), one synchronisation.
int open_cells(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, uint32_t log_cell, const uint32_t* blob_index, const uint32_t* cell_index,
               uint32_t n_cells, uint32_t* out_values, uint8_t* out_paths) {
    const uint32_t n = encs[0]->n;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ib = 4 * (size_t)n_cells, tb = sizeof(k::CellsBlobRow) * (size_t)n_blobs;
    const size_t vb = ((size_t)16 << log_cell) * n_cells, pb = 32 * (size_t)(n - log_cell) * n_cells;
    const size_t i_bidx = cells_al(ib), i_tab = i_bidx + cells_al(ib), in_bytes = blob_index ? i_tab + cells_al(tb) : cells_al(ib);
    ArenaPlan ap;
    const size_t a_in = ap.take(in_bytes), a_out = ap.take(cells_al(vb) + pb);
    int rc = ctx->ensure_arena(ap.off);
    if (rc) return rc;
    rc = ensure_pinned(ctx, in_bytes + cells_al(vb) + pb);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    memcpy(pin, cell_index, ib);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(ctx->arena + a_out);
    uint4* d_paths = reinterpret_cast<uint4*>(ctx->arena + a_out + cells_al(vb));
    const uint32_t* d_idx = reinterpret_cast<const uint32_t*>(ctx->arena + a_in);
    if (blob_index) {
        memcpy(pin + i_bidx, blob_index, ib);
        k::CellsBlobRow* rows = reinterpret_cast<k::CellsBlobRow*>(pin + i_tab);
        for (uint32_t b = 0; b < n_blobs; b++) rows[b] = k::CellsBlobRow{encs[b]->eval(), encs[b]->tree(), encs[b]->skip_log, 0};
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, in_bytes, hipMemcpyHostToDevice, s));
        k::cells_open_blobs(ctx->launch(), k::CellsOpenBlobsArgs{reinterpret_cast<const k::CellsBlobRow*>(ctx->arena + a_in + i_tab),
                                                                 reinterpret_cast<const uint32_t*>(ctx->arena + a_in + i_bidx), d_idx, n, log_cell, n_cells,
                                                                 d_out, d_paths});
    } else {
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, ib, hipMemcpyHostToDevice, s));
        k::cells_open(ctx->launch(), k::CellsOpenArgs{encs[0]->eval(), encs[0]->tree(), n, log_cell, encs[0]->skip_log, n_cells, d_idx, d_out, d_paths});
    }
    FR_HIP(ctx, hipGetLastError());
    FR_HIP(ctx, hipMemcpyAsync(pin + in_bytes, ctx->arena + a_out, cells_al(vb) + pb, hipMemcpyDeviceToHost, s));
    FR_HIP(ctx, hipStreamSynchronize(s));
    memcpy(out_values, pin + in_bytes, vb);
    if (pb) memcpy(out_paths, pin + in_bytes + cells_al(vb), pb);
    return FRIEDA_OK;
}

constexpr uint32_t CELLS_MAX_BLOBS = 65536, STRIPES_MAX_BLOBS = 256;  // (the point reconstruction takes at most 1024 columns)
// the argument rule the three (blob, cell) pair calls share; null when it holds
const char* cells_blobs_args_error(uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* blob_index, const uint32_t* cell_index,
                                   uint32_t n_cells) {
    if (n_blobs == 0 || n_blobs > CELLS_MAX_BLOBS) return "n_blobs out of range";
    for (uint32_t i = 0; i < n_cells; i++)
        if (blob_index[i] >= n_blobs) return "blob index out of range";
    return cells_args_error(log_domain, log_cell, cell_index, n_cells);
}

}  // namespace

// The tail of the block rebuilds (opened stripes, stripe bundles): one point reconstruction over 4 * n_blobs columns, commit_batch over
// the rebuilt bytes, every root against its commitment.  *n_distinct: the distinct stripes of the pool (on an error too).
int rebuild_blobs_from_stripes(frieda_ctx* ctx, const CellPool& pool, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                               uint32_t log_cell, uint8_t* out_bytes, uint32_t* n_distinct) {
    const uint32_t L = codec_shape(len).log_size, n = L + log_blowup_factor;
    // the rebuilt bytes stay on the device for the commitment check: blob b at b * stride
    const size_t stride = std::max<size_t>(256, (len + 255) & ~(size_t)255);
    std::vector<uint8_t> roots(32 * (size_t)n_blobs), bytes(len * n_blobs);
    DevBuf out;
    int rc = out.alloc(&ctx->c, stride * n_blobs, "poison(rebuilt bytes)");
    if (rc != FRIEDA_OK) return rc;
    uint8_t* d_out = static_cast<uint8_t*>(out.p);
    rc = reconstruct_pooled(ctx, pool.d_val(), pool.d_idx(), (uint32_t)pool.n, n_blobs, log_cell, L, n, len, d_out, stride, n_distinct);
    if (rc == FRIEDA_OK) rc = commit_batch(&ctx->c, d_out, stride, len, n_blobs, true, log_blowup_factor, roots.data());
    if (rc == FRIEDA_OK && len && hipMemcpy2D(bytes.data(), len, d_out, stride, len, n_blobs, hipMemcpyDeviceToHost) != hipSuccess)
        rc = ctx->c.hip_fail(hipGetLastError(), "hipMemcpy2D(rebuilt bytes)");
    (void)hipStreamSynchronize(ctx->c.stream);  // (before the buffer goes, on the error paths too)
    out.release();
    if (rc != FRIEDA_OK) return rc;
    return rebuilt_accept(&ctx->c, roots.data(), commitments, n_blobs, nullptr, bytes, out_bytes);
}

int rebuild_shape(frieda_ctx* ctx, const char* fn, uint32_t log_blowup_factor, size_t len, uint32_t* L, uint32_t* n) {
    if (log_blowup_factor > FRIEDA_MAX_LOG_DOMAIN || len > ((size_t)1 << 40)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "shape out of range");
    *L = codec_shape(len).log_size, *n = *L + log_blowup_factor;
    if (*L < 1 || *n < 2 || *n + 1 > FRIEDA_MAX_LOG_DOMAIN) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "shape out of range");
    return FRIEDA_OK;
}

int rebuild_from_pool(frieda_ctx* ctx, const CellPool& pool, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                      uint32_t log_cell, const char* noun, uint8_t* out_bytes, frieda_encoded** out_encs, size_t* n_used) {
    const uint32_t L = codec_shape(len).log_size, n = L + log_blowup_factor;
    // what the point reconstruction needs: one cell more than the coefficients fill, or two points more
    const size_t need = log_cell ? (((size_t)1 << L) >> log_cell) + 1 : ((size_t)1 << L) + 2;
    uint32_t nd = 0;
    auto counted = [&](int rc) {  // *n_used on an error too; the reconstruction's "too few" in the caller's words
        *n_used = nd;
        if (rc != FRIEDA_ERR_ARG || nd >= need) return rc;
        return ctx->c.fail(FRIEDA_ERR_ARG, std::to_string(nd) + " " + noun + ", " + std::to_string(need) + " needed");
    };
    if (pool.n == 0) return counted(FRIEDA_ERR_ARG);
    // the single-blob forms name no blob in their mismatch; the block forms name the blob (rebuilt_accept)
    const char* const mismatch = n_blobs ? nullptr : "the rebuilt blob does not commit to the commitment (wrong len?)";
    if (out_encs)
        return counted(rebuild_encoded_from_pool(ctx, pool, commitments, std::max(n_blobs, 1u), log_blowup_factor, len, log_cell, mismatch, out_bytes, &nd, out_encs));
    if (n_blobs) return counted(rebuild_blobs_from_stripes(ctx, pool, commitments, n_blobs, log_blowup_factor, len, log_cell, out_bytes, &nd));
    return rebuild_blob(ctx, len, log_blowup_factor, commitments, mismatch, out_bytes, [&](uint8_t* d_out) {
        return counted(reconstruct_pooled(ctx, pool.d_val(), pool.d_idx(), (uint32_t)pool.n, 1, log_cell, L, n, len, d_out, 0, &nd));
    });
}

const char* cells_args_error(uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells) {
    if (log_domain > FRIEDA_MAX_LOG_DOMAIN) return "log_domain out of range";
    if (log_cell > log_domain || log_cell > FRIEDA_MAX_LOG_OPEN_CELL) return "log_cell out of range";
    const uint32_t bits = log_domain - log_cell;
    for (uint32_t i = 0; i < n_cells; i++)
        if (((uint64_t)cell_index[i] >> bits) != 0) return "cell index out of range";
    return nullptr;
}

}  // namespace frieda

using namespace frieda;

extern "C" {
int frieda_open_cells(frieda_ctx* ctx, const frieda_encoded* enc, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells,
                      uint32_t* out_values, uint8_t* out_paths) {
    if (!ctx || !enc) return FRIEDA_ERR_ARG;
    if (n_cells == 0) return FRIEDA_OK;
    if (!cell_index || !out_values || (!out_paths && log_cell != enc->e.n)) return FRIEDA_ERR_ARG;
    if (const char* bad = cells_args_error(enc->e.n, log_cell, cell_index, n_cells)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string("open_cells: ") + bad);
    FR_GUARD_BEGIN
    FR_NO_JOB(&ctx->c);
    if (ctx->c.device != enc->e.device) return ctx->c.fail(FRIEDA_ERR_ARG, "open_cells: the context is not on the encoded blob's device");
    const Encoded* const one = &enc->e;
    return open_cells(&ctx->c, &one, 1, log_cell, nullptr, cell_index, n_cells, out_values, out_paths);
    FR_GUARD_END(ctx)
}

int frieda_verify_cells(const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells,
                        const uint32_t* values, const uint8_t* paths, uint8_t* out_status) {
    if (n_cells == 0) return FRIEDA_OK;
    if (!commitment || !cell_index || !values || !out_status) return FRIEDA_ERR_ARG;
    if (cells_args_error(log_domain, log_cell, cell_index, n_cells) || (!paths && log_cell != log_domain)) return FRIEDA_ERR_ARG;
    try {
        verify_cells_host(commitment, log_domain, log_cell, nullptr, cell_index, n_cells, values, paths, out_status);
    } catch (const std::bad_alloc&) {
        return FRIEDA_ERR_NOMEM;
    }
    return FRIEDA_OK;
}

int frieda_verify_cells_many(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                             uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (n_cells == 0) return FRIEDA_OK;
    if (!commitment || !cell_index || !values || !out_status || (!paths && log_cell != log_domain)) return FRIEDA_ERR_ARG;
    if (const char* bad = cells_args_error(log_domain, log_cell, cell_index, n_cells)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string("verify_cells_many: ") + bad);
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    return verify_cells_passes(&ctx->c, commitment, 0, log_domain, log_cell, nullptr, cell_index, n_cells, values, paths, out_status, nullptr);
    FR_GUARD_END(ctx)
}

namespace {
// frieda_reconstruct_from_opened_cells (out_enc == nullptr: its tail rebuild_blob, out_bytes required) and
// frieda_rebuild_encoded_from_opened_cells (the tail that returns the handle; out_bytes optional)
int reconstruct_from_opened_cells(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                  const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_bytes,
                                  uint8_t* out_status, size_t* n_cells_used, frieda_encoded** out_enc) {
    if (!ctx || !commitment || !n_cells_used || (len && !out_bytes && !out_enc) || (n_cells && (!cell_index || !values || !out_status))) return FRIEDA_ERR_ARG;
    *n_cells_used = 0;
    const char* const fn = out_enc ? "rebuild_encoded_from_opened_cells: " : "reconstruct_from_opened_cells: ";
    uint32_t L, n;
    if (const int rc = rebuild_shape(ctx, fn, log_blowup_factor, len, &L, &n)) return rc;
    if (const char* bad = cells_args_error(n, log_cell, cell_index, n_cells)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (n_cells && !paths && log_cell != n) return FRIEDA_ERR_ARG;
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    CellPool pool;
    if (n_cells)
        if (const int rc = verify_cells_passes(&ctx->c, commitment, 0, n, log_cell, nullptr, cell_index, n_cells, values, paths, out_status, &pool)) return rc;
    return rebuild_from_pool(ctx, pool, commitment, 0, log_blowup_factor, len, log_cell, "distinct accepted cells", out_bytes, out_enc, n_cells_used);
    FR_GUARD_END(ctx)
}
}  // namespace

int frieda_reconstruct_from_opened_cells(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                         const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths,
                                         uint8_t* out_bytes, uint8_t* out_status, size_t* n_cells_used) {
    return reconstruct_from_opened_cells(ctx, commitment, log_blowup_factor, len, log_cell, cell_index, n_cells, values, paths, out_bytes, out_status,
                                         n_cells_used, nullptr);
}
int frieda_rebuild_encoded_from_opened_cells(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                             const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths,
                                             uint8_t* out_bytes, uint8_t* out_status, size_t* n_cells_used, frieda_encoded** out_enc) {
    if (!out_enc) return FRIEDA_ERR_ARG;
    *out_enc = nullptr;
    return reconstruct_from_opened_cells(ctx, commitment, log_blowup_factor, len, log_cell, cell_index, n_cells, values, paths, out_bytes, out_status,
                                         n_cells_used, out_enc);
}

// ---- the cells of many blobs of one shape in one call ----
int frieda_open_cells_blobs(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, uint32_t log_cell, const uint32_t* blob_index,
                            const uint32_t* cell_index, uint32_t n_cells, uint32_t* out_values, uint8_t* out_paths) {
    if (!ctx || !encs || n_blobs == 0 || n_blobs > CELLS_MAX_BLOBS) return FRIEDA_ERR_ARG;
    for (uint32_t b = 0; b < n_blobs; b++)
        if (!encs[b]) return FRIEDA_ERR_ARG;
    FR_GUARD_BEGIN
    const uint32_t n = encs[0]->e.n;
    std::vector<const Encoded*> blobs(n_blobs);
    for (uint32_t b = 0; b < n_blobs; b++) {
        if (encs[b]->e.n != n) return ctx->c.fail(FRIEDA_ERR_ARG, "open_cells_blobs: the blobs of a call must have one log_domain");
        if (encs[b]->e.device != ctx->c.device) return ctx->c.fail(FRIEDA_ERR_ARG, "open_cells_blobs: the context is not on the encoded blobs' device");
        blobs[b] = &encs[b]->e;
    }
    if (n_cells == 0) return FRIEDA_OK;
    if (!blob_index || !cell_index || !out_values || (!out_paths && log_cell != n)) return FRIEDA_ERR_ARG;
    if (const char* bad = cells_blobs_args_error(n_blobs, n, log_cell, blob_index, cell_index, n_cells))
        return ctx->c.fail(FRIEDA_ERR_ARG, std::string("open_cells_blobs: ") + bad);
    FR_NO_JOB(&ctx->c);
    return open_cells(&ctx->c, blobs.data(), n_blobs, log_cell, blob_index, cell_index, n_cells, out_values, out_paths);
    FR_GUARD_END(ctx)
}

int frieda_verify_cells_blobs(const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* blob_index,
                              const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status) {
    if (n_cells == 0) return FRIEDA_OK;
    if (!commitments || !blob_index || !cell_index || !values || !out_status) return FRIEDA_ERR_ARG;
    if (cells_blobs_args_error(n_blobs, log_domain, log_cell, blob_index, cell_index, n_cells) || (!paths && log_cell != log_domain)) return FRIEDA_ERR_ARG;
    try {
        verify_cells_host(commitments, log_domain, log_cell, blob_index, cell_index, n_cells, values, paths, out_status);
    } catch (const std::bad_alloc&) {
        return FRIEDA_ERR_NOMEM;
    }
    return FRIEDA_OK;
}

int frieda_verify_cells_blobs_many(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell,
                                   const uint32_t* blob_index, const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths,
                                   uint8_t* out_status) {
    if (!ctx) return FRIEDA_ERR_ARG;
    if (n_cells == 0) return FRIEDA_OK;
    if (!commitments || !blob_index || !cell_index || !values || !out_status || (!paths && log_cell != log_domain)) return FRIEDA_ERR_ARG;
    if (const char* bad = cells_blobs_args_error(n_blobs, log_domain, log_cell, blob_index, cell_index, n_cells))
        return ctx->c.fail(FRIEDA_ERR_ARG, std::string("verify_cells_blobs_many: ") + bad);
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    return verify_cells_passes(&ctx->c, commitments, n_blobs, log_domain, log_cell, blob_index, cell_index, n_cells, values, paths, out_status, nullptr);
    FR_GUARD_END(ctx)
}

namespace {
// frieda_reconstruct_blobs_from_opened_stripes (out_encs == nullptr: its tail rebuild_blobs_from_stripes) and
// frieda_rebuild_encoded_blobs_from_opened_stripes (out_encs[n_blobs], all NULL on entry; out_bytes optional)
int reconstruct_blobs_from_opened_stripes(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                                          uint32_t log_cell, const uint32_t* stripe_index, uint32_t n_stripes, const uint32_t* values, const uint8_t* paths,
                                          uint8_t* out_bytes, uint8_t* out_status, size_t* n_stripes_used, frieda_encoded** out_encs) {
    if (!ctx || !commitments || !n_stripes_used || (len && !out_bytes && !out_encs) || (n_stripes && (!stripe_index || !values || !out_status))) return FRIEDA_ERR_ARG;
    *n_stripes_used = 0;
    const char* const fn = out_encs ? "rebuild_encoded_blobs_from_opened_stripes: " : "reconstruct_blobs_from_opened_stripes: ";
    if (n_blobs == 0 || n_blobs > STRIPES_MAX_BLOBS) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "n_blobs out of range (1 .. 256)");
    uint32_t L, n;
    if (const int rc = rebuild_shape(ctx, fn, log_blowup_factor, len, &L, &n)) return rc;
    if (const char* bad = cells_args_error(n, log_cell, stripe_index, n_stripes)) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + bad);
    if (n_stripes && !paths && log_cell != n) return FRIEDA_ERR_ARG;
    // the staged values are the point reconstruction's sample buffer: at most 2^32 words (its positions are 32-bit)
    if ((uint64_t)n_stripes * n_blobs > (0x100000000ull >> (log_cell + 2))) return ctx->c.fail(FRIEDA_ERR_ARG, std::string(fn) + "more than 2^32 value words");
    FR_NO_JOB(&ctx->c);
    FR_GUARD_BEGIN
    CellPool pool;
    if (n_stripes)
        if (const int rc = verify_cells_passes(&ctx->c, commitments, n_blobs, n, log_cell, nullptr, stripe_index, n_stripes * n_blobs, values, paths, out_status,
                                               &pool))
            return rc;
    return rebuild_from_pool(ctx, pool, commitments, n_blobs, log_blowup_factor, len, log_cell, "distinct fully accepted stripes", out_bytes, out_encs,
                             n_stripes_used);
    FR_GUARD_END(ctx)
}
}  // namespace

int frieda_reconstruct_blobs_from_opened_stripes(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                                                 uint32_t log_cell, const uint32_t* stripe_index, uint32_t n_stripes, const uint32_t* values,
                                                 const uint8_t* paths, uint8_t* out_bytes, uint8_t* out_status, size_t* n_stripes_used) {
    return reconstruct_blobs_from_opened_stripes(ctx, commitments, n_blobs, log_blowup_factor, len, log_cell, stripe_index, n_stripes, values, paths, out_bytes,
                                                 out_status, n_stripes_used, nullptr);
}
int frieda_rebuild_encoded_blobs_from_opened_stripes(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor,
                                                     size_t len, uint32_t log_cell, const uint32_t* stripe_index, uint32_t n_stripes,
                                                     const uint32_t* values, const uint8_t* paths, uint8_t* out_bytes, uint8_t* out_status,
                                                     size_t* n_stripes_used, frieda_encoded** out_encs) {
    if (!out_encs) return FRIEDA_ERR_ARG;
    if (n_blobs >= 1 && n_blobs <= STRIPES_MAX_BLOBS) memset(out_encs, 0, sizeof(frieda_encoded*) * n_blobs);
    return reconstruct_blobs_from_opened_stripes(ctx, commitments, n_blobs, log_blowup_factor, len, log_cell, stripe_index, n_stripes, values, paths, out_bytes,
                                                 out_status, n_stripes_used, out_encs);
}

}  // extern "C"
