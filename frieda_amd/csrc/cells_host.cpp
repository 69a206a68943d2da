// cells_host.cpp — authenticated cells: the host side of cells.hip (frieda_open_cells, frieda_verify_cells, frieda_verify_cells_many,
// frieda_reconstruct_from_opened_cells, and their forms over the blobs of a block: frieda_open_cells_blobs, frieda_verify_cells_blobs,
// frieda_verify_cells_blobs_many, frieda_reconstruct_blobs_from_opened_stripes; the exports are in capi.cpp).
//
// A cell with its path is a self-contained message (values, index, path): every cell carries its own n - log_cell siblings, nothing is
// shared between the cells of a call, and a cell's status never depends on the others.  The host verifier and the kernels hash the
// same way (blake2s.h): a leaf is the four column words of one position, a node its two children.
//
// The device verifier stages a call through the context's pinned block and arena in passes of bounded size (PASS_BYTES, or the test
// hook Tuning::test_verify_pass_bytes, as verify_many.cpp): indices, values as given (cell-major), and the paths transposed to
// level-major so that the path walk's lanes read neighbouring hashes.  With a pool, the accepted cells of a pass are copied from the
// staged values into the call's CellPool by a gather launch before the next pass overwrites them.
//
// Blobs of a block: cell i of a call is cell cell_index[i] of blob blob_index[i]; the blob numbers are staged beside the indices, the
// commitments go to the device once per call, and the provider uploads a table row per blob (evaluation, tree, skip threshold) with the
// indices.  A stripe is cell j of every blob: the stripe call cuts its passes at stripe boundaries, and a stripe whose cells are all
// accepted is gathered whole into the pool — the reconstruction's cell layout at 4 * n_blobs columns.
#include <string.h>

#include <algorithm>

#include "host.h"

namespace frieda {

namespace {

constexpr size_t PASS_BYTES = (size_t)32 << 20;

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

}  // namespace

CellPool::~CellPool() {
    if (d) (void)hipFree(d);
}

const char* cells_args_error(uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells) {
    if (log_domain > FRIEDA_MAX_LOG_DOMAIN) return "log_domain out of range";
    if (log_cell > log_domain || log_cell > FRIEDA_MAX_LOG_OPEN_CELL) return "log_cell out of range";
    const uint32_t bits = log_domain - log_cell;
    for (uint32_t i = 0; i < n_cells; i++)
        if (((uint64_t)cell_index[i] >> bits) != 0) return "cell index out of range";
    return nullptr;
}

void verify_cells_host(const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells,
                       const uint32_t* values, const uint8_t* paths, uint8_t* out_status) {
    uint32_t want[8];
    memcpy(want, commitment, 32);
    const size_t vw = (size_t)4 << log_cell, pb = 32 * (size_t)(log_domain - log_cell);
    std::vector<uint32_t> lvl;
    for (uint32_t i = 0; i < n_cells; i++)
        out_status[i] = host_cell_ok(want, log_domain, log_cell, cell_index[i], values + i * vw, paths + i * pb, lvl) ? FRIEDA_CELL_ACCEPTED : FRIEDA_CELL_REJECTED;
}

int verify_cells_device(Ctx* ctx, const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells,
                        const uint32_t* values, const uint8_t* paths, uint8_t* out_status, CellPool* pool) {
    const uint32_t depth = log_domain - log_cell;
    const size_t vb = (size_t)16 << log_cell, pb = 32 * (size_t)depth;  // bytes of a cell's values / path
    FR_HIP(ctx, hipSetDevice(ctx->device));
    if (pool) {
        pool->n = 0;
        pool->cap = n_cells;
        pool->log_cell = log_cell;
        void* d = nullptr;
        const hipError_t e = hipMalloc(&d, ((4 * pool->cap + 255) & ~(size_t)255) + vb * pool->cap);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
            return FRIEDA_ERR_NOMEM;
        }
        pool->d = static_cast<uint8_t*>(d);
        FR_HIP(ctx, ctx->poison_fresh(d, ((4 * pool->cap + 255) & ~(size_t)255) + vb * pool->cap));
    }
    const size_t pass_bytes = ctx->tuning.test_verify_pass_bytes ? (size_t)ctx->tuning.test_verify_pass_bytes : PASS_BYTES;
    const size_t per_pass = std::max<size_t>(1, pass_bytes / (4 + vb + pb));
    hipStream_t s = ctx->stream;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    for (size_t first = 0; first < n_cells; first += per_pass) {
        const size_t np = std::min(per_pass, (size_t)n_cells - first);
        // staged image: indices | values (cell-major, as given) | paths (level-major); then the status words and the gather table
        const size_t i_idx = 0, i_val = al(4 * np), i_path = i_val + al(vb * np), in_bytes = i_path + al(pb * np);
        ArenaPlan ap;
        const size_t a_in = ap.take(in_bytes), a_roots = ap.take(32 * np), a_bad = ap.take(4 * np), a_status = ap.take(4 * np), a_tab = ap.take(8 * np);
        int rc = ctx->ensure_arena(ap.off);
        if (rc) return rc;
        rc = ensure_pinned(ctx, in_bytes + al(4 * np) + 8 * np);
        if (rc) return rc;
        uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
        memcpy(pin + i_idx, cell_index + first, 4 * np);
        memcpy(pin + i_val, reinterpret_cast<const uint8_t*>(values) + vb * first, vb * np);
        for (size_t j = 0; j < np; j++)
            for (uint32_t lv = 0; lv < depth; lv++) memcpy(pin + i_path + 32 * (lv * np + j), paths + pb * (first + j) + 32 * (size_t)lv, 32);
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, in_bytes, hipMemcpyHostToDevice, s));
        k::CellsVerifyArgs va;
        va.values = reinterpret_cast<const uint32_t*>(ctx->arena + a_in + i_val);
        va.paths = reinterpret_cast<const uint4*>(ctx->arena + a_in + i_path);
        va.idx = reinterpret_cast<const uint32_t*>(ctx->arena + a_in + i_idx);
        va.roots = reinterpret_cast<uint32_t*>(ctx->arena + a_roots);
        va.bad = reinterpret_cast<uint32_t*>(ctx->arena + a_bad);
        va.status = reinterpret_cast<uint32_t*>(ctx->arena + a_status);
        va.n = log_domain;
        va.log_cell = log_cell;
        va.n_cells = (uint32_t)np;
        memcpy(va.commitment, commitment, 32);
        FR_HIP(ctx, hipMemsetAsync(ctx->arena + a_status, 0xFF, 4 * np, s));  // (a word the kernel did not write is neither 0 nor 1)
        k::cells_verify(ctx->launch(), va);
        FR_HIP(ctx, hipGetLastError());
        uint32_t* res = reinterpret_cast<uint32_t*>(pin + in_bytes);
        FR_HIP(ctx, hipMemcpyAsync(res, ctx->arena + a_status, 4 * np, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        uint32_t* tab = reinterpret_cast<uint32_t*>(pin + in_bytes + al(4 * np));
        uint32_t n_rows = 0;
        for (size_t j = 0; j < np; j++) {
            if (res[j] > 1) return ctx->fail(FRIEDA_ERR_INVARIANT, "verify_cells: the kernel left no status");
            out_status[first + j] = res[j] ? FRIEDA_CELL_ACCEPTED : FRIEDA_CELL_REJECTED;
            if (pool && res[j]) {
                tab[2 * n_rows] = (uint32_t)j, tab[2 * n_rows + 1] = (uint32_t)pool->n++;
                n_rows++;
            }
        }
        if (n_rows) {
            // (the table sits in the pinned block the next pass overwrites: wait for the copy)
            FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_tab, tab, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            k::cells_gather(ctx->launch(), reinterpret_cast<const uint32_t*>(ctx->arena + a_tab), n_rows, va.values, va.idx, log_cell, pool->d_idx(), pool->d_val());
            FR_HIP(ctx, hipGetLastError());
            FR_HIP(ctx, hipStreamSynchronize(s));
        }
    }
    return FRIEDA_OK;
}

int open_cells(Ctx* ctx, const Encoded& enc, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells, uint32_t* out_values, uint8_t* out_paths) {
    FR_NO_JOB(ctx);
    if (ctx->device != enc.device) return ctx->fail(FRIEDA_ERR_ARG, "open_cells: the context is not on the encoded blob's device");
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ib = 4 * (size_t)n_cells, vb = ((size_t)16 << log_cell) * n_cells, pb = 32 * (size_t)(enc.n - log_cell) * n_cells;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    ArenaPlan ap;
    const size_t a_idx = ap.take(ib), a_out = ap.take(al(vb) + pb);  // values | paths: one download
    int rc = ctx->ensure_arena(ap.off);
    if (rc) return rc;
    rc = ensure_pinned(ctx, al(ib) + al(vb) + pb);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    memcpy(pin, cell_index, ib);
    FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_idx, pin, ib, hipMemcpyHostToDevice, s));
    k::CellsOpenArgs oa;
    oa.eval = enc.eval();
    oa.tree = enc.tree();
    oa.n = enc.n;
    oa.log_cell = log_cell;
    oa.skip_log = enc.skip_log;
    oa.n_cells = n_cells;
    oa.idx = reinterpret_cast<const uint32_t*>(ctx->arena + a_idx);
    oa.out_values = reinterpret_cast<uint32_t*>(ctx->arena + a_out);
    oa.out_paths = reinterpret_cast<uint4*>(ctx->arena + a_out + al(vb));
    k::cells_open(ctx->launch(), oa);
    FR_HIP(ctx, hipGetLastError());
    FR_HIP(ctx, hipMemcpyAsync(pin + al(ib), ctx->arena + a_out, al(vb) + pb, hipMemcpyDeviceToHost, s));
    FR_HIP(ctx, hipStreamSynchronize(s));
    memcpy(out_values, pin + al(ib), vb);
    if (pb) memcpy(out_paths, pin + al(ib) + al(vb), pb);
    return FRIEDA_OK;
}

void verify_cells_blobs_host(const uint8_t* commitments, uint32_t log_domain, uint32_t log_cell, const uint32_t* blob_index, const uint32_t* cell_index,
                             uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status) {
    const size_t vw = (size_t)4 << log_cell, pb = 32 * (size_t)(log_domain - log_cell);
    std::vector<uint32_t> lvl;
    for (uint32_t i = 0; i < n_cells; i++) {
        uint32_t want[8];
        memcpy(want, commitments + 32 * (size_t)blob_index[i], 32);
        out_status[i] = host_cell_ok(want, log_domain, log_cell, cell_index[i], values + i * vw, paths + i * pb, lvl) ? FRIEDA_CELL_ACCEPTED : FRIEDA_CELL_REJECTED;
    }
}

int verify_cells_blobs_device(Ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* blob_index,
                              const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status,
                              CellPool* stripes) {
    const uint32_t depth = log_domain - log_cell;
    const size_t vb = (size_t)16 << log_cell, pb = 32 * (size_t)depth;  // bytes of a cell's values / path
    const size_t group = stripes ? n_blobs : 1;                          // cells that stay in one pass
    FR_HIP(ctx, hipSetDevice(ctx->device));
    if (stripes) {
        stripes->n = 0;
        stripes->cap = n_cells / n_blobs;
        stripes->log_cell = log_cell;
        void* d = nullptr;
        const hipError_t e = hipMalloc(&d, ((4 * stripes->cap + 255) & ~(size_t)255) + vb * n_cells);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
            return FRIEDA_ERR_NOMEM;
        }
        stripes->d = static_cast<uint8_t*>(d);
        FR_HIP(ctx, ctx->poison_fresh(d, ((4 * stripes->cap + 255) & ~(size_t)255) + vb * n_cells));
    }
    const size_t pass_bytes = ctx->tuning.test_verify_pass_bytes ? (size_t)ctx->tuning.test_verify_pass_bytes : PASS_BYTES;
    // (a stripe's cells never straddle two passes, and one stripe is always admitted)
    const size_t per_pass = std::min<size_t>(n_cells, std::max<size_t>(1, pass_bytes / (group * (8 + vb + pb))) * group);
    hipStream_t s = ctx->stream;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // One plan for the call, sized by its largest pass (the first): the commitments sit in front of it and are uploaded once.
    // staged image of a pass: indices | blob numbers | values (cell-major, as given) | paths (level-major); then the status words, the
    // accept words of its stripes and the gather table
    struct Plan {
        size_t i_idx, i_bidx, i_val, i_path, in_bytes, ns, res_bytes, a_com, a_in, a_roots, a_bad, a_res, a_tab, arena;
    };
    auto plan_for = [&](size_t np) {
        Plan p;
        p.ns = stripes ? np / n_blobs : 0;
        p.i_idx = 0, p.i_bidx = al(4 * np), p.i_val = p.i_bidx + al(4 * np), p.i_path = p.i_val + al(vb * np), p.in_bytes = p.i_path + al(pb * np);
        p.res_bytes = al(4 * np) + 4 * p.ns;
        ArenaPlan ap;
        p.a_com = ap.take(32 * (size_t)n_blobs), p.a_in = ap.take(p.in_bytes), p.a_roots = ap.take(32 * np), p.a_bad = ap.take(4 * np);
        p.a_res = ap.take(p.res_bytes), p.a_tab = ap.take(8 * p.ns);
        p.arena = ap.off;
        return p;
    };
    {
        const Plan p = plan_for(per_pass);
        int rc = ctx->ensure_arena(p.arena);
        if (rc) return rc;
        rc = ensure_pinned(ctx, std::max(al(32 * (size_t)n_blobs), p.in_bytes + al(p.res_bytes) + 8 * p.ns));
        if (rc) return rc;
        memcpy(ctx->pinned, commitments, 32 * (size_t)n_blobs);
        FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_com, ctx->pinned, 32 * (size_t)n_blobs, hipMemcpyHostToDevice, s));
        FR_HIP(ctx, hipStreamSynchronize(s));  // (the first pass stages over the pinned block)
    }
    for (size_t first = 0; first < n_cells; first += per_pass) {
        const size_t np = std::min(per_pass, (size_t)n_cells - first);
        const Plan p = plan_for(np);
        uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
        uint32_t* pin_idx = reinterpret_cast<uint32_t*>(pin + p.i_idx);
        uint32_t* pin_bidx = reinterpret_cast<uint32_t*>(pin + p.i_bidx);
        if (stripes) {
            for (size_t j = 0; j < np; j++) pin_idx[j] = cell_index[(first + j) / n_blobs], pin_bidx[j] = (uint32_t)((first + j) % n_blobs);
        } else {
            memcpy(pin_idx, cell_index + first, 4 * np);
            memcpy(pin_bidx, blob_index + first, 4 * np);
        }
        memcpy(pin + p.i_val, reinterpret_cast<const uint8_t*>(values) + vb * first, vb * np);
        for (size_t j = 0; j < np; j++)
            for (uint32_t lv = 0; lv < depth; lv++) memcpy(pin + p.i_path + 32 * (lv * np + j), paths + pb * (first + j) + 32 * (size_t)lv, 32);
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
        memset(va.commitment, 0, 32);  // (not read: the walk takes the cell's commitment from the table)
        uint32_t* d_accept = reinterpret_cast<uint32_t*>(ctx->arena + p.a_res + al(4 * np));
        FR_HIP(ctx, hipMemsetAsync(ctx->arena + p.a_res, 0xFF, p.res_bytes, s));  // (a word the kernels did not write is neither 0 nor 1)
        k::cells_verify_blobs(ctx->launch(), va, reinterpret_cast<const uint32_t*>(ctx->arena + p.a_in + p.i_bidx),
                              reinterpret_cast<const uint32_t*>(ctx->arena + p.a_com));
        if (stripes) k::cells_stripe_accept(ctx->launch(), va.status, (uint32_t)p.ns, n_blobs, d_accept);
        FR_HIP(ctx, hipGetLastError());
        uint32_t* res = reinterpret_cast<uint32_t*>(pin + p.in_bytes);
        FR_HIP(ctx, hipMemcpyAsync(res, ctx->arena + p.a_res, p.res_bytes, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        for (size_t j = 0; j < np; j++) {
            if (res[j] > 1) return ctx->fail(FRIEDA_ERR_INVARIANT, "verify_cells_blobs: the kernel left no status");
            out_status[first + j] = res[j] ? FRIEDA_CELL_ACCEPTED : FRIEDA_CELL_REJECTED;
        }
        if (!stripes) continue;
        // the host keeps the accept words only: they number the pool entries
        const uint32_t* acc = res + al(4 * np) / 4;
        uint32_t* tab = reinterpret_cast<uint32_t*>(pin + p.in_bytes + al(p.res_bytes));
        uint32_t n_rows = 0;
        for (size_t t = 0; t < p.ns; t++) {
            if (acc[t] > 1) return ctx->fail(FRIEDA_ERR_INVARIANT, "verify_cells_blobs: the kernel left no stripe status");
            if (acc[t]) {
                tab[2 * n_rows] = (uint32_t)t, tab[2 * n_rows + 1] = (uint32_t)stripes->n++;
                n_rows++;
            }
        }
        if (n_rows) {
            // (the table sits in the pinned block the next pass overwrites: wait for the copy)
            FR_HIP(ctx, hipMemcpyAsync(ctx->arena + p.a_tab, tab, 8 * (size_t)n_rows, hipMemcpyHostToDevice, s));
            k::cells_stripe_gather(ctx->launch(), reinterpret_cast<const uint32_t*>(ctx->arena + p.a_tab), n_rows, va.values, va.idx, n_blobs, log_cell,
                                   stripes->d_idx(), stripes->d_val());
            FR_HIP(ctx, hipGetLastError());
            FR_HIP(ctx, hipStreamSynchronize(s));
        }
    }
    return FRIEDA_OK;
}

int open_cells_blobs(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, uint32_t log_cell, const uint32_t* blob_index, const uint32_t* cell_index,
                     uint32_t n_cells, uint32_t* out_values, uint8_t* out_paths) {
    FR_NO_JOB(ctx);
    const uint32_t n = encs[0]->n;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ib = 4 * (size_t)n_cells, tb = sizeof(k::CellsBlobRow) * (size_t)n_blobs;
    const size_t vb = ((size_t)16 << log_cell) * n_cells, pb = 32 * (size_t)(n - log_cell) * n_cells;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t i_bidx = al(ib), i_tab = i_bidx + al(ib), in_bytes = i_tab + al(tb);  // indices | blob numbers | table: one upload
    ArenaPlan ap;
    const size_t a_in = ap.take(in_bytes), a_out = ap.take(al(vb) + pb);  // values | paths: one download
    int rc = ctx->ensure_arena(ap.off);
    if (rc) return rc;
    rc = ensure_pinned(ctx, in_bytes + al(vb) + pb);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint8_t* pin = static_cast<uint8_t*>(ctx->pinned);
    memcpy(pin, cell_index, ib);
    memcpy(pin + i_bidx, blob_index, ib);
    k::CellsBlobRow* rows = reinterpret_cast<k::CellsBlobRow*>(pin + i_tab);
    for (uint32_t b = 0; b < n_blobs; b++) rows[b] = k::CellsBlobRow{encs[b]->eval(), encs[b]->tree(), encs[b]->skip_log, 0};
    FR_HIP(ctx, hipMemcpyAsync(ctx->arena + a_in, pin, in_bytes, hipMemcpyHostToDevice, s));
    k::CellsOpenBlobsArgs oa;
    oa.table = reinterpret_cast<const k::CellsBlobRow*>(ctx->arena + a_in + i_tab);
    oa.bidx = reinterpret_cast<const uint32_t*>(ctx->arena + a_in + i_bidx);
    oa.idx = reinterpret_cast<const uint32_t*>(ctx->arena + a_in);
    oa.n = n;
    oa.log_cell = log_cell;
    oa.n_cells = n_cells;
    oa.out_values = reinterpret_cast<uint32_t*>(ctx->arena + a_out);
    oa.out_paths = reinterpret_cast<uint4*>(ctx->arena + a_out + al(vb));
    k::cells_open_blobs(ctx->launch(), oa);
    FR_HIP(ctx, hipGetLastError());
    FR_HIP(ctx, hipMemcpyAsync(pin + in_bytes, ctx->arena + a_out, al(vb) + pb, hipMemcpyDeviceToHost, s));
    FR_HIP(ctx, hipStreamSynchronize(s));
    memcpy(out_values, pin + in_bytes, vb);
    if (pb) memcpy(out_paths, pin + in_bytes + al(vb), pb);
    return FRIEDA_OK;
}

}  // namespace frieda
