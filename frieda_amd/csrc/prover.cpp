// prover.cpp — commit() and commit_and_generate_proof() on the device.
//
// Orchestrates the gfx950 kernels in the order of the reference call stack:
//   commit   (/root/reference/src/commit.rs:11-22): codec -> twiddles -> 4 x circle FFT -> Merkle root
//   prove    (/root/reference/src/proof.rs:32-77; stwo core/fri.rs FriProver::{commit, decommit}):
//            codec -> FFT -> first tree -> [mix root, draw alpha, fold, tree]* -> last layer interpolate ->
//            grind -> queries -> decommit (one gather launch) -> Proof
// The blob enters as raw bytes (3.75 B per felt over PCIe) and is unpacked on the device; after that nothing but the
// 2 KB transcript summary (roots, last-layer polynomial, nonce, channel state) and the gathered openings ever cross PCIe.
// The Fiat–Shamir channel runs inside the commit-phase kernels (dev_transcript.h); the host synchronises twice per proof:
// after the grind and after the gather.  prove_begin / prove_finish expose that split so several proofs can overlap.
// (Host-side channel between layers is kept as a policy: frieda_ctx_set_host_channel, and for last layers above 2^11 points.)
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <new>

#include <stddef.h>

#include "dev_transcript.h"
#include "host.h"
#include "prove_jobs_plan.h"

namespace frieda {

namespace {

void hash_to_words(const uint8_t* h, uint32_t (&w)[8]) {
    for (int i = 0; i < 8; i++)
        w[i] = (uint32_t)h[4 * i] | ((uint32_t)h[4 * i + 1] << 8) | ((uint32_t)h[4 * i + 2] << 16) | ((uint32_t)h[4 * i + 3] << 24);
}

}  // namespace

int ensure_pinned(Ctx* ctx, size_t bytes) {
    if (ctx->pinned_bytes >= bytes) return FRIEDA_OK;
    if (ctx->pinned) FR_HIP(ctx, hipHostFree(ctx->pinned));
    ctx->pinned = nullptr;
    ctx->pinned_bytes = 0;
    FR_HIP(ctx, hipHostMalloc(&ctx->pinned, bytes, hipHostMallocDefault));
    ctx->pinned_bytes = bytes;
    FR_HIP(ctx, ctx->poison_fresh_pinned(ctx->pinned, bytes));
    return FRIEDA_OK;
}

namespace {

// Small host blobs (the fused small-domain kernel, tree.hip) are not copied to the device at all: they are placed in a page-locked
// block that the kernel reads directly (one PCIe read per workgroup instead of a copy command in front of the first launch).
int ensure_pinned_in(Ctx* ctx) {
    if (ctx->pinned_in) return FRIEDA_OK;
    FR_HIP(ctx, hipHostMalloc(&ctx->pinned_in, SMALL_HOST_IN_BYTES, hipHostMallocDefault));
    FR_HIP(ctx, ctx->poison_fresh_pinned(ctx->pinned_in, SMALL_HOST_IN_BYTES));
    return FRIEDA_OK;
}

// validated domain shape shared by commit and prove
struct Shape {
    CodecShape cs;
    uint32_t L, B, n;
    size_t N;
};

// why a shape or a configuration is refused (FRIEDA_OK: it is not): an entry point makes ctx->fail(code, text) of it, a sizing function 0
struct Refusal {
    int code = FRIEDA_OK;
    const char* text = "";
};

Refusal check_shape(size_t len, uint32_t B, Shape& sh) {
    // B arrives unchecked from the caller (a ctypes c_uint32 turns -1 into 0xFFFFFFFF): bound it before any sum is formed
    if (B > FRIEDA_MAX_LOG_DOMAIN) return {FRIEDA_ERR_ARG, "log_blowup_factor larger than FRIEDA_MAX_LOG_DOMAIN"};
    if (len > ((size_t)1 << 40)) return {FRIEDA_ERR_ARG, "blob larger than 2^40 bytes"};
    sh.cs = codec_shape(len);
    sh.L = sh.cs.log_size;
    sh.B = B;
    // Coset::half_odds(L + B - 1) panics for L + B == 0 (u32 underflow)
    if ((uint64_t)sh.L + B < 1) return {FRIEDA_ERR_INVARIANT, "log_size + log_blowup_factor must be >= 1"};
    if ((uint64_t)sh.L + B > FRIEDA_MAX_LOG_DOMAIN) return {FRIEDA_ERR_ARG, "domain larger than FRIEDA_MAX_LOG_DOMAIN"};
    sh.n = sh.L + B;
    sh.N = (size_t)1 << sh.n;
    return {};
}

int make_shape(Ctx* ctx, size_t len, uint32_t B, Shape& sh) {
    const Refusal r = check_shape(len, B, sh);
    return r.code ? ctx->fail(r.code, r.text) : FRIEDA_OK;
}

// what every prove form checks of the shape and the configuration, in the order the entry points have always reported it
Refusal check_prove(size_t len, const frieda_pcs_config& cfg, Shape& sh) {
    const uint32_t last = cfg.log_last_layer_degree_bound;
    // both arrive unchecked: bound them (the blowup: check_shape's first check) before `last + B` and the shifts that use it are formed
    if (last > 10) return {FRIEDA_ERR_ARG, "log_last_layer_degree_bound > 10"};
    const Refusal r = check_shape(len, cfg.log_blowup_factor, sh);
    if (r.code) return r;
    // FriProver::commit_last_layer asserts evaluation.len() == last_layer_domain_size: needs L - 1 >= last;
    // the line domain half_odds(n - 1) needs n >= 2
    if (sh.n < 2 || sh.L < 1 + last) return {FRIEDA_ERR_INVARIANT, "polynomial too small for the FRI configuration"};
    if (cfg.n_queries == 0 || cfg.n_queries > 4096) return {FRIEDA_ERR_ARG, "n_queries out of range"};
    return {};
}

// `count` blobs of `len` bytes each as a caller hands them over: blob b at data + b * stride, or (host blobs only) at host_ptrs[b]
struct BlobsIn {
    const uint8_t* data;
    size_t stride, len;
    bool on_device;
    const uint8_t* const* host_ptrs;
};

// host blobs -> dst + b * dst_stride on the context's stream.  A pointer table travels as one copy per blob, a strided batch as one 2-D
// copy, a lone blob as a plain copy — or, lone_as_row (the batch entry points of commit and encode), as a 2-D copy of one row
int upload_blobs(Ctx* ctx, const BlobsIn& in, uint32_t count, uint8_t* dst, size_t dst_stride, bool lone_as_row = false) {
    if (!in.len) return FRIEDA_OK;
    hipStream_t s = ctx->stream;
    if (in.host_ptrs) {
        for (uint32_t b = 0; b < count; b++) FR_HIP(ctx, hipMemcpyAsync(dst + (size_t)b * dst_stride, in.host_ptrs[b], in.len, hipMemcpyHostToDevice, s));
    } else if (count == 1 && !lone_as_row) {
        FR_HIP(ctx, hipMemcpyAsync(dst, in.data, in.len, hipMemcpyHostToDevice, s));
    } else {
        FR_HIP(ctx, hipMemcpy2DAsync(dst, dst_stride, in.data, count > 1 ? in.stride : in.len, in.len, count, hipMemcpyHostToDevice, s));
    }
    return FRIEDA_OK;
}

// where the encode step leaves what: null for what the caller does not keep
struct EncodeDest {
    uint32_t* coef;  // the general route's unpacked coefficients (workspace; the fused small route keeps none)
    uint32_t* eval;  // 4 columns of eval_len words: written by the general route in every case, by the small route only together with
    size_t eval_len;  // the tree (a commit keeps neither)
    uint8_t *tree, *scratch, *root;  // first-layer tree, leaves-first (prove, encode); root scratch (commit); device root (commit, encode)
    DevTranscript* tr;  // prove: the device transcripts, and the pinned initial ones at tr_init_pitch
    const DevTranscript* tr_init;
    size_t tr_init_pitch;
};

// the fused small-domain launch or the general encode with its last pass hashing the leaves (kernels.h), for every blob of the launch
void encode_first_tree(const k::Launch& LN, const Shape& sh, const TwiddleSet& tw, const k::BlobSource& blob, const EncodeDest& d) {
    if (k::small_domain_shape(*LN.tune, sh.L, sh.n)) {
        uint32_t* eval = d.tree ? d.eval : nullptr;
        k::small_encode_and_first_tree(LN, blob.bytes, blob.len, blob.bstride, sh.L, sh.n, tw.d_tw, tw.ds, eval, eval ? d.eval_len : 0, d.tree, d.scratch, d.root, d.tr, d.tr_init, d.tr_init_pitch);
    } else {  // (the encode unpacks: in its first pass where that pass takes the blob, else by the unpack30 launch — kernels.h BlobSource)
        k::encode_and_first_tree(LN, d.coef, (size_t)1 << sh.L, sh.L, sh.n, tw.d_tw, tw.ds, d.eval, d.eval_len, d.tree, d.scratch, d.root, d.tr, d.tr_init, d.tr_init_pitch, &blob);
    }
}

// the workspace of a commit, per blob (commit_device writes its root where the caller says and asks for the part in front of o_root only)
struct CommitLayout {
    size_t o_data, o_coef, o_eval, o_scr, o_root, bstride, N;
    CommitLayout(const Shape& sh, size_t data_len) : N(sh.N) {  // data_len 0: the blob is on the device already, or in the pinned input block
        ArenaPlan plan;
        o_data = plan.take(data_len);
        o_coef = plan.take(sizeof(uint32_t) * sh.cs.n_padded);
        o_eval = plan.take(sizeof(uint32_t) * 4 * sh.N);
        o_scr = plan.take(k::merkle_root_scratch_bytes(sh.n));
        o_root = plan.take(32);
        bstride = plan.off;
    }
    EncodeDest dest(uint8_t* A, uint8_t* d_root) const {
        return {reinterpret_cast<uint32_t*>(A + o_coef), reinterpret_cast<uint32_t*>(A + o_eval), N, nullptr, A + o_scr, d_root, nullptr, nullptr, 0};
    }
};

// LineEvaluation::interpolate for the last FRI layer (stwo core/poly/line.rs), host side: <= 2^14 points.
// `v`: evaluations in bit-reversed order on LineDomain(c); returns coefficients in LinePoly's internal order.
void line_interpolate(std::vector<QM31>& v, Coset c) {
    const uint32_t lg = c.log_size;
    const size_t n = v.size();
    for (uint32_t i = 0; i < n; i++) {
        uint32_t j = bit_reverse(i, lg);
        if (i < j) std::swap(v[i], v[j]);
    }
    for (Coset d = c; d.log_size > 0; d = d.doubled()) {
        const size_t sz = (size_t)1 << d.log_size, half = sz / 2;
        std::vector<uint32_t> ix(half);
        CPoint p = point_from_index(d.initial), st = point_from_index(d.step);
        for (size_t i = 0; i < half; i++) {
            ix[i] = m31_inv(p.x);
            p = cp_add(p, st);
        }
        for (size_t base = 0; base < n; base += sz)
            for (size_t i = 0; i < half; i++) {
                QM31 a = v[base + i], b = v[base + half + i];
                v[base + i] = qm_add(a, b);
                v[base + half + i] = qm_scale(qm_sub(a, b), ix[i]);
            }
    }
    uint32_t len_inv = m31_inv((uint32_t)n);
    for (auto& q : v) q = qm_scale(q, len_inv);
}

void bit_reverse_vec(std::vector<QM31>& v, size_t count, uint32_t lg) {
    for (uint32_t i = 0; i < count; i++) {
        uint32_t j = bit_reverse(i, lg);
        if (i < j) std::swap(v[i], v[j]);
    }
}

}  // namespace

// -------------------------------------------------------------------------------------------------
// commit
// -------------------------------------------------------------------------------------------------
int commit_device(Ctx* ctx, const uint8_t* d_data, size_t len, uint32_t log_blowup, uint8_t* d_root, bool data_in_arena) {
    FR_NO_JOB(ctx);
    Shape sh;
    int rc = make_shape(ctx, len, log_blowup, sh);
    if (rc) return rc;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const CommitLayout y(sh, data_in_arena ? len : 0);
    if (!data_in_arena) {
        rc = ctx->ensure_arena(y.o_root);
        if (rc) return rc;
    } else if (y.o_root > ctx->arena_bytes) {
        return ctx->fail(FRIEDA_ERR_ARG, "internal: arena not sized by caller");
    }
    TwiddleSet tw;
    rc = ctx->get_twiddles(sh.n, tw);
    if (rc) return rc;
    encode_first_tree(ctx->launch(), sh, tw, k::BlobSource{d_data, len, 0, sh.cs.n_padded}, y.dest(ctx->arena, d_root));
    FR_HIP(ctx, hipGetLastError());
    return FRIEDA_OK;
}

int commit_host(Ctx* ctx, const uint8_t* data, size_t len, uint32_t log_blowup, uint8_t out_root[32]) {
    FR_NO_JOB(ctx);
    Shape sh;
    int rc = make_shape(ctx, len, log_blowup, sh);
    if (rc) return rc;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const CommitLayout y(sh, len);  // commit_device(data_in_arena = true) runs on it
    rc = ctx->ensure_arena(y.bstride);
    if (rc == FRIEDA_OK) rc = ensure_pinned(ctx, 4096);
    if (rc) return rc;
    const bool in_place = k::small_domain_shape(ctx->tuning, sh.L, sh.n) && len <= SMALL_HOST_IN_BYTES;
    if (in_place) {
        // no copy commands at all: the kernels read the blob from page-locked host memory and write the root into it
        rc = ensure_pinned_in(ctx);
        if (rc) return rc;
        if (len) memcpy(ctx->pinned_in, data, len);
        rc = commit_device(ctx, static_cast<const uint8_t*>(ctx->pinned_in), len, log_blowup, static_cast<uint8_t*>(ctx->pinned), true);
    } else {
        rc = upload_blobs(ctx, BlobsIn{data, 0, len, false, nullptr}, 1, ctx->arena + y.o_data, 0);
        if (rc == FRIEDA_OK) rc = commit_device(ctx, ctx->arena + y.o_data, len, log_blowup, ctx->arena + y.o_root, true);
    }
    if (rc) return rc;
    if (!in_place) FR_HIP(ctx, hipMemcpyAsync(ctx->pinned, ctx->arena + y.o_root, 32, hipMemcpyDeviceToHost, ctx->stream));
    FR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out_root, ctx->pinned, 32);
    return FRIEDA_OK;
}

// commit() of `count` blobs of one length in one pass of launches (blob b at data + b * data_stride); roots to host memory
int commit_batch(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, bool data_on_device, uint32_t log_blowup,
                 uint8_t* out_roots, const uint8_t* const* host_ptrs) {
    int rc = commit_batch_begin(ctx, data, data_stride, len, count, data_on_device, log_blowup, host_ptrs);
    if (rc) return rc;
    return commit_batch_finish(ctx, out_roots);
}

int commit_batch_finish(Ctx* ctx, uint8_t* out_roots) {
    if (!ctx->commit_pending) return ctx->fail(FRIEDA_ERR_ARG, "no commit batch in flight on this context");
    const uint32_t count = ctx->commit_pending;
    ctx->commit_pending = 0;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    FR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FR_HIP(ctx, hipGetLastError());
    memcpy(out_roots, ctx->pinned, 32 * (size_t)count);
    return FRIEDA_OK;
}

int commit_batch_begin(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, bool data_on_device, uint32_t log_blowup,
                       const uint8_t* const* host_ptrs) {
    FR_NO_JOB(ctx);
    if (count == 0 || count > 65535) return ctx->fail(FRIEDA_ERR_ARG, "batch count out of range");
    if (count > 1 && data_stride < len) return ctx->fail(FRIEDA_ERR_ARG, "batch stride smaller than the blob length");
    Shape sh;
    int rc = make_shape(ctx, len, log_blowup, sh);
    if (rc) return rc;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const CommitLayout y(sh, data_on_device ? 0 : len);
    const size_t bstride = y.bstride;
    TwiddleSet tw;
    rc = ctx->ensure_arena(bstride * count);
    if (rc == FRIEDA_OK) rc = ensure_pinned(ctx, 32 * (size_t)count + 4096);
    if (rc == FRIEDA_OK) rc = ctx->get_twiddles(sh.n, tw);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint8_t* A = ctx->arena;
    k::Launch LN = ctx->launch();
    LN.batch = count;
    LN.bstride = count > 1 ? bstride : 0;
    k::BlobSource blob{data, len, data_stride, sh.cs.n_padded};
    if (!data_on_device) {  // (host_ptrs: separate host blobs of one length, frieda_commit_many)
        rc = upload_blobs(ctx, BlobsIn{data, data_stride, len, false, host_ptrs}, count, A + y.o_data, bstride, /*lone_as_row=*/true);
        if (rc) return rc;
        blob.bytes = A + y.o_data;
        blob.bstride = bstride;
    }
    encode_first_tree(LN, sh, tw, blob, y.dest(A, A + y.o_root));
    FR_HIP(ctx, hipMemcpy2DAsync(ctx->pinned, 32, A + y.o_root, bstride, 32, count, hipMemcpyDeviceToHost, s));
    FR_HIP(ctx, hipGetLastError());
    ctx->commit_pending = count;
    return FRIEDA_OK;
}

// -------------------------------------------------------------------------------------------------
// commit_and_generate_proof
// -------------------------------------------------------------------------------------------------
namespace {

struct FriLayerDev {
    size_t o_vals;   // 4 columns of 2^log words
    size_t o_tree;   // leaves-first layers
    uint32_t log;
};

// Collects the device reads of one layer's decommitment in proof order
struct GatherPlan {
    std::vector<uint64_t> word_idx;  // u32 index from the arena base
    std::vector<uint64_t> hash_idx;  // 32-byte index from the arena base
};

// compute_decommitment_positions_and_witness_evals (fold_step = 1): positions + requests for the witness values
// `tag` (0 or k::GATHER_ALT) is set on every index pushed: the layer lives in an encoded blob, not in the arena (prove_seeds)
std::vector<uint32_t> plan_witness(const std::vector<uint32_t>& queries, const FriLayerDev& lay, GatherPlan& g, size_t& n_witness, uint64_t tag = 0) {
    std::vector<uint32_t> pos;
    n_witness = 0;
    const size_t stride = (size_t)1 << lay.log;
    for (size_t i = 0; i < queries.size();) {
        size_t j = i;
        while (j < queries.size() && (queries[j] >> 1) == (queries[i] >> 1)) j++;
        uint32_t start = (queries[i] >> 1) << 1;
        size_t kq = i;
        for (uint32_t p = start; p < start + 2; p++) {
            pos.push_back(p);
            if (kq < j && queries[kq] == p) {
                kq++;
                continue;
            }
            for (int c = 0; c < 4; c++) g.word_idx.push_back((lay.o_vals / 4 + (size_t)c * stride + p) | tag);
            n_witness++;
        }
        i = j;
    }
    return pos;
}

// MerkleProver::decommit for a tree with its columns on the leaf layer only: requests for the sibling hashes.
// stwo walks the layers from the leaves up; on layer l it visits, in increasing order, every node that has a queried leaf or a
// visited child below it, and emits the hash of each child that was not visited itself (left before right).  `positions` are
// the queried leaves (sorted, unique).  Two scratch vectors are reused across calls (this runs ~25 times per proof).
size_t plan_merkle_decommit(const std::vector<uint32_t>& positions, const FriLayerDev& lay, GatherPlan& g, uint64_t tag = 0) {
    static thread_local std::vector<uint32_t> buf_a, buf_b;
    std::vector<uint32_t>* below = &buf_a;  // visited nodes of the layer below (children), sorted
    std::vector<uint32_t>* here = &buf_b;
    below->assign(positions.begin(), positions.end());  // leaf layer: exactly the queried leaves, no hashes needed
    size_t n_hashes = 0;
    for (int layer = (int)lay.log - 1; layer >= 0; layer--) {
        const size_t child_base = (lay.o_tree + k::merkle_layer_offset(lay.log, (uint32_t)layer + 1)) / 32;
        here->clear();
        const uint32_t* c = below->data();
        const size_t nc = below->size();
        for (size_t i = 0; i < nc;) {
            const uint32_t node = c[i] >> 1;
            const bool has_left = c[i] == 2 * node;
            if (has_left) i++;
            const bool has_right = i < nc && c[i] == 2 * node + 1;
            if (has_right) i++;
            if (!has_left) {
                g.hash_idx.push_back((child_base + 2 * (size_t)node) | tag);
                n_hashes++;
            }
            if (!has_right) {
                g.hash_idx.push_back((child_base + 2 * (size_t)node + 1) | tag);
                n_hashes++;
            }
            here->push_back(node);
        }
        std::swap(below, here);
    }
    return n_hashes;
}

}  // namespace

// Capacity of a job's opening lists.  Words: per layer <= 2 positions per query (+ the evaluations).  Hashes: a batch keeps its
// long-standing loose bound, 2 * queries * (n + 1) per layer; a prove_seeds job — whose point is memory per seed — the exact one: in a
// tree of 2^m leaves opened at pairs, every level below the root has at most `queries` visited nodes and each emits at most one sibling,
// the leaf level none: queries * (m - 1) <= queries * (n - li) for layer li.
size_t opening_max_words(uint32_t n_queries, uint32_t n_inner) { return (size_t)n_queries * 4 * (1 + (n_inner + 1)); }
size_t opening_max_hashes(uint32_t n_queries, uint32_t n, uint32_t n_inner, bool seeds) {
    if (!seeds) return (size_t)n_queries * 2 * (size_t)(n + 1) * (n_inner + 1);
    size_t h = 0;
    for (uint32_t li = 0; li <= n_inner; li++) h += (size_t)n_queries * (n - li);
    return h;
}

namespace {
// What the jobs of a prove call are.  PLAIN: `count` blobs.  SEEDS (prove_seeds): `count` seeds of ONE encoded blob, enc.  BLOCK
// (prove_jobs, and prove_seeds_blobs as its rectangle): `count` jobs sorted by blob, one seed each, over the n_blobs rows of `block`
// (prove_jobs_plan.h: job y is row job_row[y], row r's jobs are [row_first[r], row_first[r + 1])); enc = block[0] stands for the shape
struct ProveForm {
    enum Kind { PLAIN, SEEDS, BLOCK } kind = PLAIN;
    const Encoded* enc = nullptr;
    const Encoded* const* block = nullptr;
    uint32_t n_blobs = 0;
    uint32_t plan_blobs = 0;  // the rows the ARENA is planned for, >= n_blobs (frieda_prove_jobs_begin sizes by the handles it was given)
    const uint32_t* job_row = nullptr;
    const uint32_t* row_first = nullptr;
    const uint32_t* groups = nullptr;  // the seed-looped fold's group entries as staged, n_groups of them (route A: none); the sizing
    uint32_t n_groups = 0;             // functions know no context and plan the arena for the most a list can have, one per job
    const uint32_t* out_slot = nullptr;  // null: proof y goes to slot y
};

// the block table of a BLOCK call, as the arena and the pinned staging hold it: rows, one row number per job, and (route B) an entry
// per group of jobs
struct BlockTablePlan {
    size_t o_job = 0, o_group = 0, bytes = 0;
    uint32_t groups = 0;  // (0: no group part)
    BlockTablePlan() = default;
    BlockTablePlan(uint32_t n_blobs, uint32_t n_jobs, uint32_t n_groups) : groups(n_groups) {
        ArenaPlan p;
        p.take(sizeof(k::SeedsBlobRow) * n_blobs);
        o_job = p.take(sizeof(uint32_t) * (size_t)n_jobs);
        o_group = p.take(sizeof(uint32_t) * groups);
        bytes = p.off;
    }
};

// Where everything of a prove call lives, in the arena and in the pinned staging block: what the call asks ensure_arena / ensure_pinned
// for, what the job keeps, and what the sizing functions report (frieda_workspace_bytes and through it the batch policy, frieda_seeds_*).
struct ProveLayout {
    uint32_t last = 0, last_log = 0, n_inner = 0;  // the last layer's degree bound and size (logs), the number of inner layers
    // arena, per job (job b's part is job 0's shifted by b * bstride, a multiple of 256).  SEEDS and BLOCK: blob, coefficients, evaluation
    // and first tree live in the encoded blob — `first` then holds no arena offsets and a job's part begins at the first inner layer
    size_t o_data = 0, o_coef = 0;
    FriLayerDev first{};
    std::vector<FriLayerDev> inner;
    size_t o_lastv = 0, o_nonce = 0, bstride = 0;
    // arena, behind the jobs' parts: transcripts, grind window counters (one cache line per job), the index and output lists of the
    // host-planner fallback's gather (max_words / max_hashes entries over all jobs) and, BLOCK, the table
    size_t o_tr = 0, o_gnext = 0, o_widx = 0, o_hidx = 0, o_wout = 0, o_hout = 0, o_blk = 0;
    size_t max_words = 0, max_hashes = 0, arena_bytes = 0;
    // pinned block: job b's transcript summary (header + last-layer polynomial) at b * tr_host_pitch, or the last layer itself on the
    // host-channel path; behind the summaries the device openings (decommit.hip), job b's header, words and hashes at dec_off +
    // b * dec_stride; the fallback writes its results at 0 and stages its index lists at gather_off instead; the block table as staged
    // and uploaded sits behind everything else, at pin_blk (nothing writes there until the next call on this context)
    size_t tr_host_pitch = 0, dec_off = 0, dec_stride = 0, dec_words_off = 0, dec_hashes_off = 0, gather_off = 0, pin_blk = 0, pinned_bytes = 0;
    uint32_t dec_max_words = 0, dec_max_hashes = 0;  // per job
    BlockTablePlan table;
};

// pure: no HIP call, no context.  host_len: the blob's bytes when it is uploaded into the arena, 0 for device data and encoded blobs
ProveLayout prove_layout(const Shape& sh, const frieda_pcs_config& cfg, uint32_t count, size_t host_len, const ProveForm& form) {
    ProveLayout y;
    const uint32_t n = sh.n, last = y.last = cfg.log_last_layer_degree_bound, last_log = y.last_log = last + cfg.log_blowup_factor;
    const uint32_t n_inner = y.n_inner = (n - 1) - last_log;
    const bool shared_first = form.kind != ProveForm::PLAIN;
    ArenaPlan plan;
    y.first.log = n;
    if (!shared_first) {
        y.o_data = plan.take(host_len);
        y.o_coef = plan.take(sizeof(uint32_t) * sh.cs.n_padded);
        y.first.o_vals = plan.take(sizeof(uint32_t) * 4 * sh.N);
        y.first.o_tree = plan.take(k::merkle_layer_offset(n, 0) + 32);
    }
    y.inner.resize(n_inner);
    for (uint32_t kx = 0; kx < n_inner; kx++) {
        const uint32_t lg = n - 1 - kx;
        y.inner[kx].log = lg;
        y.inner[kx].o_vals = plan.take(sizeof(uint32_t) * 4 << lg);
        y.inner[kx].o_tree = plan.take(k::merkle_layer_offset(lg, 0) + 32);
    }
    y.o_lastv = plan.take(sizeof(uint32_t) * 4 << last_log);
    y.o_nonce = plan.take(8);
    y.bstride = plan.off;
    plan.off = y.bstride * count;
    y.o_tr = plan.take(sizeof(DevTranscript) * count);
    y.o_gnext = plan.take(sizeof(uint32_t) * k::GRIND_NEXT_STRIDE * count);
    y.max_words = opening_max_words(cfg.n_queries, n_inner) * count;
    y.max_hashes = opening_max_hashes(cfg.n_queries, n, n_inner, shared_first) * count;
    y.o_widx = plan.take(8 * y.max_words);
    y.o_hidx = plan.take(8 * y.max_hashes);
    y.o_wout = plan.take(4 * y.max_words);
    y.o_hout = plan.take(32 * y.max_hashes);
    if (form.kind == ProveForm::BLOCK) {
        y.table = BlockTablePlan(form.n_blobs, count, form.n_groups);
        // (the table's group part is planned for the largest group count, a group per job, whatever FRIEDA_SEEDS_FOLD_GROUP and the list
        // say: the workspace of a call is a function of its shape alone)
        y.o_blk = plan.take(BlockTablePlan(form.plan_blobs, count, count).bytes);
    }
    y.arena_bytes = plan.off;
    y.tr_host_pitch = (offsetof(DevTranscript, last_poly) + ((size_t)16 << last) + 63) & ~(size_t)63;
    y.dec_max_words = (uint32_t)(y.max_words / count);
    y.dec_max_hashes = (uint32_t)(y.max_hashes / count);
    y.dec_words_off = k::DECOMMIT_HEADER_BYTES;
    y.dec_hashes_off = y.dec_words_off + ((4 * (size_t)y.dec_max_words + 15) & ~(size_t)15);
    y.dec_stride = (y.dec_hashes_off + 32 * (size_t)y.dec_max_hashes + 255) & ~(size_t)255;
    y.dec_off = (y.tr_host_pitch * count + 255) & ~(size_t)255;
    y.gather_off = (4 * y.max_words + 32 * y.max_hashes + 255) & ~(size_t)255;
    // the largest of: the summaries, the last layer, the fallback's results and lists (gather_off + 8 bytes per index), the device openings
    y.pinned_bytes = std::max({y.tr_host_pitch * count, (sizeof(uint32_t) * 4) << last_log, (4 + 8) * y.max_words + (32 + 8) * y.max_hashes + 512, y.dec_off + y.dec_stride * count});
    y.pin_blk = (y.pinned_bytes + 255) & ~(size_t)255;
    if (form.kind == ProveForm::BLOCK) y.pinned_bytes = y.pin_blk + y.table.bytes;
    return y;
}

size_t prove_arena_bytes(size_t len, const frieda_pcs_config& cfg, uint32_t count, const ProveForm& form) {
    Shape sh;
    if (check_prove(len, cfg, sh).code) return 0;
    return prove_layout(sh, cfg, count, 0, form).arena_bytes;
}
}  // namespace

// State of a proof between prove_begin (commit phase enqueued) and prove_finish (decommit + assembly).
struct ProveJob {
    frieda_pcs_config cfg{};
    Shape sh{};
    uint32_t count = 1;  // a batch of `count` jobs of one shape
    ProveLayout lay;
    bool dev_channel = false, dev_decommit = false;  // dev_decommit: openings on the device (decommit.hip), read from the pinned block by _finish
    // the tree-skip threshold the trees of THIS job were built with (k::tree_skip_threshold at begin): the openings — device kernel
    // and host-planner fallback — must use the same one even if frieda_ctx_set_option moved the knob between _begin and _finish
    uint32_t skip_log = 0;
    // SEEDS: layer 0 (values, tree) is enc's, at stride 0, with the threshold ITS tree was built with.  BLOCK: layer 0 of a job is its
    // handle's, which the kernels find through the table `blk` points at (in the arena, uploaded by _begin); row r's jobs are
    // [row_first[r], row_first[r + 1]); proof y is written to the caller's slot out_slot[y] (empty: slot y)
    const Encoded* enc = nullptr;
    uint32_t first_skip_log = 0;
    std::vector<const Encoded*> block;
    std::vector<uint32_t> row_first, out_slot;
    k::SeedsBlock blk{};
    struct Blob {
        Channel ch{};
        std::vector<Hash32> roots;
        std::vector<std::array<uint32_t, 4>> alphas;  // per layer, for frieda_ctx_last_transcript
        std::vector<QM31> lastv;
        uint64_t nonce = ~0ull;
        uint32_t digest_before_grind[8] = {0};
    };
    std::vector<Blob> blobs;
    uint64_t grind_base = 0, grind_chunk = 0;
    std::chrono::steady_clock::time_point t_start;

    // every launch of the job covers the whole batch
    k::Launch launch(const Ctx* ctx) const {
        k::Launch LN = ctx->launch();
        LN.batch = count;
        LN.bstride = count > 1 ? lay.bstride : 0;
        return LN;
    }
    // column c of a layer: in the workspace, or (layer 0 of an encoded blob) the handle's, only ever read
    uint32_t* cols(const Ctx* ctx, const FriLayerDev& l, int c) const {
        uint32_t* v = (enc && &l == &lay.first) ? const_cast<uint32_t*>(enc->eval()) : reinterpret_cast<uint32_t*>(ctx->arena + l.o_vals);
        return v + ((size_t)c << l.log);
    }
};

void ProveJobDeleter::operator()(ProveJob* j) const { delete j; }

// Device workspace one blob of `len` bytes adds to a batched call (what ensure_arena is asked for, per blob): the figure the batch
// policy (batch_plan below) divides its budget by.  0: the shape is outside what the prover accepts.
size_t workspace_bytes_per_blob(size_t len, uint32_t log_blowup, uint32_t log_last_layer, bool prove, bool data_on_device) {
    Shape sh;
    const size_t host_len = data_on_device ? 0 : len;
    if (!prove) return check_shape(len, log_blowup, sh).code ? 0 : CommitLayout(sh, host_len).bstride;
    const frieda_pcs_config cfg{0, log_blowup, log_last_layer, 1};  // (a job's own part does not depend on the queries)
    if (check_prove(len, cfg, sh).code) return 0;
    return prove_layout(sh, cfg, 1, host_len, ProveForm{}).bstride;
}

// ---- batch policy (host.h) ----
uint64_t batch_budget_bytes(const k::Tuning& t) {
    //  the figure below was measured on a 288 GB device; on a smaller one it must not ask for what the device does not have.
    // What is FREE right now is the callers' business (multi.cpp asks hipMemGetInfo before it cuts a device's run, and halves on NOMEM).
    if (t.batch_budget_mb) {
        const uint64_t b = (uint64_t)t.batch_budget_mb << 20;
        return t.device_mem_bytes ? std::min<uint64_t>(b, t.device_mem_bytes / 100 * 45) : b;
    }
    if (t.device_mem_bytes) return std::min<uint64_t>(batch_budget_bytes(k::tuning_defaults()), t.device_mem_bytes / 100 * 16);  // (16 %: a device that reports 288e9 bytes still gets the sixteen proofs the figure was measured with)
    // measured at the headline size and stated in workspace bytes so that it carries over to every other size: sixteen proofs of a
    // 2^24 domain per call (15 MiB blobs: 2^22 felts -> 2^20 coefficients per column, blowup 2^4), ~43 GB per call in flight — two
    // calls in flight hold 30 % of a 288 GB MI355X.  With the compression's throughput form a call's fixed part (the narrow launches
    // of its latency chain, ~1.6 ms at this size) weighs more than it used to: 1.89 ms per blob at 5 per call, 1.85 at 15, 1.83 at 30
    // (profiles/r05_batch_policy_sweep.txt, second block)
    static const uint64_t sixteen_headline = 16 * (uint64_t)workspace_bytes_per_blob((size_t)15 << 20, 4, 0, true, true);
    return sixteen_headline;
}

uint32_t batch_per_call(const k::Tuning& t, size_t ws_per_blob, uint32_t count, uint32_t in_flight) {
    if (count == 0) return 1;
    if (in_flight == 0) in_flight = 1;
    uint64_t per = ws_per_blob ? batch_budget_bytes(t) / ws_per_blob : 1;
    const uint64_t ways = (uint64_t)std::max<uint32_t>(1, t.batch_calls_per_ctx) * in_flight;
    const uint64_t spread = (count + ways - 1) / ways;  // every context gets its calls
    per = std::min<uint64_t>(per, spread);
    // (the batched entry points take up to 65535 blobs; beyond a few thousand per call the latency chain is amortised to nothing, while
    // the pinned staging block — ~10 KB of openings per proof — and the host-side proof objects keep growing with the count)
    per = std::min<uint64_t>(per, 4096);
    return (uint32_t)std::max<uint64_t>(per, 1);
}

void batch_cut(uint32_t count, uint32_t per_call, uint32_t in_flight, std::vector<uint32_t>& calls) {
    calls.clear();
    if (count == 0) return;
    if (per_call == 0) per_call = 1;
    if (in_flight == 0) in_flight = 1;
    // the number of calls is a multiple of the calls in flight: an odd call out would run alone on the chip, its latency chain and
    // its launches' ramps un-overlapped (20 blobs: 4 x 5, not 5 x 4); no call exceeds per_call (the budget is a ceiling)
    const uint64_t round = (uint64_t)per_call * in_flight;
    uint64_t n = (uint64_t)in_flight * ((count + round - 1) / round);
    n = std::min<uint64_t>(n, count);
    const uint32_t base = (uint32_t)(count / n), extra = (uint32_t)(count % n);
    calls.assign((size_t)n, base);
    for (uint32_t i = 0; i < extra; i++) calls[i] = base + 1;
}


static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// transcript summaries (header + last-layer polynomial) of all blobs -> pinned memory, blob b at b * tr_host_pitch
static int download_transcripts(Ctx* ctx, const ProveJob& J) {
    const size_t bytes = offsetof(DevTranscript, last_poly) + ((size_t)16 << J.lay.last);
    const uint8_t* d_tr = ctx->arena + J.lay.o_tr;
    if (J.count == 1) {
        FR_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_tr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        FR_HIP(ctx, hipMemcpy2DAsync(ctx->pinned, J.lay.tr_host_pitch, d_tr, sizeof(DevTranscript), bytes, J.count, hipMemcpyDeviceToHost, ctx->stream));
    }
    return FRIEDA_OK;
}

// decommit.hip over all blobs of the job: reads the device transcripts (nonce, channel) and the layers, writes the pinned block
static void launch_decommit(Ctx* ctx, const ProveJob& J) {
    uint8_t* A = ctx->arena;
    const ProveLayout& Y = J.lay;
    k::DecommitArgs a{};
    a.tr = reinterpret_cast<const DevTranscript*>(A + Y.o_tr);
    a.n = J.sh.n;
    a.n_layers = 1 + J.lay.n_inner;
    a.n_queries = J.cfg.n_queries;
    a.bstride = J.count > 1 ? Y.bstride : 0;
    a.out = static_cast<uint8_t*>(ctx->pinned) + Y.dec_off;
    a.out_stride = Y.dec_stride;
    a.words_off = Y.dec_words_off;
    a.hashes_off = Y.dec_hashes_off;
    a.max_words = Y.dec_max_words;
    a.max_hashes = Y.dec_max_hashes;
    a.skip_log = J.skip_log;
    a.skip_log0 = J.first_skip_log;
    a.first_shared = J.enc ? 1 : 0;
    a.vals[0] = J.cols(ctx, Y.first, 0);
    a.trees[0] = J.enc ? J.enc->tree() : A + Y.first.o_tree;
    a.blk_table = J.blk.table;  // (a block of handles: layer 0 and its threshold per job, from the table)
    a.blk_job = J.blk.job_row;
    for (uint32_t kx = 0; kx < J.lay.n_inner; kx++) {
        a.vals[1 + kx] = J.cols(ctx, Y.inner[kx], 0);
        a.trees[1 + kx] = A + Y.inner[kx].o_tree;
    }
    // a lone large proof has ~4000 hashes to fetch: several workgroups share them (each repeats the cheap table set-up)
    const uint32_t wgs = J.count >= 8 ? 1u : (J.count >= 2 ? 2u : (J.sh.n >= 16 ? 8u : 2u));
    k::decommit(J.launch(ctx), a, wgs);
}

// ---- prove_begin: the pieces, in the order they run ----
// BLOCK: the per-blob table, the row of every job and the entry of every group of jobs: one upload per call, ahead of every launch
static int upload_block_table(Ctx* ctx, ProveJob& J, const ProveForm& form) {
    const BlockTablePlan& T = J.lay.table;
    const uint32_t n_block = (uint32_t)J.block.size();
    uint8_t* hp = static_cast<uint8_t*>(ctx->pinned) + J.lay.pin_blk;
    k::SeedsBlobRow* rows = reinterpret_cast<k::SeedsBlobRow*>(hp);
    for (uint32_t r = 0; r < n_block; r++) {
        const Encoded* e = J.block[r];
        rows[r] = k::SeedsBlobRow{e->eval(), e->tree(), e->d + e->o_root, e->skip_log, 0};
    }
    memcpy(hp + T.o_job, form.job_row, sizeof(uint32_t) * J.count);
    if (T.groups) memcpy(hp + T.o_group, form.groups, sizeof(uint32_t) * T.groups);
    uint8_t* d_blk = ctx->arena + J.lay.o_blk;
    FR_HIP(ctx, hipMemcpyAsync(d_blk, hp, T.bytes, hipMemcpyHostToDevice, ctx->stream));
    J.blk = k::SeedsBlock{reinterpret_cast<const k::SeedsBlobRow*>(d_blk), reinterpret_cast<const uint32_t*>(d_blk + T.o_job),
                          T.groups ? reinterpret_cast<const uint32_t*>(d_blk + T.o_group) : nullptr, n_block, T.groups};
    return FRIEDA_OK;
}

// Every job's channel with its seed mixed in; device channel: staged as the initial transcripts.  No copy in the stream: the kernel that finishes
// the first tree reads these few words from the pinned block itself (next written by the transcript download behind the grind, i.e. after it)
static void init_transcripts(Ctx* ctx, ProveJob& J, const uint64_t* seeds) {
    for (uint32_t b = 0; b < J.count; b++) {
        ProveJob::Blob& bl = J.blobs[b];
        bl.ch.init();
        if (seeds) bl.ch.mix_u64(seeds[b]);  // src/proof.rs:40-42
        bl.roots.assign(1 + J.lay.n_inner, Hash32{});
        if (!J.dev_channel) continue;
        DevTranscript* ht = reinterpret_cast<DevTranscript*>(static_cast<uint8_t*>(ctx->pinned) + b * J.lay.tr_host_pitch);
        memset(ht, 0, offsetof(DevTranscript, last_poly));
        ht->ch = bl.ch;
        ht->nonce = ~0ull;
        ht->draw_bound = ctx->test_draw_bound;
    }
}

// the whole commit phase on the device, transcript included, then the first grind range, the transcript download and the openings: enqueued only
static int enqueue_device_channel(Ctx* ctx, ProveJob& J, const TwiddleSet& tw, const k::BlobSource& blob) {
    uint8_t* A = ctx->arena;
    const ProveLayout& Y = J.lay;
    const k::Launch LN = J.launch(ctx);
    const Encoded* enc = J.enc;
    const uint32_t n = J.sh.n, n_inner = J.lay.n_inner;
    const k::SeedsBlock* blk = J.block.empty() ? nullptr : &J.blk;
    DevTranscript* d_tr = reinterpret_cast<DevTranscript*>(A + Y.o_tr);
    const DevTranscript* tr_init = reinterpret_cast<const DevTranscript*>(ctx->pinned);
    // the encode's last pass runs fused with FriProver::commit_first_layer's leaf hashing (src/proof.rs:48-52); small domains: unpack +
    // encode + first tree in one launch, straight from the blob.  (prove_begin_impl's `small` asks for more than small_domain_shape — no
    // host channel, a last layer the tail takes — and on this branch both hold: the two conditions pick the same kernel here)
    if (enc)  // the first tree and its root exist: only the transcripts' step behind that root — mix_root, first alpha — per seed
        k::channel_after_shared_root(LN, enc->d + enc->o_root, d_tr, tr_init, Y.tr_host_pitch, blk);
    else
        encode_first_tree(LN, J.sh, tw, blob, {reinterpret_cast<uint32_t*>(A + Y.o_coef), J.cols(ctx, Y.first, 0), J.sh.N, A + Y.first.o_tree, nullptr, nullptr, d_tr, tr_init, Y.tr_host_pitch});
    // FriProver::commit_inner_layers: layers above 2^11 points, one fused fold + tree each
    const FriLayerDev* cur = &Y.first;
    bool circle = true;
    uint32_t kx = 0;
    // layers of more than 2^TAIL_RUN_LOG points go through the multi-workgroup kernels (a 2^11 layer is faster there than in
    // the one-workgroup tail); FRIEDA_TAIL_RUN_LOG is a tuning knob
    const uint32_t tail_run_log = ctx->tuning.tail_run_log;
    const uint32_t seeds_group = enc ? ctx->tuning.seeds_fold_group : 0;
    while (kx < n_inner && Y.inner[kx].log > tail_run_log) {
        k::fold_and_tree(LN, circle, J.cols(ctx, *cur, 0), (size_t)1 << cur->log, cur->log, n, tw.d_itw, tw.ds, J.cols(ctx, Y.inner[kx], 0),
                         A + Y.inner[kx].o_tree, d_tr, enc && circle, circle ? seeds_group : 0, blk);
        cur = &Y.inner[kx];
        circle = false;
        kx++;
    }
    // everything that is left, the last layer's interpolation and mix_felts included, in one workgroup
    uint32_t* tvals[16];
    uint8_t* ttrees[16];
    const uint32_t n_tail = (n_inner - kx) + 1;
    if (n_tail > 16) return ctx->fail(FRIEDA_ERR_INVARIANT, "internal: tail too long");
    for (uint32_t i = 0; i + 1 < n_tail; i++) {
        tvals[i] = J.cols(ctx, Y.inner[kx + i], 0);
        ttrees[i] = A + Y.inner[kx + i].o_tree;
    }
    tvals[n_tail - 1] = reinterpret_cast<uint32_t*>(A + Y.o_lastv);
    ttrees[n_tail - 1] = nullptr;
    uint32_t* d_gnext = reinterpret_cast<uint32_t*>(A + Y.o_gnext);
    k::fri_tail(LN, J.cols(ctx, *cur, 0), (size_t)1 << cur->log, cur->log, circle, n, tw.d_itw, tw.ds, J.lay.last_log, J.lay.last, n_tail, tvals, ttrees, d_tr,
                d_gnext, enc && circle, blk);
    // grind (src/proof.rs:58), keyed by the digest now sitting in the device transcript: first chunk + transcript download
    J.grind_base = 0;
    // first range: 16x the expected search (a miss has probability e^-16; workgroups without work leave at once)
    J.grind_chunk = (uint64_t)1 << std::max<uint32_t>(22, std::min<uint32_t>(J.cfg.pow_bits, 36) + 4);
    if (ctx->tuning.test_grind_first_log) J.grind_chunk = (uint64_t)1 << ctx->tuning.test_grind_first_log;  // test hook: the retry loop runs
    k::grind_dev(LN, d_tr, d_gnext, J.cfg.pow_bits, J.grind_base, J.grind_chunk, /*next_zeroed=*/true);
    int rc = download_transcripts(ctx, J);
    if (rc) return rc;
    // mix_u64(nonce), query sampling and every opening of the proof, written in proof order into the pinned block
    J.dev_decommit = J.cfg.n_queries <= k::DECOMMIT_MAX_QUERIES && 1 + n_inner <= k::DECOMMIT_MAX_LAYERS && n <= k::DECOMMIT_MAX_LOG_DOMAIN &&
                     !ctx->tuning.host_decommit;
    if (J.dev_decommit) launch_decommit(ctx, J);
    FR_HIP(ctx, hipGetLastError());
    ctx->phase_ms[0] = ms_since(J.t_start);  // commit phase fully enqueued
    return FRIEDA_OK;
}

// The commit phase of one blob with the channel on the host between the layers (a last layer above 2^11 points, or the host channel
// policy), a synchronisation per root.  The coefficients are in the arena (unpack30, prove_begin_impl) unless the first layer is an encoded blob's
static int run_host_channel(Ctx* ctx, ProveJob& J, const TwiddleSet& tw) {
    uint8_t* A = ctx->arena;
    hipStream_t s = ctx->stream;
    const ProveLayout& Y = J.lay;
    const k::Launch LN = J.launch(ctx);
    const uint32_t n = J.sh.n, n_inner = J.lay.n_inner, last = J.lay.last, last_log = J.lay.last_log;
    ProveJob::Blob& bl = J.blobs[0];
    Channel& ch = bl.ch;
    auto cols = [&](const FriLayerDev& lay, int c) { return J.cols(ctx, lay, c); };
    auto fetch_root = [&](const FriLayerDev& lay, Hash32& root) -> int {
        FR_HIP(ctx, hipMemcpyAsync(ctx->pinned, A + lay.o_tree + k::merkle_layer_offset(lay.log, 0), 32, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        memcpy(root.data(), ctx->pinned, 32);
        return FRIEDA_OK;
    };
    int rc;
    // ---- FriProver::commit_first_layer ----
    if (J.enc) {
        memcpy(bl.roots[0].data(), J.enc->root, 32);  // (prove_seeds, one seed: the commitment was made by encode_blob)
    } else {
        k::circle_evaluate(LN, reinterpret_cast<const uint32_t*>(A + Y.o_coef), (size_t)1 << J.sh.L, 4, J.sh.L, n, tw.d_tw, tw.ds, cols(Y.first, 0), J.sh.N);
        k::merkle_tree4(LN, cols(Y.first, 0), cols(Y.first, 1), cols(Y.first, 2), cols(Y.first, 3), n, A + Y.first.o_tree);
        rc = fetch_root(Y.first, bl.roots[0]);
        if (rc) return rc;
    }
    uint32_t rw[8];
    hash_to_words(bl.roots[0].data(), rw);
    ch.mix_root(rw);

    // ---- FriProver::commit_inner_layers ----
    QM31 alpha = ch.draw_felt(ctx->test_draw_bound);
    bl.alphas.assign(1 + n_inner, std::array<uint32_t, 4>{});
    bl.alphas[0] = {alpha.a, alpha.b, alpha.c, alpha.d};
    {
        // LineEvaluation::new_zero then fold_circle_into_line
        uint32_t* dst = (n_inner > 0) ? cols(Y.inner[0], 0) : reinterpret_cast<uint32_t*>(A + Y.o_lastv);
        FR_HIP(ctx, hipMemsetAsync(dst, 0, sizeof(uint32_t) * 4 << (n - 1), s));
        k::fold_circle_into_line(LN, dst, (size_t)1 << (n - 1), cols(Y.first, 0), J.sh.N, n, tw.d_itw, tw.ds, k::Alpha{{alpha.a, alpha.b, alpha.c, alpha.d}});
    }
    for (uint32_t kx = 0; kx < n_inner; kx++) {
        const FriLayerDev& lay = Y.inner[kx];
        k::merkle_tree4(LN, cols(lay, 0), cols(lay, 1), cols(lay, 2), cols(lay, 3), lay.log, A + lay.o_tree);
        rc = fetch_root(lay, bl.roots[kx + 1]);
        if (rc) return rc;
        hash_to_words(bl.roots[kx + 1].data(), rw);
        ch.mix_root(rw);
        alpha = ch.draw_felt(ctx->test_draw_bound);
        bl.alphas[kx + 1] = {alpha.a, alpha.b, alpha.c, alpha.d};
        uint32_t* dst = (kx + 1 < n_inner) ? cols(Y.inner[kx + 1], 0) : reinterpret_cast<uint32_t*>(A + Y.o_lastv);
        k::fold_line(LN, cols(lay, 0), (size_t)1 << lay.log, lay.log, n, tw.d_itw, tw.ds, k::Alpha{{alpha.a, alpha.b, alpha.c, alpha.d}}, dst,
                     (size_t)1 << (lay.log - 1));
    }

    // ---- FriProver::commit_last_layer ----
    std::vector<QM31>& lastv = bl.lastv;
    const size_t n_lastdom = (size_t)1 << last_log;
    FR_HIP(ctx, hipMemcpyAsync(ctx->pinned, A + Y.o_lastv, sizeof(uint32_t) * 4 * n_lastdom, hipMemcpyDeviceToHost, s));
    FR_HIP(ctx, hipStreamSynchronize(s));
    lastv.assign(n_lastdom, QM31{0, 0, 0, 0});
    {
        const uint32_t* h = reinterpret_cast<const uint32_t*>(ctx->pinned);
        for (size_t i = 0; i < n_lastdom; i++) lastv[i] = {h[i], h[n_lastdom + i], h[2 * n_lastdom + i], h[3 * n_lastdom + i]};
    }
    line_interpolate(lastv, line_coset(n, last_log));
    bit_reverse_vec(lastv, n_lastdom, last_log);  // into_ordered_coefficients
    const size_t n_poly = (size_t)1 << last;
    for (size_t i = n_poly; i < n_lastdom; i++)
        if (!qm_is_zero(lastv[i])) return ctx->fail(FRIEDA_ERR_INVARIANT, "invalid degree");  // assert! upstream
    lastv.resize(n_poly);
    bit_reverse_vec(lastv, n_poly, last);  // LinePoly::from_ordered_coefficients
    channel_mix_felts(ch, lastv);
    memcpy(bl.digest_before_grind, ch.digest, 32);

    // ---- grind (src/proof.rs:58-59) ----
    unsigned long long* d_nonce = reinterpret_cast<unsigned long long*>(A + Y.o_nonce);
    FR_HIP(ctx, hipMemsetAsync(d_nonce, 0xFF, 8, s));
    uint64_t base = 0, chunk = (uint64_t)1 << 22;
    for (;;) {
        k::grind_scan(LN, ch.digest, J.cfg.pow_bits, base, chunk, d_nonce);
        FR_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_nonce, 8, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        memcpy(&bl.nonce, ctx->pinned, 8);
        if (bl.nonce != ~0ull) break;
        base += chunk;
        if (chunk < ((uint64_t)1 << 28)) chunk <<= 1;
    }
    ctx->phase_ms[0] = ms_since(J.t_start);
    return FRIEDA_OK;
}

// `count` jobs of one shape (ProveForm); seeds: null or one per blob (PLAIN), one per job (SEEDS, BLOCK)
static int prove_begin_impl(Ctx* ctx, const BlobsIn& in, uint32_t count, const uint64_t* seeds, frieda_pcs_config cfg, ProveForm form) {
    const auto t_entry = std::chrono::steady_clock::now();
    FR_NO_JOB(ctx);  // a proof or a commit batch in flight owns the arena and the pinned block
    if (count == 0 || count > 65535) return ctx->fail(FRIEDA_ERR_ARG, "batch count out of range");
    if (!form.enc && count > 1 && in.stride < in.len) return ctx->fail(FRIEDA_ERR_ARG, "batch stride smaller than the blob length");
    std::unique_ptr<ProveJob, ProveJobDeleter> jp(new ProveJob());
    ProveJob& J = *jp;
    const Refusal refused = check_prove(in.len, cfg, J.sh);
    if (refused.code) return ctx->fail(refused.code, refused.text);
    if (cfg.pow_bits > 48) return ctx->fail(FRIEDA_ERR_ARG, "pow_bits > 48");
    FR_HIP(ctx, hipSetDevice(ctx->device));
    J.cfg = cfg;
    J.count = count;
    J.skip_log = k::tree_skip_threshold(ctx->tuning, count);
    J.enc = form.enc;
    J.first_skip_log = form.enc ? form.enc->skip_log : J.skip_log;
    if (form.kind == ProveForm::BLOCK) {
        J.block.assign(form.block, form.block + form.n_blobs);
        J.row_first.assign(form.row_first, form.row_first + form.n_blobs + 1);
        if (form.out_slot) J.out_slot.assign(form.out_slot, form.out_slot + count);
    }
    J.blobs.resize(count);
    J.lay = prove_layout(J.sh, cfg, count, in.on_device ? 0 : in.len, form);
    TwiddleSet tw;
    int rc = ctx->ensure_arena(J.lay.arena_bytes);
    if (rc == FRIEDA_OK) rc = ensure_pinned(ctx, J.lay.pinned_bytes);
    if (rc == FRIEDA_OK) rc = ctx->get_twiddles(J.sh.n, tw);
    if (rc) return rc;
    J.t_start = std::chrono::steady_clock::now();
    for (double& v : ctx->phase_ms) v = 0.0;
    // The whole commit phase runs on the device (transcript included) when the last layer fits the single-workgroup tail;
    // otherwise (log_last_layer_degree_bound + log_blowup_factor > 11) the channel is evaluated on the host between layers.
    J.dev_channel = J.lay.last_log <= k::TAIL_LOG && !ctx->host_channel;
    if (count > 1 && !J.dev_channel) return ctx->fail(FRIEDA_ERR_ARG, "batches need the device channel (last layer <= 2^11 points, host channel policy off)");
    // ---- encode (src/proof.rs:38,44-50) ----
    const bool small = k::small_domain_shape(ctx->tuning, J.sh.L, J.sh.n) && !ctx->host_channel && J.lay.last_log <= k::TAIL_LOG;
    k::BlobSource blob{in.data, in.len, in.stride, J.sh.cs.n_padded};  // device data and encoded blobs stay where they are
    if (!in.on_device && !J.enc) {
        // a lone small blob is not copied to the device: the first kernel reads it from page-locked host memory
        const bool in_place = small && count == 1 && in.len <= SMALL_HOST_IN_BYTES;
        rc = in_place ? ensure_pinned_in(ctx) : upload_blobs(ctx, in, count, ctx->arena + J.lay.o_data, J.lay.bstride);
        if (rc) return rc;
        if (in_place && in.len) memcpy(ctx->pinned_in, in.host_ptrs ? in.host_ptrs[0] : in.data, in.len);
        blob.bytes = in_place ? static_cast<const uint8_t*>(ctx->pinned_in) : ctx->arena + J.lay.o_data;
        blob.bstride = in_place ? 0 : J.lay.bstride;
    }
    // the device-channel path hands the blob to the encode (kernels.h BlobSource); the host-channel path's plain transform wants coefficients
    if (!small && !J.enc && !J.dev_channel)
        k::unpack30(J.launch(ctx), blob.bytes, blob.len, reinterpret_cast<uint32_t*>(ctx->arena + J.lay.o_coef), J.sh.cs.n_padded, blob.bstride);
    ctx->phase_ms[5] = ms_since(t_entry);  // set-up before the first launch (workspace plan, twiddle lookup, ...) + that launch call
    init_transcripts(ctx, J, seeds);
    if (form.kind == ProveForm::BLOCK) rc = upload_block_table(ctx, J, form);
    if (rc == FRIEDA_OK) rc = J.dev_channel ? enqueue_device_channel(ctx, J, tw, blob) : run_host_channel(ctx, J, tw);
    if (rc) return rc;
    ctx->job = std::move(jp);
    return FRIEDA_OK;
}

int prove_begin(Ctx* ctx, const uint8_t* data, size_t len, bool data_on_device, const uint64_t* seed, frieda_pcs_config cfg) {
    return prove_begin_batch(ctx, data, 0, len, 1, data_on_device, seed, cfg);
}

// the same for `count` separate HOST blobs of one length (blob b at blobs[b]): what frieda_prove_many hands a device
int prove_begin_batch_ptrs(Ctx* ctx, const uint8_t* const* blobs, size_t len, uint32_t count, const uint64_t* seeds, frieda_pcs_config cfg) {
    if (!blobs || count == 0) return ctx->fail(FRIEDA_ERR_ARG, "null blob table");
    return prove_begin_batch(ctx, blobs[0], len, len, count, false, seeds, cfg, blobs);
}

// `count` blobs of `len` bytes each, blob b at data + b * data_stride (or, host blobs only, at host_ptrs[b]); seeds: null or one per blob
int prove_begin_batch(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, bool data_on_device,
                      const uint64_t* seeds, frieda_pcs_config cfg, const uint8_t* const* host_ptrs) {
    return prove_begin_impl(ctx, BlobsIn{data, data_stride, len, data_on_device, host_ptrs}, count, seeds, cfg, ProveForm{});
}

int prove_seeds_begin(Ctx* ctx, const Encoded* enc, const uint64_t* seeds, uint32_t n_seeds, frieda_pcs_config cfg) {
    if (!enc || !enc->d) return ctx->fail(FRIEDA_ERR_ARG, "null encoded blob");
    if (!seeds) return ctx->fail(FRIEDA_ERR_ARG, "null seeds");
    if (n_seeds == 0 || n_seeds > 65535) return ctx->fail(FRIEDA_ERR_ARG, "n_seeds out of range");
    if (cfg.log_blowup_factor != enc->log_blowup) return ctx->fail(FRIEDA_ERR_ARG, "log_blowup_factor differs from the one the blob was encoded with");
    if (enc->device != ctx->device) return ctx->fail(FRIEDA_ERR_ARG, "the encoded blob lives on another device");
    return prove_begin_impl(ctx, BlobsIn{nullptr, 0, enc->len, true, nullptr}, n_seeds, seeds, cfg, ProveForm{ProveForm::SEEDS, enc});
}

// The block form: n_seeds seeds (one list) of each of n_blobs encoded blobs of one shape, n_blobs * n_seeds jobs in one launch chain.
// One handle is prove_seeds itself.
int prove_seeds_blobs_begin(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, const uint64_t* seeds, uint32_t n_seeds, frieda_pcs_config cfg) {
    if (!encs) return ctx->fail(FRIEDA_ERR_ARG, "null list of encoded blobs");
    if (!seeds) return ctx->fail(FRIEDA_ERR_ARG, "null seeds");
    if (n_blobs == 0 || n_seeds == 0 || (uint64_t)n_blobs * n_seeds > 65535) return ctx->fail(FRIEDA_ERR_ARG, "n_blobs * n_seeds out of range");
    for (uint32_t b = 0; b < n_blobs; b++) {
        if (!encs[b] || !encs[b]->d) return ctx->fail(FRIEDA_ERR_ARG, "null encoded blob");
        if (encs[b]->len != encs[0]->len || encs[b]->log_blowup != encs[0]->log_blowup) return ctx->fail(FRIEDA_ERR_ARG, "the encoded blobs of a block have one length and one blowup");
        if (encs[b]->device != ctx->device) return ctx->fail(FRIEDA_ERR_ARG, "the encoded blob lives on another device");
    }
    if (cfg.log_blowup_factor != encs[0]->log_blowup) return ctx->fail(FRIEDA_ERR_ARG, "log_blowup_factor differs from the one the blobs were encoded with");
    if (n_blobs == 1) return prove_seeds_begin(ctx, encs[0], seeds, n_seeds, cfg);
    // the rectangle is the list that names every blob under every seed, blob-major: sorted as it stands
    const uint32_t n_jobs = n_blobs * n_seeds;
    std::vector<uint32_t> blob_of(n_jobs);
    std::vector<uint64_t> seed_of(n_jobs);
    for (uint32_t y = 0; y < n_jobs; y++) blob_of[y] = y / n_seeds, seed_of[y] = seeds[y % n_seeds];
    return prove_jobs_pass_begin(ctx, encs, blob_of.data(), seed_of.data(), n_jobs, n_blobs, nullptr, cfg);
}

// The list form: `n` jobs sorted by blob (sorted_blob[y] indexes encs and does not decrease), job y under sorted_seeds[y], in one launch
// chain.  The table holds the distinct blobs of the list; plan_blobs >= that many: the rows the arena is sized for.  One row planned is
// prove_seeds itself.  Every handle named was checked by the caller (prove_jobs_check, prove_seeds_blobs_begin)
int prove_jobs_pass_begin(Ctx* ctx, const Encoded* const* encs, const uint32_t* sorted_blob, const uint64_t* sorted_seeds, uint32_t n, uint32_t plan_blobs,
                          const uint32_t* out_slot, frieda_pcs_config cfg) {
    if (n == 0 || n > PROVE_JOBS_PASS_MAX) return ctx->fail(FRIEDA_ERR_ARG, "n_jobs out of range");
    if (plan_blobs == 1) return prove_seeds_begin(ctx, encs[sorted_blob[0]], sorted_seeds, n, cfg);  // (one blob: the stable sort moved nothing)
    ProveJobsRows rows;
    prove_jobs_rows(sorted_blob, n, rows);
    std::vector<const Encoded*> block(rows.blobs.size());
    for (size_t r = 0; r < block.size(); r++) block[r] = encs[rows.blobs[r]];
    std::vector<uint32_t> groups;
    prove_jobs_groups(rows.row_first, ctx->tuning.seeds_fold_group, groups);
    ProveForm form{ProveForm::BLOCK, block[0], block.data(), (uint32_t)block.size()};
    form.plan_blobs = std::max(plan_blobs, form.n_blobs);
    form.job_row = rows.job_row.data();
    form.row_first = rows.row_first.data();
    form.groups = groups.data();
    form.n_groups = (uint32_t)groups.size();
    form.out_slot = out_slot;
    return prove_begin_impl(ctx, BlobsIn{nullptr, 0, block[0]->len, true, nullptr}, n, sorted_seeds, cfg, form);
}

// the argument rules of a prove_jobs call, whole (a call cut into passes refuses what it refuses before its first pass)
int prove_jobs_check(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, const uint32_t* blob_index, const uint64_t* seeds, uint64_t n_jobs, frieda_pcs_config cfg) {
    FR_NO_JOB(ctx);
    if (!encs) return ctx->fail(FRIEDA_ERR_ARG, "null list of encoded blobs");
    if (!blob_index) return ctx->fail(FRIEDA_ERR_ARG, "null blob_index");
    if (!seeds) return ctx->fail(FRIEDA_ERR_ARG, "null seeds");
    if (n_blobs == 0 || n_jobs == 0) return ctx->fail(FRIEDA_ERR_ARG, "n_blobs or n_jobs is 0");
    for (uint32_t b = 0; b < n_blobs; b++) {
        if (!encs[b] || !encs[b]->d) return ctx->fail(FRIEDA_ERR_ARG, "null encoded blob");
        if (encs[b]->len != encs[0]->len || encs[b]->log_blowup != encs[0]->log_blowup) return ctx->fail(FRIEDA_ERR_ARG, "the encoded blobs of a block have one length and one blowup");
        if (encs[b]->device != ctx->device) return ctx->fail(FRIEDA_ERR_ARG, "the encoded blob lives on another device");
    }
    if (cfg.log_blowup_factor != encs[0]->log_blowup) return ctx->fail(FRIEDA_ERR_ARG, "log_blowup_factor differs from the one the blobs were encoded with");
    for (uint64_t j = 0; j < n_jobs; j++)
        if (blob_index[j] >= n_blobs) return ctx->fail(FRIEDA_ERR_ARG, "blob_index out of range");
    Shape sh;
    const Refusal refused = check_prove(encs[0]->len, cfg, sh);
    if (refused.code) return ctx->fail(refused.code, refused.text);
    if (n_jobs > 1 && (cfg.log_last_layer_degree_bound + cfg.log_blowup_factor > k::TAIL_LOG || ctx->host_channel))
        return ctx->fail(FRIEDA_ERR_ARG, "batches need the device channel (last layer <= 2^11 points, host channel policy off)");
    return FRIEDA_OK;
}

// the list sorted (prove_jobs_plan.h): order, and the blob and the seed of every sorted job
void prove_jobs_sorted(const uint32_t* blob_index, const uint64_t* seeds, size_t n_jobs, uint32_t n_blobs, std::vector<uint32_t>& order,
                       std::vector<uint32_t>& sorted_blob, std::vector<uint64_t>& sorted_seeds) {
    prove_jobs_sort(blob_index, n_jobs, n_blobs, order);
    sorted_blob.resize(n_jobs);
    sorted_seeds.resize(n_jobs);
    for (size_t y = 0; y < n_jobs; y++) sorted_blob[y] = blob_index[order[y]], sorted_seeds[y] = seeds[order[y]];
}

// one pass of everything, sized by the handles given (frieda_prove_jobs_workspace_bytes); the finish writes the caller's order
int prove_jobs_begin(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, const uint32_t* blob_index, const uint64_t* seeds, uint32_t n_jobs, frieda_pcs_config cfg) {
    int rc = prove_jobs_check(ctx, encs, n_blobs, blob_index, seeds, n_jobs, cfg);
    if (rc) return rc;
    if (n_jobs > PROVE_JOBS_PASS_MAX) return ctx->fail(FRIEDA_ERR_ARG, "n_jobs out of range");
    std::vector<uint32_t> order, sorted_blob;
    std::vector<uint64_t> sorted_seeds;
    prove_jobs_sorted(blob_index, seeds, n_jobs, n_blobs, order, sorted_blob, sorted_seeds);
    return prove_jobs_pass_begin(ctx, encs, sorted_blob.data(), sorted_seeds.data(), n_jobs, n_blobs, order.data(), cfg);
}

int prove_finish(Ctx* ctx, uint8_t out_commitment[32], ProofData& out) {
    if (ctx->job && ctx->job->count != 1) return ctx->fail(FRIEDA_ERR_ARG, "the proof in flight is a batch: use the batch finish");
    std::vector<ProofData> outs(1);
    outs[0] = std::move(out);  // assemble into the caller's object: a recycled one keeps its vectors' capacity
    int rc = prove_finish_batch(ctx, out_commitment, outs);
    if (!outs.empty()) out = std::move(outs[0]);
    return rc;
}

uint32_t job_count(const Ctx* ctx) { return ctx->job ? ctx->job->count : 0; }

// ---- prove_finish: the pieces, in the order they run ----
namespace {
// a job's openings, however they were made: the evaluations and then every layer's witness values; every layer's hash witness; the list sizes
struct Openings {
    struct LayerCounts {
        size_t n_witness, n_hashes;
    };
    std::vector<LayerCounts> counts;  // job b's layers at b * (1 + n_inner)
    std::vector<size_t> n_evals;
    std::vector<const uint32_t*> words_of;
    std::vector<const uint8_t*> hashes_of;
    Openings(uint32_t count, uint32_t n_layers) : counts((size_t)count * n_layers), n_evals(count), words_of(count), hashes_of(count) {}
};

// The first synchronisation of a proof: commit phase and grind done for every job (a job whose first range held no nonce gets further
// ones); then the downloaded transcript summaries -> ProveJob::Blob (nonce, channel, roots, alphas, last-layer polynomial)
int wait_for_transcripts(Ctx* ctx, ProveJob& J) {
    const k::Launch LN = J.launch(ctx);
    const uint32_t n_inner = J.lay.n_inner;
    const size_t n_poly = (size_t)1 << J.lay.last;
    auto host_transcript = [&](uint32_t b) { return reinterpret_cast<const DevTranscript*>(static_cast<const uint8_t*>(ctx->pinned) + b * J.lay.tr_host_pitch); };
    for (;;) {
        FR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool all_found = true;
        for (uint32_t b = 0; b < J.count; b++) {
            if (host_transcript(b)->status & 1u) return ctx->fail(FRIEDA_ERR_INVARIANT, "invalid degree");  // assert! upstream
            all_found &= host_transcript(b)->nonce != ~0ull;
        }
        if (all_found) break;
        // next range for the blobs still searching (the others leave at once: their minimum is below every new nonce)
        J.grind_base += J.grind_chunk;
        if (J.grind_chunk < ((uint64_t)1 << 28)) J.grind_chunk <<= 1;
        k::grind_dev(LN, reinterpret_cast<DevTranscript*>(ctx->arena + J.lay.o_tr), reinterpret_cast<uint32_t*>(ctx->arena + J.lay.o_gnext), J.cfg.pow_bits, J.grind_base, J.grind_chunk);
        int rc = download_transcripts(ctx, J);
        if (rc) return rc;
        if (J.dev_decommit) launch_decommit(ctx, J);
    }
    FR_HIP(ctx, hipGetLastError());
    for (uint32_t b = 0; b < J.count; b++) {
        const DevTranscript* ht = host_transcript(b);
        ProveJob::Blob& bl = J.blobs[b];
        if (ht->n_roots != 1 + n_inner || ht->n_last_poly != n_poly) return ctx->fail(FRIEDA_ERR_INVARIANT, "internal: transcript out of step");
        bl.nonce = ht->nonce;
        bl.ch = ht->ch;
        memcpy(bl.digest_before_grind, ht->ch.digest, 32);  // downloaded behind the grind, ahead of the decommit kernel
        bl.alphas.resize(1 + n_inner);
        for (uint32_t li = 0; li <= n_inner; li++) {
            for (int w = 0; w < 8; w++)
                for (int bb = 0; bb < 4; bb++) bl.roots[li][4 * w + bb] = (uint8_t)(ht->roots[li][w] >> (8 * bb));
            bl.alphas[li] = {ht->alphas[li][0], ht->alphas[li][1], ht->alphas[li][2], ht->alphas[li][3]};
        }
        bl.lastv.resize(n_poly);
        for (size_t i = 0; i < n_poly; i++)
            bl.lastv[i] = {ht->last_poly[4 * i], ht->last_poly[4 * i + 1], ht->last_poly[4 * i + 2], ht->last_poly[4 * i + 3]};
    }
    return FRIEDA_OK;
}

// the openings the device wrote behind the grind: per job a header with the list sizes, then the lists in proof order.  `complete` false:
// a job's table overflowed on the device, the host plans and gathers instead
int read_device_openings(Ctx* ctx, const ProveJob& J, Openings& op, bool& complete) {
    const uint32_t n = J.sh.n, n_inner = J.lay.n_inner;
    complete = true;
    for (uint32_t b = 0; b < J.count; b++) {
        const uint8_t* reg = static_cast<const uint8_t*>(ctx->pinned) + J.lay.dec_off + (size_t)b * J.lay.dec_stride;
        const uint32_t* hdr = reinterpret_cast<const uint32_t*>(reg);
        if (hdr[0] == k::DECOMMIT_OVERFLOW) {
            complete = false;
            return FRIEDA_OK;
        }
        if (hdr[0] != k::DECOMMIT_OK) return ctx->fail(FRIEDA_ERR_INVARIANT, "internal: device decommit out of step with the grind");
        op.n_evals[b] = hdr[1];
        op.words_of[b] = reinterpret_cast<const uint32_t*>(reg + J.lay.dec_words_off);
        op.hashes_of[b] = reg + J.lay.dec_hashes_off;
        Openings::LayerCounts* cnt = &op.counts[(size_t)b * (1 + n_inner)];
        // layer li: n_witness = |E_{li+1}|, n_hashes = |E_{li+2}| + ... + |E_n|   (hdr[3 + s] = |E_s|)
        size_t suffix[40] = {0};  // suffix[s] = |E_s| + ... + |E_n|, s <= n + 1 <= 33
        for (uint32_t sft = n; sft >= 1; sft--) suffix[sft] = suffix[sft + 1] + hdr[3 + sft];
        for (uint32_t li = 0; li <= n_inner; li++) {
            cnt[li].n_witness = hdr[3 + li + 1];
            cnt[li].n_hashes = li + 2 <= n ? suffix[li + 2] : 0;
        }
    }
    return FRIEDA_OK;
}

// FriProver::decommit by the host (more than 1024 queries, an opening table too large for the kernel, FRIEDA_HOST_DECOMMIT): it draws the
// queries, plans the openings and runs one gather.  It plans against COMPLETE trees; the large ones were built without the two levels
// above their leaves (the device decommitment re-hashes those, tree.hip TreeArgs::skip_bc): such a tree is rebuilt from its layer's values
// first (a rare path).  An encoded blob is only ever read (other contexts may be proving from it): when ITS tree lacks those levels a
// complete copy is built in a temporary allocation and layer 0's hashes are gathered from there.  One handle is a block of one row
int host_decommit(Ctx* ctx, ProveJob& J, Openings& op) {
    hipStream_t s = ctx->stream;
    uint8_t* A = ctx->arena;
    const ProveLayout& Y = J.lay;
    const uint32_t n = J.sh.n, n_inner = J.lay.n_inner, count = J.count;
    const size_t N = J.sh.N;
    // the rows of first layers the jobs read: none (the arena's own), the handle, or the block's; row r's jobs are [row_first[r], row_first[r + 1])
    const Encoded* const one_row[1] = {J.enc};
    const uint32_t one_first[2] = {0, count};
    const Encoded* const* rows = J.block.empty() ? one_row : J.block.data();
    const uint32_t* row_first = J.block.empty() ? one_first : J.row_first.data();
    const size_t n_rows = J.block.empty() ? (J.enc ? 1 : 0) : J.block.size();
    // one complete copy per DISTINCT blob that needs one (a handle may be listed more than once), freed when the call leaves, by whichever path
    std::vector<DevBuf> row_full(n_rows);
    std::vector<const uint8_t*> row_tree(n_rows, nullptr);
    for (size_t r = 0; r < n_rows; r++) {
        const Encoded* e = rows[r];
        row_tree[r] = e->tree();
        if (Y.first.log < e->skip_log) continue;
        size_t seen = r;
        for (size_t q = 0; q < r && seen == r; q++)
            if (rows[q]->d == e->d) seen = q;
        if (seen != r) {
            row_tree[r] = row_tree[seen];
            continue;
        }
        const int arc = row_full[r].alloc(ctx, k::merkle_layer_offset(n, 0) + 32, "poison(complete first-layer tree)");
        if (arc != FRIEDA_OK) {
            (void)hipStreamSynchronize(s);  // (the copies built so far are being written)
            return arc == FRIEDA_ERR_NOMEM ? ctx->fail(FRIEDA_ERR_NOMEM, "no device memory for the complete first-layer tree of the host decommitment") : arc;
        }
        const uint32_t* c0 = e->eval();
        k::merkle_tree4(ctx->launch(), c0, c0 + N, c0 + 2 * N, c0 + 3 * N, n, static_cast<uint8_t*>(row_full[r].p));
        row_tree[r] = static_cast<const uint8_t*>(row_full[r].p);
    }
    // (from here on every exit waits for the stream before the copies go: fail_synced)
    auto fail_synced = [&](int rc_) {
        if (n_rows) (void)hipStreamSynchronize(s);
        return rc_;
    };
    {
        k::Launch Lb = ctx->launch();  // single-blob launches
        for (uint32_t b = 0; b < count; b++) {
            const size_t boff = (size_t)b * Y.bstride;
            auto rebuild = [&](const FriLayerDev& lay) {
                if (lay.log < J.skip_log) return;
                const uint32_t* c0 = reinterpret_cast<const uint32_t*>(A + lay.o_vals + boff);
                const size_t cs = (size_t)1 << lay.log;
                k::merkle_tree4(Lb, c0, c0 + cs, c0 + 2 * cs, c0 + 3 * cs, lay.log, A + lay.o_tree + boff);
            };
            if (!J.enc) rebuild(Y.first);
            for (uint32_t kx = 0; kx < n_inner; kx++) rebuild(Y.inner[kx]);
        }
    }
    static thread_local GatherPlan g;  // capacity is kept from proof to proof
    g.word_idx.clear();
    g.hash_idx.clear();
    std::vector<size_t> w_begin(count), h_begin(count);
    for (uint32_t b = 0; b < count; b++) {
        ProveJob::Blob& bl = J.blobs[b];
        bl.ch.mix_u64(bl.nonce);  // src/proof.rs:59
        const std::vector<uint32_t> queries = generate_queries(bl.ch, n, J.cfg.n_queries);
        op.n_evals[b] = queries.size();
        w_begin[b] = g.word_idx.size();
        h_begin[b] = g.hash_idx.size();
        const size_t boff = (size_t)b * Y.bstride;  // this blob's workspace (a multiple of 256 bytes)
        auto shifted = [&](FriLayerDev lay) {
            lay.o_vals += boff;
            lay.o_tree += boff;
            return lay;
        };
        Openings::LayerCounts* cnt = &op.counts[(size_t)b * (1 + n_inner)];
        // Proof.evaluations (src/proof.rs:62-66)
        // (an encoded blob: `first` holds offsets 0 — indices relative to the handle's columns / tree, marked GATHER_ALT)
        const uint64_t tag0 = J.enc ? k::GATHER_ALT : 0;
        const FriLayerDev lay0 = J.enc ? Y.first : shifted(Y.first);
        for (uint32_t q : queries)
            for (int c = 0; c < 4; c++) g.word_idx.push_back((lay0.o_vals / 4 + (size_t)c * N + q) | tag0);
        {
            std::vector<uint32_t> pos = plan_witness(queries, lay0, g, cnt[0].n_witness, tag0);
            cnt[0].n_hashes = plan_merkle_decommit(pos, lay0, g, tag0);
        }
        std::vector<uint32_t> lq = fold_queries(queries, 1);
        for (uint32_t kx = 0; kx < n_inner; kx++) {
            const FriLayerDev lay = shifted(Y.inner[kx]);
            std::vector<uint32_t> pos = plan_witness(lq, lay, g, cnt[kx + 1].n_witness);
            cnt[kx + 1].n_hashes = plan_merkle_decommit(pos, lay, g);
            lq = fold_queries(lq, 1);
        }
    }
    ctx->phase_ms[2] = ms_since(J.t_start);  // queries drawn, openings planned
    if (g.word_idx.size() > Y.max_words || g.hash_idx.size() > Y.max_hashes) return fail_synced(ctx->fail(FRIEDA_ERR_INVARIANT, "internal: gather plan overflow"));
    // one upload (word indices then hash indices, staged in pinned memory), one launch, one download
    const size_t nw = g.word_idx.size(), nh = g.hash_idx.size();
    const size_t wbytes = 4 * nw, out_bytes = wbytes + 32 * nh;
    uint8_t* hp = reinterpret_cast<uint8_t*>(ctx->pinned);
    uint64_t* hidx = reinterpret_cast<uint64_t*>(hp + Y.gather_off);
    memcpy(hidx, g.word_idx.data(), 8 * nw);
    memcpy(hidx + nw, g.hash_idx.data(), 8 * nh);
    // the index and output regions of the arena are laid out back to back (words region, then hashes region), so the
    // hash part may start right behind the words actually used
    k::Launch L1 = ctx->launch();  // the gather works on absolute indices: a single-blob launch
    // the tagged indices of row r's jobs (consecutive in both lists) are relative to THAT handle — one launch per row over the row's
    // slices of the lists (one handle: one launch over the whole lists); the untagged ones go through the arena base as ever
    auto gather_all = [&](const uint64_t* widx, uint32_t* wout, const uint64_t* hidx_, uint8_t* hout) {
        if (!n_rows) k::gather(L1, reinterpret_cast<const uint32_t*>(A), widx, nw, wout, hidx_, nh, hout, nullptr, nullptr);
        for (size_t r = 0; r < n_rows; r++) {
            const size_t j0 = row_first[r], j1 = row_first[r + 1];
            if (j0 == j1) continue;
            const size_t w0 = w_begin[j0], w1 = j1 < count ? w_begin[j1] : nw, h0 = h_begin[j0], h1 = j1 < count ? h_begin[j1] : nh;
            k::gather(L1, reinterpret_cast<const uint32_t*>(A), widx + w0, w1 - w0, wout + w0, hidx_ + h0, h1 - h0, hout + 32 * h0, rows[r]->eval(), row_tree[r]);
        }
    };
    if (out_bytes <= ((size_t)1 << 20) && !ctx->tuning.gather_copy) {
        // small openings (the usual case): the kernel reads its index lists from, and writes its results to, the pinned
        // staging block directly over PCIe — one launch instead of copy + launch + copy (each copy costs 10-20 us of setup)
        gather_all(hidx, reinterpret_cast<uint32_t*>(hp), hidx + nw, hp + wbytes);
    } else {
        if (const hipError_t ce = hipMemcpyAsync(A + Y.o_widx, hidx, 8 * (nw + nh), hipMemcpyHostToDevice, s); ce != hipSuccess)
            return fail_synced(ctx->hip_fail(ce, "hipMemcpyAsync(gather lists)"));
        gather_all(reinterpret_cast<const uint64_t*>(A + Y.o_widx), reinterpret_cast<uint32_t*>(A + Y.o_wout),
                   reinterpret_cast<const uint64_t*>(A + Y.o_widx) + nw, A + Y.o_wout + wbytes);
        if (const hipError_t ce = hipMemcpyAsync(hp, A + Y.o_wout, out_bytes, hipMemcpyDeviceToHost, s); ce != hipSuccess)
            return fail_synced(ctx->hip_fail(ce, "hipMemcpyAsync(gathered openings)"));
    }
    FR_HIP(ctx, hipStreamSynchronize(s));
    FR_HIP(ctx, hipGetLastError());
    ctx->phase_ms[3] = ms_since(J.t_start);  // gather done (second and last synchronise)
    for (uint32_t b = 0; b < count; b++) {
        op.words_of[b] = reinterpret_cast<const uint32_t*>(hp) + w_begin[b];
        op.hashes_of[b] = hp + wbytes + 32 * h_begin[b];
    }
    return FRIEDA_OK;
}

// the Proofs (src/proof.rs:67-76) from the transcripts and the openings
void assemble_proofs(ProveJob& J, const Openings& op, uint8_t* out_commitments, std::vector<ProofData>& outs) {
    const uint32_t n_inner = J.lay.n_inner, count = J.count;
    if (outs.size() != count) outs.assign(count, ProofData{});  // else: the caller's (recycled) objects, every field rewritten below
    for (uint32_t b = 0; b < count; b++) {
        ProveJob::Blob& bl = J.blobs[b];
        const size_t slot = J.out_slot.empty() ? b : J.out_slot[b];
        ProofData& out = outs[slot];
        const Openings::LayerCounts* cnt = &op.counts[(size_t)b * (1 + n_inner)];
        const uint32_t* wv = op.words_of[b];
        const uint8_t* hv = op.hashes_of[b];
        size_t wi = 0, hi = 0;
        auto take_qm = [&]() {
            QM31 q{wv[wi], wv[wi + 1], wv[wi + 2], wv[wi + 3]};
            wi += 4;
            return q;
        };
        out.pcs_config = J.cfg;
        out.log_size_bound = J.sh.L;
        out.proof_of_work = bl.nonce;
        out.last_layer_poly = std::move(bl.lastv);
        out.evaluations.resize(op.n_evals[b]);
        for (auto& q : out.evaluations) q = take_qm();
        out.inner_layers.resize(n_inner);
        for (uint32_t li = 0; li <= n_inner; li++) {
            LayerProof& lp = li == 0 ? out.first_layer : out.inner_layers[li - 1];
            lp.commitment = bl.roots[li];
            lp.fri_witness.resize(cnt[li].n_witness);
            for (auto& q : lp.fri_witness) q = take_qm();
            lp.hash_witness.resize(cnt[li].n_hashes);
            if (cnt[li].n_hashes) memcpy(lp.hash_witness.data(), hv + 32 * hi, 32 * cnt[li].n_hashes);
            hi += cnt[li].n_hashes;
            lp.column_witness.clear();
        }
        memcpy(out_commitments + 32 * slot, bl.roots[0].data(), 32);
    }
}
}  // namespace

int prove_finish_batch(Ctx* ctx, uint8_t* out_commitments, std::vector<ProofData>& outs) {
    if (!ctx->job) return ctx->fail(FRIEDA_ERR_ARG, "no proof in flight on this context");
    std::unique_ptr<ProveJob, ProveJobDeleter> jp = std::move(ctx->job);  // released on every exit path
    ProveJob& J = *jp;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if (J.dev_channel) {
        rc = wait_for_transcripts(ctx, J);
        if (rc) return rc;
    }
    ctx->phase_ms[1] = ms_since(J.t_start);  // commit phase + grind complete on the device (first synchronise)
    ctx->last_transcript.roots = J.blobs[0].roots;
    ctx->last_transcript.alphas = J.blobs[0].alphas;
    memcpy(ctx->last_transcript.digest_before_grind, J.blobs[0].digest_before_grind, 32);

    // ---- FriProver::decommit: normally the device has already done it (launched behind the grind) ----
    Openings op(J.count, 1 + J.lay.n_inner);
    bool from_device = J.dev_decommit;
    if (from_device) {
        rc = read_device_openings(ctx, J, op, from_device);
        if (rc) return rc;
        ctx->phase_ms[2] = ctx->phase_ms[3] = ms_since(J.t_start);
    }
    if (!from_device) {
        rc = host_decommit(ctx, J, op);
        if (rc) return rc;
    }
    assemble_proofs(J, op, out_commitments, outs);
    ctx->phase_ms[4] = ms_since(J.t_start);  // proofs assembled
    return FRIEDA_OK;
}

int prove(Ctx* ctx, const uint8_t* data, size_t len, bool data_on_device, const uint64_t* seed, frieda_pcs_config cfg,
          uint8_t out_commitment[32], ProofData& out) {
    int rc = prove_begin(ctx, data, len, data_on_device, seed, cfg);
    if (rc) return rc;
    return prove_finish(ctx, out_commitment, out);
}

// -------------------------------------------------------------------------------------------------
// one blob under many seeds: the encoded blob (host.h)
// -------------------------------------------------------------------------------------------------
size_t encoded_bytes(uint32_t n, size_t* o_tree, size_t* o_root) {
    ArenaPlan plan;
    plan.take(sizeof(uint32_t) * 4 << n);
    const size_t ot = plan.take(k::merkle_layer_offset(n, 0) + 32);
    const size_t orr = plan.take(32);
    if (o_tree) *o_tree = ot;
    if (o_root) *o_root = orr;
    return plan.off;
}

namespace {
// the slab's injected free (encoded_slab.h): on the slab's device, the caller's current device restored
void slab_hip_free(void* base, int device) {
    int cur = 0;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != device;
    if (sw) (void)hipSetDevice(device);
    (void)hipFree(base);
    if (sw) (void)hipSetDevice(cur);
}
}  // namespace

void encoded_release(Encoded& e) {
    if (!e.d) return;
    if (e.slab) slab_drop(e.slab);
    e.slab = nullptr;
    e.d = nullptr;
}

int EncodedBlock::alloc(Ctx* ctx, size_t len, uint32_t log_blowup, uint32_t L, uint32_t n, uint32_t count, uint32_t skip_log) {
    size_t o_tree = 0, o_root = 0;
    bstride = encoded_bytes(n, &o_tree, &o_root);
    e.assign(count, Encoded());  // (before the allocation: nothing to undo when the host is out of memory)
    uint8_t* base = nullptr;
    if (hipMalloc((void**)&base, bstride * count) != hipSuccess) {
        (void)hipGetLastError();
        e.clear();
        return ctx->fail(FRIEDA_ERR_NOMEM, "hipMalloc(encoded blob" + std::string(count > 1 ? "s " : " ") + std::to_string(bstride * count) + " B) failed");
    }
    EncodedSlab* slab = nullptr;
    try {
        slab = slab_create(base, ctx->device, count, slab_hip_free);
    } catch (...) {
        (void)hipFree(base);
        e.clear();
        throw;
    }
    for (uint32_t b = 0; b < count; b++) {
        Encoded& x = e[b];
        x.device = ctx->device;
        x.len = len;
        x.log_blowup = log_blowup;
        x.n = n;
        x.L = L;
        x.skip_log = skip_log;
        x.slab = slab;
        x.d = base + (size_t)b * bstride;
        x.bytes = bstride;
        x.o_tree = o_tree;
        x.o_root = o_root;
    }
    FR_HIP(ctx, ctx->poison_fresh(base, bstride * count));
    return FRIEDA_OK;
}

int EncodedBlock::publish(const uint8_t* roots, frieda_encoded** out) {
    std::vector<frieda_encoded*> hs(e.size(), nullptr);
    for (size_t b = 0; b < e.size(); b++) {
        hs[b] = new (std::nothrow) frieda_encoded();
        if (!hs[b]) {
            for (size_t i = 0; i < b; i++) delete hs[i];
            return FRIEDA_ERR_NOMEM;
        }
    }
    for (size_t b = 0; b < e.size(); b++) {
        memcpy(e[b].root, roots + 32 * b, 32);
        hs[b]->e = e[b];  // the handle holds the reference from here on
        e[b].d = nullptr;
        e[b].slab = nullptr;
        out[b] = hs[b];
    }
    return FRIEDA_OK;
}
void encoded_free(Encoded* e) {
    if (!e) return;
    encoded_release(*e);
    delete e;
}

int encode_blob(Ctx* ctx, const uint8_t* data, size_t len, bool data_on_device, uint32_t log_blowup, Encoded** out) {
    FR_NO_JOB(ctx);
    Shape sh;
    int rc = make_shape(ctx, len, log_blowup, sh);
    if (rc) return rc;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    // the arena holds what encoding needs and the handle does not keep: the blob (a host blob) and the coefficients
    ArenaPlan plan;
    const size_t o_data = plan.take(data_on_device ? 0 : len);
    const size_t o_coef = plan.take(sizeof(uint32_t) * sh.cs.n_padded);
    TwiddleSet tw;
    rc = ctx->ensure_arena(plan.off);
    if (rc == FRIEDA_OK) rc = ensure_pinned(ctx, 4096);
    if (rc == FRIEDA_OK) rc = ctx->get_twiddles(sh.n, tw);
    if (rc) return rc;
    std::unique_ptr<Encoded, void (*)(Encoded*)> e(new Encoded(), encoded_free);
    {
        // the slab of one.  A lone launch builds the tree: the threshold of a call of one blob (what k::build_tree applies to a Launch of batch 1)
        EncodedBlock one;
        rc = one.alloc(ctx, len, log_blowup, sh.L, sh.n, 1, k::tree_skip_threshold(ctx->tuning, 1));
        if (rc) return rc;
        *e = one.e[0];
        one.e.clear();  // (the reference moved to *e)
    }
    hipStream_t s = ctx->stream;
    uint8_t* A = ctx->arena;
    const uint8_t* d_data = data;
    if (!data_on_device) {
        rc = upload_blobs(ctx, BlobsIn{data, 0, len, false, nullptr}, 1, A + o_data, 0);
        if (rc) return rc;
        d_data = A + o_data;
    }
    encode_first_tree(ctx->launch(), sh, tw, k::BlobSource{d_data, len, 0, sh.cs.n_padded},
                      EncodeDest{reinterpret_cast<uint32_t*>(A + o_coef), reinterpret_cast<uint32_t*>(e->d), sh.N, e->d + e->o_tree, nullptr, e->d + e->o_root, nullptr,
                                 nullptr, 0});
    FR_HIP(ctx, hipMemcpyAsync(ctx->pinned, e->d + e->o_root, 32, hipMemcpyDeviceToHost, s));
    FR_HIP(ctx, hipStreamSynchronize(s));
    FR_HIP(ctx, hipGetLastError());
    memcpy(e->root, ctx->pinned, 32);
    *out = e.release();
    return FRIEDA_OK;
}

// commit_batch_begin with everything kept.  The kernels take ONE batch stride for every pointer but the blob's (BlobSource has its own),
// and what they write — evaluation, tree, root — sits in the slab at encoded_bytes(n) per blob: so the launches run at the slab's
// stride.  The arena holds the blobs back to back at their own stride and, for the general route, the coefficients at the slab's stride
// (blob b's 4 * 2^L words at b * bstride: the gaps are address space the call never touches; the fused small route keeps no coefficients).
int encode_batch(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, uint32_t log_blowup, frieda_encoded** out_encs) {
    FR_NO_JOB(ctx);
    if (count == 0 || count > 65535) return ctx->fail(FRIEDA_ERR_ARG, "batch count out of range");
    if (count > 1 && data_stride < len) return ctx->fail(FRIEDA_ERR_ARG, "batch stride smaller than the blob length");
    Shape sh;
    int rc = make_shape(ctx, len, log_blowup, sh);
    if (rc) return rc;
    FR_HIP(ctx, hipSetDevice(ctx->device));
    const bool small = k::small_domain_shape(ctx->tuning, sh.L, sh.n);
    const size_t bstride = encoded_bytes(sh.n);
    const size_t dstride = std::max<size_t>(256, (len + 255) & ~(size_t)255);
    ArenaPlan plan;
    const size_t o_data = plan.take(dstride * count);
    const size_t o_coef = plan.take(small ? 0 : bstride * (count - 1) + sizeof(uint32_t) * sh.cs.n_padded);
    TwiddleSet tw;
    rc = ctx->ensure_arena(plan.off);
    if (rc == FRIEDA_OK) rc = ensure_pinned(ctx, 32 * (size_t)count + 4096);
    if (rc == FRIEDA_OK) rc = ctx->get_twiddles(sh.n, tw);
    if (rc) return rc;
    EncodedBlock blk;
    rc = blk.alloc(ctx, len, log_blowup, sh.L, sh.n, count, k::tree_skip_threshold(ctx->tuning, count));
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint8_t* A = ctx->arena;
    uint8_t* S = blk.base();
    const size_t o_tree = blk.e[0].o_tree, o_root = blk.e[0].o_root;
    k::Launch LN = ctx->launch();
    LN.batch = count;
    LN.bstride = count > 1 ? bstride : 0;
    auto run = [&]() -> int {
        int urc = upload_blobs(ctx, BlobsIn{data, data_stride, len, false, nullptr}, count, A + o_data, dstride, /*lone_as_row=*/true);
        if (urc) return urc;
        encode_first_tree(LN, sh, tw, k::BlobSource{A + o_data, len, dstride, sh.cs.n_padded},
                          EncodeDest{reinterpret_cast<uint32_t*>(A + o_coef), reinterpret_cast<uint32_t*>(S), sh.N, S + o_tree, nullptr, S + o_root, nullptr, nullptr, 0});
        FR_HIP(ctx, hipMemcpy2DAsync(ctx->pinned, 32, S + o_root, bstride, 32, count, hipMemcpyDeviceToHost, s));
        FR_HIP(ctx, hipStreamSynchronize(s));
        FR_HIP(ctx, hipGetLastError());
        return FRIEDA_OK;
    };
    rc = run();
    if (rc != FRIEDA_OK) {
        (void)hipStreamSynchronize(s);  // (before the slab goes)
        return rc;
    }
    rc = blk.publish(static_cast<const uint8_t*>(ctx->pinned), out_encs);
    return rc == FRIEDA_OK ? rc : ctx->fail(rc, "host allocation failed");
}

// what prove_begin_impl plans for a prove_seeds job (prove_layout)
size_t seeds_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_seeds) {
    if (n_seeds == 0 || n_seeds > 65535) return 0;
    return prove_arena_bytes(len, cfg, n_seeds, ProveForm{ProveForm::SEEDS});
}

// ... and for a prove_seeds_blobs job: the same plan at n_blobs * n_seeds jobs, then the block table (rows, a row number per job, the
// entry of every group of jobs at their largest count).  One blob is prove_seeds, table and all
size_t seeds_blobs_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint32_t n_seeds) {
    if (n_blobs == 0 || n_seeds == 0 || (uint64_t)n_blobs * n_seeds > 65535) return 0;
    if (n_blobs == 1) return seeds_workspace_bytes(len, cfg, n_seeds);
    return prove_jobs_workspace_bytes(len, cfg, n_blobs, n_blobs * n_seeds);
}

// ... and for a pass of prove_jobs: a function of the two counts alone (the rectangle K x S is the list (K, K * S))
size_t prove_jobs_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint32_t n_jobs) {
    if (n_blobs == 0 || n_jobs == 0 || n_jobs > PROVE_JOBS_PASS_MAX) return 0;
    if (n_blobs == 1) return seeds_workspace_bytes(len, cfg, n_jobs);
    ProveForm form{ProveForm::BLOCK, nullptr, nullptr, n_blobs};
    form.plan_blobs = n_blobs;
    return prove_arena_bytes(len, cfg, n_jobs, form);
}

// the pass rule of frieda_prove_jobs (prove_jobs_plan.h) under `limit` bytes; 0: a refused shape
uint32_t prove_jobs_per_pass_under(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint64_t n_jobs, uint64_t limit) {
    if (!prove_jobs_workspace_bytes(len, cfg, 1, 1) || n_blobs == 0 || n_jobs == 0) return 0;
    return prove_jobs_per_pass(n_jobs, n_blobs, limit, [&](uint32_t kb, uint32_t p) { return prove_jobs_workspace_bytes(len, cfg, kb, p); });
}
uint64_t prove_jobs_limit(const k::Tuning& t) {
    const uint64_t budget = batch_budget_bytes(t);
    return t.test_arena_limit && t.test_arena_limit < budget ? t.test_arena_limit : budget;
}

}  // namespace frieda
