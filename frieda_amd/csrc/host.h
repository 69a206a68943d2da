// host.h — host-side data structures of libfrieda_hip: context, proof container, prover / verifier entry points.
// C++ mirror of the Rust types frieda exposes (/root/reference/src/proof.rs:19-26, src/lib.rs:22-44); the C ABI in
// include/frieda_hip.h is a thin shell over these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/frieda_hip.h"
#include "channel.h"
#include "encoded_slab.h"
#include "field.h"
#include "kernels.h"

namespace frieda {

using Hash32 = std::array<uint8_t, 32>;

// stwo FriLayerProof { fri_witness, decommitment: MerkleDecommitment { hash_witness, column_witness }, commitment }
struct LayerProof {
    std::vector<QM31> fri_witness;
    std::vector<Hash32> hash_witness;
    std::vector<uint32_t> column_witness;
    Hash32 commitment{};
};

// frieda::proof::Proof (src/proof.rs:19-26) with stwo's FriProof flattened in
struct ProofData {
    LayerProof first_layer;
    std::vector<LayerProof> inner_layers;
    std::vector<QM31> last_layer_poly;  // LinePoly coefficients in stwo's internal (bit-reversed) order
    uint64_t proof_of_work = 0;
    frieda_pcs_config pcs_config{};
    uint32_t log_size_bound = 0;
    std::vector<QM31> evaluations;
};

std::vector<uint8_t> serialize_proof(const ProofData& p);
bool deserialize_proof(const uint8_t* buf, size_t len, ProofData& out);

// ---- circle-group helpers on the host (index arithmetic mod 2^31, stwo core/circle.rs) ----
struct Coset {
    uint32_t initial, step, log_size;
    static Coset half_odds(uint32_t log_size);
    Coset doubled() const;
    uint32_t index_at(uint32_t i) const;
    CPoint at(uint32_t i) const;
};
CPoint point_from_index(uint32_t index);
// coset of the FRI line layer of log size m inside the circle domain of log size n
Coset line_coset(uint32_t n, uint32_t m);

// shape of polynomial_from_bytes (src/utils.rs:21-33) by integer arithmetic
struct CodecShape {
    size_t n_felts, n_padded;
    uint32_t log_size;  // L: per-column log size
};
CodecShape codec_shape(size_t len);

// ---- device context ----
struct TwiddleSet {
    uint32_t* d_tw = nullptr;
    uint32_t* d_itw = nullptr;
    void* d_scratch = nullptr;  // 8 KiB for the generator's point table
    k::DomainScalars ds{};
};

struct ProveJob;  // state of a proof between prove_begin and prove_finish (prover.cpp)
struct ProveJobDeleter {
    void operator()(ProveJob* j) const;
};

// per-kernel HIP-event timer: events are recorded on the ctx stream around each launch; durations are read back
// (after a stream synchronise) by report()
struct KernelTimerImpl;

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool cache_twiddles = true;
    k::Tuning tuning = k::tuning_from_env();  // per-context knobs (kernels.h): environment defaults, frieda_ctx_set_option overrides
    uint32_t test_draw_bound = 2u * P31;  // test hook: acceptance bound of draw_felt (see frieda_ctx_test_set_draw_bound)
    bool host_channel = false;  // evaluate the Fiat-Shamir channel on the host between layers (diagnostic / fallback path)
    std::map<uint32_t, TwiddleSet> twiddles;
    uint8_t* arena = nullptr;
    size_t arena_bytes = 0;
    void* pinned = nullptr;  // small pinned staging block for D2H of roots / nonces
    size_t pinned_bytes = 0;
    void* pinned_in = nullptr;  // page-locked input block for lone small host blobs (read by the fused small-domain kernel in place)
    std::string err;
    std::string notes;  // what context creation degraded (refused LDS opt-ins ...), one line each: frieda_ctx_notes — never in `err`
    double phase_ms[8] = {0};  // host wall-clock marks of the last prove() (ms since entry): enqueued, device done, queries, gather, assembled
    KernelTimerImpl* timer = nullptr;  // non-null while kernel timing is enabled
    std::unique_ptr<ProveJob, ProveJobDeleter> job;  // the proof in flight, if any
    uint32_t commit_pending = 0;  // roots of a commit_batch_begin not yet collected by commit_batch_finish (they sit in `pinned`)
    // Fiat-Shamir transcript of the last finished proof (blob 0 of a batch), kept for frieda_ctx_last_transcript
    struct LastTranscript {
        std::vector<Hash32> roots;                      // one per FRI layer (first + inner)
        std::vector<std::array<uint32_t, 4>> alphas;    // the folding challenge drawn after each root
        uint32_t digest_before_grind[8] = {0};          // channel digest after mix_felts(last_layer_poly)
    } last_transcript;

    k::Launch launch() const;
    int set_kernel_timing(bool enabled);
    std::string kernel_timing_report(bool reset);  // JSON; synchronises the stream

    int fail(int code, const std::string& what);
    int hip_fail(hipError_t e, const char* what);
    int ensure_arena(size_t bytes);
    // test hook (frieda_ctx_test_poison): fill `bytes` of device memory with `word` on the ctx stream; a page-locked host block is
    // filled by the host once the stream has drained (nothing of the context is in flight on it: FR_NO_JOB)
    hipError_t poison_device(void* d, size_t bytes, uint32_t word);
    hipError_t poison_pinned(void* p, size_t bytes, uint32_t word);
    // the sticky mode's sites: a no-op unless tuning.test_poison; `d` is an allocation the context has just made for itself
    hipError_t poison_fresh(void* d, size_t bytes) { return tuning.test_poison ? poison_device(d, bytes, tuning.test_poison_word) : hipSuccess; }
    hipError_t poison_fresh_pinned(void* p, size_t bytes) { return tuning.test_poison ? poison_pinned(p, bytes, tuning.test_poison_word) : hipSuccess; }
    int get_twiddles(uint32_t n, TwiddleSet& out);
    void drop_twiddles();
    ~Ctx();
};

#define FR_HIP(ctx, expr)                                            \
    do {                                                             \
        hipError_t e__ = (expr);                                     \
        if (e__ != hipSuccess) return (ctx)->hip_fail(e__, #expr);   \
    } while (0)

// One proof (or batch) may be in flight per context between prove_begin and prove_finish: its workspace offsets point into the
// arena and its transcript summary sits in the pinned block.  Every other entry point that (re)allocates or writes either of
// them refuses to run meanwhile.
#define FR_NO_JOB(ctx)                                                                                                 \
    do {                                                                                                               \
        if ((ctx)->job || (ctx)->commit_pending)                                                                        \
            return (ctx)->fail(FRIEDA_ERR_ARG, "a proof is in flight on this context (finish it first, or use another context)"); \
    } while (0)

// bump allocator over the ctx arena (sizes are planned before ensure_arena)
struct ArenaPlan {
    size_t off = 0;
    size_t take(size_t bytes) {
        size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    }
};

// Device memory of one call (pools, rebuilt bytes): freed when it leaves scope, whichever way.  Not for what outlives a call (Encoded, the
// arena, the twiddle sets: they have their own owners).  The destructor does not wait for the stream: a path that launched work on
// the buffer synchronises before it lets go.
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    // hipMalloc + poison_fresh; poison_what: the text of a failed poison fill (test hook)
    int alloc(Ctx* ctx, size_t bytes, const char* poison_what) {
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();  // (not sticky for the next call)
            ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
            return FRIEDA_ERR_NOMEM;
        }
        if (const hipError_t pe = ctx->poison_fresh(p, bytes); pe != hipSuccess) return ctx->hip_fail(pe, poison_what);
        return FRIEDA_OK;
    }
};

// A call's pool of verified samples on the device, in the layout the point reconstruction reads: an index block (256-byte rounded),
// then `entry_bytes` of values per entry.  Outside the arena: the verify passes and the reconstruction re-plan that.
struct DevPool {
    DevBuf buf;
    size_t cap = 0, n = 0;  // entries allocated / pooled
    static size_t index_bytes(size_t cap) { return (4 * cap + 255) & ~(size_t)255; }
    uint32_t* d_idx() const { return static_cast<uint32_t*>(buf.p); }
    uint32_t* d_val() const { return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf.p) + index_bytes(cap)); }
    int alloc(Ctx* ctx, size_t entries, size_t entry_bytes, const char* poison_what) {
        cap = entries;
        return buf.alloc(ctx, index_bytes(cap) + entry_bytes * cap, poison_what);
    }
};

// the size of Ctx::pinned_in (prover.cpp)
constexpr size_t SMALL_HOST_IN_BYTES = 7680;  // 15 << 9: up to 32 workgroups read the block over PCIe; larger small blobs are copied to the device first
// the pinned staging block (Ctx::pinned) of at least `bytes` (reallocated when smaller; callers hold no job: FR_NO_JOB)
int ensure_pinned(Ctx* ctx, size_t bytes);

// ---- prover / verifier ----
int commit_device(Ctx* ctx, const uint8_t* d_data, size_t len, uint32_t log_blowup, uint8_t* d_root, bool data_in_arena);
int commit_host(Ctx* ctx, const uint8_t* data, size_t len, uint32_t log_blowup, uint8_t out_root[32]);
int prove(Ctx* ctx, const uint8_t* data, size_t len, bool data_on_device, const uint64_t* seed, frieda_pcs_config cfg,
          uint8_t out_commitment[32], ProofData& out);
// split form: prove_begin enqueues the whole commit phase and returns without synchronising; prove_finish waits for it,
// opens the queries and assembles the proof.  One proof in flight per ctx; use several ctxs to overlap proofs.
int prove_begin(Ctx* ctx, const uint8_t* data, size_t len, bool data_on_device, const uint64_t* seed, frieda_pcs_config cfg);
int prove_finish(Ctx* ctx, uint8_t out_commitment[32], ProofData& out);
// batches: `count` blobs of `len` bytes each (blob b at data + b * data_stride), one seed per blob or null; every kernel of the
// commit phase processes all blobs in one launch (Fiat-Shamir and launch latency are paid once per batch).  Needs the device
// channel (last layer <= 2^11 points).  prove_finish_batch writes count * 32 bytes of commitments.
int prove_begin_batch(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, bool data_on_device,
                      const uint64_t* seeds, frieda_pcs_config cfg, const uint8_t* const* host_ptrs = nullptr);
// `count` separate host blobs of one length
int prove_begin_batch_ptrs(Ctx* ctx, const uint8_t* const* blobs, size_t len, uint32_t count, const uint64_t* seeds, frieda_pcs_config cfg);
int prove_finish_batch(Ctx* ctx, uint8_t* out_commitments, std::vector<ProofData>& outs);
uint32_t job_count(const Ctx* ctx);  // blobs of the job in flight (0: none)

// ---- one blob proved under many seeds (a provider serving sampling clients: every sample is a proof of the same blob) ----
// The seed enters the channel before the first root, so unpack + encode + the first-layer tree do not depend on it: an Encoded keeps
// them on the device — one allocation of its own (not the context's arena: it survives other calls and release_workspace) holding the
// 4 evaluation columns, the first-layer tree (leaves-first layout, leaf hashes unwritten, large trees without the two levels above
// the leaves: `skip_log` is the threshold the tree was BUILT with) and the root.  Proving only reads it.
// The allocation belongs to a reference-counted slab (encoded_slab.h): the handles of a block (frieda_encode_batch, the
// frieda_rebuild_encoded_* calls) share one, blob b's share at b * encoded_bytes(n); a lone frieda_encode is the slab of one.
struct Encoded {
    int device = 0;
    size_t len = 0;
    uint32_t log_blowup = 0, n = 0, L = 0;
    uint32_t skip_log = 0;
    EncodedSlab* slab = nullptr;  // owner of the allocation `d` points into; this handle holds one reference while d != nullptr
    uint8_t* d = nullptr;  // [evaluation: 4 x 2^n words][tree: merkle_layer_offset(n, 0) + 32 bytes][root: 32 bytes], each from a 256-byte boundary
    size_t bytes = 0, o_tree = 0, o_root = 0;
    uint8_t root[32] = {0};
    // an aggregate handle (frieda_aggregate_encoded): of how many blobs (0: a blob's own handle) and under which challenge
    uint32_t aggregate_of = 0;
    QM31 aggregate_rho{0, 0, 0, 0};
    const uint32_t* eval() const { return reinterpret_cast<const uint32_t*>(d); }
    const uint8_t* tree() const { return d + o_tree; }
};
size_t encoded_bytes(uint32_t n, size_t* o_tree = nullptr, size_t* o_root = nullptr);  // the size of that allocation for a 2^n domain
// synchronous (the root comes back); the context's arena holds the blob and the coefficients meanwhile
int encode_blob(Ctx* ctx, const uint8_t* data, size_t len, bool data_on_device, uint32_t log_blowup, Encoded** out);
void encoded_release(Encoded& e);  // drops the handle's reference: the slab is freed (on its device) with its last handle
void encoded_free(Encoded* e);     // release + delete
// `count` handles of one shape in one fresh slab (hipMalloc + poison_fresh), blob b's share at b * encoded_bytes(n): every field but the
// root is set.  Releases whatever it still holds when it leaves scope; publish() hands the handles to the caller.
struct EncodedBlock {
    std::vector<Encoded> e;
    size_t bstride = 0;
    EncodedBlock() = default;
    EncodedBlock(const EncodedBlock&) = delete;
    EncodedBlock& operator=(const EncodedBlock&) = delete;
    ~EncodedBlock() {
        for (Encoded& x : e) encoded_release(x);
    }
    uint8_t* base() const { return e[0].d; }
    // FRIEDA_ERR_NOMEM (the context's error set, nothing allocated) when the slab does not fit
    int alloc(Ctx* ctx, size_t len, uint32_t log_blowup, uint32_t L, uint32_t n, uint32_t count, uint32_t skip_log);
    // roots[count][32] into the handles, then out[b] = a new frieda_encoded owning handle b; FRIEDA_ERR_NOMEM leaves `out` untouched
    int publish(const uint8_t* roots, frieda_encoded** out);
};
// `count` host blobs of one length (blob b at data + b * data_stride) -> `count` handles in one slab: one upload, the batched launches of
// commit_batch with the evaluation and the tree kept, one download of the roots, one synchronisation.  Not cut into passes.
int encode_batch(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, uint32_t log_blowup, frieda_encoded** out_encs);
// n_seeds proofs of enc's blob, proof i under seeds[i]: the batch machinery with the first layer at stride 0 (the per-seed workspace
// holds the inner layers, the last layer and the nonce only).  n_seeds > 1 needs the device channel, as every batch does.  Finished by
// prove_finish_batch (the commitments it writes are n_seeds copies of enc's root).
int prove_seeds_begin(Ctx* ctx, const Encoded* enc, const uint64_t* seeds, uint32_t n_seeds, frieda_pcs_config cfg);
// arena bytes prove_seeds_begin asks for (the Encoded excluded); 0: a shape the prover refuses
size_t seeds_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_seeds);
// A block of encoded blobs of one shape under ONE seed list: n_blobs * n_seeds jobs in one launch chain, job b * n_seeds + s = encs[b] under
// seeds[s].  Finished by prove_finish_batch like every batch.  The handles are only read.
int prove_seeds_blobs_begin(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, const uint64_t* seeds, uint32_t n_seeds, frieda_pcs_config cfg);
size_t seeds_blobs_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint32_t n_seeds);
// Any list of (handle, seed) jobs over encoded blobs of one shape (frieda_prove_jobs; prove_jobs_plan.h): job j = encs[blob_index[j]]
// under seeds[j].  The jobs run sorted by blob — the rectangle above is the list that is sorted as it stands — and the one finish writes
// proof j to the caller's slot j.  _check: the argument rules of a whole call; _pass_begin: `n` <= 65535 SORTED jobs in one launch chain,
// the table holding the distinct blobs they name and the arena planned for plan_blobs rows (1: prove_seeds), proof y to out_slot[y]
// (null: y); _begin: check, sort, one pass of everything planned for n_blobs rows.
int prove_jobs_check(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, const uint32_t* blob_index, const uint64_t* seeds, uint64_t n_jobs, frieda_pcs_config cfg);
void prove_jobs_sorted(const uint32_t* blob_index, const uint64_t* seeds, size_t n_jobs, uint32_t n_blobs, std::vector<uint32_t>& order,
                       std::vector<uint32_t>& sorted_blob, std::vector<uint64_t>& sorted_seeds);
int prove_jobs_pass_begin(Ctx* ctx, const Encoded* const* encs, const uint32_t* sorted_blob, const uint64_t* sorted_seeds, uint32_t n, uint32_t plan_blobs,
                          const uint32_t* out_slot, frieda_pcs_config cfg);
int prove_jobs_begin(Ctx* ctx, const Encoded* const* encs, uint32_t n_blobs, const uint32_t* blob_index, const uint64_t* seeds, uint32_t n_jobs, frieda_pcs_config cfg);
size_t prove_jobs_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint32_t n_jobs);
// the most jobs a pass takes under `limit` bytes (0: a refused shape), and the limit of a context: the batch policy's budget, or the
// test hook's arena limit when that is smaller
uint32_t prove_jobs_per_pass_under(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint64_t n_jobs, uint64_t limit);
uint64_t prove_jobs_limit(const k::Tuning& t);
int commit_batch(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, bool data_on_device, uint32_t log_blowup,
                 uint8_t* out_roots, const uint8_t* const* host_ptrs = nullptr);
// split form (frieda_commit_many alternates two contexts: the upload of one unit runs under the kernels of the other): _begin
// enqueues upload, kernels and the download of the roots into the pinned block; _finish waits and copies `count * 32` bytes out
int commit_batch_begin(Ctx* ctx, const uint8_t* data, size_t data_stride, size_t len, uint32_t count, bool data_on_device, uint32_t log_blowup,
                       const uint8_t* const* host_ptrs = nullptr);
int commit_batch_finish(Ctx* ctx, uint8_t* out_roots);
// ---- batch policy: how a run of equal-length blobs is cut into batched calls ("bytes in flight") ----
// Every kernel of a batched call covers all its blobs, so the launch / Fiat-Shamir latency chain is paid once per call: small blobs
// want many per call, large ones few (the workspace grows with the count).  Measured on MI355X (profiles/r04 larger_batch rows, r05):
// what matters is the bytes of workspace a call keeps in flight, not the blob count.
//   per_call = clamp(budget / workspace_bytes_per_blob, 1, ceil(count / (calls_per_ctx * in_flight))),
//   calls    = the smallest multiple of in_flight (no context idles while the last call runs alone) with no call above per_call,
//              sizes equal to within one.
// One implementation for frieda_prove_many / frieda_commit_many (multi.cpp), frieda_batch_plan (callers that drive _begin / _finish
// themselves: frieda_amd.BatchPipeline, bench.py) and the tests.
size_t workspace_bytes_per_blob(size_t len, uint32_t log_blowup, uint32_t log_last_layer, bool prove, bool data_on_device);
// FRIEDA_BATCH_BUDGET_MB, or the default: sixteen proofs of a 2^24 domain (blowup 2^4), ~43 GB — clamped to the device the context sits on:
// the default to 16 % of its memory (two calls in flight: a third; 43 GB are 15 % of an MI355X's 288 GB), an explicit value to 45 %
uint64_t batch_budget_bytes(const k::Tuning& t);
uint32_t batch_per_call(const k::Tuning& t, size_t ws_per_blob, uint32_t count, uint32_t in_flight);
void batch_cut(uint32_t count, uint32_t per_call, uint32_t in_flight, std::vector<uint32_t>& calls);

// returns FRIEDA_OK with *ok set, or FRIEDA_ERR_INVARIANT where the reference panics
// out_queries (optional): on acceptance, the sorted distinct query positions the transcript sampled — evaluations[i] of the proof is
// the value of the 4 columns at position out_queries[i] of the bit-reversed codeword (src/proof.rs:62-66)
// out_pairs (optional): on acceptance, both members of every opened first-layer pair {2v, 2v + 1} — ascending distinct positions and
// their column values, from `evaluations` where the position was queried and from first_layer.fri_witness otherwise.  The verifier
// hashed every one of them into the Merkle path it checked against the commitment: a sibling is as verified as an evaluation.
struct PairPoints {
    std::vector<uint32_t> pos;
    std::vector<QM31> val;
};
int verify(const ProofData& proof, const uint64_t* seed, int* ok, std::vector<uint32_t>* out_queries = nullptr, PairPoints* out_pairs = nullptr);

// Pairs mode of verify_many (frieda_verify_pairs_many, frieda_reconstruct_from_proof_pairs): the pair points of every accepted proof, pooled
// in the caller's order.  The kernel's proofs leave theirs in the pool's device allocation, gathered there pass by pass
// (k::verify_pairs_gather); host-route proofs keep theirs in `host` until upload_host_rows.  Entry e: d_pos()[e], d_val()[4 e .. 4 e + 3]
// — the cell layout of the point reconstruction (log_cell 0).
struct PairPool : DevPool {
    std::vector<size_t> off;          // per proof: its first entry
    std::vector<uint32_t> cnt;        // per proof: its entries (0 unless accepted)
    std::vector<PairPoints> host;     // per proof: the points of an accepted host-route proof
    uint32_t* d_pos() const { return d_idx(); }
    int upload_host_rows(Ctx* ctx);   // synchronous; a no-op without host-route proofs
};
// Many proofs in one call (verify_many.cpp, verify.hip): out_status[i] = a k::VerifyStatus, per proof the result of verify() whatever the
// route (device passes for the shapes the kernel takes, from Tuning::verify_device_min eligible proofs on — one launch per pass, or the
// two of verify_split.hip for a pass of at most Tuning::verify_split_max proofs; verify() for the rest).
// samples: an accepted proof must also hold one evaluation per distinct query (frieda_verify_samples), else VERIFY_INVARIANT;
// positions (optional): the sampled positions of every accepted proof.  Uses the arena and the pinned block (callers: FR_NO_JOB).
// pairs (optional, with samples): the pairs mode above.
// expected_commitments (optional): per proof the 32 bytes its first-layer commitment must equal (an entry may be null: not compared),
// else VERIFY_WRONG_COMMITMENT; the one-commitment entry points pass the same pointer for every proof.
int verify_many(Ctx* ctx, const ProofData* const* proofs, const uint64_t* seeds, uint32_t count, const uint8_t* const* expected_commitments, bool samples,
                uint8_t* out_status, std::vector<std::vector<uint32_t>>* positions, PairPool* pairs = nullptr);
// The point reconstruction with the pool already on the device, outside the arena: d_index[n_entries] next to
// d_cells[n_entries][n_blobs][4][2^log_cell] — ONE reconstruction over 4 * n_blobs columns (one locator for all of them), then blob b
// packed to d_out_bytes + b * out_stride.  Pair points: (n_blobs 1, log_cell 0); the cells of a blob: (n_blobs 1); stripes: n_blobs <= 256.
// *n_distinct receives the number of distinct entries whenever the call got as far as counting them (it is what decides the "too few"
// errors); count_distinct_points stops there.
int reconstruct_pooled(frieda_ctx* ctx, const uint32_t* d_cells, const uint32_t* d_index, uint32_t n_entries, uint32_t n_blobs, uint32_t log_cell,
                       uint32_t log_coef, uint32_t log_domain, size_t len, uint8_t* d_out_bytes, size_t out_stride, uint32_t* n_distinct);
int count_distinct_points(frieda_ctx* ctx, const uint32_t* d_index, uint32_t n_points, uint32_t log_domain, uint32_t* n_distinct);
// The tail of the single-blob rebuilds (from proofs, proof pairs, opened cells): a DevBuf of `len` bytes, rebuild(d_out) — the
// reconstruction, which also turns its "too few" into the caller's words —, download, commit_host, rebuilt_accept.  The stream is
// drained before the buffer is released, whatever rebuild returned.
int rebuild_blob(frieda_ctx* ctx, size_t len, uint32_t log_blowup, const uint8_t commitment[32], const char* mismatch, uint8_t* out_bytes,
                 const std::function<int(uint8_t* d_out)>& rebuild);
// roots[n_blobs][32] against commitments[n_blobs][32], then `bytes` to out_bytes.  mismatch: the error of a single blob; null: blob b's
int rebuilt_accept(Ctx* ctx, const uint8_t* roots, const uint8_t* commitments, uint32_t n_blobs, const char* mismatch, const std::vector<uint8_t>& bytes,
                   uint8_t* out_bytes);

// ---- authenticated cells (cells_host.cpp, cells.hip; the exports are in cells_host.cpp) ----
// The accepted cells (or fully accepted stripes) of a rebuild call, in the caller's order.  Entry e: d_idx()[e],
// d_val()[e][group][4][2^log_cell], group = 1, or the blobs of a stripe.
struct CellPool : DevPool {};
// the argument rule of every cells entry point: log_cell <= min(log_domain, FRIEDA_MAX_LOG_OPEN_CELL), every index < 2^(log_domain - log_cell);
// null when it holds, else what is wrong
const char* cells_args_error(uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells);
// the tail of the block rebuilds (opened stripes, stripe bundles): the pool's fully accepted stripes -> one point reconstruction over
// 4 * n_blobs columns, commit_batch, every root against its commitment, out_bytes[n_blobs][len]; *n_distinct also on an error
int rebuild_blobs_from_stripes(frieda_ctx* ctx, const CellPool& pool, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                               uint32_t log_cell, uint8_t* out_bytes, uint32_t* n_distinct);
// The sibling of rebuild_blob and rebuild_blobs_from_stripes that also returns handles (frieda_rebuild_encoded_*; n_blobs 1: a blob's
// cells, else the fully accepted stripes of a block): the point reconstruction with its step-5 re-encode landing in a fresh slab, the
// blob-image check (blob_image.h) on the coefficients, tree_first_layer over the slab (batched over the blobs), every root against its
// commitment by rebuilt_accept's rule, pack30 + download only when out_bytes is given.  No commit_host / commit_batch: the bytes are
// never uploaded.  *n_distinct also on an error; out_encs[n_blobs] is written on FRIEDA_OK only.
int rebuild_encoded_from_pool(frieda_ctx* ctx, const CellPool& pool, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup, size_t len,
                              uint32_t log_cell, const char* mismatch, uint8_t* out_bytes, uint32_t* n_distinct, frieda_encoded** out_encs);
// The shape rule of the four cell / bundle rebuilds (cells_host.cpp): *L = log2 of the coefficients `len` bytes take, *n = *L + log_blowup_factor,
// or FRIEDA_ERR_ARG "<fn>shape out of range".
int rebuild_shape(frieda_ctx* ctx, const char* fn, uint32_t log_blowup_factor, size_t len, uint32_t* L, uint32_t* n);
// Their one tail, once the verify passes have filled `pool` (a pool nothing was verified into is empty).  n_blobs 0: one blob from its cells
// (rebuild_blob over reconstruct_pooled, the single-blob mismatch text); n_blobs >= 1: a block from its stripes (rebuild_blobs_from_stripes,
// the mismatch names the blob).  out_encs non-null: rebuild_encoded_from_pool instead, for either.  *n_used: the distinct entries, on an
// error too.  Fewer than the reconstruction needs: FRIEDA_ERR_ARG "<d> distinct <noun>, <need> needed".
int rebuild_from_pool(frieda_ctx* ctx, const CellPool& pool, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                      uint32_t log_cell, const char* noun, uint8_t* out_bytes, frieda_encoded** out_encs, size_t* n_used);

// ---- bundles (bundles_host.cpp serves stripe_bundles_host.cpp too; bundles.hip, stripe_bundles.hip) ----
// The one pass driver of both bundle forms.  MALFORMED on the host, once per bundle, the rest from the kernels, staged in passes
// (bundles_pass.h, factor max(n_blobs, 1)).  Uses the arena and the pinned block (callers: FR_NO_JOB).
//   n_blobs 0        cell bundles: one commitment, in the kernel arguments; bundle_walk; out_status[n_bundles]
//   n_blobs >= 1     stripe bundles: commitments[n_blobs][32], uploaded once; stripe_bundle_walk (for one blob too); out_status[n_bundles][n_blobs],
//                    MALFORMED in the bundle's whole row; a pass stages at most 2^30 bytes
// pool (optional): receives, in the caller's order, the cells (stripes) of the bundles whose status bytes are all ACCEPTED.
int verify_bundles_passes(Ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                          const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness, const uint64_t* witness_first,
                          uint8_t* out_status, CellPool* pool);
// The openers' shared pieces.  open_bundles_front: what frieda_open_cell_bundles (n_blobs 1) and frieda_open_stripe_bundles check before they
// launch — null arguments, shape, structure, the first malformed bundle by name —, wfirst[n_bundles + 1] (hashes per blob), the size query
// (out_witness null) and cap_hashes against n_blobs * wfirst.  *go: the caller goes on to launch; else the call ends with the returned code.
int open_bundles_front(frieda_ctx* ctx, const char* fn, uint32_t log_domain, uint32_t n_blobs, uint32_t log_cell, const uint32_t* index,
                       const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* out_values, const uint8_t* out_witness, size_t cap_hashes,
                       uint64_t* out_witness_first, std::vector<uint64_t>& wfirst, bool* go);
// the bundle table and the per-(bundle, level) witness offsets of an opener's upload, rows[n_bundles] and base[n_bundles][depth].  n_blobs 0:
// offsets from wfirst[b], no first_hash; n_blobs >= 1: the offsets of blob 0's piece, from n_blobs * wfirst[b], and first_hash = wfirst[b]
void open_bundles_fill(k::BundleRow* rows, uint64_t* base, uint32_t depth, uint32_t n_blobs, const uint32_t* index, const uint32_t* bundle_first,
                       uint32_t n_bundles, const uint64_t* wfirst);
// an opener's end: the launch error, one download of (values | witness) from the arena at a_out to the pinned block behind the upload, one
// synchronisation, the two copies out
int open_bundles_finish(Ctx* ctx, size_t in_bytes, size_t a_out, size_t vb, size_t wb, uint32_t* out_values, uint8_t* out_witness);

// transcript pieces shared by prover and verifier (transcript.cpp)
void channel_mix_felts(Channel& ch, const std::vector<QM31>& felts);
std::vector<uint32_t> generate_queries(Channel& ch, uint32_t log_domain_size, uint32_t n_queries);
std::vector<uint32_t> fold_queries(const std::vector<uint32_t>& q, uint32_t n_folds);

// host Merkle node hash (verifier)
Hash32 hash_node_host(const uint8_t* left, const uint8_t* right, const uint32_t* values, size_t n_values);

}  // namespace frieda

// Recycled proof objects of one context.  A proof of a 2^24 domain is ~140 KB in ~50 vectors; allocating them afresh costs
// 30-40 us per proof (page faults on heap memory the allocator had trimmed after the previous proof was freed) — more than
// copying the openings into them.  frieda_proof_free hands the object back to the pool of the context that made it (the pool
// outlives the context while proofs of it are alive), and the next proof is assembled into the recycled vectors.
struct frieda_proof;
struct ProofPool {
    std::mutex mu;
    std::vector<frieda_proof*> free_list;
    size_t bytes = 0;                                  // approximate capacity held by the free list
    static constexpr size_t MAX_BYTES = 64u << 20;     // beyond this, freed proofs are really freed
    static constexpr size_t MAX_ENTRIES = 4096;
    frieda_proof* get();            // a recycled object (contents unspecified, capacities kept) or a new one; never null (throws bad_alloc)
    void put(frieda_proof* p);      // takes ownership
    ~ProofPool();
};
struct frieda_ctx {
    frieda::Ctx c;
    std::shared_ptr<ProofPool> pool = std::make_shared<ProofPool>();
};

// the extern "C" entry points' exception fence: no exception crosses the ABI
#define FR_GUARD_BEGIN try {
#define FR_GUARD_END(ctxptr)                                          \
    }                                                                 \
    catch (const std::bad_alloc&) {                                   \
        if (ctxptr) (ctxptr)->c.err = "host allocation failed";       \
        return FRIEDA_ERR_NOMEM;                                      \
    }                                                                 \
    catch (const std::exception& e) {                                 \
        if (ctxptr) (ctxptr)->c.err = e.what();                       \
        return FRIEDA_ERR_INVARIANT;                                  \
    }
struct frieda_encoded {
    frieda::Encoded e;
};
struct frieda_proof {
    frieda::ProofData p;
    std::shared_ptr<ProofPool> home;  // set while the object is out with the caller; null inside the pool and for clones / parsed proofs
};
