/*
 * frieda_hip.h — C ABI of the MI355X-native FRI-DAS commit / prove path (libfrieda_hip.so).
 *
 * This is the drop-in boundary: the entry points a Rust `extern "C"` block in a frieda fork (Level A) or
 * an stwo `HipBackend` (Level B) would bind.  Plain pointers and sizes only; no C++/torch types; no
 * exceptions or unwinding cross it.  Every function returns an int status (FRIEDA_OK == 0).  Where the
 * reference panics (assert!/unwrap) the status is FRIEDA_ERR_INVARIANT and a Rust shim re-raises with
 * panic!; verifier rejections are reported through *ok, exactly like the reference's `bool`.
 *
 * Reference interfaces replaced (paths under /root/reference):
 *   Level A  src/lib.rs:31-43  api::{commit, generate_proof, verify}
 *            src/proof.rs:32-36 commit_and_generate_proof; src/proof.rs:19-26 struct Proof
 *   Level B  the stwo backend traits frieda instantiates with `CpuBackend`
 *            (src/commit.rs:15,17; src/proof.rs:47,48,52,58; src/utils.rs:21,28):
 *            PolyOps::{precompute_twiddles, evaluate}, MerkleOps::commit_on_layer,
 *            FriOps::{fold_circle_into_line, fold_line}, GrindOps::grind, plus the codec of
 *            src/utils.rs:10-33.
 *
 * Threading: a frieda_ctx owns one device, one stream, its twiddle cache and workspace.  A ctx is not
 * thread-safe; distinct ctxs are independent (one per GPU / host thread).  No global mutable state.
 */
#ifndef FRIEDA_HIP_H
#define FRIEDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FRIEDA_OK 0
#define FRIEDA_ERR_ARG 1       /* null pointer / size out of the supported range */
#define FRIEDA_ERR_HIP 2       /* a HIP runtime call failed (see frieda_last_error) */
#define FRIEDA_ERR_INVARIANT 3 /* the reference would panic here */
#define FRIEDA_ERR_NOMEM 4
#define FRIEDA_ERR_FORMAT 5    /* malformed proof image */

#define FRIEDA_ABI_VERSION 1
#define FRIEDA_MAX_LOG_DOMAIN 28
#define FRIEDA_MAX_LOG_CELLS 12 /* reconstruction from up to 2^12 scattered cells */

typedef struct frieda_ctx frieda_ctx;
typedef struct frieda_proof frieda_proof;

/* stwo PcsConfig { pow_bits, fri_config: FriConfig { log_blowup_factor, log_last_layer_degree_bound,
 * n_queries } } as passed at src/lib.rs:36, src/proof.rs:109-116, benches/proof.rs:5-12 */
typedef struct {
    uint32_t pow_bits;
    uint32_t log_blowup_factor;
    uint32_t log_last_layer_degree_bound;
    uint32_t n_queries;
} frieda_pcs_config;

uint32_t frieda_abi_version(void);
const char* frieda_status_string(int status);
/* detail of the last failure on this ctx (valid until the next call on it) */
const char* frieda_last_error(const frieda_ctx* ctx);
/* What context creation had to degrade on this device (an LDS opt-in refused ...), one line each; "" when nothing was.  A
 * successful frieda_ctx_create leaves frieda_last_error empty: notes are not errors. */
const char* frieda_ctx_notes(const frieda_ctx* ctx);

/* ---- context -------------------------------------------------------------------------------- */
/* stream: a hipStream_t to run on (e.g. torch's current stream), or NULL to create a private one */
int frieda_ctx_create(int device, void* stream, frieda_ctx** out);
int frieda_ctx_destroy(frieda_ctx* ctx);
int frieda_ctx_synchronize(frieda_ctx* ctx);
/* twiddle policy: 1 (default) keep the per-domain twiddle tables in the ctx across calls; 0 regenerate
 * them on every call as the reference does (src/commit.rs:15) */
int frieda_ctx_set_twiddle_cache(frieda_ctx* ctx, int enabled);

/* The ctx keeps its device workspace (sized by the largest call so far: a few hundred bytes per blob byte, times the batch),
 * its pinned staging block and its twiddle tables between calls.  This frees them; the next call allocates what it needs. */
int frieda_ctx_release_workspace(frieda_ctx* ctx);

/* transcript policy: 0 (default) the Fiat-Shamir channel of generate_proof runs on the device inside the commit-phase
 * kernels; 1 evaluates it on the host between layers (one 32-byte D2H + synchronise per layer).  Proofs are identical;
 * configurations whose last FRI layer exceeds 2^11 points always use the host policy. */
int frieda_ctx_set_host_channel(frieda_ctx* ctx, int enabled);

/* Tuning and A/B options of THIS context (none is needed in normal use; every option selects another kernel or plan for the SAME
 * result — DESIGN.md §10 lists them).  `name` is the name of the environment variable that sets the option's default when a context
 * is created, e.g. "FRIEDA_TAIL_RUN_LOG", "FRIEDA_NO_ENCODE_TREE_FUSION", "FRIEDA_HOST_DECOMMIT"; a context never re-reads the
 * environment after creation and no option is process-wide.  FRIEDA_ERR_ARG: unknown name or value out of range. */
int frieda_ctx_set_option(frieda_ctx* ctx, const char* name, int64_t value);

/* measurement aid: when enabled, HIP events are recorded on the ctx stream around every kernel launch.
 * frieda_ctx_kernel_timing_report synchronises the stream and writes a JSON object
 * {"kernels": [{"name", "launches", "total_ms", "alg_bytes"}]} (alg_bytes = algorithmic HBM bytes by the byte model
 * of DESIGN.md §5); returns the bytes needed including the NUL; reset != 0 clears the accumulated spans. */
int frieda_ctx_set_kernel_timing(frieda_ctx* ctx, int enabled);
/* host wall-clock marks of the last generate_proof on this ctx, ms since entry: [0] everything enqueued, [1] device work
 * complete (the one synchronisation), [2] queries drawn, [3] openings gathered ([2] = [3] = [1] unless the host fallback
 * planned the openings), [4] proof assembled, [5] host set-up before the first launch */
int frieda_ctx_last_prove_phases(const frieda_ctx* ctx, double out_ms[8]);
size_t frieda_ctx_kernel_timing_report(frieda_ctx* ctx, char* buf, size_t cap, int reset);
/* measurement aid: the pure-compute rate of the Merkle compression on THIS device, now — compressions per second with every
 * lane chaining Blake2s compressions on register-resident data (8 workgroups per CU), leaf-shaped (4 message words, 12 zero) and
 * node-shaped (16 words).  The path is bound by this rate, which differs by a few per cent between devices; bench.py quotes it
 * beside the measured kernels (roofline_valu) instead of a constant.  ~5 ms; synchronises the stream. */
int frieda_ctx_blake2s_ceiling(frieda_ctx* ctx, double* leaf_per_s, double* node_per_s);
/* the same after ~0.25 s of that load per shape (~0.5 s in all), with the clock the chip holds under it read inside the kernel (shader-clock counter against
 * the 100 MHz wall-clock counter, median over the workgroups): out = {leaf compressions/s, node compressions/s, leaf clock GHz,
 * leaf SIMD cycles per wave-compression, node clock GHz, node SIMD cycles per wave-compression}.  On MI355X the clock stays at
 * 2.3 - 2.4 GHz under this load and a compression costs ~2250 (leaf) / ~2400 (node) cycles per wave in the library's throughput
 * form (runs of one VALU rate class, the wave's priority raised for its slow-class runs; ~3950 for the scheduler's own fine
 * interleave, ~3150 / ~3300 with idle issue states instead of priorities: profiles/r05_blake2s_prio.txt, r05_blake2s_idle_sweep.txt):
 * the ceiling is the instruction stream and how the waves of a SIMD share the vector pipe. */
int frieda_ctx_blake2s_ceiling_ex(frieda_ctx* ctx, double out[6]);
/* diagnostic: the Fiat-Shamir transcript of the last finished generate_proof on this ctx (blob 0 of a batch) — what
 * FriProver::commit derives between src/proof.rs:52 and :58 and the Proof does not carry: per FRI layer (first, then inner)
 * the folding alpha drawn after its root (4 u32 each; the roots themselves are the layer commitments of the Proof), and the
 * channel digest the proof of work was keyed by (after mix_felts(last_layer_poly)).  *n_layers receives the layer count;
 * at most cap_layers alphas are written.  Exists so that a cargo-side dump of the reference's transcript can be diffed
 * against this path value by value (tools/dump_trace.py, tests/golden/trace_selfcheck.json). */
int frieda_ctx_last_transcript(const frieda_ctx* ctx, uint32_t* n_layers, uint32_t* alphas, size_t cap_layers,
                               uint8_t digest_before_grind[32]);

/* ---- Level A: frieda's public API ------------------------------------------------------------- */
/* api::commit(data, log_blowup_factor) -> [u8; 32]   (src/lib.rs:31, src/commit.rs:11-22) */
int frieda_commit(frieda_ctx* ctx, const uint8_t* data, size_t len, uint32_t log_blowup_factor, uint8_t out_root[32]);
/* same with the blob already resident in device memory; the root is written to device memory
 * (d_out_root, 32 B, 4-byte aligned) asynchronously on the ctx stream — no host synchronisation.  d_data (here and in every
 * _device form below) is a byte pointer: any address, and any stride >= len between the blobs of a batch. */
int frieda_commit_device(frieda_ctx* ctx, const void* d_data, size_t len, uint32_t log_blowup_factor, void* d_out_root);

/* proof::commit_and_generate_proof(data, seed, cfg) -> (Commitment, Proof)   (src/proof.rs:32-77);
 * seed == NULL is Option::None */
int frieda_commit_and_generate_proof(frieda_ctx* ctx, const uint8_t* data, size_t len, const uint64_t* seed,
                                     frieda_pcs_config cfg, uint8_t out_commitment[32], frieda_proof** out);
int frieda_commit_and_generate_proof_device(frieda_ctx* ctx, const void* d_data, size_t len, const uint64_t* seed,
                                            frieda_pcs_config cfg, uint8_t out_commitment[32], frieda_proof** out);
/* The same, split in two so that several proofs can overlap on one GPU: _begin enqueues everything — encode, FRI commit
 * phase, proof of work, query sampling and openings — on the ctx stream and returns without synchronising; _finish waits
 * for it (once) and builds the proof from the openings the device left in pinned memory.  At most one proof (or batch) in
 * flight per ctx — use one ctx (= one stream + workspace) per in-flight proof.  While one is in flight, every other entry
 * point that sizes or writes the ctx's workspace or pinned block returns FRIEDA_ERR_ARG ("a proof is in flight on this
 * context") and leaves the proof untouched: frieda_commit*, frieda_commit_batch*, a second _begin, frieda_merkle_root,
 * frieda_merkle_commit_layer, frieda_grind, frieda_reconstruct*_device, frieda_circle_interpolate_cells,
 * frieda_ctx_release_workspace, frieda_dev_gather, frieda_dev_gather_hashes, frieda_merkle_decommit (and
 * frieda_merkle_decommit_device beyond 512 positions), frieda_verify_many, frieda_verify_blobs_many, frieda_verify_samples_many, frieda_reconstruct_from_proofs,
 * frieda_verify_pairs_many, frieda_reconstruct_from_proof_pairs (frieda_verify_pairs is host-only and takes no context),
 * frieda_open_cells, frieda_verify_cells_many, frieda_reconstruct_from_opened_cells (frieda_verify_cells is host-only and takes no context),
 * frieda_open_cells_blobs, frieda_verify_cells_blobs_many, frieda_reconstruct_blobs_from_opened_stripes (frieda_verify_cells_blobs is host-only
 * and takes no context), frieda_open_cell_bundles, frieda_verify_cell_bundles_many, frieda_reconstruct_from_cell_bundles
 * (frieda_cell_bundle_witness_count and frieda_verify_cell_bundles are host-only and take no context), frieda_open_stripe_bundles,
 * frieda_verify_stripe_bundles_many, frieda_reconstruct_blobs_from_stripe_bundles (frieda_verify_stripe_bundles is host-only and takes no
 * context), frieda_encode_batch, the four frieda_rebuild_encoded_* calls, frieda_aggregate_encoded and frieda_prove_block_seeds.  Level B calls that only read the twiddle cache and caller
 * buffers stay available.
 * A blob passed to _begin_device must stay valid until _finish returns. */
int frieda_prove_begin(frieda_ctx* ctx, const uint8_t* data, size_t len, const uint64_t* seed, frieda_pcs_config cfg);
int frieda_prove_begin_device(frieda_ctx* ctx, const void* d_data, size_t len, const uint64_t* seed, frieda_pcs_config cfg);
int frieda_prove_finish(frieda_ctx* ctx, uint8_t out_commitment[32], frieda_proof** out);
/* Batches of small blobs (the reference's own bench sizes, benches/commit.rs:6-10, benches/proof.rs:14-21,
 * are 1 KiB .. 64 KiB blobs, where one proof is a chain of ~50 dependent launches on an almost idle chip).  `count` blobs of
 * `len` bytes each, blob i at data + i * stride (stride >= len); seeds == NULL is None for all, else seeds[i] is Some for blob i.
 * Every kernel of the path handles the whole batch in one launch, so the launch and Fiat-Shamir latency is paid once per batch;
 * results are exactly those of `count` separate calls.  out_commitments / out_roots: count * 32 bytes (host);
 * out_proofs: count handles, each released with frieda_proof_free.  Proof batches need the last FRI layer to have <= 2^11
 * points (log_last_layer_degree_bound + log_blowup_factor <= 11) and the default (device) transcript policy. */
int frieda_commit_and_generate_proof_batch(frieda_ctx* ctx, const uint8_t* data, size_t stride, size_t len, uint32_t count,
                                           const uint64_t* seeds, frieda_pcs_config cfg, uint8_t* out_commitments,
                                           frieda_proof** out_proofs);
int frieda_commit_and_generate_proof_batch_device(frieda_ctx* ctx, const void* d_data, size_t stride, size_t len, uint32_t count,
                                                  const uint64_t* seeds, frieda_pcs_config cfg, uint8_t* out_commitments,
                                                  frieda_proof** out_proofs);
/* split form, as frieda_prove_begin / _finish: _begin enqueues the device work of the whole batch and returns; _finish (same
 * count) waits and builds the proofs.  Two contexts alternating _begin / _finish keep the host-side assembly of one batch
 * under the device work of the next. */
int frieda_prove_batch_begin(frieda_ctx* ctx, const uint8_t* data, size_t stride, size_t len, uint32_t count, const uint64_t* seeds,
                             frieda_pcs_config cfg);
int frieda_prove_batch_begin_device(frieda_ctx* ctx, const void* d_data, size_t stride, size_t len, uint32_t count,
                                    const uint64_t* seeds, frieda_pcs_config cfg);
int frieda_prove_batch_finish(frieda_ctx* ctx, uint32_t count, uint8_t* out_commitments, frieda_proof** out_proofs);
int frieda_commit_batch(frieda_ctx* ctx, const uint8_t* data, size_t stride, size_t len, uint32_t count, uint32_t log_blowup_factor,
                        uint8_t* out_roots);
/* One blob proved under many seeds.  In data-availability sampling a sample IS a proof: every client sends a seed and the provider
 * answers with commit_and_generate_proof(data, seed, cfg) of the SAME blob.  The seed enters the transcript before the first root is
 * mixed, so unpacking, the Reed-Solomon encode and the first-layer Merkle tree do not depend on it (about half of a large proof); every
 * alpha, inner layer, nonce, query and opening does.  frieda_encode does the shared half once and keeps it on the device:
 * a frieda_encoded owns ONE device allocation of its own — the 4 evaluation columns, the first-layer tree and the root,
 * frieda_encoded_bytes() bytes — outside the context's workspace: it survives every other call on the context,
 * frieda_ctx_release_workspace and the context itself, until frieda_encoded_free.  Proving only READS it, so several contexts on the
 * same device may prove from one frieda_encoded at the same time (it must not be freed while a job that uses it is in flight).
 * frieda_encode* synchronise (the commitment comes back); frieda_encoded_commitment == frieda_commit(data, log_blowup_factor). */
typedef struct frieda_encoded frieda_encoded;
int frieda_encode(frieda_ctx* ctx, const uint8_t* data, size_t len, uint32_t log_blowup_factor, frieda_encoded** out);
int frieda_encode_device(frieda_ctx* ctx, const void* d_data, size_t len, uint32_t log_blowup_factor, frieda_encoded** out);
int frieda_encoded_commitment(const frieda_encoded* enc, uint8_t out_root[32]);
size_t frieda_encoded_bytes(const frieda_encoded* enc); /* device memory it holds */
void frieda_encoded_free(frieda_encoded* enc);
/* the shape of the encoded codeword: 2^log_size_bound coefficients per column, 2^log_domain evaluations (log_domain = log_size_bound +
 * log_blowup_factor): what frieda_open_cells and the frieda_verify_cells* calls of its clients go by */
int frieda_encoded_shape(const frieda_encoded* enc, uint32_t* log_size_bound, uint32_t* log_domain);
/* n_seeds proofs of the encoded blob: out_proofs[i] serialises to exactly the bytes of frieda_commit_and_generate_proof(data,
 * &seeds[i], cfg); repeated seeds are allowed (identical proofs), the order is the caller's.  seeds != NULL, 1 <= n_seeds <= 65535,
 * cfg.log_blowup_factor == the one the blob was encoded with, the ctx on the blob's device, and every argument rule of the batch
 * entry points — else FRIEDA_ERR_ARG / FRIEDA_ERR_INVARIANT as there.  n_seeds > 1 is a batch: device transcript only (last FRI
 * layer <= 2^11 points, host-channel policy off), else FRIEDA_ERR_ARG; n_seeds == 1 works under both policies.  _begin enqueues and
 * returns without synchronising, _finish waits once and builds the n_seeds proofs of the job in flight (one job per ctx, as above).
 * Memory: a call's workspace grows with n_seeds and is NOT cut into passes: frieda_seeds_workspace_bytes(len, cfg, n_seeds) is what
 * the call asks of the ctx (the encoded blob excluded; 0 = a shape the prover refuses) — per seed the inner layers only, about half
 * of frieda_workspace_bytes(.., prove).  A call the device cannot hold returns FRIEDA_ERR_NOMEM and leaves the ctx usable: size
 * n_seeds per call with that function.  The seed-looped first fold is selected by the option FRIEDA_SEEDS_FOLD_GROUP. */
int frieda_prove_seeds_begin(frieda_ctx* ctx, const frieda_encoded* enc, const uint64_t* seeds, uint32_t n_seeds, frieda_pcs_config cfg);
int frieda_prove_seeds_finish(frieda_ctx* ctx, frieda_proof** out_proofs);
int frieda_prove_seeds(frieda_ctx* ctx, const frieda_encoded* enc, const uint64_t* seeds, uint32_t n_seeds, frieda_pcs_config cfg,
                       frieda_proof** out_proofs);
/* convenience for a caller that has all seeds at once: encode, prove, free */
int frieda_commit_and_generate_proofs_for_seeds(frieda_ctx* ctx, const uint8_t* data, size_t len, const uint64_t* seeds, uint32_t n_seeds,
                                                frieda_pcs_config cfg, uint8_t out_commitment[32], frieda_proof** out_proofs);
size_t frieda_seeds_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_seeds);
int frieda_commit_batch_device(frieda_ctx* ctx, const void* d_data, size_t stride, size_t len, uint32_t count,
                               uint32_t log_blowup_factor, uint8_t* out_roots);
/* api::generate_proof (src/lib.rs:36) */
int frieda_generate_proof(frieda_ctx* ctx, const uint8_t* data, size_t len, const uint64_t* seed, frieda_pcs_config cfg,
                          frieda_proof** out);
/* api::verify(proof, seed) -> bool  (src/lib.rs:41, src/proof.rs:79-101).  Host-only, one proof, one core (the reference's
 * verifier is O(n_queries * log N) hashes; many proofs: frieda_verify_many below).  *ok receives the bool; FRIEDA_ERR_INVARIANT where the
 * reference panics (src/proof.rs:166-173). */
int frieda_verify(const frieda_proof* proof, const uint64_t* seed, int* ok);
/* The sampling client's half of the README's flow (/root/reference/README.md:56-69; in src/ a sample IS a proof: the seed of
 * generate_proof decides, through the transcript, which positions are opened, src/proof.rs:40-42,60-66): verify as above and, when the
 * proof is accepted, also return WHERE it sampled — out_positions[i] (ascending, distinct) is the position in the bit-reversed
 * codeword of length 2^(log_size_bound + log_blowup_factor) whose four column values are evaluations[i]
 * (frieda_proof_evaluations).  Verified (position, value) pairs pooled from proofs with different seeds are exactly the input of
 * frieda_circle_interpolate_points / frieda_reconstruct_points_device (log_cell 0, cell r = evaluations[r]).  *n_positions receives
 * the count (0 when the proof is rejected); FRIEDA_ERR_ARG when cap is smaller than that. */
int frieda_verify_samples(const frieda_proof* proof, const uint64_t* seed, int* ok, uint32_t* out_positions, size_t cap, size_t* n_positions);
/* Many proofs in one call, verified on the GPU (verify.hip: one wave per proof replays the transcript, draws the queries, folds the
 * value chain and walks every layer's Merkle tree).  A sampling client checks thousands of proofs before it can rebuild a blob, and the
 * host verifier above costs 0.24 - 0.66 ms per proof on one core (profiles/r09_verify_many.txt).  proofs[count]: host array of
 * handles, which may differ in config, size and seed; seeds: NULL (None for all) or seeds[i] = Some for proof i.  Every proof gets one
 * status byte, always the result frieda_verify gives for it — proofs of a shape the kernel does not take (more than 1024 queries, a
 * last layer above 2^11 coefficients, more than 40 layers) run through the host verifier inside the same call:
 *   FRIEDA_VERIFY_REJECTED          frieda_verify: *ok = 0
 *   FRIEDA_VERIFY_ACCEPTED          frieda_verify: *ok = 1
 *   FRIEDA_VERIFY_INVARIANT         frieda_verify returns FRIEDA_ERR_INVARIANT (the reference panics)
 *   FRIEDA_VERIFY_WRONG_COMMITMENT  expected_commitment (32 bytes; NULL: not compared) differs from the proof's first-layer
 *                                   commitment: not verified at all (api::verify never sees the commitment, a sampling client has it)
 * The option FRIEDA_VERIFY_DEVICE_MIN is the number of kernel-eligible proofs from which a call uses the GPU
 * (0: always, 2^31: never; the default is 2: a lone proof is no slower through frieda_verify, profiles/r23_verify_split.txt).  The calls stage through the context's workspace in passes of bounded size: FRIEDA_ERR_ARG while a
 * proof is in flight on the context. */
#define FRIEDA_VERIFY_REJECTED 0
#define FRIEDA_VERIFY_ACCEPTED 1
#define FRIEDA_VERIFY_INVARIANT 2
#define FRIEDA_VERIFY_WRONG_COMMITMENT 3
int frieda_verify_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                       const uint8_t* expected_commitment, uint8_t* out_status);
/* The proofs of a block in one call: the one step a sampling client takes before it trusts any cell is one ordinary proof per
 * commitment, and a block has n_blobs of them (what frieda_prove_seeds_blobs made for its K commitments).  commitments[n_blobs][32] is
 * the table, blob_index[count] names the commitment of every proof; blob_index NULL: proof i belongs to commitment i, and count must be
 * n_blobs.  out_status[i] is exactly what frieda_verify_many gives for proof i alone with expected_commitment =
 * commitments[blob_index[i]], FRIEDA_VERIFY_WRONG_COMMITMENT included, whichever route the proof takes.  out_accepted_per_blob[n_blobs]
 * (may be NULL) receives per blob the number of ACCEPTED proofs that name it: a client reads "proximity checked" as > 0.
 * FRIEDA_ERR_ARG before anything runs, out_status and out_accepted_per_blob untouched: a blob_index entry >= n_blobs; NULL blob_index
 * with count != n_blobs; n_blobs == 0 with count > 0; NULL commitments; a proof in flight on the context.
 * Launch shapes (every entry point of this section): a pass of at most FRIEDA_VERIFY_SPLIT_MAX kernel-eligible proofs (DESIGN.md
 * section 10; 0: never, 2^31: always) runs as two launches, one wave per proof for the value chain and one wave per (proof, layer) for
 * the Merkle walks (verify_split.hip), for calls whose proof count is far below the number of waves the chip holds; statuses,
 * positions and pair rows are the same on both. */
int frieda_verify_blobs_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                             const uint8_t* commitments, uint32_t n_blobs, const uint32_t* blob_index, uint8_t* out_status,
                             uint32_t* out_accepted_per_blob);
/* The same as frieda_verify_many, and WHERE every accepted proof sampled, exactly as frieda_verify_samples reports it: row i of out_positions (pitch
 * entries per row) holds out_n_positions[i] ascending positions, 0 for a proof that is not accepted.  A proof frieda_verify_samples
 * answers with FRIEDA_ERR_INVARIANT (accepted, but not one evaluation per distinct query) has status FRIEDA_VERIFY_INVARIANT here.
 * pitch < n_queries of any proof: FRIEDA_ERR_ARG before anything runs. */
int frieda_verify_samples_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                               const uint8_t* expected_commitment, uint8_t* out_status, uint32_t* out_positions, size_t pitch,
                               uint32_t* out_n_positions);
/* The sampling client's whole flow: verify all proofs against expected_commitment, pool the (position, evaluation) pairs of the
 * accepted ones (de-duplicated by position, first occurrence kept), rebuild the blob from them (frieda_reconstruct_points_device with
 * log_cell 0, log_coef = the proofs' log_size_bound, log_domain = log_size_bound + log_blowup_factor) and require frieda_commit of
 * the len rebuilt bytes to equal expected_commitment.  *n_points receives the number of distinct verified points (where accepted
 * proofs disagree on the shape: those pooled before the proof that disagrees); fewer than
 * 2^log_size_bound + 2 of them, accepted proofs that disagree on the shape, or a result that does not commit to expected_commitment
 * (a wrong len): FRIEDA_ERR_ARG with out_bytes untouched.  out_status[count] as frieda_verify_samples_many. */
int frieda_reconstruct_from_proofs(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                                   const uint8_t expected_commitment[32], size_t len, uint8_t* out_bytes, uint8_t* out_status,
                                   size_t* n_points);
/* Every point an accepted proof authenticates.  A proof opens the first FRI layer in pairs {2v, 2v + 1} of the bit-reversed codeword;
 * where only one member of a pair was queried, the other's four column values travel in the first layer's fri_witness, and the verifier
 * hashes that leaf into the Merkle path it checks against the commitment.  In an accepted proof the sibling is therefore exactly as
 * verified as an evaluation, and a client that pools both needs about half as many proofs for the same number of distinct points.
 * frieda_verify_pairs (host, one proof; the counterpart of frieda_verify_samples): on acceptance out_positions receives the ascending,
 * distinct positions of both members of every opened pair and out_values[4 i .. 4 i + 3] the column words at out_positions[i] — from
 * the proof's evaluations where the position was queried, from the first layer's fri_witness otherwise.  *n_points receives the count
 * (at most 2 * n_queries; 0 when the proof is rejected); FRIEDA_ERR_ARG when cap (in points) is smaller than that;
 * FRIEDA_ERR_INVARIANT as frieda_verify_samples: accepted, but not one evaluation per distinct query. */
int frieda_verify_pairs(const frieda_proof* proof, const uint64_t* seed, int* ok, uint32_t* out_positions, uint32_t* out_values, size_t cap,
                        size_t* n_points);
/* The same for many proofs in one call, with the status bytes of frieda_verify_samples_many: row i holds out_n_points[i] points, its
 * positions at out_positions + i * pitch and its values at out_values + 4 * i * pitch (pitch in points).  Rows of proofs that are
 * not accepted are not written (their count is 0), and neither is the part of a row beyond out_n_points[i].  pitch < 2 * n_queries
 * of any proof: FRIEDA_ERR_ARG before anything runs.  Status and points are the same whichever route a proof takes
 * (FRIEDA_VERIFY_DEVICE_MIN and the shapes the kernel refuses, as above). */
int frieda_verify_pairs_many(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                             const uint8_t* expected_commitment, uint8_t* out_status, uint32_t* out_positions, uint32_t* out_values,
                             size_t pitch, uint32_t* out_n_points);
/* frieda_reconstruct_from_proofs with the pair points as the pool: same contract, same error cases (the shape rule, the len check, the
 * commitment check, out_bytes untouched on error), about half as many proofs needed.  *n_points receives the number of distinct
 * verified points pooled.  The points of the proofs the kernel verified are pooled and de-duplicated inside the library's own
 * workspace and go straight into the reconstruction; proofs that took the host verifier add theirs to the same pool.  WHICH
 * occurrence of a position that several proofs opened is kept is unspecified — it cannot matter: two accepted proofs under one
 * commitment cannot hold different values for a position without a Blake2s collision, and the reconstruction compares every distinct
 * sample it keeps with the re-encoded result.  *n_points and the bytes are deterministic. */
int frieda_reconstruct_from_proof_pairs(frieda_ctx* ctx, const frieda_proof* const* proofs, const uint64_t* seeds, uint32_t count,
                                        const uint8_t expected_commitment[32], size_t len, uint8_t* out_bytes, uint8_t* out_status,
                                        size_t* n_points);

/* ---- authenticated cells: open, verify and rebuild from cells of the codeword ------------------------------------------------
 * The FRIDA flow (/root/reference/README.md:56-69): proximity is checked ONCE per commitment — a client verifies one ordinary proof of
 * the blob — and every further sample is a cell of the codeword opened against the same first-layer root.  A cell is what the
 * reconstruction entry points below call a cell: cell c = entries c * 2^log_cell .. (c + 1) * 2^log_cell of every column of the
 * bit-reversed codeword, c < 2^(log_domain - log_cell), 0 <= log_cell <= min(log_domain, FRIEDA_MAX_LOG_OPEN_CELL).  Layouts, all host
 * arrays: values[n_cells][4][2^log_cell], cell-major (what frieda_reconstruct_points_device takes);
 * paths[n_cells][log_domain - log_cell][32], bottom-up: entry s is the sibling of the node above the cell at tree layer log_domain -
 * log_cell - s, and that node is the left child when bit s of the cell's index is 0.  With log_cell == log_domain the path is empty and the
 * cell's subtree root must be the commitment itself.  Hashing is the prover's trees (stwo's hash_node): a leaf is the four column words of
 * one position, a node its two children.  A cell with its path is a self-contained message: paths are per cell, not compacted across
 * the cells of a call, and cells served to different peers share nothing.
 * A cell is ACCEPTED when every word is a canonical M31 (< 2^31 - 1) and the subtree root over its 2^log_cell leaves, carried up its
 * path, equals the commitment.  One status byte per cell; a cell's status never depends on the other cells of the call.
 * What a cell shares with a proof: the encoded blob, the first-layer tree and its root.  What it does not: no transcript, no seed, no
 * fold chain, no proof of work, no proximity claim — a cell alone says nothing about the degree of the codeword.
 * Every call: cell_index in any order, repeats allowed; an index >= 2^(log_domain - log_cell) or a log_cell out of range gives
 * FRIEDA_ERR_ARG before anything runs, outputs untouched; n_cells == 0 is a no-op. */
#define FRIEDA_MAX_LOG_OPEN_CELL 10
#define FRIEDA_CELL_REJECTED 0
#define FRIEDA_CELL_ACCEPTED 1
/* Provider: cells of an encoded blob, each with its own path to frieda_encoded_commitment.  Only reads the blob, as proving does: it may
 * be in use by a frieda_prove_seeds job on another context.  Uses ctx's workspace and pinned staging (FRIEDA_ERR_ARG while a proof is in
 * flight on ctx); ctx must sit where the blob does, else FRIEDA_ERR_ARG.  One upload of the indices, the launches, one download, one
 * synchronisation.  log_domain here is the blob's (frieda_encoded_shape).  out_paths may be NULL when log_cell == log_domain.
 * The call is NOT cut into passes: the workspace and the pinned block hold the whole answer, 16 * 2^log_cell + 32 * (log_domain -
 * log_cell) + 4 bytes per cell, and a request they cannot hold fails with FRIEDA_ERR_NOMEM (the ctx stays usable): a provider serves
 * large requests as several calls. */
int frieda_open_cells(frieda_ctx* ctx, const frieda_encoded* enc, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells,
                      uint32_t* out_values, uint8_t* out_paths);
/* Client, host verifier: no context, one core, the Blake2s of frieda_verify.  2^log_cell + log_domain - log_cell compressions per cell. */
int frieda_verify_cells(const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells,
                        const uint32_t* values, const uint8_t* paths, uint8_t* out_status);
/* Client, thousands of cells in one call: the same status bytes from the GPU (cells.hip: a lane per leaf pair and an LDS reduction to
 * every subtree root, then a lane per cell up its path).  Stages through the context's workspace in passes of bounded size, as
 * frieda_verify_many does: FRIEDA_ERR_ARG while a proof is in flight on the context.  Measured on the 128 KiB fixture (a 2^19 codeword),
 * 513 cells of 64 entries, one MI355X against one host core (profiles/r11_open_cells.txt): 0.15 ms for the
 * call (staging, two launches, status download) against 3.54 ms for frieda_verify_cells on the same cells — the device verifier is the
 * faster one there, about 24 times. */
int frieda_verify_cells_many(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                             uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status);
/* The client's whole flow for a blob of len bytes committed with log_blowup_factor (log_size_bound follows from len as in
 * frieda_codec_shape, log_domain = log_size_bound + log_blowup_factor): verify all cells as frieda_verify_cells_many does, drop the
 * rejected ones, de-duplicate by index, rebuild through frieda_reconstruct_points_device's route, pack, and require frieda_commit of the
 * len rebuilt bytes to equal commitment.  That route needs 2^(log_size_bound - log_cell) + 1 distinct cells for log_cell >= 1 and
 * 2^log_size_bound + 2 points for log_cell == 0.  *n_cells_used receives the number of distinct accepted cells.  Too few of them, or a
 * result that does not commit to commitment (a wrong len): FRIEDA_ERR_ARG with out_bytes untouched and out_status[n_cells] valid.  A
 * rejected cell is never used.  Per call: two allocations of the call's own beside the workspace (the pool of accepted cells, the
 * rebuilt bytes), freed before it returns, and the final commitment check uploads the rebuilt bytes again; the measured time of the
 * whole call includes all of that (0.63 ms from 513 cells to the checked bytes of the fixture, same record). */
int frieda_reconstruct_from_opened_cells(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                         const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths,
                                         uint8_t* out_bytes, uint8_t* out_status, size_t* n_cells_used);

/* ---- the cells of a block: many blobs of one shape in one call ------------------------------------------------------------------
 * A block carries n_blobs blobs of one shape (one len, one log_blowup_factor, hence one log_domain), and a node answers for the same cell
 * indices of every blob.  The calls below are the four calls above over (blob, cell) pairs: cell i of a call is cell cell_index[i] of blob
 * blob_index[i].  A STRIPE j of a block is cell j of each of its blobs.  All pointers are host arrays or handles.
 * Layouts are unchanged per cell — values [4][2^log_cell], path [log_domain - log_cell][32] bottom-up with the same left / right rule —
 * and cell i of the call occupies slot i of values, paths and out_status.
 * Status bytes are FRIEDA_CELL_REJECTED / FRIEDA_CELL_ACCEPTED, and cell i's status is exactly what
 *   frieda_verify_cells(commitments + 32 * blob_index[i], log_domain, log_cell, cell_index + i, 1, values_i, paths_i, .)
 * gives: it never depends on the other cells of the call, and the host and the GPU routes agree.
 * Arguments: 1 <= n_blobs <= 65536 (256 for the reconstruction: 4 * n_blobs columns, and frieda_circle_interpolate_points takes at most
 * 1024); every blob_index[i] < n_blobs; the rules of the single-blob calls on the shared log_domain; for frieda_open_cells_blobs every
 * encs[b] non-NULL, where ctx sits, and all of one log_domain (an entry may repeat).  Anything else: FRIEDA_ERR_ARG before anything
 * runs, outputs untouched.  n_cells == 0 is a no-op, n_stripes == 0 is "too few".  The three context calls return FRIEDA_ERR_ARG while
 * a proof is in flight on ctx.
 * Measured on a block of 16 blobs of 128 KiB (2^19 codewords, blowup 16), 513 stripes of 64 entries, every new call against the loop
 * of 16 single-blob calls on the same stripes in the same run (profiles/r12_stripes.txt):
 * open 0.93 ms against 1.38 ms (1.49 times), verify 0.96 against 2.11 ms (2.21 times), the whole rebuild 3.32 against 10.03 ms (3.02 times). */
/* Provider.  Only reads the blobs: opening from a second context beside a frieda_prove_seeds job works as for one blob.  One upload
 * (the indices, the blob numbers and a table row per blob), the launches, one download, one synchronisation; not cut into passes, and
 * FRIEDA_ERR_NOMEM leaves ctx usable, as frieda_open_cells does.  The blobs of a call may have been encoded under different tree-skip
 * thresholds: the threshold is a field of the table row, not of the call. */
int frieda_open_cells_blobs(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, uint32_t log_cell, const uint32_t* blob_index,
                            const uint32_t* cell_index, uint32_t n_cells, uint32_t* out_values, uint8_t* out_paths);
/* Client, host verifier: no context.  commitments[n_blobs][32]. */
int frieda_verify_cells_blobs(const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* blob_index,
                              const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths, uint8_t* out_status);
/* Client, GPU verifier: a lane per cell whatever its blob, so a handful of cells of each of many blobs fills the launch one blob's cells
 * leave empty.  Stages through the workspace in passes under the budget of frieda_verify_cells_many; the commitment table is uploaded
 * once per call. */
int frieda_verify_cells_blobs_many(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell,
                                   const uint32_t* blob_index, const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths,
                                   uint8_t* out_status);
/* The client's whole flow for a block sampled by stripes: values[n_stripes][n_blobs][4][2^log_cell], paths[n_stripes][n_blobs][log_domain -
 * log_cell][32], out_status[n_stripes][n_blobs], out_bytes[n_blobs][len]; log_size_bound follows from len as in frieda_codec_shape, and one
 * len holds for all blobs.  Every cell is verified as above (out_status is always valid).  A stripe is USED only when all n_blobs of its
 * cells are accepted; used stripes are de-duplicated by index; all blobs are then rebuilt by ONE point reconstruction over 4 * n_blobs
 * columns — the erasure locator depends on the positions alone, so one serves every blob — each blob is packed, and frieda_commit_batch
 * over the rebuilt bytes (still in GPU memory) must give every blob's commitment.  *n_stripes_used receives the number of distinct fully
 * accepted stripes.  Fewer than 2^(log_size_bound - log_cell) + 1 of them for log_cell >= 1, or than 2^log_size_bound + 2 for log_cell == 0:
 * FRIEDA_ERR_ARG with out_bytes untouched.  A blob that does not commit to its commitment (a wrong len): FRIEDA_ERR_ARG with out_bytes
 * untouched, and frieda_last_error names the blob.  There is NO per-blob fallback when stripes are only partly accepted: a caller left
 * with too few whole stripes has frieda_reconstruct_from_opened_cells per blob.  The verify passes of this call are cut at stripe
 * boundaries (one stripe is always admitted).  Also FRIEDA_ERR_ARG: n_stripes * n_blobs * 4 * 2^log_cell beyond 2^32 words. */
int frieda_reconstruct_blobs_from_opened_stripes(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                                                 uint32_t log_cell, const uint32_t* stripe_index, uint32_t n_stripes, const uint32_t* values,
                                                 const uint8_t* paths, uint8_t* out_bytes, uint8_t* out_status, size_t* n_stripes_used);

/* ---- cell bundles: many cells under one shared Merkle witness -------------------------------------------------------------------
 * Every opened cell above travels with its own path of log_domain - log_cell siblings, and the paths of the cells one peer asks for
 * share most of their upper nodes.  A BUNDLE is the answer to one request: k cells of one blob at one log_cell, 1 <= k <=
 * FRIEDA_MAX_BUNDLE_CELLS, cell indices STRICTLY ASCENDING, values[k][4][2^log_cell] as the cell calls lay them out, and ONE hash witness:
 * stwo's (MerkleProver::decommit / MerkleVerifier::verify) for the tree cut at level d = log_domain - log_cell with the cell indices as
 * positions — bottom-up, and within a level ascending, the hash of every child that the verifier cannot compute from the cells.  Its
 * length depends on the indices alone (frieda_cell_bundle_witness_count): d for one cell, strictly below k * d for k >= 2, 0 when the
 * bundle holds every cell of the domain.  At log_cell 0 a point is 16 bytes and its path 32 * log_domain, so there the path is almost the
 * whole message: 64 random cells of a depth-13 tree need 402 hashes instead of 832, 499 need 1659 instead of 6487.
 * A bundle is accepted or not AS A WHOLE — that is the price of sharing; the per-cell calls stay for callers who want independent cells.
 * A call carries n_bundles bundles back to back: cell i of the call belongs to bundle b when bundle_first[b] <= i < bundle_first[b + 1];
 * bundle_first and witness_first have n_bundles + 1 entries each, and witness_first counts in hashes of 32 bytes.  All pointers are host
 * arrays or handles.
 * MALFORMED: a bundle that is empty, above the cap, not strictly ascending or holds an index >= 2^(log_domain - log_cell); for the
 * verifiers also one whose witness_first[b + 1] - witness_first[b] is not the count its indices give.  The verifiers decide that on the
 * host before anything is hashed (one function for both), never stage such a bundle, and report it in its own status byte: bundles
 * come from untrusted peers, so a bad one costs only itself.  The provider's call refuses a malformed bundle outright.  FRIEDA_ERR_ARG
 * is kept for the call's own structure: null pointers, a *_first array that does not start at 0 or that decreases, log_cell or the shape
 * out of range (0 <= log_cell <= min(log_domain, FRIEDA_MAX_LOG_OPEN_CELL)).  n_bundles == 0 is a no-op.
 * ACCEPTED: every word is a canonical M31, and the subtree roots of the cells, merged upward with the witness consumed in order, give
 * exactly the commitment.  With log_cell == log_domain the witness is empty and the one cell's root must be the commitment.
 * The times of these calls are records, not gates: one wave verifies one bundle, so a call of few large bundles is latency-bound by
 * design.  Measured on the 128 KiB fixture (a 2^19 codeword), 513 cells of 64 entries as one bundle / as eight bundles, against the
 * per-cell calls on the same cells in the same run on one MI355X (profiles/r15_cell_bundles.txt, tools/cell_bundles_timing.py): 1673 /
 * 3132 witness hashes instead of 6669 path hashes; open 0.090 / 0.089 ms against 0.071 ms; GPU verify 0.243 / 0.135 ms against 0.108 ms;
 * host verify on one core 3.79 / 3.89 ms against 3.52 ms; the whole rebuild 0.67 / 0.56 ms against 0.54 ms.  The bundle form buys bytes,
 * not time.  Other cell sizes and domains are not measured. */
#define FRIEDA_MAX_BUNDLE_CELLS 1024
#define FRIEDA_BUNDLE_REJECTED 0
#define FRIEDA_BUNDLE_ACCEPTED 1
#define FRIEDA_BUNDLE_MALFORMED 2
/* Host only, no context: *n_hashes receives the witness length of one bundle.  FRIEDA_ERR_ARG for a malformed bundle. */
int frieda_cell_bundle_witness_count(uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, uint32_t n_cells, size_t* n_hashes);
/* Provider: out_values[n_cells][4][2^log_cell] for all cells of the call, the witnesses of the bundles back to back in out_witness
 * (cap_hashes hashes of room), and out_witness_first[n_bundles + 1].  out_witness == NULL fills out_witness_first only and launches
 * nothing (out_values may then be NULL too).  One upload (indices, a table row per bundle, a witness offset per bundle and level: the
 * host computes them from the indices), the launches, one download, one synchronisation.  Like frieda_open_cells the call is NOT cut
 * into passes, and FRIEDA_ERR_NOMEM when the workspace cannot hold the answer leaves ctx usable.  A malformed bundle, or cap_hashes
 * below the total, refuses the whole call: FRIEDA_ERR_ARG, outputs untouched, and frieda_last_error names the bundle.  Only reads the
 * blob: it may be in use by a frieda_prove_seeds job on another context.  FRIEDA_ERR_ARG while a proof is in flight on ctx. */
int frieda_open_cell_bundles(frieda_ctx* ctx, const frieda_encoded* enc, uint32_t log_cell, const uint32_t* cell_index, const uint32_t* bundle_first,
                             uint32_t n_bundles, uint32_t* out_values, uint8_t* out_witness, size_t cap_hashes, uint64_t* out_witness_first);
/* Client, host verifier: no context, one core; a bottom-up merge written independently of the kernel.  One status byte per bundle
 * (FRIEDA_BUNDLE_*). */
int frieda_verify_cell_bundles(const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index, const uint32_t* bundle_first,
                               uint32_t n_bundles, const uint32_t* values, const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_status);
/* Client, the same status bytes from the GPU (bundles.hip): per pass the subtree roots of all cells as frieda_verify_cells_many computes
 * them, then one wave per bundle merges its (position, hash) list upward.  Stages the well-formed bundles through the workspace in
 * passes under the budget of frieda_verify_cells_many; a bundle never straddles two passes.  FRIEDA_ERR_ARG while a proof is in flight
 * on ctx. */
int frieda_verify_cell_bundles_many(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_domain, uint32_t log_cell, const uint32_t* cell_index,
                                    const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                    const uint64_t* witness_first, uint8_t* out_status);
/* The client's whole flow from bundles: verify them as frieda_verify_cell_bundles_many does, pool the cells of the ACCEPTED bundles,
 * de-duplicate by index, and rebuild as frieda_reconstruct_from_opened_cells does — the same cell counts needed, *n_cells_used = the
 * distinct cells of accepted bundles, FRIEDA_ERR_ARG with out_bytes untouched when they are too few or the result does not commit to
 * commitment (a wrong len).  out_status[n_bundles] is always valid.  A cell of a rejected or malformed bundle is never used. */
int frieda_reconstruct_from_cell_bundles(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                         const uint32_t* cell_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values,
                                         const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_bytes, uint8_t* out_status,
                                         size_t* n_cells_used);

/* ---- stripe bundles: a block's stripes under one shared witness per blob -----------------------------------------------------------
 * The bundle form of the block calls above.  A STRIPE BUNDLE is the answer to one request over a block of n_blobs blobs of one shape:
 * k stripes (a stripe is cell j of every blob; 1 <= k <= FRIEDA_MAX_BUNDLE_CELLS, stripe indices strictly ascending) with ONE hash
 * witness per blob instead of one path per (stripe, blob) cell.  Every blob of a bundle has the same indices, so the witness length,
 * the per-level offsets and the malformed rule are computed once per bundle, not once per (bundle, blob); all blobs are rebuilt with
 * one erasure locator.  A call carries n_bundles bundles back to back: stripe t of the call belongs to bundle b when
 * bundle_first[b] <= t < bundle_first[b + 1].  All pointers are host memory.  Layouts:
 *   values          [n_stripes_total][n_blobs][4][2^log_cell], stripe-major: exactly what frieda_reconstruct_blobs_from_opened_stripes takes.
 *   witness_first   [n_bundles + 1], counts hashes PER BLOB: W_b = witness_first[b + 1] - witness_first[b] must equal
 *                   frieda_cell_bundle_witness_count of bundle b's indices.
 *   witness         bundle b's block starts at hash n_blobs * witness_first[b]; blob j's piece is the W_b hashes at offset j * W_b inside
 *                   that block, byte for byte the witness frieda_open_cell_bundles gives for blob j on the same indices.  cap_hashes
 *                   counts against n_blobs * witness_first[n_bundles].
 *   out_status      [n_bundles][n_blobs] bytes FRIEDA_BUNDLE_*.  Byte (b, j) is exactly what frieda_verify_cell_bundles(commitments + 32 j, ...)
 *                   gives for blob j's piece alone; it never depends on another blob or bundle, and the host and GPU routes agree.
 * MALFORMED depends on the indices and W_b only: it is decided once per bundle, on the host, by the rule of the cell bundles, and written
 * to all n_blobs bytes of that bundle; such a bundle is never staged.  The provider's call refuses it outright.  FRIEDA_ERR_ARG
 * (statuses untouched) is for what makes the call itself meaningless: the argument rules of the block cell calls and of the bundle calls
 * combined — 1 <= n_blobs <= 65536 for open and verify (<= 256 for the rebuild), every encs[b] non-NULL, where ctx sits and of one
 * log_domain (an entry may repeat, and the blobs' tree-skip thresholds may differ), NULL pointers, *_first arrays that do not start at 0
 * or decrease, log_domain or log_cell out of range.  n_bundles == 0 is a no-op.
 * The times of these calls are records, not gates; what the form buys is bytes.  Measured on a block of 16 blobs of 128 KiB, 513 stripes
 * of 64 entries as one bundle / as eight bundles, against the loop of 16 single-blob bundle calls and against the per-cell stripe calls on
 * the same stripes in the same run on one MI355X (profiles/r16_stripe_bundles.txt, tools/stripe_bundles_timing.py): 16 x 1673 / 16 x 3132
 * witness hashes instead of 16 x 6669 path hashes (arithmetic); open 0.78 / 0.84 ms against 1.51 ms (loop) and 0.94 ms (per cell); device
 * verify 0.80 / 0.74 ms against 3.91 / 2.26 ms and 0.92 ms; host verify on one core 61.9 / 63.4 ms against 61.6 / 63.2 ms and 56.8 ms; the
 * whole rebuild 3.23 / 3.16 ms against 11.01 / 9.40 ms (sixteen locators) and 3.25 ms.  Other block sizes, cell sizes and domains are not
 * measured. */
/* Provider: out_values for all stripes of the call, the witness blocks of the bundles back to back in out_witness (cap_hashes hashes of
 * room) and out_witness_first[n_bundles + 1].  out_witness == NULL is the size query: it fills out_witness_first only and launches
 * nothing (out_values may then be NULL too).  One upload, the launches (stripe_bundles.hip: one wave per (bundle, blob, level)), one
 * download, one synchronisation.  A malformed bundle, or cap_hashes below n_blobs * the per-blob total, refuses the whole call:
 * FRIEDA_ERR_ARG, outputs untouched, and frieda_last_error names the bundle.  Only reads the encoded blobs; FRIEDA_ERR_ARG while a proof
 * is in flight on ctx. */
int frieda_open_stripe_bundles(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, uint32_t log_cell, const uint32_t* stripe_index,
                               const uint32_t* bundle_first, uint32_t n_bundles, uint32_t* out_values, uint8_t* out_witness, size_t cap_hashes,
                               uint64_t* out_witness_first);
/* Client, host verifier: no context, one core; the independent bottom-up merge of frieda_verify_cell_bundles run per blob piece.
 * commitments[n_blobs][32]. */
int frieda_verify_stripe_bundles(const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell, const uint32_t* stripe_index,
                                 const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                 const uint64_t* witness_first, uint8_t* out_status);
/* Client, the same status bytes from the GPU: per pass the subtree roots of all (stripe, blob) cells, then one wave per (bundle, blob)
 * merges that blob's list upward.  A bundle stages its indices once and its values and witness n_blobs times; a bundle never straddles
 * two passes.  FRIEDA_ERR_ARG while a proof is in flight on ctx. */
int frieda_verify_stripe_bundles_many(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_domain, uint32_t log_cell,
                                      const uint32_t* stripe_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values,
                                      const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_status);
/* The client's whole block flow from stripe bundles: verify as frieda_verify_stripe_bundles_many does; a bundle is USED only when all
 * n_blobs of its bytes are ACCEPTED; the stripes of the used bundles are de-duplicated by index and all blobs rebuilt by ONE point
 * reconstruction over 4 * n_blobs columns, then every rebuilt blob must commit to its commitment.  The stripe counts needed,
 * *n_stripes_used (the distinct stripes of used bundles), the FRIEDA_ERR_ARG cases (too few stripes, a wrong len: out_bytes untouched,
 * out_status[n_bundles][n_blobs] valid), n_blobs <= 256 and the 2^32-word bound are those of frieda_reconstruct_blobs_from_opened_stripes.
 * out_bytes[n_blobs][len].  There is no per-blob fallback. */
int frieda_reconstruct_blobs_from_stripe_bundles(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor, size_t len,
                                                 uint32_t log_cell, const uint32_t* stripe_index, const uint32_t* bundle_first, uint32_t n_bundles,
                                                 const uint32_t* values, const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_bytes,
                                                 uint8_t* out_status, size_t* n_stripes_used);

/* ---- encoded handles for a block in one call, and straight from a rebuild ---------------------------------------------------------
 * Everything a provider serves starts from a frieda_encoded handle.  The calls below make handles without one frieda_encode per blob:
 * the K handles of a call share ONE allocation in GPU memory, reference-counted: each handle is freed on its own with
 * frieda_encoded_free (from any thread; two threads may free different handles of one call at once), the allocation goes with the last
 * one, and frieda_encoded_bytes of a handle is its own share.  A handle made here is indistinguishable from frieda_encode of the same
 * bytes through every call that takes a handle: the same commitment and shape, byte-identical answers from the openers and
 * byte-identical proofs from frieda_prove_seeds; it outlives the context that made it, as every handle does.  (The tree-skip threshold
 * recorded in a handle may differ: the trees of a call of several blobs are built under FRIEDA_TREE_SKIP_LOG, a lone one under
 * FRIEDA_TREE_SKIP_LONE_LOG; the openers read the threshold from the handle.)  All pointers are host arrays or handles.
 * What the code saves is one allocation and one latency chain per block instead of K, and per rebuild one encode, one tree and two
 * transfers.  Measured on one MI355X against what each call replaces, in one run (profiles/r18_encoded_block.txt,
 * tools/encoded_block_timing.py; records, not gates): frieda_encode_batch 3.00 ms against 6.31 ms for the loop of frieda_encode over 16
 * blobs of 128 KiB, 0.50 ms against 2.61 ms over 64 blobs of 1 KiB; a block of 16 rebuilt from 513 stripes of 64 entries with its handles
 * 3.85 ms (stripe bundles 3.57 ms) against 11.47 ms (11.20 ms) for the reconstruct call followed by 16 frieda_encode, 2.76 / 2.49 ms when
 * the bytes are not wanted; ONE 128 KiB blob rebuilt from 513 cells with its handle 1.00 ms against 1.02 ms (bundles: 1.01 against
 * 1.05 ms) — level with the pair it replaces when the bytes are wanted, not a gain; 0.89 / 0.90 ms without them.  A 2^24 domain: not measured. */
/* Provider of a block: count blobs of len bytes each, blob b at data + b * stride (the layout and the argument rules of
 * frieda_commit_batch: 1 <= count <= 65535, stride >= len when count > 1) -> out_encs[count].  One upload, the batched launches of
 * frieda_commit_batch with the evaluation and the tree kept, one download of the count roots, one synchronisation.  The fused small-domain
 * route and the general route are chosen as frieda_encode chooses.  NOT cut into passes: FRIEDA_ERR_NOMEM when the workspace (blobs plus
 * coefficients) or the allocation of the handles does not fit; ctx stays usable.  Memory: the handles take count * frieda_encoded_bytes;
 * on the general route (domains above 2^15) the workspace is about as large AGAIN, although the blobs and coefficients fill a fraction
 * of it: the kernels take one stride per launch for everything they write, so the coefficients sit at the handles' stride (16 blobs of
 * 128 KiB: 640 MiB of handles and about as much workspace).  The fused small route needs count * len of workspace only.  On any error out_encs is untouched.  FRIEDA_ERR_ARG
 * while a proof is in flight on ctx. */
int frieda_encode_batch(frieda_ctx* ctx, const uint8_t* data, size_t stride, size_t len, uint32_t count, uint32_t log_blowup_factor,
                        frieda_encoded** out_encs);
/* The node that rebuilds in order to serve: each call below is the reconstruct call named beside it plus handles.  On any input it
 * returns FRIEDA_OK exactly when that call does on the same arguments, with the same status bytes and the same *n_..._used, and on
 * FRIEDA_OK the same out_bytes.  (Apart from memory: once the accepted cells are known to suffice, the allocation of the handles is made,
 * n_blobs * frieda_encoded_bytes, and FRIEDA_ERR_NOMEM is possible where the twin needs less.  A call with too few cells allocates
 * nothing for handles.)  out_bytes may be NULL here: the caller wants only the handle, and nothing is packed or downloaded.
 * On FRIEDA_OK out_enc / out_encs[n_blobs] receive handles of the rebuilt blobs; on any error every entry is NULL.
 * Route: verify and pool as the twin does; the point reconstruction's closing re-encode (the one every offered sample is compared
 * with) IS the handle's evaluation; the coefficients must be the image of a blob of len bytes (every felt below 2^30, no bit above the
 * blob's last one, zero padding: otherwise the twin's "does not commit" FRIEDA_ERR_ARG — a committer can publish the root of a
 * polynomial that is no blob's image); one tree over the evaluation gives the root that must equal the commitment.  The rebuilt bytes
 * are never uploaded again.  The block calls keep n_blobs <= 256. */
/* frieda_reconstruct_from_opened_cells + the handle */
int frieda_rebuild_encoded_from_opened_cells(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                             const uint32_t* cell_index, uint32_t n_cells, const uint32_t* values, const uint8_t* paths,
                                             uint8_t* out_bytes, uint8_t* out_status, size_t* n_cells_used, frieda_encoded** out_enc);
/* frieda_reconstruct_from_cell_bundles + the handle */
int frieda_rebuild_encoded_from_cell_bundles(frieda_ctx* ctx, const uint8_t commitment[32], uint32_t log_blowup_factor, size_t len, uint32_t log_cell,
                                             const uint32_t* cell_index, const uint32_t* bundle_first, uint32_t n_bundles, const uint32_t* values,
                                             const uint8_t* witness, const uint64_t* witness_first, uint8_t* out_bytes, uint8_t* out_status,
                                             size_t* n_cells_used, frieda_encoded** out_enc);
/* frieda_reconstruct_blobs_from_opened_stripes + out_encs[n_blobs] */
int frieda_rebuild_encoded_blobs_from_opened_stripes(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor,
                                                     size_t len, uint32_t log_cell, const uint32_t* stripe_index, uint32_t n_stripes,
                                                     const uint32_t* values, const uint8_t* paths, uint8_t* out_bytes, uint8_t* out_status,
                                                     size_t* n_stripes_used, frieda_encoded** out_encs);
/* frieda_reconstruct_blobs_from_stripe_bundles + out_encs[n_blobs] */
int frieda_rebuild_encoded_blobs_from_stripe_bundles(frieda_ctx* ctx, const uint8_t* commitments, uint32_t n_blobs, uint32_t log_blowup_factor,
                                                     size_t len, uint32_t log_cell, const uint32_t* stripe_index, const uint32_t* bundle_first,
                                                     uint32_t n_bundles, const uint32_t* values, const uint8_t* witness,
                                                     const uint64_t* witness_first, uint8_t* out_bytes, uint8_t* out_status,
                                                     size_t* n_stripes_used, frieda_encoded** out_encs);

/* ---- a block under many seeds: n_blobs handles x n_seeds seeds in one call ---------------------------------------------------
 * A sampling client verifies one ordinary proof per commitment before it trusts a cell, so a provider of a block of n_blobs blobs
 * with n_seeds clients owes n_blobs * n_seeds proofs.  frieda_prove_seeds_blobs produces them in ONE launch chain with one wait
 * instead of a loop of n_blobs frieda_prove_seeds calls.
 * Result: out_proofs has n_blobs * n_seeds entries, blob-major; out_proofs[b * n_seeds + s] serialises to exactly the bytes of
 * frieda_prove_seeds(encs[b], &seeds[s], 1, ...), i.e. of frieda_commit_and_generate_proof of blob b under seeds[s].  The one seed
 * list is shared by all blobs: a client's seed asks for the whole block.  Entries are released with frieda_proof_free.
 * Arguments: all pointers non-null; 1 <= n_blobs, 1 <= n_seeds, n_blobs * n_seeds <= 65535 (the batch count limit); every handle of
 * the list has the same len and log_blowup, cfg.log_blowup_factor equals it, and every handle belongs to the device of ctx; a breach
 * returns FRIEDA_ERR_ARG.  Every other rule of frieda_prove_seeds_begin applies as there.
 * Handles: from one frieda_encode_batch, from lone frieda_encode calls, from a rebuild, or any mix; encoded under different tree-skip
 * thresholds; the same handle more than once.  The call only reads them: another context may open cells of them or prove from them
 * meanwhile.
 * Channel: more than one job needs the transcript kernels (last layer <= 2^11 points, host-channel policy off), else FRIEDA_ERR_ARG,
 * as frieda_prove_seeds for two seeds; n_blobs == n_seeds == 1 works under both policies (it IS frieda_prove_seeds).
 * _begin enqueues without synchronising, _finish waits once; one job per context.  The two finishes frieda_prove_seeds_finish and
 * frieda_prove_seeds_blobs_finish are one function: each completes whichever proving job is in flight and writes one proof per job.
 * Memory: the call is NOT cut into passes.  frieda_seeds_blobs_workspace_bytes(len, cfg, n_blobs, n_seeds) is what the call asks of
 * the context, the handles excluded; 0 for a refused shape; at n_blobs == 1 it equals frieda_seeds_workspace_bytes.  A call too
 * large for the GPU returns FRIEDA_ERR_NOMEM and leaves ctx usable: cut the seed list or the block — or hand the same jobs to
 * frieda_prove_jobs (below), which cuts them into passes itself. */
int frieda_prove_seeds_blobs_begin(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, const uint64_t* seeds, uint32_t n_seeds,
                                   frieda_pcs_config cfg);
int frieda_prove_seeds_blobs_finish(frieda_ctx* ctx, frieda_proof** out_proofs);
int frieda_prove_seeds_blobs(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, const uint64_t* seeds, uint32_t n_seeds,
                             frieda_pcs_config cfg, frieda_proof** out_proofs);
size_t frieda_seeds_blobs_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint32_t n_seeds);

/* ---- any list of (handle, seed) jobs in one call, cut into passes -------------------------------------------------------------
 * A provider's request queue is no rectangle: one client asks for blobs 0, 3 and 7 under its seed, another for blob 3 under its own,
 * a third for the whole block.  frieda_prove_jobs takes the queue as it is: job j is encs[blob_index[j]] under seeds[j].
 * Result: out_proofs has n_jobs entries in the CALLER's order; out_proofs[j] serialises to exactly the bytes of
 * frieda_prove_seeds(encs[blob_index[j]], &seeds[j], 1, cfg).  Any list is legal: a blob with many jobs or with one, a handle of the
 * list that no job names, the same (blob, seed) pair twice (proved twice: nothing is de-duplicated), the same handle at two positions.
 * Inside, the jobs run sorted by blob (a stable sort), so that the seed-looped first fold reads a blob's evaluation once per group of
 * FRIEDA_SEEDS_FOLD_GROUP jobs of that blob; the rectangle of frieda_prove_seeds_blobs is the list that is sorted as it stands, and runs
 * through the same code.
 * Arguments: all pointers non-null, every handle non-null; n_blobs >= 1, n_jobs >= 1, every blob_index[j] < n_blobs; the handle rules,
 * the channel rule (more than one job needs the transcript kernels) and the one-job-per-context rule are those of
 * frieda_prove_seeds_blobs_begin; a breach returns FRIEDA_ERR_ARG.  No parameter is device memory.
 * _begin / _finish are ONE pass: n_jobs <= 65535, frieda_prove_jobs_workspace_bytes(len, cfg, n_blobs, n_jobs) is what _begin asks of
 * the context (0 for a refused shape; at n_blobs == 1 it equals frieda_seeds_workspace_bytes(len, cfg, n_jobs), at (K, K * S) it equals
 * frieda_seeds_blobs_workspace_bytes(len, cfg, K, S): the table is the same table), and a call too large returns FRIEDA_ERR_NOMEM and
 * leaves ctx usable.  frieda_prove_jobs_finish is the one finish frieda_prove_seeds_finish is.
 * frieda_prove_jobs, the synchronous form, is cut into passes and has no cap on n_jobs.  The rule is what frieda_prove_jobs_plan
 * returns: jobs_per_pass is the largest p in [1, min(n_jobs, 65535)] with frieda_prove_jobs_workspace_bytes(len, cfg, min(n_blobs, p), p)
 * within the limit (1 when not even one job is), the limit being the batch policy's budget (FRIEDA_BATCH_BUDGET_MB, see below; ctx ==
 * NULL: the default options) or the arena limit of the test hook when that is set and smaller; n_passes = ceil(n_jobs / jobs_per_pass),
 * the pass sizes equal to within one.  A pass takes consecutive jobs of the sorted list — it may take only some of one blob's jobs —
 * and its table holds only the blobs it names.  A pass that still meets FRIEDA_ERR_NOMEM (the device holds less than the budget)
 * makes the call halve jobs_per_pass and go on from the first unfinished job, down to one job per pass; only then does the error
 * reach the caller.  On any failure every proof already produced is freed and out_proofs is all null.
 * Measured on MI355X on sparse queues (every client names a quarter of the blobs; blow-up 16, 20 queries, 20-bit proof of work; HIP-event
 * medians of 21 alternated calls, profiles/r22_prove_jobs.txt) against the loop of frieda_prove_seeds per distinct blob and against
 * frieda_prove_seeds_blobs on the bounding rectangle: 256 jobs over 64 handles of 1 KiB 5.29 against 16.91 and 19.67 ms, 128 jobs over 16
 * handles of 128 KiB 6.62 against 13.84 and 22.80 ms, 16 jobs over 4 handles of a 2^22 domain 3.64 against 5.16 and 12.67 ms; the
 * rectangle's own list costs 0.06 - 0.27 ms more through this call than through frieda_prove_seeds_blobs (host work per job), and an
 * extra pass 0.4 - 0.7 ms.  Other shapes are not measured. */
int frieda_prove_jobs_begin(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, const uint32_t* blob_index,
                            const uint64_t* seeds, uint32_t n_jobs, frieda_pcs_config cfg);
int frieda_prove_jobs_finish(frieda_ctx* ctx, frieda_proof** out_proofs);
int frieda_prove_jobs(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, const uint32_t* blob_index, const uint64_t* seeds,
                      uint32_t n_jobs, frieda_pcs_config cfg, frieda_proof** out_proofs);
size_t frieda_prove_jobs_workspace_bytes(size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint32_t n_jobs);
int frieda_prove_jobs_plan(const frieda_ctx* ctx, size_t len, frieda_pcs_config cfg, uint32_t n_blobs, uint32_t n_jobs, uint32_t* jobs_per_pass,
                           uint32_t* n_passes);

/* ---- block proofs: ONE FRI proof for all blobs of a block ---------------------------------------------------------------------
 * Everything above rests on one ordinary proof per commitment: n_blobs * n_seeds fold chains for the provider of a block, n_blobs
 * proofs to download and verify for a client before it may trust one cell.  Batched FRI removes the factor n_blobs.  The blobs stay
 * committed exactly as they are (commitments[k] = frieda_commit of blob k); a challenge rho in QM31 is drawn from ALL the commitments;
 * ONE FRI instance runs over g = sum over k of rho^k * f_k, f_k the codeword of blob k read as QM31 values; where that proof queried g,
 * every f_k is opened against its own commitment, and the client checks the linear combination there.  A provider owes n_seeds proofs
 * per block instead of n_blobs * n_seeds; a client verifies one proof per block instead of n_blobs.
 * THIS IS A PROTOCOL OF THIS PROJECT, not of the reference and not of stwo's FRI prover: the reference passes one column to
 * FriProver::commit, and stwo batches equal-size columns in its PCS quotient step, which is out of scope here.
 * Soundness is the usual random-linear-combination argument for FRI (if some f_k is far from the code, g is far from it for all but a
 * negligible fraction of rho; rho is a Fiat-Shamir challenge over all the commitments, drawn from the 2^124-element field); the argument
 * as applied here is UNREVIEWED.  A block proof is not a frieda Proof and no reference verifier takes it; its FRI
 * part IS an ordinary proof, of a polynomial that is no blob's image.
 * rho (frieda_block_challenge; host only, no context, no GPU): a default Blake2sChannel, mix_u64(n_blobs), mix_root(commitments[k]) for
 * k = 0 .. n_blobs - 1 in order, one draw_felt.  commitments[n_blobs][32]; 1 <= n_blobs <= 65535.
 * The aggregate handle (frieda_aggregate_encoded): an ordinary frieda_encoded of the blobs' shape in an allocation of its own, whose
 * evaluation at every domain position p is sum over k of rho^k * f_k(p) — f_k(p) the four coordinate columns of encs[k] at p, rho from
 * the handles' commitments — and whose tree and root are the tree build of a lone call over that evaluation.  It does not depend on any
 * seed: make it once per block.  Every call that takes a handle takes it unchanged (frieda_prove_seeds, frieda_prove_jobs, the cell
 * openers: they read the evaluation and the tree); frieda_encoded_shape is the blobs'; frieda_encoded_aggregate_of returns n_blobs (0 for
 * a blob's own handle).  Its coefficients are no blob's image: it cannot come out of a frieda_rebuild_encoded_* call.  Handles as for
 * frieda_prove_seeds_blobs_begin: one shape, on ctx's device, from any mix of slabs and tree-skip thresholds, an entry may repeat; the
 * call only reads them.  One upload (the table of n_blobs evaluation pointers), the combination kernel (aggregate.hip: per position 16
 * bytes read per blob and 16 written, one multiplication by rho and one addition per blob; for >= 8 blobs on domains below 2^18 points
 * the blob range is split over the waves of a workgroup, option FRIEDA_AGG_SPLIT — identical words either way), the tree, one download,
 * one synchronisation.  FRIEDA_ERR_ARG: a NULL entry, mixed shapes, n_blobs out of 1 .. 65535, another device, a proof in flight on ctx.
 * Block proofs under many seeds (frieda_prove_block_seeds): out[n_seeds], out[s] under seeds[s], each released with
 * frieda_block_proof_free.  A frieda_block_proof holds
 *   the FRI part      exactly the frieda_proof that frieda_prove_seeds(agg, &seeds[s], 1, cfg) gives, and
 *   the opening part  exactly what frieda_open_stripe_bundles(encs, n_blobs, log_cell = 1, idx, {0, k}, 1, ...) gives as one bundle,
 *                     idx the strictly ascending distinct q >> 1 over the FRI part's first-layer queries q: FRI opens the bit-reversed
 *                     evaluation in pairs {2 i, 2 i + 1}, and pair i is cell i at log_cell 1.
 * Route: frieda_prove_seeds on agg (one pass, its limits; first synchronisation), the query positions of every proof by replaying its
 * transcript on the host (nothing is verified to learn them), the n_seeds bundles in ONE frieda_open_stripe_bundles launch chain (second
 * synchronisation).  Arguments: cfg.n_queries <= FRIEDA_MAX_BUNDLE_CELLS; agg an aggregate of exactly n_blobs blobs whose recorded rho
 * equals frieda_block_challenge of these handles' commitments (nothing is aggregated again to check); otherwise the rules of the two
 * calls it is made of.  On failure nothing is returned (out is all NULL), everything is freed and ctx stays usable.
 * Accessors, in the layouts of frieda_verify_stripe_bundles (which can be applied to them directly with log_cell 1, one bundle,
 * bundle_first {0, n_stripes}, witness_first {0, witness_hashes}): stripe_index[n_stripes], values[n_stripes][n_blobs][4][2],
 * witness[n_blobs][witness_hashes][32]; pointers stay valid until frieda_block_proof_free.  frieda_block_proof_fri is owned by the
 * block proof.  Wire image (little-endian): magic "FBP1", version 1, n_blobs, n_stripes (u32 each), witness_hashes, proof_bytes (u64
 * each), the proof's image, then the three arrays; buf == NULL returns the size needed.  Deserialising applies the
 * bundle's malformed rule to the indices on the proof's domain, requires witness_hashes to be the count they give and the image to have
 * exactly the length its header gives: any violation, a bad proof image included, is FRIEDA_ERR_ARG.
 * The client's check (frieda_verify_block; host only, one core): *ok is set exactly when, in this order, (a) n_blobs and the shape
 * agree, (b) frieda_verify_pairs accepts the FRI part under seed, (c) the stripe indices are exactly the ascending distinct q >> 1 of
 * that proof's queries, (d) frieda_verify_stripe_bundles gives ACCEPTED for every blob against commitments, (e) at every opened pair and
 * both of its entries sum over k of rho^k * value_k equals the value frieda_verify_pairs returned there, rho =
 * frieda_block_challenge(commitments, n_blobs).  *out_reason (may be NULL) names the first failing step, FRIEDA_BLOCK_OK when none does.
 * FRIEDA_ERR_INVARIANT where frieda_verify_pairs returns it.  A device form for many block proofs does not exist yet.
 * Measured on one MI355X in one run (profiles/r24_block_proof.txt, tools/block_proof_timing.py; blow-up 16, 20 queries, 20-bit proof of work;
 * HIP-event medians of 21 alternated calls; records, not gates): frieda_prove_block_seeds against frieda_prove_seeds_blobs on the same
 * handles and seeds: 64 blobs of 1 KiB x 4 seeds 0.46 against 5.15 ms, 16 blobs of 128 KiB x 8 seeds 1.10 against 6.36 ms, 4 blobs of a
 * 2^22 domain x 4 seeds 1.45 against 3.71 ms; frieda_aggregate_encoded, once per block, 0.08 / 0.35 / 0.51 ms (its kernel alone 12 / 26 / 78
 * us: 0.68 of the 8.0 TB/s HBM specification at 16 x 128 KiB, 0.54 at 4 x 2^22).  One serialised block proof against the K proofs of the same
 * seed: 0.26 against 0.81 MB, 0.20 against 1.02 MB, 0.13 against 0.38 MB.  frieda_verify_block on one core against K x frieda_verify: 0.80
 * against 4.88 ms, 0.59 against 4.04 ms, 0.43 against 1.35 ms.  The block form won at every measured shape: use it where a client can
 * take this project's own proof; use frieda_prove_seeds_blobs where the proofs must be ones the reference's verifier accepts.  Other
 * shapes are not measured. */
#define FRIEDA_BLOCK_OK 0
#define FRIEDA_BLOCK_SHAPE 1
#define FRIEDA_BLOCK_FRI 2
#define FRIEDA_BLOCK_INDICES 3
#define FRIEDA_BLOCK_BUNDLE 4
#define FRIEDA_BLOCK_COMBINATION 5
typedef struct frieda_block_proof frieda_block_proof;
int frieda_block_challenge(const uint8_t* commitments, uint32_t n_blobs, uint32_t out_rho[4]);
int frieda_aggregate_encoded(frieda_ctx* ctx, const frieda_encoded* const* encs, uint32_t n_blobs, frieda_encoded** out);
uint32_t frieda_encoded_aggregate_of(const frieda_encoded* enc);
int frieda_prove_block_seeds(frieda_ctx* ctx, const frieda_encoded* agg, const frieda_encoded* const* encs, uint32_t n_blobs, const uint64_t* seeds,
                             uint32_t n_seeds, frieda_pcs_config cfg, frieda_block_proof** out);
int frieda_verify_block(const uint8_t* commitments, uint32_t n_blobs, const frieda_block_proof* bp, const uint64_t* seed, int* ok, uint32_t* out_reason);
void frieda_block_proof_free(frieda_block_proof* bp);
const frieda_proof* frieda_block_proof_fri(const frieda_block_proof* bp);
uint32_t frieda_block_proof_n_blobs(const frieda_block_proof* bp);
uint32_t frieda_block_proof_n_stripes(const frieda_block_proof* bp);
const uint32_t* frieda_block_proof_stripe_index(const frieda_block_proof* bp);
const uint32_t* frieda_block_proof_values(const frieda_block_proof* bp);
const uint8_t* frieda_block_proof_witness(const frieda_block_proof* bp);
uint64_t frieda_block_proof_witness_hashes(const frieda_block_proof* bp);
size_t frieda_block_proof_serialize(const frieda_block_proof* bp, uint8_t* buf, size_t cap);
int frieda_block_proof_deserialize(const uint8_t* buf, size_t len, frieda_block_proof** out);

/* ---- batch policy: how a stream of equal-length blobs is cut into batched calls ("bytes in flight") -------------------------
 * Every kernel of a batched call covers all its blobs, so the launch / Fiat-Shamir latency chain is paid once per call: small
 * blobs want many per call, large blobs few (the device workspace grows with the count).  The library's rule — what
 * frieda_prove_many / frieda_commit_many apply per device, offered here to callers that drive _begin / _finish themselves (the
 * caller loop of benches/proof.rs:30-44 over many blobs):
 *     per_call = clamp(budget / frieda_workspace_bytes(blob), 1, min(4096, ceil(count / (calls_per_ctx * in_flight))))
 *     calls    = the smallest multiple of in_flight with no call above per_call, sizes equal to within one
 * budget: context option "FRIEDA_BATCH_BUDGET_MB" (0 = default: the workspace of sixteen proofs on a 2^24 domain, ~43 GB per call in flight — lower it on a shared device);
 * calls_per_ctx: option "FRIEDA_BATCH_CALLS_PER_CTX" (default 1: one call per context when the budget allows — measured equal to
 * two at the 2^22 / 2^24 domains and faster below, where a call is mostly its latency chain; raise it to bound a call's latency).
 * in_flight = the contexts taking turns (frieda_prove_many uses 2 per device).
 * frieda_workspace_bytes: device workspace one blob of `len` bytes adds to a batched call (prove != 0: commit_and_generate_proof,
 * else commit); 0 when the shape is outside what the entry points accept.
 * frieda_batch_plan: out_calls[0 .. *n_calls) receive the blob count of each call, in order (sum = count); ctx == NULL uses the
 * default options; out_calls == NULL only counts; FRIEDA_ERR_ARG when cap is too small or the shape is invalid. */
size_t frieda_workspace_bytes(size_t len, uint32_t log_blowup_factor, uint32_t log_last_layer_degree_bound, int prove);
int frieda_batch_plan(const frieda_ctx* ctx, size_t len, uint32_t log_blowup_factor, uint32_t log_last_layer_degree_bound, int prove,
                      uint32_t count, uint32_t in_flight, uint32_t* out_calls, size_t cap, uint32_t* n_calls);

/* ---- multi-GPU: a batch of independent blobs across the GPUs of one node ---------------------------------------------
 * What a caller looping api::commit / commit_and_generate_proof over blobs gets on an 8 x MI355X node
 * (src/lib.rs:31-38; benches/commit.rs:11-15, benches/proof.rs:30-44).  The path shards at blob granularity: blob i runs
 * on devices[i mod n], one host thread and two contexts per device (two calls in flight; a run of equal-length blobs on a
 * device goes through the batched kernels, cut into calls by the batch policy above — options set on frieda_multi_ctx(m, d)
 * apply to device slot d), no data-path collective.  The
 * only exchange is the gather of the 32-byte commitment roots: one ncclAllGather per device on a single-process
 * communicator (ncclCommInitAll; RCCL over xGMI), after which every device holds every root; the host reads device 0's
 * copy.  n == 1 needs no exchange and does not touch RCCL.  RCCL is bound at frieda_multi_create by dlopen("librccl.so.1")
 * (an instance already in the process — PyTorch's — is shared); creation fails with FRIEDA_ERR_HIP if it cannot be loaded.
 * blobs / lens: host arrays of `count` pointers / byte lengths (lengths may differ); out_roots / out_commitments:
 * count * 32 bytes in blob order; out_proofs: count handles, each released with frieda_proof_free; seeds == NULL is None
 * for every blob, else seeds[i] is Some.  A handle is not thread-safe; results are exactly those of `count` separate
 * single-GPU calls. */
typedef struct frieda_multi frieda_multi;
int frieda_multi_create(const int* devices, uint32_t n_devices, frieda_multi** out);
int frieda_multi_destroy(frieda_multi* m);
uint32_t frieda_multi_device_count(const frieda_multi* m);
const char* frieda_multi_last_error(const frieda_multi* m);
/* 1 when root gathers go through RCCL (n > 1, or FRIEDA_MULTI_FORCE_RCCL=1); collectives issued so far */
int frieda_multi_uses_rccl(const frieda_multi* m);
uint64_t frieda_multi_gather_count(const frieda_multi* m);
/* Each device's worker thread is pinned to the CPUs of that GPU's NUMA node (sysfs numa_node of its PCI function, intersected with
 * the process's affinity; FRIEDA_MULTI_NO_NUMA_PIN=1 or a platform that reports none: not pinned).  Returns how many CPUs slot d's
 * worker is pinned to (0: not pinned) and writes up to cap of them. */
uint32_t frieda_multi_near_cpus(const frieda_multi* m, uint32_t device_slot, int* out_cpus, size_t cap);
/* Frees the device workspaces (two per device, up to the batch budget each) and upload rings the handle keeps between calls;
 * twiddle caches stay.  The next call allocates again.  FRIEDA_ERR_ARG while a call is in flight. */
int frieda_multi_release_workspace(frieda_multi* m);
/* the first context of device slot d (e.g. to set a policy on it); owned by the handle */
frieda_ctx* frieda_multi_ctx(frieda_multi* m, uint32_t device_slot);
int frieda_commit_many(frieda_multi* m, const uint8_t* const* blobs, const size_t* lens, uint32_t count, uint32_t log_blowup_factor,
                       uint8_t* out_roots);
int frieda_prove_many(frieda_multi* m, const uint8_t* const* blobs, const size_t* lens, uint32_t count, const uint64_t* seeds,
                      frieda_pcs_config cfg, uint8_t* out_commitments, frieda_proof** out_proofs);

/* ---- struct Proof (src/proof.rs:19-26) accessors; fields are `pub` upstream, hence the setters --- */
void frieda_proof_free(frieda_proof* p);
int frieda_proof_clone(const frieda_proof* p, frieda_proof** out);
uint64_t frieda_proof_proof_of_work(const frieda_proof* p);
void frieda_proof_set_proof_of_work(frieda_proof* p, uint64_t nonce);
frieda_pcs_config frieda_proof_pcs_config(const frieda_proof* p);
uint32_t frieda_proof_log_size_bound(const frieda_proof* p);
/* evaluations: Vec<QM31>, 4 little-endian u32 coordinates each; pointer stays valid until the next
 * resize/free */
size_t frieda_proof_n_evaluations(const frieda_proof* p);
uint32_t* frieda_proof_evaluations(frieda_proof* p);
int frieda_proof_resize_evaluations(frieda_proof* p, size_t n);
/* FriProof: layer 0 = first_layer, 1..n_inner = inner_layers */
size_t frieda_proof_n_inner_layers(const frieda_proof* p);
const uint8_t* frieda_proof_layer_commitment(const frieda_proof* p, size_t layer);
const uint32_t* frieda_proof_layer_fri_witness(const frieda_proof* p, size_t layer, size_t* n_qm31);
const uint8_t* frieda_proof_layer_hash_witness(const frieda_proof* p, size_t layer, size_t* n_hashes);
const uint32_t* frieda_proof_layer_column_witness(const frieda_proof* p, size_t layer, size_t* n_m31);
const uint32_t* frieda_proof_last_layer_poly(const frieda_proof* p, size_t* n_qm31);
/* canonical little-endian wire image (layout in DESIGN.md §6).  buf == NULL returns the size needed. */
size_t frieda_proof_serialize(const frieda_proof* p, uint8_t* buf, size_t cap);
int frieda_proof_deserialize(const uint8_t* buf, size_t len, frieda_proof** out);

/* ---- Level B: backend-trait granular operations on device buffers ------------------------------- */
/* The buffer contract of every device pointer of this header (Level A's d_data / d_out_root included):
 * A device pointer to words needs 4-byte alignment, a pointer to bytes none, and a pointer to hashes 16 bytes, unless the function says otherwise. No call writes outside the extents it documents. No call modifies a `const` argument.
 * Anything beyond those alignments only selects a faster kernel for the same result (16-byte aligned columns whose stride is a multiple
 * of 4 words take the vector routes).  A hash pointer that is not 16-byte aligned is refused with FRIEDA_ERR_ARG before anything is
 * launched.  The exceptions: frieda_merkle_root's d_root and frieda_commit_device's d_out_root (one hash, stored by words: 4-byte
 * alignment is enough) and frieda_dev_gather_device's d_idx (64-bit indices: 8-byte alignment, else FRIEDA_ERR_ARG). */
/* Column<T> storage */
int frieda_dev_alloc(frieda_ctx* ctx, size_t bytes, void** d_out);
int frieda_dev_free(frieda_ctx* ctx, void* d);
int frieda_dev_upload(frieda_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int frieda_dev_download(frieda_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

/* Column::at(index) (stwo core/backend Column<T>; CpuBackend is `Vec<T>` indexing — the accessor frieda's evaluation gather
 * uses, src/proof.rs:62-66): one element of a device column to the host.  Synchronises the ctx stream (it is a debugging /
 * trait-completeness accessor, not a hot path — the prover gathers its openings on the device).
 * frieda_dev_at: M31 column.  frieda_dev_at_secure: QM31 from a SecureColumn d_cols[4][stride] (SoA), out = 4 coordinates. */
int frieda_dev_at(frieda_ctx* ctx, const uint32_t* d_col, size_t index, uint32_t* out);
int frieda_dev_at_secure(frieda_ctx* ctx, const uint32_t* d_cols, size_t stride, size_t index, uint32_t out[4]);

/* Batched Column::at — what frieda's evaluation gather (src/proof.rs:62-66, `column.at(q)` per query) and a HipBackend's openings
 * want instead of one synchronised copy per value.  d_cols: ncols columns `stride` words apart, each `stride` words long (ncols = 4,
 * stride = 2^log_size: a SecureColumn); idx: host array of n indices in any order, repeats allowed.  out[n][ncols] (host, row-major
 * per index: with ncols = 4 each row is the QM31 frieda_dev_at_secure returns).  One upload of the indices through the context's
 * pinned staging, one kernel, one download, one synchronisation.  Any index >= stride: FRIEDA_ERR_ARG before anything is launched,
 * out untouched.  n = 0 is a no-op.  Uses the context's workspace: FRIEDA_ERR_ARG while a proof is in flight on it. */
int frieda_dev_gather(frieda_ctx* ctx, const uint32_t* d_cols, size_t stride, uint32_t ncols, const uint64_t* idx, size_t n, uint32_t* out);
/* the same for a column of 32-byte hashes (one layer of a stored tree: layer_len hashes, 16-byte aligned); out: n x 32 bytes (host) */
int frieda_dev_gather_hashes(frieda_ctx* ctx, const void* d_layer, size_t layer_len, const uint64_t* idx, size_t n, uint8_t* out);
/* asynchronous form on the ctx stream: d_idx[n] (8-byte aligned, else FRIEDA_ERR_ARG) and d_out[n][ncols] in device memory.  The
 * indices are not checked on the host: the row of an index >= stride is filled with 0xFFFFFFFF (not a canonical M31).  Available while
 * a proof is in flight. */
int frieda_dev_gather_device(frieda_ctx* ctx, const uint32_t* d_cols, size_t stride, uint32_t ncols, const uint64_t* d_idx, size_t n,
                             uint32_t* d_out);

/* MerkleProver::decommit (stwo core/vcs/prover.rs) for a tree whose columns all sit on the leaf layer — the shape of every tree
 * frieda builds and of frieda_merkle_commit's.  Restriction: trees with columns above the leaf layer are not supported; for this
 * shape the column witness is always empty, so it is not returned.
 * d_layers: host array of log_size + 1 device pointers by layer log (layer j: 2^j hashes, 16-byte aligned; layer 0, the root, is not
 * read) — either a frieda_merkle_commit buffer with pointers d_layers[j] = buf + frieda_merkle_layer_offset(log_size, j), or layers
 * built one by one with frieda_merkle_commit_layer into separate buffers.  d_cols: the ncols leaf columns (2^log_size words each,
 * `stride` words apart; ncols = 0: no values).  positions: host, strictly ascending, < 2^log_size (else FRIEDA_ERR_ARG before any
 * launch); any count up to 2^log_size.  out_values[n_pos][ncols]: the queried column values.  out_hashes: the hash witness in
 * stwo's order (bottom-up; per layer, per node in ascending order, the left then the right child's hash when that child is not
 * already known).  *n_hashes receives its length; a cap_hashes smaller than that gives FRIEDA_ERR_ARG (out_hashes == NULL asks
 * for the size).  No witness is longer than sum over s = 1 .. log_size of min(n_pos, 2^(log_size - s)) <= n_pos * log_size hashes.
 * One upload, the launches, one download, one synchronisation; uses the context's workspace (FRIEDA_ERR_ARG while a proof is in
 * flight on it). */
int frieda_merkle_decommit(frieda_ctx* ctx, const void* const* d_layers, uint32_t log_size, const uint32_t* d_cols, uint32_t ncols, size_t stride,
                           const uint32_t* positions, size_t n_pos, uint32_t* out_values, uint8_t* out_hashes, size_t cap_hashes, size_t* n_hashes);
/* asynchronous form on the ctx stream, everything on the device: d_positions[n_pos] in, d_out_values[n_pos][ncols] and the hash witness
 * (d_out_hashes, 16-byte aligned, sized by the caller for n_pos * log_size hashes) out; the witness length goes to the device word
 * *d_n_hashes, 0xFFFFFFFF when the positions are not strictly ascending and below 2^log_size (then nothing else is written).  Lists of
 * up to 512 positions take one launch and no workspace (option FRIEDA_OPEN_SMALL_MAX); longer ones use the context's workspace
 * (FRIEDA_ERR_ARG while a proof is in flight).  Queue every layer's decommitment, then download once. */
int frieda_merkle_decommit_device(frieda_ctx* ctx, const void* const* d_layers, uint32_t log_size, const uint32_t* d_cols, uint32_t ncols,
                                  size_t stride, const uint32_t* d_positions, size_t n_pos, uint32_t* d_out_values, void* d_out_hashes,
                                  uint32_t* d_n_hashes);
/* ColumnOps::bit_reverse_column (stwo core/backend/mod.rs; the trait surface `CirclePoly::<CpuBackend>::new` and
 * `SecureCirclePoly` are instantiated over at src/utils.rs:21,28 and src/proof.rs:47-52): in place, v[i] <-> v[brev(i)] over
 * log_size bits, for each of ncols columns of 2^log_size words laid out `stride` words apart (ncols = 1: a BaseField
 * column; ncols = 4, stride = 2^log_size: a SecureColumn).  Asynchronous on the ctx stream. */
int frieda_bit_reverse_column(frieda_ctx* ctx, uint32_t* d_cols, size_t stride, uint32_t ncols, uint32_t log_size);

/* codec, src/utils.rs:10-33: d_bytes[len] -> d_coef[n_out] felts (30-bit LSB-first chunks), zero padded
 * to n_out words.  frieda_codec_shape gives F (felts), F' (padded) and L (per-column log size). */
int frieda_codec_shape(size_t len, size_t* n_felts, size_t* n_padded, uint32_t* log_size);
int frieda_unpack30(frieda_ctx* ctx, const void* d_bytes, size_t len, uint32_t* d_coef, size_t n_out);

/* PolyOps::precompute_twiddles(Coset::half_odds(log_domain - 1)): device tables of 2^(log_domain-1) words
 * each (levels N/4, N/8, ..., 1, pad 1) owned by the ctx */
int frieda_precompute_twiddles(frieda_ctx* ctx, uint32_t log_domain, const uint32_t** d_twiddles,
                               const uint32_t** d_inv_twiddles);
/* PolyOps::evaluate on CircleDomain of log size log_domain for ncols polynomials of 2^log_coef coefficients
 * each: d_coef[ncols][2^log_coef] -> d_out[ncols][2^log_domain], bit-reversed order */
int frieda_circle_evaluate(frieda_ctx* ctx, const uint32_t* d_coef, uint32_t ncols, uint32_t log_coef,
                           uint32_t log_domain, uint32_t* d_out);

/* ---- reconstruction side (not called by frieda's three functions) ----
 * PolyOps::interpolate generalised to one aligned block of the codeword: d_block[ncols][2^log_coef] holds entries
 * block * 2^log_coef .. (block + 1) * 2^log_coef of each column of the bit-reversed evaluation on the 2^log_domain domain
 * (any block < 2^(log_domain - log_coef), i.e. any 1 / 2^B of the codeword); d_coef[ncols][2^log_coef] receives the
 * coefficients.  block = 0 with log_coef == log_domain is stwo's CpuBackend::interpolate. */
int frieda_circle_interpolate(frieda_ctx* ctx, const uint32_t* d_block, uint32_t ncols, uint32_t log_coef, uint32_t log_domain,
                              uint32_t block, uint32_t* d_coef);
/* inverse of frieda_unpack30 (src/utils.rs:10-19 read backwards): n_felts 30-bit felts -> the first len bytes */
int frieda_pack30(frieda_ctx* ctx, const uint32_t* d_felts, size_t n_felts, void* d_bytes, size_t len);
/* both together for frieda's 4-column layout: a block of the 4 evaluation columns -> the original len bytes */
int frieda_reconstruct_device(frieda_ctx* ctx, const uint32_t* d_block, uint32_t log_coef, uint32_t log_domain, uint32_t block,
                              size_t len, void* d_out_bytes);

/* Reconstruction from scattered cells — what a sampling client holds.  A cell is an aligned run of 2^log_cell consecutive
 * entries (log_cell >= 0; log_cell == 0: single sampled points, README.md:56-69's sample() flow) of the bit-reversed evaluation, the same run of every column: cell c = entries c * 2^log_cell ..
 * (c + 1) * 2^log_cell, c < 2^(log_domain - log_cell).  ANY n_cells = 2^(log_coef - log_cell) distinct cells (at most
 * 2^FRIEDA_MAX_LOG_CELLS = 4096) determine the polynomial: every cell's block transform is undone on the device, then a
 * n_cells x n_cells linear system recombines the coefficient slices (inverted on the host up to 256 cells, by a blocked
 * Gauss-Jordan on the device beyond: cubic in n_cells, ~50 ms at 4096).  d_cells[n_cells][ncols][2^log_cell] (cell-major),
 * cell_index: host array.  n_cells == 1 is frieda_circle_interpolate with block = cell_index[0].  FRIEDA_ERR_ARG for repeated or
 * out-of-range cells (and for a singular system, which distinct cells have never produced). */
int frieda_circle_interpolate_cells(frieda_ctx* ctx, const uint32_t* d_cells, const uint32_t* cell_index, uint32_t n_cells, uint32_t ncols,
                                    uint32_t log_cell, uint32_t log_coef, uint32_t log_domain, uint32_t* d_coef);
/* Over-determined form (what a client that sampled a few positions too many holds): n_avail >= 2^(log_coef - log_cell) cells are
 * offered (d_cells[n_avail][ncols][2^log_cell], cell_index[n_avail]; repeated indices are tolerated); the call takes, in the order
 * given, 2^(log_coef - log_cell) of them whose rows of the cell matrix are linearly independent and reconstructs from those — so a
 * point set that happens to be singular (possible with single points, log_cell == 0) costs a spare sample instead of an error.
 * out_used (optional, 2^(log_coef - log_cell) words): positions in the caller's list of the cells used.  At most 256 needed cells
 * (the selection runs on the host); FRIEDA_ERR_ARG when the offered cells do not span the polynomial space.  A client holding at
 * least two points more than the polynomial has coefficients needs neither the selection nor the bound: see
 * frieda_circle_interpolate_points below. */
int frieda_circle_interpolate_cells_any(frieda_ctx* ctx, const uint32_t* d_cells, const uint32_t* cell_index, uint32_t n_avail, uint32_t ncols,
                                        uint32_t log_cell, uint32_t log_coef, uint32_t log_domain, uint32_t* d_coef, uint32_t* out_used);
/* the same for frieda's 4-column layout, followed by the packer: scattered cells -> the original len bytes */
int frieda_reconstruct_cells_device(frieda_ctx* ctx, const uint32_t* d_cells, const uint32_t* cell_index, uint32_t n_cells, uint32_t log_cell,
                                    uint32_t log_coef, uint32_t log_domain, size_t len, void* d_out_bytes);

/* Reconstruction from ANY sufficiently large set of samples, with no bound on their number (the README's sample() flow at blob
 * scale: the reference's 128 KiB `blob` fixture has 2^15 coefficients per column — 2^15 + 2 single sampled points of its 2^19
 * codeword rebuild it).  Same cell layout as above (d_cells[n_cells][ncols][2^log_cell], cell_index[n_cells] on the host; repeated
 * cells are ignored); the distinct points offered must number at least 2^log_coef + 2.  No system is solved: with S the first
 * 2^log_coef + 2 points, V_D the vanishing polynomial of the domain and Z_S the product of the lines through pairs of S, the
 * quotient Z = V_D / Z_S vanishes on everything outside S, Z * p is known on the whole domain, and p follows by transforms and one
 * pointwise division on a disjoint domain (erasure.hip).  With log_cell >= 1, S is the first 2^(log_coef - log_cell) + 1 whole
 * cells and Z_S the product of their cell polynomials pi^(log_cell - 1)(x) - k_cell instead.  Cost: five transforms + ~2^(2 log_coef
 * - log_cell) multiplications below 2^15 coefficients; from there on (single points, or many small cells) Z_S comes from a product
 * tree, O(K log^2 K) (a 15.7 MB blob from 2^20 + 2 points of its 2^24 codeword: 3.2 ms).
 * 1 <= log_coef <= log_domain <= FRIEDA_MAX_LOG_DOMAIN - 1, log_domain >= 2.  Every DISTINCT cell offered,
 * used or not, is then compared with the re-encoded result: samples that are not values of one polynomial of 2^log_coef
 * coefficients give FRIEDA_ERR_ARG (and unspecified d_coef contents) instead of a wrong answer.  A repeated cell index is dropped
 * before that (the first occurrence in the list counts; later ones are neither used nor checked): a caller pooling samples from
 * several peers should de-duplicate by index itself if it wants a conflicting repeat reported.  The first call at a size builds the
 * twiddle tables of the product tree's domains (2^7 .. 2^(log_coef + 1) points, about twice the largest in total, kept by the
 * context): the times quoted are for the calls after it. */
int frieda_circle_interpolate_points(frieda_ctx* ctx, const uint32_t* d_cells, const uint32_t* cell_index, uint32_t n_cells, uint32_t ncols,
                                     uint32_t log_cell, uint32_t log_coef, uint32_t log_domain, uint32_t* d_coef);
/* the same for frieda's 4-column layout, followed by the packer: sampled points -> the original len bytes */
int frieda_reconstruct_points_device(frieda_ctx* ctx, const uint32_t* d_cells, const uint32_t* cell_index, uint32_t n_cells, uint32_t log_cell,
                                     uint32_t log_coef, uint32_t log_domain, size_t len, void* d_out_bytes);

/* MerkleOps::commit_on_layer(log_size, prev_layer, columns): d_prev is NULL or 2^(log_size+1) hashes;
 * d_cols is a host array of ncols device column pointers (2^log_size words each, any 4-byte aligned addresses: sub-slices of
 * one SecureColumn are fine); d_out gets 2^log_size 32-byte hashes.  d_prev and d_out are hash pointers (16-byte aligned, else
 * FRIEDA_ERR_ARG). */
int frieda_merkle_commit_layer(frieda_ctx* ctx, uint32_t log_size, const void* d_prev, const uint32_t* const* d_cols,
                               uint32_t ncols, void* d_out);
/* MerkleProver::commit over 4 equal-length columns d_cols[4][2^log_size]: all layers, leaves first
 * (layer log_size at offset 0, ..., root last; offsets from frieda_merkle_layer_offset), 32*(2^(log_size+1)-1)
 * bytes */
int frieda_merkle_commit(frieda_ctx* ctx, const uint32_t* d_cols, uint32_t log_size, void* d_layers);
size_t frieda_merkle_layer_offset(uint32_t log_size, uint32_t layer_log);
/* root only (no layer is stored): the commit() shape.  d_root: 32 bytes, 4-byte aligned. */
int frieda_merkle_root(frieda_ctx* ctx, const uint32_t* d_cols, uint32_t log_size, void* d_root);

/* FriOps::fold_circle_into_line: d_dst[4][N/2] (accumulated: dst*alpha^2 + f') from d_src[4][N] */
int frieda_fold_circle_into_line(frieda_ctx* ctx, uint32_t* d_dst, const uint32_t* d_src, uint32_t log_domain,
                                 const uint32_t alpha[4]);
/* FriOps::fold_line: d_src[4][2^line_log] on the line domain reached from half_odds(log_domain-1) by
 * doubling -> d_dst[4][2^(line_log-1)] */
int frieda_fold_line(frieda_ctx* ctx, const uint32_t* d_src, uint32_t line_log, uint32_t log_domain,
                     const uint32_t alpha[4], uint32_t* d_dst);

/* PolyOps::evaluate of the four coordinate columns of a SecureCirclePoly (d_coeffs[4][2^log_size] -> d_evals[4][2^log_domain]) +
 * FriOps::fold_circle_into_line with alpha0 (accumulate_line1 != 0: the trait's form d_line1 = d_line1 * alpha0^2 + fold; 0: d_line1 =
 * fold) + one FriOps::fold_line with alpha1 (d_line2[4][2^(log_domain-2)]), in ONE pass over the evaluation where the shape allows
 * (log_size >= 12, 16-byte aligned buffers), as the three operations otherwise; the results are those of the three separate calls.
 * For callers that hold both folding challenges: a verifier re-executing a round, FRI with fold_step 2, BASELINE configs[1].  The
 * prover of src/proof.rs draws alpha1 only after committing to line 1 (its fused fold + tree launches are inside
 * frieda_commit_and_generate_proof).  The four buffers must not overlap (FRIEDA_ERR_ARG): the one-pass form writes the lines while
 * other workgroups are still writing the evaluation. */
int frieda_circle_evaluate_fold2(frieda_ctx* ctx, const uint32_t* d_coeffs, uint32_t log_size, uint32_t log_domain, uint32_t* d_evals,
                                 const uint32_t alpha0[4], int accumulate_line1, uint32_t* d_line1, const uint32_t alpha1[4],
                                 uint32_t* d_line2);

/* ---- the trait methods frieda's three functions never call (SURVEY.md §8b lists them on the plug-in surface behind `CpuBackend`,
 * src/commit.rs:15-17, src/proof.rs:47-58): an `impl PolyOps / FriOps for HipBackend` needs them ----
 * PolyOps::extend(poly, log_size): d_coef[ncols][2^log_coef] -> d_out[ncols][2^log_size], zero-extended (FRIEDA_ERR_INVARIANT for
 * log_size < log_coef, stwo's assert).  Asynchronous on the ctx stream; the buffers must not overlap (FRIEDA_ERR_ARG). */
int frieda_circle_extend(frieda_ctx* ctx, const uint32_t* d_coef, uint32_t ncols, uint32_t log_coef, uint32_t log_size, uint32_t* d_out);
/* PolyOps::eval_at_point(poly, point): each of the ncols polynomials d_coef[ncols][2^log_coef] at the circle point (x, y) over
 * the secure field (QM31 coordinates as 4 canonical words each); out[ncols][4] on the host.  Synchronises the ctx stream. */
int frieda_circle_eval_at_point(frieda_ctx* ctx, const uint32_t* d_coef, uint32_t ncols, uint32_t log_coef, const uint32_t point_x[4],
                                const uint32_t point_y[4], uint32_t* out);
/* FriOps::decompose(eval) -> (g, lambda): d_eval[4][2^log_size] (a SecureColumn in bit-reversed order) split into the part inside
 * the FFT space, d_g[4][2^log_size], and the coefficient lambda of the half-coset vanishing polynomial (out_lambda, host):
 * lambda = (sum of the first half - sum of the second half) / 2^log_size; g = eval -/+ lambda.  Synchronises the ctx stream;
 * d_g may be d_eval. */
int frieda_fri_decompose(frieda_ctx* ctx, const uint32_t* d_eval, uint32_t log_size, uint32_t* d_g, uint32_t out_lambda[4]);

/* GrindOps::grind: smallest nonce with trailing_zeros(mix_u64(digest, nonce)) >= pow_bits */
int frieda_grind(frieda_ctx* ctx, const uint8_t digest[32], uint32_t pow_bits, uint64_t* nonce);

#ifdef __cplusplus
}
#endif
#endif
