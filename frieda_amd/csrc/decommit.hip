// decommit.hip — query sampling and the openings of a proof, on the device (gfx950).
//
// Replaces, for the prover, `channel.mix_u64(nonce)`, `Queries::generate`, `FriProver::decommit` (per layer
// `compute_decommitment_positions_and_witness_evals` + `MerkleProver::decommit`) and the evaluations gather of
// /root/reference/src/proof.rs:59-66 (stwo core/queries.rs, core/fri.rs, core/vcs/prover.rs).  The host used to do the
// transcript step and the planning between two synchronisations (nonce download -> plan -> gather launch -> download); here
// one launch behind the grind writes the openings in proof order straight into pinned host memory, so a proof needs a single
// synchronisation and no host-side planning.  prover.cpp keeps the host planner as the fallback (more than 1024 queries, an
// opening list that does not fit LDS, FRIEDA_HOST_DECOMMIT=1) and as the cross-check in the tests.
//
// The E_s tables every output is a slice of, and the query sampling, are queries_dev.h's (shared with the verifier's walk in verify.hip):
// the kernel computes the E_s once, one wave per s, and writes fri_witness of layer li = the values at E_{li+1} and hash_witness of
// layer li = the hashes of E_{li+2} .. E_n.
#include <hip/hip_runtime.h>

#include "dev_transcript.h"
#include "kernels.h"
#include "queries_dev.h"
#include "tree_dev.h"

namespace frieda {
namespace k {

namespace {

// 16 bytes in flight between a load and its store.  A native vector, not HIP's uint4: an array of that struct is copied with memcpy and
// stays a private array (64 bytes per thread of LDS or scratch) instead of four registers.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int DC_THREADS = 256;
constexpr uint32_t DC_MAX_Q = DECOMMIT_MAX_QUERIES;  // 1024
constexpr uint32_t DC_E_CAP = 11264;                 // n * (unique queries) slots for the E_s tables (44 KiB of LDS)

// A node of the two levels above the leaves, re-hashed from the layer's values (4 columns of 2^m words): the large trees of a proof
// do not store these levels (tree.hip TreeArgs::skip_bc).  level = log2 of the level's size: m - 1 (the parent of leaves 2 c, 2 c + 1)
// or m - 2 (of leaves 4 c .. 4 c + 3): three or seven compressions in the plain form.
__device__ void node_from_values(const uint32_t* __restrict__ v, uint32_t m, uint32_t level, uint32_t child, uint32_t (&h)[8]) {
    const size_t cs = (size_t)1 << m;
    const bool two = level + 2 == m;  // two level-(m-1) nodes under the requested one
    auto pair = [&](size_t b, uint32_t (&o)[8]) {  // node b of level m - 1: the parent of leaves 2 b, 2 b + 1
        const size_t j = 2 * b;
        const uint32_t l[4] = {v[j], v[cs + j], v[2 * cs + j], v[3 * cs + j]}, r[4] = {v[j + 1], v[cs + j + 1], v[2 * cs + j + 1], v[3 * cs + j + 1]};
        treedev::pair_node<B2_LAT>(l, r, o);
    };
    if (!two) {
        pair(child, h);
        return;
    }
    uint32_t hb[2][8], mm[16];
    pair(2 * (size_t)child, hb[0]);
    pair(2 * (size_t)child + 1, hb[1]);
#pragma unroll
    for (int w = 0; w < 8; w++) mm[w] = hb[0][w], mm[8 + w] = hb[1][w];
    b2_merkle_block<B2_LAT>(mm, h);
}

__global__ __launch_bounds__(DC_THREADS) void decommit_kernel(DecommitArgs a) {
#ifndef FRIEDA_NO_LATENCY_PRIO
    __builtin_amdgcn_s_setprio(3);  // a latency chain that may share the chip with another proof's wide kernels (tree.hip)
#endif
    __shared__ uint32_t s_q[DC_MAX_Q];        // raw draws, then sorted
    __shared__ uint32_t s_u[DC_MAX_Q];        // sorted unique queries
    __shared__ uint32_t s_E[DC_E_CAP];        // E_s at [(s - 1) * nu, (s - 1) * nu + |E_s|)
    __shared__ uint32_t s_cnt[64], s_base[66], s_hoff[64];
    __shared__ uint32_t s_digest[8];
    __shared__ uint32_t s_status;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t blob = blockIdx.y;
    const size_t boff = (size_t)blob * a.bstride;
    const size_t boff0 = a.first_shared ? 0 : boff;  // layer 0 of a prove_seeds job: the encoded blob every seed shares
    // ... or, for a block of encoded blobs, the one of this job's row (the job number is uniform: scalar loads)
    const uint32_t* vals0 = a.vals[0];
    const uint8_t* tree0 = a.trees[0];
    uint32_t skip_log0 = a.skip_log0;
    if (a.blk_table) {
        const SeedsBlobRow& row = a.blk_table[a.blk_job[blob]];
        vals0 = row.eval;
        tree0 = row.tree;
        skip_log0 = row.skip_log;
    }
    const DevTranscript* tr = a.tr + blob;
    uint8_t* out = a.out + (size_t)blob * a.out_stride;
    uint32_t* hdr = reinterpret_cast<uint32_t*>(out);
    const uint32_t n = a.n, nq = a.n_queries, nl = a.n_layers;

    // ---- channel.mix_u64(nonce) (src/proof.rs:59) ----
    if (t == 0) {
        const unsigned long long nonce = tr->nonce;  // both loads first (independent)
        Channel ch = tr->ch;
        uint32_t st = 0;
        if (nonce == ~0ull) {
            st = DECOMMIT_NO_NONCE;
        } else {
            ch.mix_u64(nonce);
#pragma unroll
            for (int i = 0; i < 8; i++) s_digest[i] = ch.digest[i];
        }
        s_status = st;
    }
    __syncthreads();
    if (s_status) {
        if (blockIdx.x == 0 && t == 0) hdr[0] = s_status;
        return;
    }
    // ---- Queries::generate ----
    Channel ch;
    ch.init();
#pragma unroll
    for (int i = 0; i < 8; i++) ch.digest[i] = s_digest[i];
    const uint32_t nu = qdev::generate_queries<DC_THREADS>(ch, n, nq, s_q, s_u);
    if (n * nu > DC_E_CAP) {  // uniform: the E tables would not fit — the host plans this proof
        if (blockIdx.x == 0 && t == 0) hdr[0] = DECOMMIT_OVERFLOW;
        return;
    }

    // ---- the E_s tables: one wave per s, each into the slot of its s ----
    for (uint32_t s = 1 + wave; s <= n; s += DC_THREADS / 64) {
        const uint32_t c = qdev::build_level(s_u, nu, s, s_E + (s - 1) * nu);
        if (lane == 0) s_cnt[s] = c;
    }
    __syncthreads();
    // prefix sums by one wave: base[s] = |E_1| + ... + |E_{s-1}|;  hash_witness of layer li = E_{li+2} .. E_n, so its size is
    // total - base[li + 2] and hoff[li] = the sizes of the layers before it
    if (wave == 0) {
        const uint32_t c = (lane >= 1 && lane <= n) ? s_cnt[lane] : 0u;  // lane s holds |E_s|
        uint32_t inc = c;
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
            if (lane >= off) inc += o;
        }
        s_base[lane + 1] = inc;  // base[s + 1] = |E_1| + ... + |E_s|
        if (lane == 0) s_base[0] = 0, s_base[1] = 0;
        const uint32_t total = (uint32_t)__shfl((int)inc, 63);
        // lane li: hashes of layer li = total - base[li + 2] = total - (inclusive sum at lane li + 1)
        const uint32_t inc_next = (uint32_t)__shfl_down((int)inc, 1);
        const uint32_t hl = lane < nl ? total - (lane + 1 <= 63 ? inc_next : total) : 0u;
        uint32_t hinc = hl;
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)hinc, off);
            if (lane >= off) hinc += o;
        }
        s_hoff[lane] = hinc - hl;  // exclusive
        const uint32_t n_hashes = (uint32_t)__shfl((int)hinc, 63);
        const uint32_t wit = (uint32_t)__shfl((int)inc, (int)nl);  // |E_1| + ... + |E_nl|  (nl <= n <= 27)
        const uint32_t n_words = 4 * nu + 4 * wit;
        const uint32_t st = (n_words > a.max_words || n_hashes > a.max_hashes) ? (uint32_t)DECOMMIT_OVERFLOW : (uint32_t)DECOMMIT_OK;
        if (lane == 0) s_status = st;
        if (blockIdx.x == 0) {
            if (lane >= 1 && lane <= n) hdr[3 + lane] = c;
            if (lane == 0) {
                hdr[1] = nu;
                hdr[2] = n_words;
                hdr[3] = n_hashes;
                hdr[0] = st;
            }
        }
    }
    __syncthreads();
    if (s_status) return;

    // ---- outputs, in proof order; the workgroups of a blob (gridDim.x) take interleaved slices ----
    const uint32_t gt = blockIdx.x * DC_THREADS + t, gstride = gridDim.x * DC_THREADS;
    uint32_t* ow = reinterpret_cast<uint32_t*>(out + a.words_off);
    u32x4* oh = reinterpret_cast<u32x4*>(out + a.hashes_off);
    // Proof.evaluations (src/proof.rs:62-66): the four coordinates at every query
    {
        const uint32_t* v0 = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(vals0) + boff0);
        for (uint32_t e = gt; e < 4 * nu; e += gstride) ow[e] = v0[((size_t)(e & 3) << n) + s_u[e >> 2]];
    }
    // fri_witness of layer li: the values at E_{li+1}.  Dense grid (layer, slot, coordinate); empty slots are skipped.
    for (uint32_t e = gt; e < 4 * nu * nl; e += gstride) {
        const uint32_t li = e / (4 * nu), r = e - li * 4 * nu, k = r >> 2, c = r & 3;
        if (k < s_cnt[li + 1]) {
            const uint32_t* v = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(li ? a.vals[li] : vals0) + (li ? boff : boff0));
            ow[4 * nu + 4 * (s_base[li + 1] + k) + c] = v[((size_t)c << (n - li)) + s_E[li * nu + k]];
        }
    }
    // hash_witness: entry k of E_s is opened in every layer li <= s - 2, at level n - s + 1 of that layer's tree, and lands at
    // hash position hoff[li] + (base[s] + k - base[li + 2]) of the output.  Dense grid (s, slot, 16-byte half); the layers of
    // an entry are independent loads, issued four at a time.
    if (n >= 2) {
        for (uint32_t e = gt; e < 2 * nu * (n - 1); e += gstride) {
            const uint32_t s = 2 + e / (2 * nu), r = e - (s - 2) * 2 * nu, k = r >> 1, half = r & 1;
            if (k >= s_cnt[s]) continue;
            const uint32_t child = s_E[(s - 1) * nu + k], idx = s_base[s] + k;
            const uint32_t level = n - s + 1;
            const uint32_t li_end = s - 1 < nl ? s - 1 : nl;  // layers 0 .. li_end - 1
            for (uint32_t li0 = 0; li0 < li_end; li0 += 4) {
                u32x4 v[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t li = li0 + j;
                    // (a level the tree does not hold is re-hashed below, by the thread of the entry's first half)
                    if (li < li_end && !(n - li >= (li ? a.skip_log : skip_log0) && level + 2 >= n - li)) {
                        const uint8_t* tree = (li ? a.trees[li] : tree0) + (li ? boff : boff0) + (((size_t)64 << (n - li)) - ((size_t)64 << level));
                        v[j] = reinterpret_cast<const u32x4*>(tree + 32 * (size_t)child)[half];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint32_t li = li0 + j;
                    if (li < li_end && !(n - li >= (li ? a.skip_log : skip_log0) && level + 2 >= n - li)) oh[2 * (size_t)(s_hoff[li] + (idx - s_base[li + 2])) + half] = v[j];
                }
            }
            // the (at most two) layers in which this entry sits one or two levels above the leaves of a tree that keeps neither
            if (half == 0) {
#pragma unroll 1
                for (uint32_t li = (s >= 3 ? s - 3 : 0); li < li_end; li++) {  // level + 2 >= n - li  <=>  li >= s - 3
                    if (n - li < (li ? a.skip_log : skip_log0)) continue;
                    uint32_t h[8];
                    node_from_values(reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(li ? a.vals[li] : vals0) + (li ? boff : boff0)), n - li, level, child, h);
                    u32x4* o = oh + 2 * (size_t)(s_hoff[li] + (idx - s_base[li + 2]));
                    o[0] = u32x4{h[0], h[1], h[2], h[3]};
                    o[1] = u32x4{h[4], h[5], h[6], h[7]};
                }
            }
        }
    }
}

}  // namespace

void decommit(const Launch& L, const DecommitArgs& a, uint32_t wgs_per_blob) {
    Scope scope(L, "decommit", 0.0);
    decommit_kernel<<<dim3(wgs_per_blob ? wgs_per_blob : 1, L.batch), DC_THREADS, 0, L.stream>>>(a);
}

}  // namespace k
}  // namespace frieda
