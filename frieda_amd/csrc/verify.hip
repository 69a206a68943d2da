// verify.hip — many proofs verified in one launch (gfx950): the device restatement of verifier.cpp::verify.
//
// One wave (a 64-thread workgroup) per proof.  The proof arrives as a packed image of 32-bit words (VerifyHeader + layer table +
// data, built by verify_many.cpp); the wave
//   1. replays the transcript (init, optional mix_u64(seed), per layer mix_root + draw_felt, mix_felts(last_layer_poly),
//      mix_u64(nonce), the trailing-zeros test),
//   2. draws the queries, sorted and de-duplicated (queries_dev.h, the code the prover's decommit.hip runs),
//   3. walks the layers: with U_li = unique(queries >> li) the positions of layer li, every pair {2v, 2v + 1}, v in U_{li+1}, takes its
//      members from the running values or — the index is a prefix count of "not queried" (ballot + popcount) — from fri_witness,
//      folds it with the layer's alpha, and
//   4. hashes the pair's two leaves and their parent, then walks the tree level by level: the nodes of a level are unique(positions
//      >> s), a child that was not computed below comes from hash_witness at the prefix count of the missing children (the E_s tables
//      of queries_dev.h, read from the verifier's side), and the root is compared with the layer's commitment.
// Every list lives in LDS and is compacted in place: entry k of a level is written after the entries >= k of the level below were
// read (a wave executes its LDS accesses in program order), the neighbour below a 64-entry chunk is carried in a register.
//
// Every count of the image is checked arithmetically before a word is read through it (witness too short / too long, too few
// evaluations, a non-empty column witness), so a malformed proof never reads outside its own image.
#include <hip/hip_runtime.h>

#include "dev_transcript.h"
#include "kernels.h"
#include "queries_dev.h"
#include "tree_dev.h"
#include "verify_dev.h"
#include "walk_dev.h"

namespace frieda {
namespace k {

namespace {

using walkdev::Group;
using walkdev::group_of;

// PAIRS: the first layer's opened pairs also go to the proof's row of a.pair_pos / a.pair_val (frieda_verify_pairs_many) — tentatively:
// a later layer may still reject the proof, and nothing reads the row unless the final status is VERIFY_ACCEPTED.
template <bool PAIRS>
__global__ __launch_bounds__(64) void verify_many_kernel(VerifyArgs a) {
    extern __shared__ uint32_t lds[];
    const uint32_t Q = a.q_cap;
    uint32_t* s_pos = lds;           // positions of the current layer: U_li
    uint32_t* s_hp = lds + Q;        // sort scratch, then the node positions of the Merkle walk
    uint32_t* s_ev = lds + 2 * Q;    // the current layer's values at s_pos, 4 words each
    uint32_t* s_h = lds + 6 * Q;     // node hashes of the Merkle walk, 8 words each
    __shared__ uint32_t s_alpha[4 * DT_MAX_LAYERS];
    __shared__ uint32_t s_misc[2];

    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    const VerifyHeader hd = reinterpret_cast<const VerifyHeader*>(a.img)[slot];
    const uint32_t* img = a.img + hd.off_words;
    constexpr uint32_t HEAD = PAIRS ? 3 : 2;  // words of the output row before the queries
    uint32_t* out = a.out + (size_t)slot * (HEAD + a.q_cap);
    const uint32_t n = hd.n, nl = hd.n_inner, nq = hd.n_queries;
    const uint32_t* tab = img;  // per layer: n_fri_witness, n_hash_witness, n_column_witness, offset of the layer's words
    const uint32_t* last_poly = img + hd.off_last;
    const uint32_t* evals = img + hd.off_evals;
    const uint32_t np = hd.n_last;

#define VK_FINISH(st)                  \
    do {                               \
        if (lane == 0) out[0] = (st);  \
        return;                        \
    } while (0)

    // ---- 1. the transcript: every lane computes the same chain; lane 0 keeps the alphas ----
    Channel ch;
    ch.init();
    if (hd.has_seed) ch.mix_u64((uint64_t)hd.seed_lo | ((uint64_t)hd.seed_hi << 32));
    for (uint32_t li = 0; li <= nl; li++) {
        const uint32_t* c = img + tab[4 * li + 3];
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = c[i];
        ch.mix_root(w);
        const QM31 al = ch.draw_felt();
        if (lane == 0) s_alpha[4 * li] = al.a, s_alpha[4 * li + 1] = al.b, s_alpha[4 * li + 2] = al.c, s_alpha[4 * li + 3] = al.d;
    }
    ch.mix_felts(last_poly, np);
    ch.mix_u64((uint64_t)hd.nonce_lo | ((uint64_t)hd.nonce_hi << 32));
    if (ch.trailing_zeros() < hd.pow_bits) VK_FINISH(VERIFY_REJECTED);

    // ---- 2. Queries::generate, sorted in s_hp and de-duplicated into s_pos ----
    const uint32_t nu = qdev::generate_queries<64>(ch, n, nq, s_hp, s_pos);
    for (uint32_t i = lane; i < nu; i += 64) out[HEAD + i] = s_pos[i];
    if (lane == 0) out[1] = nu;

    // ---- 3 + 4. the layers ----
    const uint32_t ne = hd.n_evals;
    for (uint32_t i = lane; i < 4 * nu; i += 64) s_ev[i] = i < 4 * ne ? evals[i] : 0u;  // (too few evaluations: decided below, nothing is read past them)
    if (lane == 0) s_misc[0] = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t eval_fail_pos = ne < nu ? s_pos[ne] : 0u;  // the query at which the reference runs out of evaluations
    uint32_t c = nu;  // |U_li|
    for (uint32_t li = 0; li <= nl; li++) {
        const uint32_t m = n - li;  // log size of the layer
        const uint32_t nw = tab[4 * li], nh = tab[4 * li + 1], ncw = tab[4 * li + 2];
        const uint32_t* lay = img + tab[4 * li + 3];
        const uint32_t* wit = lay + 8;
        const uint32_t* hw = wit + 4 * (size_t)nw;
        const QM31 alpha = load_qm(s_alpha + 4 * li);
        bool bad = false;
        uint32_t kbase = 0, wbase = 0, carry = 0;
        for (uint32_t i0 = 0; i0 < c; i0 += 64) {
            const Group g = group_of(s_pos, c, i0, lane, carry, kbase, wbase);
            const uint32_t i = i0 + lane;
            QM31 l{0, 0, 0, 0}, r{0, 0, 0, 0};
            if (g.first) {
                QM31 wv{0, 0, 0, 0};
                if (g.miss) {
                    if (g.w < nw)
                        wv = load_qm(wit + 4 * (size_t)g.w);
                    else
                        bad = true;  // InsufficientWitness
                    if (li == 0 && g.w == nw) s_misc[0] = g.x ^ 1u;  // the position at which the reference runs out of witness
                }
                const QM31 own = load_qm(s_ev + 4 * i);
                l = g.has_l ? own : wv;
                r = (g.x & 1u) ? own : (g.has_r ? load_qm(s_ev + 4 * (i + 1)) : wv);
            }
            carry = (uint32_t)__shfl((int)g.x, 63);
            __syncthreads();
            if (g.first) {
                const uint32_t v = g.x >> 1;
                // the pair's two leaves and their parent: node v of level m - 1
                const uint32_t lw[4] = {l.a, l.b, l.c, l.d}, rw[4] = {r.a, r.b, r.c, r.d};
                uint32_t hp[8];
                treedev::pair_node<B2_LAT>(lw, rw, hp);
#pragma unroll
                for (int w = 0; w < 8; w++) s_h[8 * g.k + w] = hp[w];
                s_hp[g.k] = v;
                // fold: the twiddle is the inverse of the domain point's y (circle layer) or x (line layers) at bit_reverse(2 v)
                const CPoint pt = dev_point_from_index(coset_index(n, li ? li - 1 : 0, bit_reverse(2 * v, m)));
                const uint32_t it = m31_inv(li ? pt.x : pt.y);
                const QM31 f0 = qm_add(l, r), f1 = qm_scale(qm_sub(l, r), it);
                const QM31 f = qm_add(f0, qm_mul(alpha, f1));
                if constexpr (PAIRS) {
                    if (li == 0) {
                        // both members of the opened pair, as the leaves above hashed them: entries 2 k, 2 k + 1 of the proof's row
                        // (k < |U_1| <= n_queries <= q_cap; positions ascend with k)
                        const size_t e = (size_t)slot * 2 * Q + 2 * g.k;
                        *reinterpret_cast<uint2*>(a.pair_pos + e) = make_uint2(2 * v, 2 * v + 1);
                        uint4* pv = reinterpret_cast<uint4*>(a.pair_val + 4 * e);
                        pv[0] = make_uint4(l.a, l.b, l.c, l.d);
                        pv[1] = make_uint4(r.a, r.b, r.c, r.d);
                    }
                }
                s_pos[g.k] = v;
                s_ev[4 * g.k] = f.a, s_ev[4 * g.k + 1] = f.b, s_ev[4 * g.k + 2] = f.c, s_ev[4 * g.k + 3] = f.d;
            }
            __syncthreads();
        }
        if (li == 0 && ne < nu) {
            // QueryEvalsExhausted (the reference panics) unless the witness ran out at a smaller position first
            const uint32_t wit_fail_pos = s_misc[0];
            if (!(wbase > nw && wit_fail_pos < eval_fail_pos)) VK_FINISH(VERIFY_INVARIANT);
        }
        if (__any(bad) || wbase != nw || ncw != 0) VK_FINISH(VERIFY_REJECTED);
        c = kbase;  // |U_{li+1}|: the nodes of level m - 1
        if constexpr (PAIRS) {
            if (li == 0 && lane == 0) out[2] = kbase;  // the opened pairs of the first layer
        }
        // ---- the Merkle walk of this layer: levels m - 2 .. 0 ----
        uint32_t cn = c, hbase = 0;
        for (uint32_t lv = m - 1; lv > 0; lv--) {
            const uint32_t kb = walkdev::walk_level(s_hp, s_h, cn, lane, hw, nh, hbase, bad);  // (WitnessTooShort sets bad)
            cn = kb;
            if (__any(bad)) VK_FINISH(VERIFY_REJECTED);
        }
        if (hbase != nh || cn != 1) VK_FINISH(VERIFY_REJECTED);  // WitnessTooLong
        {
            const bool diff = lane < 8 && s_h[lane] != lay[lane];
            if (__any(diff)) VK_FINISH(VERIFY_REJECTED);
        }
        if (nl == 0) VK_FINISH(VERIFY_INVARIANT);  // assert!(first_layer_columns.is_empty()) upstream
        __syncthreads();
    }

    // ---- decommit_last_layer: LinePoly::eval_at_point at every remaining position ----
    if (np == 0 || (np & (np - 1))) VK_FINISH(VERIFY_REJECTED);
    {
        const uint32_t plog = 31 - (uint32_t)__clz((int)np);
        const uint32_t ml = n - nl - 1;
        bool bad = false;
        for (uint32_t i = lane; i < c; i += 64) {
            const uint32_t x = dev_point_from_index(coset_index(n, nl, bit_reverse(s_pos[i], ml))).x;
            const QM31 acc = last_poly_eval_at(last_poly, np, plog, x);
            if (!qm_eq(acc, load_qm(s_ev + 4 * i))) bad = true;  // LastLayerEvaluationsInvalid
        }
        if (__any(bad)) VK_FINISH(VERIFY_REJECTED);
    }
    VK_FINISH(VERIFY_ACCEPTED);
#undef VK_FINISH
}

// One wave per accepted proof of a pass: row tab[3 w] of the pass's pair buffer (tab[3 w + 1] entries) -> entry tab[3 w + 2] on of the
// call's pool: positions to pool_pos, the four column words of an entry to pool_val[.][4] — the cell layout of erasure_sample_lists /
// interpolate_points for log_cell 0, ncols 4.  The table comes from the host, which has the counts from the status rows.
__global__ __launch_bounds__(256) void pairs_gather_kernel(const uint32_t* __restrict__ tab, uint32_t n_rows, const uint32_t* __restrict__ pair_pos,
                                                           const uint32_t* __restrict__ pair_val, uint32_t q_cap, uint32_t* __restrict__ pool_pos,
                                                           uint32_t* __restrict__ pool_val) {
    const uint32_t w = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (w >= n_rows) return;
    const uint32_t row = tab[3 * w], cnt = tab[3 * w + 1];
    const size_t src = (size_t)row * 2 * q_cap, dst = tab[3 * w + 2];
    const uint4* sv = reinterpret_cast<const uint4*>(pair_val) + src;
    uint4* dv = reinterpret_cast<uint4*>(pool_val) + dst;
    for (uint32_t i = lane; i < cnt; i += 64) {
        pool_pos[dst + i] = pair_pos[src + i];
        dv[i] = sv[i];
    }
}

}  // namespace

size_t verify_many_lds_bytes(uint32_t q_cap) { return sizeof(uint32_t) * 14 * (size_t)q_cap; }

hipError_t verify_many_init(const CPoint (&gen_pow2)[31]) { return upload_gen_pow2(gen_pow2); }

void verify_many(const Launch& L, const VerifyArgs& a, uint32_t n_proofs) {
    Scope scope(L, "verify_many", 0.0);
    if (a.pair_pos)
        verify_many_kernel<true><<<dim3(n_proofs), 64, verify_many_lds_bytes(a.q_cap), L.stream>>>(a);
    else
        verify_many_kernel<false><<<dim3(n_proofs), 64, verify_many_lds_bytes(a.q_cap), L.stream>>>(a);
}

void verify_pairs_gather(const Launch& L, const uint32_t* d_tab, uint32_t n_rows, const uint32_t* d_pair_pos, const uint32_t* d_pair_val, uint32_t q_cap,
                         uint32_t* d_pool_pos, uint32_t* d_pool_val) {
    if (!n_rows) return;
    Scope scope(L, "verify_pairs_gather", 0.0);
    pairs_gather_kernel<<<dim3((n_rows + 3) / 4), 256, 0, L.stream>>>(d_tab, n_rows, d_pair_pos, d_pair_val, q_cap, d_pool_pos, d_pool_val);
}

}  // namespace k
}  // namespace frieda
