// verify_split.hip — a pass of the proof verifier as two launches (gfx950), for passes of few proofs (FRIEDA_VERIFY_SPLIT_MAX).
//
// verify.hip gives a proof one wave, and that wave one dependent chain: the transcript, then per layer the pair hashes and a Merkle
// walk of m - 1 compressions, layer after layer.  Nothing in a layer's walk depends on another layer's walk: only the value chain
// (the fold of layer li gives the values of layer li + 1) is sequential, and it hashes nothing.  So
//   verify_chain_kernel<PAIRS>  one wave per proof: steps 1 - 3 of verify_many_kernel (transcript, PoW, queries, per layer the pairs
//                               from the running values and fri_witness and their fold, the last-layer check) without one Merkle
//                               hash.  For every layer whose value stage passed it leaves the assembled pairs (v, l, r) and their
//                               number in the pass's scratch; every other layer of the grid gets the number 0.
//   verify_walk_kernel          one wave per (proof, layer): the pair hashes, the walk of levels m - 2 .. 0 (walk_dev.h, unchanged),
//                               the witness-length rules and the root compare.
// The status is the sequential verifier's: word 0 of a proof's output row holds the key of the first event (verify_pass.h, "the rule").
// The chain wave stores its own first event or "accepted"; a failing walk wave lowers it with atomicMin.  The two launches follow
// each other on one stream; no wave waits for another.
//
// Bounds: the chain checks every count of the image before it reads through it, as verify.hip does; a pair index is below the
// number of positions of its layer, at most n_queries <= q_cap; a layer index is at most n_inner < max_layers (the host sizes the
// scratch by the pass's largest layer count, and the chain refuses a proof beyond it before it writes).
#include <hip/hip_runtime.h>

#include "dev_transcript.h"
#include "kernels.h"
#include "queries_dev.h"
#include "tree_dev.h"
#include "verify_dev.h"
#include "verify_pass.h"
#include "walk_dev.h"

namespace frieda {
namespace k {

namespace {

using walkdev::Group;
using walkdev::group_of;

static_assert(DT_MAX_LAYERS <= 64, "lane li of the chain wave keeps the pair count of layer li");

template <bool PAIRS>
__global__ __launch_bounds__(64) void verify_chain_kernel(VerifySplitArgs sa) {
    const VerifyArgs& a = sa.v;
    extern __shared__ uint32_t lds[];
    const uint32_t Q = a.q_cap, ML = sa.max_layers;
    uint32_t* s_pos = lds;         // positions of the current layer: U_li
    uint32_t* s_srt = lds + Q;     // sort scratch of the query generation
    uint32_t* s_ev = lds + 2 * Q;  // the current layer's values at s_pos, 4 words each
    __shared__ uint32_t s_alpha[4 * DT_MAX_LAYERS];
    __shared__ uint32_t s_misc[2];

    const uint32_t lane = threadIdx.x, slot = blockIdx.x;
    const VerifyHeader hd = reinterpret_cast<const VerifyHeader*>(a.img)[slot];
    const uint32_t* img = a.img + hd.off_words;
    constexpr uint32_t HEAD = PAIRS ? 3 : 2;  // words of the output row before the queries
    uint32_t* out = a.out + (size_t)slot * (HEAD + a.q_cap);
    uint32_t* cnt = sa.cnt + (size_t)slot * ML;
    const uint32_t n = hd.n, nl = hd.n_inner, nq = hd.n_queries;
    const uint32_t* tab = img;  // per layer: n_fri_witness, n_hash_witness, n_column_witness, offset of the layer's words
    const uint32_t* last_poly = img + hd.off_last;
    const uint32_t* evals = img + hd.off_evals;
    const uint32_t np = hd.n_last;
    uint32_t my_cnt = 0;  // lane li: the pairs of layer li, once its value stage has passed

    // every exit writes the count of every layer of the grid (0 where the chain did not get to) and the key of the first event
#define VC_FINISH(key)                     \
    do {                                   \
        if (lane < ML) cnt[lane] = my_cnt; \
        if (lane == 0) out[0] = (key);     \
        return;                            \
    } while (0)

    if (nl >= ML) VC_FINISH(verify_key(verify_order_pow(), VERIFY_INVARIANT));  // (not a pass the host builds: nothing is written past the scratch)

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
    if (ch.trailing_zeros() < hd.pow_bits) VC_FINISH(verify_key(verify_order_pow(), VERIFY_REJECTED));

    // ---- 2. Queries::generate, sorted in s_srt and de-duplicated into s_pos ----
    const uint32_t nu = qdev::generate_queries<64, 8>(ch, n, nq, s_srt, s_pos);  // (the rank loop in steps of 8: no SGPR of this kernel leaves its file)
    for (uint32_t i = lane; i < nu; i += 64) out[HEAD + i] = s_pos[i];
    if (lane == 0) out[1] = nu;

    // ---- 3. the value chain ----
    const uint32_t ne = hd.n_evals;
    for (uint32_t i = lane; i < 4 * nu; i += 64) s_ev[i] = i < 4 * ne ? evals[i] : 0u;  // (too few evaluations: decided below, nothing is read past them)
    if (lane == 0) s_misc[0] = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t eval_fail_pos = ne < nu ? s_pos[ne] : 0u;  // the query at which the reference runs out of evaluations
    uint32_t c = nu;  // |U_li|
    for (uint32_t li = 0; li <= nl; li++) {
        const uint32_t m = n - li;  // log size of the layer
        const uint32_t nw = tab[4 * li], ncw = tab[4 * li + 2];
        const uint32_t* wit = img + tab[4 * li + 3] + 8;
        const QM31 alpha = load_qm(s_alpha + 4 * li);
        uint32_t* blk = sa.pairs + ((size_t)slot * ML + li) * (VERIFY_SPLIT_ENTRY_WORDS * Q);  // v[Q] | (l, r)[Q]
        uint4* blk_lr = reinterpret_cast<uint4*>(blk + Q);
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
                // the pair as the walk wave of this layer hashes it: node v of level m - 1 (g.k < |U_{li+1}| <= n_queries <= Q)
                blk[g.k] = v;
                blk_lr[2 * g.k] = make_uint4(l.a, l.b, l.c, l.d);
                blk_lr[2 * g.k + 1] = make_uint4(r.a, r.b, r.c, r.d);
                // fold: the twiddle is the inverse of the domain point's y (circle layer) or x (line layers) at bit_reverse(2 v)
                const CPoint pt = dev_point_from_index(coset_index(n, li ? li - 1 : 0, bit_reverse(2 * v, m)));
                const uint32_t it = m31_inv(li ? pt.x : pt.y);
                const QM31 f0 = qm_add(l, r), f1 = qm_scale(qm_sub(l, r), it);
                const QM31 f = qm_add(f0, qm_mul(alpha, f1));
                if constexpr (PAIRS) {
                    if (li == 0) {
                        // both members of the opened pair: entries 2 k, 2 k + 1 of the proof's row, as verify_many_kernel leaves them
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
            if (!(wbase > nw && wit_fail_pos < eval_fail_pos)) VC_FINISH(verify_key(verify_order_values(0), VERIFY_INVARIANT));
        }
        if (__any(bad) || wbase != nw || ncw != 0) VC_FINISH(verify_key(verify_order_values(li), VERIFY_REJECTED));
        c = kbase;  // |U_{li+1}|: the nodes of level m - 1, at least one
        if (lane == li) my_cnt = c;
        if constexpr (PAIRS) {
            if (li == 0 && lane == 0) out[2] = kbase;  // the opened pairs of the first layer
        }
        if (nl == 0) VC_FINISH(verify_key(verify_order_no_inner(), VERIFY_INVARIANT));  // assert!(first_layer_columns.is_empty()) upstream, after layer 0's walk
    }

    // ---- decommit_last_layer: LinePoly::eval_at_point at every remaining position ----
    if (np == 0 || (np & (np - 1))) VC_FINISH(verify_key(verify_order_last(nl), VERIFY_REJECTED));
    {
        const uint32_t plog = 31 - (uint32_t)__clz((int)np);
        const uint32_t ml = n - nl - 1;
        bool bad = false;
        for (uint32_t i = lane; i < c; i += 64) {
            const uint32_t x = dev_point_from_index(coset_index(n, nl, bit_reverse(s_pos[i], ml))).x;
            const QM31 acc = last_poly_eval_at(last_poly, np, plog, x);
            if (!qm_eq(acc, load_qm(s_ev + 4 * i))) bad = true;  // LastLayerEvaluationsInvalid
        }
        if (__any(bad)) VC_FINISH(verify_key(verify_order_last(nl), VERIFY_REJECTED));
    }
    VC_FINISH(VERIFY_KEY_ACCEPTED);
#undef VC_FINISH
}

// One wave per (proof, layer): blockIdx.x the proof's slot, blockIdx.y the layer.  LDS: node positions [Q], node hashes [Q][8].
__global__ __launch_bounds__(64) void verify_walk_kernel(VerifySplitArgs sa) {
    extern __shared__ uint32_t lds[];
    const uint32_t Q = sa.v.q_cap, ML = sa.max_layers;
    const uint32_t lane = threadIdx.x, slot = blockIdx.x, li = blockIdx.y;
    const uint32_t c = sa.cnt[(size_t)slot * ML + li];
    if (c == 0) return;  // not reached, or its value stage failed
    if (c > Q) {         // not a count the chain writes: the proof gets no verdict from a row nobody wrote
        if (lane == 0) atomicMin(sa.v.out + (size_t)slot * ((sa.v.pair_pos ? 3 : 2) + Q), verify_key(verify_order_pow(), VERIFY_INVARIANT));
        return;
    }
    const VerifyHeader hd = reinterpret_cast<const VerifyHeader*>(sa.v.img)[slot];
    if (li > hd.n_inner) return;
    uint32_t* s_hp = lds;     // node positions of the walk
    uint32_t* s_h = lds + Q;  // node hashes, 8 words each
    const uint32_t* img = sa.v.img + hd.off_words;
    const uint32_t m = hd.n - li;  // log size of the layer
    const uint32_t nw = img[4 * li], nh = img[4 * li + 1];
    const uint32_t* lay = img + img[4 * li + 3];
    const uint32_t* hw = lay + 8 + 4 * (size_t)nw;
    uint32_t* key = sa.v.out + (size_t)slot * ((sa.v.pair_pos ? 3 : 2) + Q);

#define VW_FAIL()                                                                              \
    do {                                                                                       \
        if (lane == 0) atomicMin(key, verify_key(verify_order_walk(li), VERIFY_REJECTED));     \
        return;                                                                                \
    } while (0)

    // the pairs' two leaves and their parents: the nodes of level m - 1
    const uint32_t* blk = sa.pairs + ((size_t)slot * ML + li) * (VERIFY_SPLIT_ENTRY_WORDS * Q);
    const uint4* blk_lr = reinterpret_cast<const uint4*>(blk + Q);
    for (uint32_t i = lane; i < c; i += 64) {
        const uint4 l = blk_lr[2 * i], r = blk_lr[2 * i + 1];
        const uint32_t lw[4] = {l.x, l.y, l.z, l.w}, rw[4] = {r.x, r.y, r.z, r.w};
        uint32_t hp[8];
        treedev::pair_node<B2_LAT>(lw, rw, hp);
#pragma unroll
        for (int w = 0; w < 8; w++) s_h[8 * i + w] = hp[w];
        s_hp[i] = blk[i];
    }
    __syncthreads();
    // ---- the Merkle walk of this layer: levels m - 2 .. 0 ----
    bool bad = false;
    uint32_t cn = c, hbase = 0;
    for (uint32_t lv = m - 1; lv > 0; lv--) {
        cn = walkdev::walk_level(s_hp, s_h, cn, lane, hw, nh, hbase, bad);  // (WitnessTooShort sets bad)
        if (__any(bad)) VW_FAIL();
    }
    if (hbase != nh || cn != 1) VW_FAIL();  // WitnessTooLong
    const bool diff = lane < 8 && s_h[lane] != lay[lane];
    if (__any(diff)) VW_FAIL();
#undef VW_FAIL
}

}  // namespace

size_t verify_chain_lds_bytes(uint32_t q_cap) { return sizeof(uint32_t) * 6 * (size_t)q_cap; }
size_t verify_walk_lds_bytes(uint32_t q_cap) { return sizeof(uint32_t) * VERIFY_SPLIT_ENTRY_WORDS * (size_t)q_cap; }

hipError_t verify_split_init(const CPoint (&gen_pow2)[31]) { return upload_gen_pow2(gen_pow2); }

void verify_split(const Launch& L, const VerifySplitArgs& a, uint32_t n_proofs) {
    {
        Scope scope(L, "verify_many", 0.0);  // (the timer name of a verify pass's launches, whichever shape: kernels.h)
        if (a.v.pair_pos)
            verify_chain_kernel<true><<<dim3(n_proofs), 64, verify_chain_lds_bytes(a.v.q_cap), L.stream>>>(a);
        else
            verify_chain_kernel<false><<<dim3(n_proofs), 64, verify_chain_lds_bytes(a.v.q_cap), L.stream>>>(a);
    }
    Scope scope(L, "verify_many", 0.0);
    verify_walk_kernel<<<dim3(n_proofs, a.max_layers), 64, verify_walk_lds_bytes(a.v.q_cap), L.stream>>>(a);
}

}  // namespace k
}  // namespace frieda
