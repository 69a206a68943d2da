// queries_dev.h — query sampling and the opening tables, on the device: what decommit.hip (the prover's openings), verify.hip (the
// verifier's walk) and opening.hip (Level B decommitment) share, so that the prover and the verifier cannot drift apart.
//
// Queries.  stwo core/queries.rs Queries::generate: draw d of the channel yields eight positions (the draws of one digest are
// independent: Channel::draw_block), masked to the domain; the list is sorted and de-duplicated.
//
// Opening tables.  Let p be strictly ascending positions (leaf indices of a tree of 2^L leaves; in a proof the queries of the 2^n
// circle domain), U_s = unique(p >> s), and E_s = the children (at shift s - 1) of the nodes of U_s that are NOT in U_{s-1}: a node
// of U_s has one or two children in U_{s-1}, so it contributes at most one entry, and E_s is ascending.  Position i emits at level s
// iff it is the first of its parent group and lies in the right child (the left is missing), or the last and lies in the left child
// (emit_of).  Every level needs only p, so all levels are computed independently.
//   * stwo's hash witness (core/vcs/prover.rs MerkleProver::decommit: the bottom-up merge walk that pushes, per layer and per node
//     in ascending order, the hash of every child it does not already know) is E_1, E_2, ..., E_L, E_s read at tree layer L - s + 1.
//   * In a proof, FRI layer li (log size n - li; li = 0 is the circle evaluation) is queried at U_li; folding a query and walking one
//     tree level up are the same shift, so every list the reference builds for that layer is one of the E_s:
//       fri_witness  = the values at E_{li+1}                    (the pair members the verifier cannot derive)
//       hash_witness = for s = li+2 .. n: the hashes of E_s at tree level n - s + 1   (bottom-up, left to right)
//     (the leaf level contributes no hashes: both members of every queried pair are opened).  The verifier reads the same tables from
//     the other side: a child that it did not compute comes from the witness at the prefix count of the missing children.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "channel.h"

namespace frieda {
namespace k {
namespace qdev {

// Queries::generate by a workgroup of THREADS threads (all of them call): the nq draws of `ch` masked to 2^log_domain go to q —
// LDS, room for P = the next power of two >= max(2, nq) words, padded with 0xFFFFFFFF — are sorted there, and the distinct ones go
// to u (LDS, nq words), ascending.  Returns their number, the same in every thread; q and u are ready for all threads on return.
// RANK_UNROLL: how far the 64-lane rank loop is unrolled.  Fully (the default) it holds all 64 broadcast values in SGPRs at once; a
// kernel that keeps many uniform values of its own across the call asks for less (verify_split.hip), for the same result.
template <int THREADS, int RANK_UNROLL = 64>
__device__ __forceinline__ uint32_t generate_queries(const Channel& ch, uint32_t log_domain, uint32_t nq, uint32_t* q, uint32_t* u) {
    static_assert(THREADS % 64 == 0, "whole waves");
    const uint32_t t = threadIdx.x, lane = t & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const uint32_t mask = (1u << log_domain) - 1;
    uint32_t P = 2;
    while (P < nq) P <<= 1;
    for (uint32_t d = t; d < (nq + 7) / 8; d += THREADS) {
        uint32_t r[8];
        ch.draw_block(d, r);
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (8 * d + j < nq) q[8 * d + j] = r[j] & mask;
    }
    for (uint32_t i = nq + t; i < P; i += THREADS) q[i] = 0xFFFFFFFFu;
    __syncthreads();
    if (P > 64) {  // bitonic sort by the whole workgroup
        for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t i = t; i < P; i += THREADS) {
                    const uint32_t ixj = i ^ j;
                    if (ixj > i) {
                        const uint32_t x = q[i], y = q[ixj];
                        const bool asc = (i & k2) == 0;
                        if ((x > y) == asc) {
                            q[i] = y;
                            q[ixj] = x;
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
    // the rest is one wave's work and needs no barrier: a wave executes its LDS accesses in program order
    uint32_t nu = 0;
    if (THREADS == 64 || t < 64) {
        if (P <= 64) {  // the usual case: sort by rank
            const uint32_t v = q[lane < P ? lane : 0];
            uint32_t rank = 0;
#pragma unroll RANK_UNROLL
            for (int j = 0; j < 64; j++) {  // lanes >= P hold a copy of lane 0's value and are masked out
                const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)v, j);
                rank += ((uint32_t)j < P && (o < v || (o == v && (uint32_t)j < lane))) ? 1u : 0u;
            }
            if (lane < P) q[rank] = v;
        }
        // the first occurrences, 64 at a time, compacted with ballot + popcount
        for (uint32_t i0 = 0; i0 < nq; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool first = i < nq && (i == 0 || q[i] != q[i - 1]);
            const unsigned long long m = __ballot(first);
            if (first) u[nu + (uint32_t)__popcll(m & lt_mask)] = q[i];
            nu += (uint32_t)__popcll(m);
        }
    }
    if constexpr (THREADS > 64) {
        __shared__ uint32_t s_nu;
        if (t == 0) s_nu = nu;
        __syncthreads();
        nu = s_nu;
    } else {
        __syncthreads();
    }
    return nu;
}

// The emit rule of the E_s tables: does position i of the ascending p[0 .. c) contribute to E_s, and which child
__device__ __forceinline__ bool emit_of(const uint32_t* p, uint32_t c, uint32_t i, uint32_t s, uint32_t& child) {
    if (i >= c) return false;
    const uint32_t x = p[i], v = x >> s, bit = (x >> (s - 1)) & 1u;
    const bool first = i == 0 || (p[i - 1] >> s) != v;
    const bool last = i + 1 == c || (p[i + 1] >> s) != v;
    if (first && bit) {  // every position below v lies in the right child: the left one is missing
        child = 2 * v;
        return true;
    }
    if (last && !bit) {  // every position below v lies in the left child
        child = 2 * v + 1;
        return true;
    }
    return false;
}

// E_s of p[0 .. c), built by one wave (all 64 lanes call) into E, entries compacted with ballot + popcount.  Returns |E_s|.
__device__ __forceinline__ uint32_t build_level(const uint32_t* p, uint32_t c, uint32_t s, uint32_t* E) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1;
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < c; i0 += 64) {
        uint32_t child = 0;
        const bool e = emit_of(p, c, i0 + lane, s, child);
        const unsigned long long m = __ballot(e);
        if (e) E[run + (uint32_t)__popcll(m & lt_mask)] = child;
        run += (uint32_t)__popcll(m);
    }
    return run;
}

}  // namespace qdev
}  // namespace k
}  // namespace frieda
